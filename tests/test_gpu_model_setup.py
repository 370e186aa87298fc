"""The constant workspace of a model handle (csrc/model_setup.h carve_const behind mdm_const_bytes and mdm_prepare) on the MI355X:
mdm_prepare fills exactly the mdm_const_bytes bytes it reports -- nothing behind them, the last region up to their end, nothing at all
when the block is one byte short -- and fills them the same way twice (tests/model_setup_cases.py; the option table is host logic and
is tested on the emulator library, tests/test_emu_model_setup.py)."""
import pytest
import torch

import model_setup_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "these tests need the MI355X"


@pytest.mark.parametrize("name", list(mc.CONFIGS))
def test_prepare_fills_exactly_const_bytes(name):
    mc.check_block_is_exactly_as_large_as_reported(mc.bound_engine(name, DEV))


@pytest.mark.parametrize("name", mc.PURE_CONFIGS)
def test_prepare_is_a_pure_function_of_the_weights(name):
    mc.check_prepare_is_a_pure_function_of_the_weights(mc.bound_engine(name, DEV))
