"""The model handle's set-up (csrc/model_setup.h) on the CPU emulator of tests/emu.  The constant workspace: mdm_prepare fills exactly
the mdm_const_bytes bytes that carve_const lays out -- nothing behind them, the last region up to their end, nothing at all when the
block is one byte short -- and fills them the same way twice (tests/model_setup_cases.py).  The option table: every MDM_OPT_* key's
default, its whole range through mdm_set_option / mdm_get_option, and each refusal with its text and without a change of the value."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
from emu_lib import emu  # noqa: E402
import model_setup_cases as mc  # noqa: E402
from mdm_amd import _native  # noqa: E402

MDM_EINVAL = -1


@pytest.mark.parametrize("name", list(mc.CONFIGS))
def test_emulated_prepare_fills_exactly_const_bytes(name):
    mc.check_block_is_exactly_as_large_as_reported(mc.bound_engine(name, "cpu", emu()))


@pytest.mark.parametrize("name", mc.PURE_CONFIGS)
def test_emulated_prepare_is_a_pure_function_of_the_weights(name):
    mc.check_prepare_is_a_pure_function_of_the_weights(mc.bound_engine(name, "cpu", emu()))


# key -> (name, default of include/mdm_hip.h, values to round-trip, text of the range)
I32_MAX = 2 ** 31 - 1
OPTIONS = {
    1: ("MDM_OPT_SMALL_GEMM_MAX_SEQS", 80, [0, 1, 80, I32_MAX], "must be >= 0"),
    2: ("MDM_OPT_SMALL_GEMM_ROW_TILES", 0, [0, 1, 2], "must be 0 (by size), 1 or 2"),
    3: ("MDM_OPT_DEC_FUSED_XATTN", 3, [0, 1, 2, 3], "must be 0, 1, 2 or 3"),
    4: ("MDM_OPT_DEC_FUSED_SELFATTN", 1, [0, 1], "must be 0 or 1"),
    5: ("MDM_OPT_ATTN_DIRECT_OUT", 0, [0, 1], "must be 0 or 1"),
    6: ("MDM_OPT_DEC_TIME_TOKEN", 0, [0, 1], "must be 0 or 1"),
    7: ("MDM_OPT_ENC_SHARED_LAYER0", 1, [0, 1], "must be 0 or 1"),
    8: ("MDM_OPT_ATTN_WIDE", 1, [0, 1], "must be 0 or 1"),
}
TIME_TOKEN_TEXT = b"mdm_set_option: MDM_OPT_DEC_TIME_TOKEN needs a trans_dec model created with context_len = 1 (the class-token row)"


@pytest.fixture()
def handle():
    lib, made = emu(), []

    def create(arch="trans_dec", context_len=1):
        cfg = _native.MdmConfig(njoints=263, nfeats=1, latent_dim=256, ff_size=1024, num_layers=2, num_heads=2, clip_dim=512, max_len=512,
                                mask_frames=1, arch=_native.ARCH[arch], context_len=context_len)
        h = C.c_void_p()
        assert lib.mdm_create(C.byref(cfg), C.byref(h)) == 0, lib.mdm_last_error()
        made.append(h)
        return h
    yield create
    for h in made:
        lib.mdm_destroy(h)


def _get(lib, h, key):
    v = C.c_int32(-12345)
    assert lib.mdm_get_option(h, key, C.byref(v)) == 0, lib.mdm_last_error()
    return v.value


@pytest.mark.parametrize("key", sorted(OPTIONS))
def test_every_option_both_ways(handle, key):
    lib, h = emu(), handle()          # trans_dec with context_len 1: the one handle that takes every value of every key
    name, default, values, text = OPTIONS[key]
    assert _get(lib, h, key) == default
    for v in values:
        assert lib.mdm_set_option(h, key, v) == 0, lib.mdm_last_error()
        assert _get(lib, h, key) == v
    for bad in [values[0] - 1] + ([values[-1] + 1] if values[-1] != I32_MAX else []):
        assert lib.mdm_set_option(h, key, bad) == MDM_EINVAL
        assert lib.mdm_last_error() == f"mdm_set_option: {name} {text}".encode()
        assert _get(lib, h, key) == values[-1]
    for other in OPTIONS:             # ... and no other key's value moved
        if other != key:
            assert _get(lib, h, other) == OPTIONS[other][1]


def test_unknown_keys_and_null_arguments_are_refused(handle):
    lib, h = emu(), handle()
    v = C.c_int32(7)
    for key in (0, 9):
        assert lib.mdm_set_option(h, key, 0) == MDM_EINVAL and lib.mdm_last_error() == f"mdm_set_option: unknown key {key}".encode()
        assert lib.mdm_get_option(h, key, C.byref(v)) == MDM_EINVAL and lib.mdm_last_error() == f"mdm_get_option: unknown key {key}".encode()
        assert v.value == 7
    assert lib.mdm_set_option(None, 1, 0) == MDM_EINVAL and lib.mdm_last_error() == b"mdm_set_option: null model"
    assert lib.mdm_get_option(None, 1, C.byref(v)) == MDM_EINVAL and lib.mdm_last_error() == b"mdm_get_option: null argument"
    assert lib.mdm_get_option(h, 1, None) == MDM_EINVAL and lib.mdm_last_error() == b"mdm_get_option: null argument"


@pytest.mark.parametrize("arch,context_len,allowed", [("trans_enc", 0, False), ("trans_dec", 20, False), ("trans_dec", 1, True)])
def test_time_token_needs_the_class_token_row(handle, arch, context_len, allowed):
    lib, h = emu(), handle(arch, context_len)
    if allowed:
        assert lib.mdm_set_option(h, 6, 1) == 0 and _get(lib, h, 6) == 1
    else:
        assert lib.mdm_set_option(h, 6, 1) == MDM_EINVAL and lib.mdm_last_error() == TIME_TOKEN_TEXT
        assert _get(lib, h, 6) == 0
    assert lib.mdm_set_option(h, 6, 0) == 0 and _get(lib, h, 6) == 0
