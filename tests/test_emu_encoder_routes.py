"""A subset of tests/test_gpu_encoder_routes.py on the CPU wave emulator of tests/emu, through the same checker and under the same
bound (tests/gemm_helpers.py check_route): one-layer models of width 256 (ff 256) against the fp64 oracle on every encoder GEMM route,
at the sequence lengths where a route changes its tiling -- S = 32 / 33 (a 32-row tile edge), 65 (a 64-row tile edge), 207 (the paired
layer-0 launch's last length; S = 208, its first refusal, and the unpaired launch bit for bit against it are
tests/test_emu_path.py test_emulated_forward_branches and tests/test_emu_shared_layer0.py) -- and the hostile weights (large row means
through the folded statistics' Chan merge) on the row-tile kernel, the sequence-tile kernel and the fp32 route."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import gemm_helpers as gh  # noqa: E402
from emu_lib import emu  # noqa: E402


@pytest.mark.parametrize("route,B,T,lengths", [
    ("small", 2, 31, None), ("small", 1, 32, None),
    ("small64", 1, 64, [17]), ("small64", 1, 32, None),
    ("seq", 1, 32, [20]), ("seq", 1, 64, None),
    ("seq_shared1", 1, 31, None), ("seq_shared1", 1, 206, [100]),
    ("f32", 2, 32, [32, 5]),
])
def test_emulated_routes(engine_options, route, B, T, lengths):
    gh.check_route(engine_options, route, "cpu", emu(), "plain", 256, 256, B, T, lengths)


@pytest.mark.parametrize("route", ["small", "seq", "f32"])
def test_emulated_routes_on_hostile_weights(engine_options, route):
    gh.check_route(engine_options, route, "cpu", emu(), "hostile", 256, 256, 2, 32, [32, 11])
