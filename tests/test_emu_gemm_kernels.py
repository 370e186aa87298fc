"""A subset of tests/test_gpu_gemm_kernels.py on the CPU wave emulator of tests/emu, through the same helpers and under the same bound
(tests/gemm_helpers.py: err <= k * max(e_ref, floor), `integer` bit for bit, guard rows, NaN `out`, 0xFF scratch): the row, column and
k edges of mdm_linear_x3's 224 x 256 x 32 tile, every operand regime, every epilogue and the refused calls; both tile forms of
mdm_linear on their edges; mdm_layernorm's regimes.  The emulator's persistent grid is three workgroups, so every case with more than
three tiles (M = 449 with N = 516: nine) rolls over."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import gemm_helpers as gh  # noqa: E402
from emu_lib import emu  # noqa: E402
from helpers import memo  # noqa: E402


@pytest.fixture(scope="module")
def backend():
    return memo(("gemm_backend", "emu"), lambda: gh.EmuBackend(emu()))


# ---- mdm_linear_x3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 33, 223, 224, 225, 449])
def test_emulated_row_edges(backend, M):
    for regime in ("flat", "integer"):
        gh.check_linear(backend, "x3", M, 260, 64, regime, gh.ACT_NONE, True)


@pytest.mark.parametrize("N", [4, 28, 36, 252, 256, 260, 516])
def test_emulated_column_edges(backend, N):
    for regime in ("flat", "integer"):
        gh.check_linear(backend, "x3", 225, N, 64, regime, gh.ACT_NONE, True)


@pytest.mark.parametrize("K", [32, 96, 288])
def test_emulated_k_steps(backend, K):
    for regime in ("flat", "integer") if K < 288 else ("integer",):
        gh.check_linear(backend, "x3", 225, 260, K, regime, gh.ACT_NONE, False)


@pytest.mark.parametrize("regime", gh.REGIMES)
def test_emulated_regimes(backend, regime):
    gh.check_linear(backend, "x3", 225, 260, 96, regime, gh.ACT_NONE, True)
    gh.check_linear(backend, "f32", 129, 132, 96, regime, gh.ACT_NONE, True)


def test_emulated_regimes_roll_over_the_grid(backend):
    for regime in ("wide", "integer"):
        gh.check_linear(backend, "x3", 449, 516, 96, regime, gh.ACT_NONE, True)


def test_emulated_epilogues_and_refused_calls(backend):
    for act, res in [(gh.ACT_NONE, False), (gh.ACT_GELU, False), (gh.ACT_GELU, True), (gh.ACT_SILU, False)]:
        gh.check_linear(backend, "x3", 225, 260, 64, "flat", act, res)
        gh.check_linear(backend, "x3", 5, 260, 64, "flat", act, res)
    gh.check_linear_refused(backend, "x3", 225, 260, 64, gh.ACT_SILU, True, gh.MDM_EUNSUPPORTED)
    gh.check_linear_refused(backend, "x3", 33, 258, 64, gh.ACT_NONE, False, gh.MDM_EINVAL)
    gh.check_linear_refused(backend, "x3", 33, 260, 48, gh.ACT_NONE, False, gh.MDM_EINVAL)


def test_emulated_rows_do_not_depend_on_the_batch(backend):
    N, K = 260, 64
    a, w, b, _, _, _ = gh.linear_case(448, N, K, "flat")
    whole = gh.run_linear(backend, "x3", 448, N, K, "flat")
    for half in range(2):
        rc, full = backend.linear("x3", np.ascontiguousarray(a[224 * half:224 * (half + 1)]), w, b, None, 224, N, K, gh.ACT_NONE)
        assert rc == gh.MDM_OK
        assert np.array_equal(full[gh.GUARD_ROWS:gh.GUARD_ROWS + 224].view(np.uint32), whole[224 * half:224 * (half + 1)].view(np.uint32))


# ---- mdm_linear -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,form", [(64, 260, 64), (129, 132, 64), (63, 264, 64), (63, 260, 128), (127, 128, 128), (1, 260, 128),
                                      (33, 36, 128)])
def test_emulated_f32_tile_forms(backend, M, N, form):
    assert gh.f32_tile_form(M, N) == form
    for regime in ("flat", "integer"):
        gh.check_linear(backend, "f32", M, N, 36, regime, gh.ACT_NONE, True)


@pytest.mark.parametrize("K", [4, 28, 32, 68])
def test_emulated_f32_k_edges(backend, K):
    for regime in ("flat", "integer"):
        gh.check_linear(backend, "f32", 129, 132, K, regime, gh.ACT_NONE, False)
    gh.check_linear(backend, "f32", 33, 36, K, "flat", gh.ACT_SILU, True)


# ---- mdm_layernorm --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", gh.LN_REGIMES)
def test_emulated_layernorm(backend, regime):
    for rows, D in [(1, 256), (65, 512), (63, 1024)]:
        gh.check_layernorm(backend, rows, D, regime)
