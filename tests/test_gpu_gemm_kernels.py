"""The GEMM kernels on the MI355X at kernel level -- mdm_linear_x3 (csrc/gemm_x3.h, gemm_x3_kernel<ACT, RES, X3_OUT_F32>: 224-row x 256-column tiles,
32 k per step), mdm_linear (csrc/gemm_f32.h: 64x64 and 128x128 tiles, 32 k per step, K % 4 == 0) -- and mdm_layernorm against fp64:
both sides of every tile edge in M, N and K, six operand regimes, every epilogue, the persistent grid's roll-over, and the memory
contracts.

Bound (tests/gemm_helpers.py): err <= k * max(e_ref, floor), e_ref = the torch fp32 reference's own error against fp64 on that case,
k per kernel from profiles/r11a_gemm_parity.md; the `integer` regime bit for bit.  Every call runs with sentinel rows in front of and
behind `out` (must stay untouched), `out` starting as NaN (must come back finite) and the f16x3 scratch as 0xFF bytes.  Every test
prints its figures (`[gemm] gpu kernel=... ratio=...`) before it asserts."""
import numpy as np
import pytest
import torch

import gemm_helpers as gh
from helpers import memo

pytestmark = pytest.mark.gpu

EPILOGUES = [(gh.ACT_NONE, False), (gh.ACT_NONE, True), (gh.ACT_GELU, False), (gh.ACT_GELU, True), (gh.ACT_SILU, False)]


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mdm_amd import _native
    return memo(("gemm_backend", "gpu"), lambda: gh.GpuBackend(_native.load_native()))       # raises if the library is not built


# ---- mdm_linear_x3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["flat", "integer"])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 208, 223, 224, 225, 447, 448, 449])
def test_every_row_edge(gpu, M, regime):
    """One row, both sides of a 32-row sub-tile, the 208-row form's last row, both sides of one and of two 224-row tiles; N = 260 is a
    second column tile of 4 columns."""
    gh.check_linear(gpu, "x3", M, 260, 64, regime, gh.ACT_NONE, True)


@pytest.mark.parametrize("regime", ["flat", "integer"])
@pytest.mark.parametrize("N", [4, 28, 32, 36, 252, 256, 260, 516])
def test_every_column_edge(gpu, N, regime):
    """Both sides of a wave's 32 columns and of the 256-column tile, three column tiles; every N that is no multiple of 32 reads pad
    rows of the fragment-ordered weight planes, which start as 0xFF bytes here."""
    gh.check_linear(gpu, "x3", 225, N, 64, regime, gh.ACT_NONE, True)


@pytest.mark.parametrize("K,regime", [(K, r) for K in (32, 64, 96, 160, 288, 1024) for r in ("flat", "integer") if (K, r) != (1024, "integer")])
def test_k_steps(gpu, K, regime):
    """1, 2, 3, 5, 9 and 32 k-steps: a single step, odd and even counts.  (`integer` is exact up to K = 288: 1024 * 64 * 2^8 >= 2^24.)"""
    gh.check_linear(gpu, "x3", 225, 260, K, regime, gh.ACT_NONE, False)


@pytest.mark.parametrize("shape", [(225, 260, 96), (449, 516, 288)])
@pytest.mark.parametrize("regime", gh.REGIMES)
def test_regimes(gpu, regime, shape):
    gh.check_linear(gpu, "x3", *shape, regime, gh.ACT_NONE, True)


@pytest.mark.parametrize("M", [225, 5])
@pytest.mark.parametrize("act,res", EPILOGUES)
def test_epilogues(gpu, act, res, M):
    gh.check_linear(gpu, "x3", M, 260, 64, "flat", act, res)


def test_unsupported_and_invalid_calls_are_refused(gpu):
    """silu + residual has no instantiation (MDM_EUNSUPPORTED); N % 4 != 0 and K % 32 != 0 are outside the contract (MDM_EINVAL).  `out`
    stays all NaN."""
    gh.check_linear_refused(gpu, "x3", 225, 260, 64, gh.ACT_SILU, True, gh.MDM_EUNSUPPORTED)
    gh.check_linear_refused(gpu, "x3", 33, 258, 64, gh.ACT_NONE, False, gh.MDM_EINVAL)
    gh.check_linear_refused(gpu, "x3", 33, 260, 48, gh.ACT_NONE, False, gh.MDM_EINVAL)


@pytest.mark.parametrize("regime", ["integer", "flat"])
def test_rollover_on_the_real_grid(gpu, regime):
    """131 row tiles x 2 column tiles = 262 tiles on a persistent grid of one workgroup per CU (256 on the MI355X): six workgroups walk
    a second tile, the last row tile has 5 rows."""
    M, N, K = 224 * 130 + 5, 260, 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = ((M + 223) // 224) * ((N + 255) // 256)
    print(f"[gemm] roll-over: {tiles} tiles on {cus // 8 * 8} workgroups")
    assert tiles == 262 and tiles > cus // 8 * 8
    gh.check_linear(gpu, "x3", M, N, K, regime, gh.ACT_NONE, False)


def test_rows_do_not_depend_on_the_batch(gpu):
    """448 rows in one call against two calls of 224: a row's products and their order do not depend on the tile it lands in."""
    N, K = 260, 64
    a, w, b, _, _, _ = gh.linear_case(448, N, K, "flat")
    whole = gh.run_linear(gpu, "x3", 448, N, K, "flat")
    for half in range(2):
        ah = np.ascontiguousarray(a[224 * half:224 * (half + 1)])
        rc, full = gpu.linear("x3", ah, w, b, None, 224, N, K, gh.ACT_NONE)
        assert rc == gh.MDM_OK
        part = full[gh.GUARD_ROWS:gh.GUARD_ROWS + 224]
        assert np.array_equal(part.view(np.uint32), whole[224 * half:224 * (half + 1)].view(np.uint32)), half


# ---- mdm_linear -----------------------------------------------------------------------------------------------------------------------
# (M, N) -> the tile form csrc/gemm_f32.h launch_gemm_f32_t takes: 64x64 tiles when tiles128 < 512 and M * N >= 16384, else 128x128
_GRID = [(M, N) for M in (63, 64, 65, 129) for N in (64, 68, 132, 260)]
F32_64 = [mn for mn in _GRID if mn[0] * mn[1] >= 16384] + [(63, 264)]        # (64, 260), (65, 260), (129, 132), (129, 260); a 63-row tile
F32_128_TINY = [mn for mn in _GRID if mn[0] * mn[1] < 16384] + [(5, 512), (1, 260), (127, 128), (33, 36)]    # (63, 260) = 16380 among them
F32_128_LARGE = (128 * 256 + 1, 130)                                                            # 257 x 2 = 514 tiles >= 512


def test_the_shape_rule_pins_each_tile_form():
    assert len(F32_64) == 5 and len(F32_128_TINY) == 16 and all(gh.f32_tile_form(M, N) == 64 for M, N in F32_64)
    assert all(M * N < 16384 and gh.f32_tile_form(M, N) == 128 for M, N in F32_128_TINY)
    assert gh.f32_tile_form(*F32_128_LARGE) == 128 and gh.f32_tile_form(128 * 255, 130) == 64       # 514 tiles; 255 x 2 = 510


@pytest.mark.parametrize("regime", ["flat", "integer"])
@pytest.mark.parametrize("M,N", F32_64 + F32_128_TINY)
def test_f32_tile_edges(gpu, M, N, regime):
    """Both tile forms on their own edges, K = 36 (one whole k-step and a 4-wide tail), with a residual."""
    gh.check_linear(gpu, "f32", M, N, 36, regime, gh.ACT_NONE, True)


@pytest.mark.parametrize("regime", ["flat", "integer"])
def test_f32_large_output_takes_128_tiles(gpu, regime):
    gh.check_linear(gpu, "f32", *F32_128_LARGE, 36, regime, gh.ACT_NONE, False)


@pytest.mark.parametrize("M,N", [(129, 132), (33, 36)])
@pytest.mark.parametrize("K,regime", [(K, r) for K in (4, 28, 32, 36, 68, 288, 1024) for r in ("flat", "integer") if (K, r) != (1024, "integer")])
def test_f32_k_edges(gpu, K, regime, M, N):
    """K % 4 == 0 is the contract and 32 the k-step: less than one step, both sides of one, two steps and a tail, nine, thirty-two."""
    gh.check_linear(gpu, "f32", M, N, K, regime, gh.ACT_NONE, False)


@pytest.mark.parametrize("M,N", [(129, 132), (33, 36)])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("act", [gh.ACT_NONE, gh.ACT_GELU, gh.ACT_SILU])
def test_f32_epilogues(gpu, act, res, M, N):
    gh.check_linear(gpu, "f32", M, N, 68, "flat", act, res)


@pytest.mark.parametrize("M,N,K", [(129, 132, 96), (33, 36, 288)])
@pytest.mark.parametrize("regime", gh.REGIMES)
def test_f32_regimes(gpu, regime, M, N, K):
    gh.check_linear(gpu, "f32", M, N, K, regime, gh.ACT_NONE, True)


# ---- mdm_layernorm --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", gh.LN_REGIMES)
@pytest.mark.parametrize("D", [256, 512, 1024])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
def test_layernorm(gpu, rows, D, regime):
    gh.check_layernorm(gpu, rows, D, regime)
