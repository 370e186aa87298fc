"""The four attention kernels on the MI355X at kernel level (mdm_attention = csrc/attention_f32.h and attention_f32_long_kernel,
mdm_attention_x3 = csrc/attention_x3.h and attention_x3_long_kernel) against fp64: every key-tile count and `last_group` edge, seven
score regimes, every form of the `lengths` array, the persistent item loop on the real grid, and the memory contracts of the headers.

Bound (tests/attention_helpers.py): err <= k * max(e_ref, floor(S)), e_ref = the fp32 reference's own error against fp64 on that
case, k per kernel family from profiles/r10a_attention_parity.md.  Single-key cases and `ties` have bounds derived from the number
formats.  Every call runs with 64 sentinel rows behind `out` (must stay untouched), `out` itself starting as NaN (rows [0, nseq * S)
must come back finite) and the f16x3 scratch starting as 0xFF bytes.  Every test prints its figures before it asserts.

Shape unless stated: nseq = 2, H = 2 (D = 256)."""
import time

import pytest
import torch

import attention_helpers as ah
from helpers import memo

pytestmark = pytest.mark.gpu

EXACT_S = [1, 16, 17, 31, 32, 33, 48, 49, 64, 65, 96, 97, 112, 113, 128, 129, 144, 145, 160, 161, 192, 193, 208, 209, 224]
LONG_S = [225, 256, 257, 384, 385]


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mdm_amd import _native
    return memo(("attn_backend", "gpu"), lambda: ah.GpuBackend(_native.load_native()))       # raises if the library is not built


# ---- 1. every tile count ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["none", "counts"])
@pytest.mark.parametrize("profile", ["flat", "peaked"])
@pytest.mark.parametrize("S", EXACT_S + LONG_S)
def test_every_tile_count(gpu, S, profile, mask):
    """Both sides of every 32-key tile edge and of every 16-key `last_group` edge for NKT = 1 .. 7 (the second query half from
    S = 129 on), and the streaming kernels at 2 and 3+ query blocks with partial last key and query tiles."""
    spec = None if mask == "none" else ("counts", [S - 1, S // 2])
    if S == 1:
        ah.check_single_key(gpu, 2, 2, S, 2, spec, profile=profile)       # one token: V[0], under the bound derived for one valid key
    else:
        ah.check_parity(gpu, 2, 2, S, 2, profile, spec)


# ---- 2. score regimes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["none", "midtile"])
@pytest.mark.parametrize("profile", ah.PROFILES)
@pytest.mark.parametrize("S", [65, 197, 300])
def test_score_regimes(gpu, S, profile, mask):
    """Near one-hot rows, scores around +100 and -100 (exp without the maximum subtracted over- / underflows), the maximum in the last
    valid tile (the streaming kernels rescale at every tile) or in the first (never), exact ties."""
    spec = None if mask == "none" else ("counts", [S - 12, S // 2 + 5])      # 53 / 37, 185 / 103, 288 / 155: all end inside a tile
    ah.check_parity(gpu, 2, 2, S, 2, profile, spec)


@pytest.mark.parametrize("mask", ["none", "midtile", "bits_alt"])
@pytest.mark.parametrize("S", [65, 197, 257])
def test_ties_give_the_mean_of_the_valid_rows(gpu, S, mask):
    spec = {"none": None, "midtile": ("counts", [S - 12, S // 2 + 5]), "bits_alt": "bits_alt"}[mask]
    ah.check_ties(gpu, 2, 2, S, 2, spec)


# ---- 3. mask forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["flat", "peaked"])
@pytest.mark.parametrize("spec", ah.MASK_SPECS)
@pytest.mark.parametrize("S", [65, 197, 257])
def test_mask_forms(gpu, S, spec, profile):
    """Counts 0, 1, 31, 32, 33, S - 1 and S + 5 (clamped); bitmaps that are all zero, keep the last frame only, alternate, or leave whole
    key tiles without a valid key behind the lead token; a count / bitmap / full batch of three samples under six sequences."""
    if spec in ("count0", "bits_zero"):
        ah.check_single_key(gpu, 2, 2, S, 2, spec, profile=profile)
    elif spec == "mixed":
        ah.check_parity(gpu, 6, 3, S, 2, profile, spec)
    else:
        ah.check_parity(gpu, 2, 2, S, 2, profile, spec)


@pytest.mark.parametrize("S,spec", [(197, "mixed"), (300, ("counts", [288, 155, 0]))])
def test_four_heads(gpu, S, spec):
    """H = 4, D = 512 (the model's width): the head stride of the packed rows and of the output."""
    ah.check_parity(gpu, 6, 3, S, 4, "peaked", spec)


# ---- 4. item roll-over on the real grid ---------------------------------------------------------------------------------------------
def test_item_rollover_on_the_real_grid(gpu):
    """More (sequence, head) items than the persistent grid of attention_x3_kernel holds (two workgroups per CU, two per item): with
    2 nseq > 2 CUs + 8 every workgroup walks a third item, and 2 nseq not a multiple of 8 leaves the last group of eight ragged.  Nine
    samples cycle count / bitmap / full, so consecutive items of a workgroup carry different mask forms (the LDS key mask is rewritten,
    the next item's first tile prefetched, ring slots reused for output staging)."""
    t0 = time.time()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nseq = cus + 5
    while (2 * nseq) % 8 == 0:
        nseq += 1
    assert 2 * nseq > 2 * cus + 8 and (2 * nseq) % 8 != 0
    ah.check_parity(gpu, nseq, 9, 65, 2, "peaked", "mixed")
    print(f"[attention] roll-over: {cus} CUs, nseq = {nseq}, {time.time() - t0:.2f} s with the CPU references")
