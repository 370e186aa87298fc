"""The 8-wave form of the split-precision attention kernel (csrc/attention_x3.h attention_x3_kernel_wide, MDM_OPT_ATTN_WIDE) on the
MI355X against the 4-wave kernel: torch.equal on the bits of the fp32 rows and of both output planes, through mdm_probe_attention_x3 of
the probe library (tests/attention_wide_cases.py).  Sequence lengths on both sides of every tile edge and `last_group` edge of five to
seven key tiles (three, two and one copy waves), two and four heads, three to six sequences, no mask / counts ending inside a tile / an
alternating bitmap / count 0, lead = 0 and 1; and the item loop on the real grid.  Every buffer starts as NaN."""
import pytest
import torch

import attention_helpers as ah
import attention_wide_cases as wc
from helpers import memo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def probe():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mdm_amd import _native
    return _native.load_probe()                                    # raises if the library is not built


def _run(lib, wide, qd, ld, nseq, B, S, H, lead):
    D = H * ah.HD
    rows = nseq * S
    out = torch.full((rows + ah.GUARD_ROWS, D), float("nan"), device=DEV)
    out[rows:] = ah.SENTINEL
    planes = [torch.full((rows + ah.GUARD_ROWS, D), -1, dtype=torch.int16, device=DEV) for _ in range(2)]     # 0xFFFF: an fp16 NaN
    for p in planes:
        p[rows:] = 0x1234
    nb = lib.mdm_attention_x3_scratch_bytes(nseq, S, D)
    scratch = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)
    lib.check(lib.mdm_probe_attention_x3(qd.data_ptr(), out.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr(),
                                         ld.data_ptr() if ld is not None else None, nseq, B, S, D, H, lead, wide, scratch.data_ptr(), nb,
                                         torch.cuda.current_stream().cuda_stream), "mdm_probe_attention_x3")
    torch.cuda.synchronize()
    assert bool((out[rows:] == ah.SENTINEL).all()) and all(bool((p[rows:] == 0x1234).all()) for p in planes), "wrote behind row nseq * S"
    return out[:rows].view(torch.int32), planes[0][:rows], planes[1][:rows]


def _compare(lib, S, H, nseq, spec, lead, B=None):
    def build():
        qkv, lengths, B_ = wc.inputs(S, H, nseq, spec)
        return torch.from_numpy(qkv).to(DEV), None if lengths is None else torch.from_numpy(lengths).to(DEV), B_
    if B is None:
        qd, ld, B = memo(("attn_wide_in", S, H, nseq, str(spec)), build)          # shared by lead = 0 and 1, never written to
    else:
        qd = torch.from_numpy(ah.make_qkv(1, nseq, S, H, "peaked")).to(DEV)
        ld = torch.from_numpy(ah.make_lengths(B, S, spec)[0]).to(DEV)
    wide = _run(lib, 1, qd, ld, nseq, B, S, H, lead)
    narrow = _run(lib, 0, qd, ld, nseq, B, S, H, lead)
    if wc.expect_finite(spec, lead):
        assert bool(torch.isfinite(wide[0].view(torch.float32)).all()) and bool(torch.isfinite(narrow[0].view(torch.float32)).all())
    for name, a, b in zip(("fp32 rows", "hi plane", "lo plane"), wide, narrow):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ (S={S} H={H} nseq={nseq} mask={spec} lead={lead})"


@pytest.mark.parametrize("lead", wc.LEADS)
@pytest.mark.parametrize("mi", range(4))
@pytest.mark.parametrize("H", wc.HEADS)
@pytest.mark.parametrize("S", wc.SEQ_LENS)
def test_wide_attention_is_bit_identical(probe, S, H, mi, lead):
    _compare(probe, S, H, wc.nseq_of(S, H, mi), wc.mask_specs(S)[mi], lead)


def test_wide_attention_rolls_over_the_real_grid_with_changing_mask_forms(probe):
    """More (sequence, head) items than CUs (one persistent 8-wave workgroup each), their number not divisible by 8, at S = 197 (one copy
    wave): seven samples cycle count / bitmap / full count, so a workgroup's consecutive items carry different mask forms while the copy
    wave streams on across the item boundary."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nseq = cus // 2 + 3
    while (2 * nseq) % 8 == 0:
        nseq += 1
    assert 2 * nseq > cus and (2 * nseq) % 8 != 0
    _compare(probe, 197, 2, nseq, "mixed", 1, B=7)
