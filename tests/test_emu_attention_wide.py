"""The 8-wave form of the split-precision attention kernel (csrc/attention_x3.h attention_x3_kernel_wide, MDM_OPT_ATTN_WIDE) on the CPU
wave emulator of tests/emu, against the 4-wave kernel with torch.equal on the bits of the fp32 rows and of both output planes
(tests/attention_wide_cases.py).  Every sequence length of the matrix runs with two (heads, mask, lead, nseq) combinations chosen so that
each mask form meets each head count and each lead; the emulator's grid holds three workgroups, so every case rolls over.  The same cases
run again under the LATE asynchronous model (MDM_EMU_LATE=1, latched per process: a child interpreter), where an LDS-DMA piece lands only
at the counted wait that covers it -- a copy wave's wait count that is too lenient, or a barrier a compute wave passes too early, reads a
poisoned ring slot."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_helpers as ah
import attention_wide_cases as wc
from emu.emu_lib import emu
from helpers import ROOT


def _run(lib, wide, qkv, lengths, nseq, B, S, H, lead):
    """-> (fp32 rows, hi plane, lo plane) as int tensors of their bits; every buffer starts as NaN (0xFF bytes in the 16-bit planes and
    the operand scratch), the guard rows behind each output as a sentinel."""
    D = H * ah.HD
    rows = nseq * S
    out = np.full((rows + ah.GUARD_ROWS, D), np.nan, np.float32)
    out[rows:] = ah.SENTINEL
    planes = [np.full((rows + ah.GUARD_ROWS, D), 0xFFFF, np.uint16) for _ in range(2)]
    for p in planes:
        p[rows:] = 0x1234
    nb = lib.mdm_attention_x3_scratch_bytes(nseq, S, D)
    scratch = np.full(nb, 0xFF, np.uint8)
    lp = lengths.ctypes.data if lengths is not None else None
    lib.check(lib.mdm_probe_attention_x3(qkv.ctypes.data, out.ctypes.data, planes[0].ctypes.data, planes[1].ctypes.data, lp, nseq, B, S, D,
                                         H, lead, wide, scratch.ctypes.data, nb, None), "mdm_probe_attention_x3")
    assert (out[rows:] == ah.SENTINEL).all() and all((p[rows:] == 0x1234).all() for p in planes), "wrote behind row nseq * S"
    return (torch.from_numpy(out[:rows].view(np.int32).copy()), torch.from_numpy(planes[0][:rows].view(np.int16).copy()),
            torch.from_numpy(planes[1][:rows].view(np.int16).copy()))


def _compare(lib, S, H, nseq, spec, lead, profile="peaked"):
    qkv, lengths, B = wc.inputs(S, H, nseq, spec, profile)
    wide = _run(lib, 1, qkv, lengths, nseq, B, S, H, lead)
    narrow = _run(lib, 0, qkv, lengths, nseq, B, S, H, lead)
    if wc.expect_finite(spec, lead):
        assert np.isfinite(wide[0].numpy().view(np.float32)).all() and np.isfinite(narrow[0].numpy().view(np.float32)).all()
    for name, a, b in zip(("fp32 rows", "hi plane", "lo plane"), wide, narrow):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} elements differ (S={S} H={H} nseq={nseq} mask={spec} lead={lead})"


def _cases():
    out = []
    for si, S in enumerate(wc.SEQ_LENS):
        for hi, H in enumerate(wc.HEADS):
            mi = (si + 2 * hi + si // 4) % 4          # every mask form meets both head counts and both leads over the nine lengths
            lead = (si + hi + si // 2) % 2
            out.append((S, H, mi, lead, (3 if H == 4 else 5) + si % 2))     # at most 16 items: the emulator runs them one lane at a time
    return out


def test_the_case_list_covers_every_combination_it_claims():
    cs = _cases()
    assert {(H, mi) for _, H, mi, _, _ in cs} == {(H, mi) for H in wc.HEADS for mi in range(4)}
    assert {(mi, lead) for _, _, mi, lead, _ in cs} == {(mi, lead) for mi in range(4) for lead in wc.LEADS}
    assert {(H, lead) for _, H, _, lead, _ in cs} == {(H, lead) for H in wc.HEADS for lead in wc.LEADS}
    assert {nseq for _, _, _, _, nseq in cs} == {3, 4, 5, 6}


@pytest.mark.parametrize("S,H,mi,lead,nseq", _cases())
def test_emulated_wide_attention_is_bit_identical(S, H, mi, lead, nseq):
    _compare(emu(), S, H, nseq, wc.mask_specs(S)[mi], lead)


def test_emulated_wide_attention_rolls_over_the_grid_with_changing_mask_forms():
    """Ten items on the emulator's three workgroups: a workgroup's consecutive items (b, b + 3, ...) belong to different sequences, whose
    masks cycle through a count, a bitmap and a full count -- the key mask in LDS is rebuilt per item while the copy wave already
    streams the next item's tiles."""
    _compare(emu(), 197, 2, 5, "mixed", 1)


@pytest.mark.slow
def test_emulated_wide_attention_under_the_late_async_model():
    emu()                                              # build once, in this process
    env = dict(os.environ, MDM_EMU_LATE="1", MDM_TEST_SERIAL="1", OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
    env.pop("PYTEST_XDIST_WORKER", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "bit_identical or rolls_over"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=3000)
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail
