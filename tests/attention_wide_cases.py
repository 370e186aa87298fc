"""Shared by tests/test_emu_attention_wide.py and tests/test_gpu_attention_wide.py: the 8-wave form of csrc/attention_x3.h
(MDM_OPT_ATTN_WIDE, attention_x3_kernel_wide) against the 4-wave kernel, bit for bit, through mdm_probe_attention_x3 of the probe /
emulator library -- the entry point that lets the caller choose the form, the lead tokens and both output forms (fp32 rows and hi / lo
planes).  The wide form runs the 4-wave kernel's per-tile body on the same fragments in the same order, so there is no tolerance: every
bit of every output agrees, or the schedule (copy waves, ring slots, wait counts, item roll-over) is wrong.

Inputs and masks come from tests/attention_helpers.py.  Its `lengths` arrays count FRAMES; with lead = 1 key 0 is the condition token and
always valid, with lead = 0 the same array masks keys directly (trans_dec), so `count0` leaves a sequence without a valid key there:
both forms then return the same NaN rows, which is why the comparison is on the bit patterns."""
import numpy as np

import attention_helpers as ah

SEQ_LENS = (129, 160, 161, 192, 193, 197, 208, 209, 224)    # both sides of every tile edge and `last_group` edge, NKT 5 .. 7
HEADS = (2, 4)
LEADS = (0, 1)


def mask_specs(S):
    """none, counts ending inside a tile, an alternating bitmap, count 0."""
    return (None, ("counts", [S - 21, 37, 130]), "bits_alt", "count0")


def nseq_of(S, H, mi):
    """3 .. 6 sequences, spread over the cases of the GPU matrix."""
    return 3 + (SEQ_LENS.index(S) + HEADS.index(H) + mi) % 4


def inputs(S, H, nseq, spec, profile="peaked"):
    B = max(2, nseq - 1)                                     # (a sequence takes row seq % B of the mask)
    qkv = ah.make_qkv(1, nseq, S, H, profile)
    lengths, _ = ah.make_lengths(B, S, spec)
    return qkv, lengths, B


def expect_finite(spec, lead):
    return not (spec == "count0" and lead == 0)
