"""The attention kernels' sources on the CPU wave emulator of tests/emu, through the helpers and under the bound of
tests/test_gpu_attention_kernels.py (tests/attention_helpers.py: err <= k * max(e_ref, floor(S)), guard rows, poisoned scratch): one
sequence length per key-tile count on peaked scores under a bitmap, the streaming kernels where they rescale at every tile, never, and
around +100, the single-key and ties cases with their derived bounds, and the mixed count / bitmap batch on the emulator's three-workgroup
limit (16 workgroups for 12 items: the persistent loop of attention_x3_kernel rolls over).  Plus, without any kernel: the mask builder
against mdm_amd/mdm.py frame_mask_lengths."""
import numpy as np
import pytest
import torch

import attention_helpers as ah
from emu.emu_lib import emu
from helpers import memo


@pytest.fixture(scope="module")
def backend():
    return memo(("attn_backend", "emu"), lambda: ah.EmuBackend(emu()))


@pytest.mark.parametrize("S", [33, 65, 97, 129, 161, 209])
def test_emulated_tile_counts_peaked_under_a_bitmap(backend, S):
    """NKT = 2 .. 7: 33 and 65 stop in the first 16-key group of their last tile (`last_group` false), 97, 129, 161 likewise, 209
    reaches into the second; from 129 on the second query half runs with idle waves."""
    ah.check_parity(backend, 2, 2, S, 2, "peaked", "bits_alt")


@pytest.mark.parametrize("profile,spec", [("ascending", ("counts", [245, 133])), ("descending", None), ("offset_pos", None)])
def test_emulated_streaming_kernels(backend, profile, spec):
    ah.check_parity(backend, 2, 2, 257, 2, profile, spec)


@pytest.mark.parametrize("S", [33, 257])
def test_emulated_count_zero_gives_the_first_value_row(backend, S):
    ah.check_single_key(backend, 2, 2, S, 2, "count0")


@pytest.mark.parametrize("S,spec", [(65, "bits_alt"), (257, None)])
def test_emulated_ties_give_the_mean_of_the_valid_rows(backend, S, spec):
    ah.check_ties(backend, 2, 2, S, 2, spec)


def test_emulated_mixed_batch_rolls_over_the_grid(backend):
    ah.check_parity(backend, 6, 3, 65, 2, "peaked", "mixed")


@pytest.mark.parametrize("S", [65, 197, 257])
def test_mask_builder_agrees_with_frame_mask_lengths(S):
    """make_lengths builds the ABI's array on its own; wherever a row has holes, mdm_amd/mdm.py frame_mask_lengths (the product's
    builder) must give the same ints from the validity matrix, and for prefix masks the same counts."""
    from mdm_amd.mdm import MDM
    for B, spec in [(2, "bits_last"), (2, "bits_alt"), (2, "bits_from63"), (3, "mixed")]:
        mine, valid = ah.make_lengths(B, S, spec)
        assert valid[:, 0].all() and valid.shape == (B, S)
        theirs = MDM.frame_mask_lengths(torch.from_numpy(valid[:, 1:].copy())).numpy()
        assert mine.dtype == np.int32 and np.array_equal(mine, theirs), spec
    for spec in ah.COUNT_SPECS:
        mine, valid = ah.make_lengths(2, S, spec)
        theirs = MDM.frame_mask_lengths(torch.from_numpy(valid[:, 1:].copy())).numpy()
        assert np.array_equal(np.minimum(mine, S - 1), theirs), spec          # (a count beyond the frames is clamped by the kernels)
    # an all-zero bitmap means what count 0 means (frame_mask_lengths itself writes the count form for it)
    mine, valid = ah.make_lengths(2, S, "bits_zero")
    assert np.array_equal(mine, np.array([-1, -1] + [0] * 16, np.int32))
    assert np.array_equal(valid, ah.make_lengths(2, S, "count0")[1])
    assert ah.make_lengths(2, S, None)[0] is None and ah.make_lengths(2, S, None)[1].all()
