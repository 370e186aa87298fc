"""csrc/evaluator.h (the mdm_eval_* entry points behind mdm_amd/evaluator.py) on the CPU wave emulator of tests/emu, at the narrowest
widths the kernels take: the reduced fixtures against the fp64 restatement, a one-step sequence beside a full-length one, and NaN
poison in the workspace and in what lies behind the sequences' ends.

Bound: the accuracy condition of the GPU test -- max-abs error against fp64 <= 4 x e_ref, e_ref being the reference's own fp32 error
on that fixture (tests/golden/PIN_REPORT_evaluator.json).  The cases without a fixture of their own take 4 x the e_ref of
the reduced fixture of the same network, widths and kind of weights (default or trained-like), named at each use: same depth of sums,
no more steps."""
import types

import numpy as np
import pytest
import torch

from emu.emu_lib import emu
import evaluator_helpers as eh
from helpers import maxabs


@pytest.fixture(scope="module")
def lib():
    return emu()


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _bound(name):
    return 4 * eh.pin_report()[name]["e_ref"]


def test_emulated_motion_fixture_matches_fp64(lib):
    name = "motion_b3_reduced"
    inp, g = eh.fixture_inputs(name), eh.load_fixture(name)
    w = eh.make_wrapper(name, eh.fixture_weights(name), "cpu", native_lib=lib)
    got = w.get_motion_embeddings(_t(inp["motions"]), _t(inp["m_lens"]))
    err, bound = maxabs(got, g["fp64_motion"]), 4 * eh.pin_report()[name]["e_ref"]
    print(f"[evaluator] {name}: max-abs vs fp64 = {err:.3e} (bound {bound:.3e})")
    assert got.shape == g["fp64_motion"].shape and got.dtype == torch.float32
    assert err <= bound


def test_emulated_text_fixture_matches_fp64(lib):
    name = "text_b4_reduced"
    inp, g = eh.fixture_inputs(name), eh.load_fixture(name)
    w = eh.make_wrapper(name, eh.fixture_weights(name), "cpu", native_lib=lib)
    got = w._text_rows(_t(inp["word_embs"]), _t(inp["pos_ohot"]), inp["cap_lens"].tolist())
    err, bound = maxabs(got, g["fp64_text"]), 4 * eh.pin_report()[name]["e_ref"]
    print(f"[evaluator] {name}: max-abs vs fp64 = {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_emulated_one_step_sequence_beside_a_full_one(lib):
    """m_lens 4 and 40 at T = 40: one recurrent step (both directions read movement step 0) beside ten; and the one-step row alone
    gives the same bits (a row's result does not depend on the batch)."""
    weights = eh.build_weights(21, eh.REDUCED, trained=True)
    w = eh.make_wrapper(eh.REDUCED, weights, "cpu", native_lib=lib)
    m_lens = [40, 4]
    motions = eh.make_motion_inputs(21, 2, 40, 263, m_lens)
    got = w.get_motion_embeddings(_t(motions), torch.tensor(m_lens))
    want, _ = eh.motion_embeddings_fp64(weights, motions, m_lens)
    err = maxabs(got, want)
    print(f"[evaluator] one step beside ten: max-abs vs fp64 = {err:.3e} (bound {_bound('motion_b5_short_reduced'):.3e})")
    assert err <= _bound("motion_b5_short_reduced")           # trained-like weights, reduced widths
    alone = w.get_motion_embeddings(_t(motions[1:]), torch.tensor(m_lens[1:]))
    assert torch.equal(alone[0], got[1])


@pytest.fixture()
def poisoned(monkeypatch, lib):
    import mdm_amd.evaluator as ev_mod
    real = torch

    class PoisonTorch(types.ModuleType):
        def __getattr__(self, k):
            return getattr(real, k)

        def empty(self, *a, **k):
            t = real.empty(*a, **k)
            return t.fill_(0xFF) if t.dtype == real.uint8 else (t.fill_(float("nan")) if t.is_floating_point() else t)

    monkeypatch.setattr(ev_mod, "torch", PoisonTorch("torch"))
    return lib


def test_poison_in_workspace_and_padding_does_not_reach_the_output(poisoned):
    """Workspace and outputs start as NaN (0xFF bytes); so do the frames no convolution window of a valid movement step reaches
    (frame 4 (len // 4) + 3 on: the last valid step's windows end at 4 (len // 4) + 2) and the words behind every caption's end."""
    weights = eh.build_weights(22, eh.REDUCED)
    w = eh.make_wrapper(eh.REDUCED, weights, "cpu", native_lib=poisoned)
    m_lens, T = [33, 18, 9], 36
    motions = eh.make_motion_inputs(22, 3, T, 263, m_lens)
    want, _ = eh.motion_embeddings_fp64(weights, motions, m_lens)
    bad = motions.copy()
    for b, l in enumerate(m_lens):
        bad[b, 4 * (l // 4) + 3:] = np.nan
    assert np.isnan(bad).any()
    got = w.get_motion_embeddings(_t(bad), torch.tensor(m_lens))
    assert not bool(torch.isnan(got).any())
    assert maxabs(got, want) <= _bound("motion_b3_reduced")     # default weights, reduced widths

    cap_lens, L = [7, 3, 1], 8
    word, pos = eh.make_text_inputs(22, 3, L, 300, 15, cap_lens)
    want = eh.text_encoder_fp64(weights[1], word, pos, cap_lens)
    for b, l in enumerate(cap_lens):
        word[b, l:] = np.nan
        pos[b, l:] = np.nan
    got = w._text_rows(_t(word), _t(pos), cap_lens)
    assert not bool(torch.isnan(got).any())
    assert maxabs(got, want) <= _bound("text_b4_reduced")
