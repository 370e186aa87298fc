"""Host side of mdm_amd/evaluator.py (no GPU): the fp64 restatement against the reference's recorded outputs, the state-dict contract,
the finest.tar loader, every refusal, the reference's tie order, and the exported mdm_eval_* symbols."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import evaluator_helpers as eh
from helpers import maxabs


@pytest.mark.parametrize("name", list(eh.FIXTURES))
def test_fp64_restatement_reproduces_the_fixture_within_the_pin_report(name):
    """The restatement is pinned twice: to its own recorded output (it has not drifted) and to the reference's fp32 output within
    e_ref, the figure the generator measured -- which is itself at fp32 rounding level (a few 1e-6 on outputs of magnitude 3)."""
    g, rep = eh.load_fixture(name), eh.pin_report()[name]
    now = eh.run_fp64(name)
    assert rep["e_ref"] == rep["fp64_vs_reference_fp32"] and 0 < rep["e_ref"] < 1e-5
    for k, v in now.items():
        assert maxabs(v, g[f"fp64_{k}"]) < 1e-12
        assert maxabs(v, g[f"ref_{k}"]) <= rep["e_ref"] * (1 + 1e-9)
        assert list(v.shape) == rep["shape"][k]


def test_fixture_set_covers_the_issue_cases():
    f = eh.FIXTURES
    assert len(set(f["motion_b3_reduced"]["m_lens"])) < 3 and f["motion_b3_reduced"]["T"] == 60                 # ragged, with a tie
    assert sorted(f["motion_b32_full_default"]["m_lens"])[0] == 40 and max(f["motion_b32_full_default"]["m_lens"]) == 196
    assert f["motion_b32_full_trained"]["trained"] and not f["motion_b32_full_default"]["trained"]
    short = f["motion_b5_short_reduced"]
    assert short["T"] == 200 and sum(4 <= l <= 7 for l in short["m_lens"]) == 1 and max(short["m_lens"]) // 4 == 50
    for n in ("text_b4_reduced", "text_b4_full"):
        assert f[n]["L"] == 22 and f[n]["cap_lens"][-1] == 1 and f[n]["cap_lens"] == sorted(f[n]["cap_lens"], reverse=True)
    co = f["co_b32_full"]
    assert len(co["m_lens"]) == 32 and list(np.argsort(co["m_lens"])[::-1]) != list(range(32))     # align_idx is a real permutation
    rep = eh.pin_report()["co_b32_full"]
    assert rep["nearest_distance_gap"] > 100 * rep["e_ref"]


def _wrapper(dims=None, seed=3, device="cpu"):
    weights = eh.build_weights(seed, dims or eh.REDUCED)
    return eh.make_wrapper(dims or eh.REDUCED, weights, device), weights


def test_state_dict_keys_are_the_reference_s():
    """tests/golden/evaluator_state_dict_keys.json: keys, order and shapes of the reference's three modules at full width."""
    from mdm_amd import evaluator as ev
    with open(eh.KEYS_FILE) as fh:
        ref = json.load(fh)
    text, motion, movement = ev.build_containers(ev.default_opt("humanml", "cpu"))
    for name, enc in (("movement_encoder", movement), ("text_encoder", text), ("motion_encoder", motion)):
        sd = enc.state_dict()
        assert list(sd.keys()) == list(ref[name].keys()), name
        assert {k: list(v.shape) for k, v in sd.items()} == ref[name]
    w, _ = _wrapper()
    for attr in ("opt", "device", "text_encoder", "motion_encoder", "movement_encoder"):
        assert hasattr(w, attr)
    assert w.opt["unit_length"] == 4 and w.opt["dim_pose"] == 263 and w.opt["max_motion_length"] == 196
    assert ev.default_opt("kit", "cpu")["dim_pose"] == 251
    assert not any(p.requires_grad for p in w.motion_encoder.parameters()) and not w.motion_encoder.training
    with pytest.raises(RuntimeError):                                   # load_state_dict is strict, as the reference's
        w.movement_encoder.load_state_dict({"main.0.weight": torch.zeros(1)})


def test_finest_tar_loader_agrees_with_from_state_dicts(tmp_path, monkeypatch):
    """The constructor reads ./t2m/text_mot_match/model/finest.tar (./kit/... for KIT) relative to the working directory, as
    build_evaluators does; a tar written here gives the parameters from_state_dicts gives."""
    from mdm_amd.evaluator import EvaluatorMDMWrapper
    weights = eh.build_weights(5, eh.FULL)
    d = tmp_path / "t2m" / "text_mot_match" / "model"
    d.mkdir(parents=True)
    torch.save({"movement_encoder": weights[0], "text_encoder": weights[1], "motion_encoder": weights[2], "epoch": 7}, str(d / "finest.tar"))
    monkeypatch.chdir(tmp_path)
    a = EvaluatorMDMWrapper("humanml", "cpu")
    b = EvaluatorMDMWrapper.from_state_dicts(*weights, "humanml", "cpu")
    for n in ("movement_encoder", "text_encoder", "motion_encoder"):
        sa, sb = getattr(a, n).state_dict(), getattr(b, n).state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert a.opt == b.opt
    with pytest.raises(FileNotFoundError):
        EvaluatorMDMWrapper("kit", "cpu")                               # ./kit/text_mot_match/model/finest.tar is not there


def test_refusals():
    from mdm_amd.evaluator import EvaluatorMDMWrapper
    w, weights = _wrapper()
    B, T, L = 3, 40, 8
    motions = torch.zeros(B, T, 263)
    word, pos = torch.zeros(B, L, 300), torch.zeros(B, L, 15)
    ok_m, ok_c = torch.tensor([40, 20, 8]), torch.tensor([8, 3, 1])
    with pytest.raises(RuntimeError, match="decreasing"):                # unsorted cap_lens: pack_padded_sequence refuses them
        w.get_co_embeddings(word, pos, torch.tensor([3, 8, 1]), motions, ok_m)
    with pytest.raises(RuntimeError, match="greater than 0"):            # a caption of no words
        w.get_co_embeddings(word, pos, torch.tensor([8, 3, 0]), motions, ok_m)
    with pytest.raises(RuntimeError, match="beyond"):                    # a caption longer than the padded input
        w.get_co_embeddings(word, pos, torch.tensor([9, 3, 1]), motions, ok_m)
    with pytest.raises(RuntimeError, match="greater than 0"):            # m_len // 4 == 0
        w.get_motion_embeddings(motions, torch.tensor([40, 20, 3]))
    with pytest.raises(RuntimeError, match="beyond"):                    # m_len // 4 beyond the conv output
        w.get_motion_embeddings(motions, torch.tensor([44, 20, 8]))
    with pytest.raises(ValueError, match="motions must be"):
        w.get_motion_embeddings(torch.zeros(B, T, 251), ok_m)
    with pytest.raises(ValueError, match="at least 4"):
        w.get_motion_embeddings(torch.zeros(B, 3, 263), torch.tensor([3, 3, 3]))
    with pytest.raises(ValueError, match="entries"):
        w.get_motion_embeddings(motions, torch.tensor([40, 20]))
    with pytest.raises(ValueError, match="word_embs must be"):
        w.get_co_embeddings(torch.zeros(B, L, 200), pos, ok_c, motions, ok_m)
    with pytest.raises(ValueError, match="pos_ohot must be"):
        w.get_co_embeddings(word, torch.zeros(B, L + 1, 15), ok_c, motions, ok_m)
    # widths the tiles cannot take: refused when the wrapper is created
    for bad in (dict(dim_motion_hidden=384), dict(dim_text_hidden=128), dict(dim_movement_latent=30), dict(dim_coemb_hidden=62),
                dict(dim_word=301), dict(unit_length=2)):
        with pytest.raises(ValueError):
            EvaluatorMDMWrapper.from_state_dicts(*weights, "humanml", "cpu", dims=dict(eh.REDUCED, **bad))
    with pytest.raises(ValueError, match="unknown entry"):
        EvaluatorMDMWrapper.from_state_dicts(*weights, "humanml", "cpu", dims=dict(eh.REDUCED, dim_nothing=1))
    with pytest.raises(Exception, match="no eager PyTorch forward"):
        w.motion_encoder(torch.zeros(1))


def test_argsort_ties_are_ordered_as_the_reference_orders_them(monkeypatch):
    """align_idx = np.argsort(m_lens.data.tolist())[::-1]: among equal lengths the LATER input row comes first.  The rows handed to the
    native path, and the permutation applied to the text side, are exactly that."""
    w, _ = _wrapper()
    m_lens = torch.tensor([20, 36, 20, 36, 8])
    want = np.argsort(m_lens.data.tolist())[::-1].copy()
    assert list(want) == [3, 1, 2, 0, 4]
    motions = torch.arange(5, dtype=torch.float32)[:, None, None].expand(5, 36, 263).contiguous()
    seen = {}

    def fake_motion_rows(mo, lens):
        seen["rows"], seen["lens"] = mo[:, 0, 0].tolist(), list(lens)
        return torch.zeros(5, 64)

    def fake_text_rows(word, pos, lens):
        return torch.arange(5, dtype=torch.float32)[:, None].expand(5, 64)

    monkeypatch.setattr(w, "_motion_rows", fake_motion_rows)
    monkeypatch.setattr(w, "_text_rows", fake_text_rows)
    te, me = w.get_co_embeddings(torch.zeros(5, 4, 300), torch.zeros(5, 4, 15), torch.tensor([4, 3, 2, 1, 1]), motions, m_lens)
    assert seen["rows"] == [3.0, 1.0, 2.0, 0.0, 4.0] and seen["lens"] == [36, 36, 20, 20, 8]
    assert te[:, 0].tolist() == [3.0, 1.0, 2.0, 0.0, 4.0]


def test_every_declared_eval_symbol_is_exported_and_validates_on_the_host():
    import __graft_entry__ as ge
    ge.build()
    from mdm_amd import _native
    lib = _native.MdmLib(_native.LIB_PATH)
    names = [n for n in _native.EXPORTED_SYMBOLS if n.startswith("mdm_eval_")]
    assert sorted(names) == ["mdm_eval_motion_embeddings", "mdm_eval_text_embeddings", "mdm_eval_workspace_bytes"]
    for n in names:
        assert hasattr(lib.lib, n)
    assert lib.mdm_abi_version() == 10
    # validation comes before anything touches the device: refusals work on a machine without one
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    gru = dict(in_w=p, in_b=p, w_ih=p, b_ih=p, w_hh=p, b_hh=p, h0=p, o1_w=p, o1_b=p, ln_g=p, ln_b=p, o2_w=p, o2_b=p)
    top = dict(conv1_w=p, conv1_b=p, conv2_w=p, conv2_b=p, out_w=p, out_b=p, pos_w=p, pos_b=p)

    def model(hm=1024, ht=512, **over):
        kw = dict(dim_pose=263, conv_hidden=512, latent=512, word=300, pos=15, unit_length=4)
        kw.update(over)
        return _native.MdmEvalModel(motion=_native.MdmEvalGru(in_dim=kw["latent"], hidden=hm, out=512, **gru),
                                    text=_native.MdmEvalGru(in_dim=kw["word"], hidden=ht, out=512, **gru), **top, **kw)

    m = model()
    n = lib.mdm_eval_workspace_bytes(C.byref(m), 32, 196, 22)
    assert n >= 4 * 32 * (98 * 512 + 49 * (2 * 512 + 7 * 1024)) + 4 * 5 * 32 * 1024
    assert lib.mdm_eval_workspace_bytes(C.byref(model(hm=384)), 32, 196, 22) == 0 and b"hidden must be" in lib.lib.mdm_last_error()
    assert lib.mdm_eval_workspace_bytes(C.byref(model(latent=30)), 32, 196, 22) == 0
    assert lib.mdm_eval_workspace_bytes(C.byref(m), 0, 196, 22) == 0
    assert lib.mdm_eval_workspace_bytes(None, 1, 196, 22) == 0 and b"null model" in lib.lib.mdm_last_error()
    assert lib.mdm_eval_motion_embeddings(C.byref(m), p, p, p, 2, 3, 0, p, n, None) < 0 and b"at least 4" in lib.lib.mdm_last_error()
    assert lib.mdm_eval_motion_embeddings(C.byref(m), p, None, p, 2, 40, 0, p, n, None) < 0 and b"null" in lib.lib.mdm_last_error()
    assert lib.mdm_eval_motion_embeddings(C.byref(m), p, p, p, 2, 40, 0, p, 16, None) < 0 and b"workspace too small" in lib.lib.mdm_last_error()
    assert lib.mdm_eval_text_embeddings(C.byref(m), p, p, p, p, 2, 0, 0, p, n, None) < 0
    assert lib.mdm_eval_text_embeddings(C.byref(m), p, p, p, p, 2, 22, 0, p, 16, None) < 0 and b"workspace too small" in lib.lib.mdm_last_error()
