"""csrc/gru_recogniser.h (mdm_gru_cls_forward behind mdm_amd/gru_recogniser.py) on the CPU wave emulator of tests/emu, on reduced nets
(H = 32, I = 10, one and two layers, 12 and 13 classes) against the fp64 restatement; ragged lengths; `hidden_unit=None` under a
torch seed; row invariance bit for bit; NaN poison in the workspace and the outputs.

Bound: the accuracy condition of the GPU test -- max-abs error of features and of yhat against fp64 <= 4 x e_ref, e_ref the
reference's own fp32 error pooled per (net, regime, output) (tests/golden/PIN_REPORT_gru_recogniser.json: the reference ran the same
reduced nets)."""
import ctypes as C

import numpy as np
import pytest
import torch

from emu.emu_lib import emu
import gru_recogniser_helpers as gh
from helpers import memo

R = gh.ROWS


@pytest.fixture(scope="module")
def lib():
    return emu()


def _model(lib, net, regime, fid=False):
    weights = memo(("gru_w", net, regime), lambda: gh.build_weights(net, regime))
    return memo(("gru_emu", net, regime, fid), lambda: gh.loaded_model(net, weights, "cpu", lib, fid)), weights


def _check(tag, got, want, net, regime):
    ef, ey = gh.errors(got, want)
    bf, by = gh.bound(net, regime)
    print(f"[gru] {tag}: max-abs vs fp64 features = {ef:.3e} (bound {bf:.3e})  yhat = {ey:.3e} (bound {by:.3e})")
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[0].dtype == np.float32
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert ef <= bf and ey <= by


@pytest.mark.parametrize("name", gh.EMU_CASES)
def test_emulated_case_meets_the_accuracy_condition(lib, name):
    """(B, T): (1, 1), (1, 2); (2, 13) with a length-1 row beside a length-T row; (R, 5), (R + 1, 5) whose second tile's longest row
    ends in front of T, (2 R + 1, 3): one, two and three tiles, ragged lengths including 1 and T; one and two layers, 12 and 13 classes."""
    c = gh.CASES[name]
    model, weights = _model(lib, c["net"], c["regime"])
    x, lens, h0 = gh.case_input(name)
    if c["lens"] == "ragged":
        assert lens[0] == 1 and lens[-1] == c["T"]
    if c["lens"] == "short":
        assert lens[R:].max() < c["T"] and lens[:R].max() == c["T"]
    got = gh.run_model(model, x, lens, h0)
    _check(name, got, gh.forward_fp64(c["net"], weights, x, lens, h0), c["net"], c["regime"])


def test_both_classes_are_views_of_one_call(lib):
    """MotionDiscriminator returns yhat, MotionDiscriminatorForFID the tanh(linear1) that yhat was formed from."""
    cls, weights = _model(lib, "red2", "trained")
    fid, _ = _model(lib, "red2", "trained", fid=True)
    x, lens, h0 = gh.case_input("red2_trained_2x13")
    xt, lt, ht = torch.from_numpy(x), torch.from_numpy(lens), torch.from_numpy(h0)
    yhat, feat = cls(xt, lt, ht), fid(xt, lt, ht)
    assert yhat.shape == (2, 12) and feat.shape == (2, 30) and yhat.dtype == feat.dtype == torch.float32
    both = gh.run_model(cls, x, lens, h0)
    assert np.array_equal(both[0], feat.numpy()) and np.array_equal(both[1], yhat.numpy())
    # linear2 over the RETURNED features is yhat up to the rounding of one fp32 chain of 30 fused multiply-adds and the bias add:
    # at most 31 roundings of u = 2^-24 relative to the sum of the terms' magnitudes (no term of another row, no other features)
    w2, b2 = weights["linear2.weight"].double().numpy(), weights["linear2.bias"].double().numpy()
    again = feat.double().numpy() @ w2.T + b2
    slack = 31 * 2.0 ** -24 * (np.abs(feat.double().numpy()) @ np.abs(w2).T + np.abs(b2))
    assert (np.abs(again - yhat.double().numpy()) <= slack).all()
    # a double input is cast as upstream casts it (`.float()`)
    assert torch.equal(cls(xt.double(), lt, ht), yhat)
    # int32 lengths and int64 lengths agree
    assert torch.equal(cls(xt, lt.int(), ht), yhat)


def test_hidden_unit_none_draws_torch_randn_as_upstream(lib):
    """After torch.manual_seed(s) the call equals, bit for bit, the call given torch.randn(L, B, H) drawn after the same seed -- and
    reproduces the reference's outputs under that seed (tests/golden/gru_recogniser_seeded.npz) within the bound."""
    s, g = gh.SEEDED, gh.load_seeded()
    cls, weights = _model(lib, s["net"], s["regime"])
    fid, _ = _model(lib, s["net"], s["regime"], fid=True)
    f = gh.NETS[s["net"]]
    xt, lt = torch.from_numpy(g["x"]), torch.from_numpy(g["lens"])
    seed = int(g["torch_seed"])
    torch.manual_seed(seed)
    yhat = cls(xt, lt)
    after_call = torch.rand(1)
    torch.manual_seed(seed)
    feat = fid(xt, lt)
    torch.manual_seed(seed)
    h0 = torch.randn(f["L"], s["B"], f["H"])
    after_draw = torch.rand(1)
    assert torch.equal(after_call, after_draw)                       # the generator advanced by exactly that one draw
    assert torch.equal(cls(xt, lt, h0), yhat) and torch.equal(fid(xt, lt, h0), feat)
    bf, by = gh.bound(s["net"], s["regime"])
    ef, ey = gh.errors((feat.numpy(), yhat.numpy()), (g["fp64_features"], g["fp64_yhat"]))
    rf, ry = gh.errors((feat.numpy(), yhat.numpy()), (g["ref_features"].astype(np.float64), g["ref_yhat"].astype(np.float64)))
    print(f"[gru] seeded: vs fp64 features = {ef:.3e} yhat = {ey:.3e}; vs the reference's fp32 run features = {rf:.3e} yhat = {ry:.3e}; "
          f"bounds {bf:.3e} {by:.3e}")
    assert ef <= bf and ey <= by
    assert np.array_equal(yhat.numpy().argmax(1), g["ref_yhat"].argmax(1))


@pytest.mark.parametrize("net", ["red1", "red2"])
def test_a_samples_bits_do_not_depend_on_the_batch(lib, net):
    """A sample alone, twice, as the first and the last row of a batch of 3, in a batch that spans two tiles, and beside other lengths."""
    model, _ = _model(lib, net, "trained")
    B, T = R + 2, 6
    x, h0 = gh.make_input(net, 78, B, T)
    lens = gh.make_lens("ragged", B, T, 78)
    lens[3] = 4
    one = lambda idx, ln: gh.run_model(model, x[idx], np.asarray(ln), h0[:, idx])      # noqa: E731
    alone, again = one([3], [4]), one([3], [4])
    first, last = one([3, 0, 1], [4, 6, 1]), one([0, 1, 3], [1, 6, 4])
    other_lens = one([0, 3, 1], [6, 4, 2])
    big = gh.run_model(model, x, lens, h0)
    order = [i for i in range(B) if i != 3] + [3]
    big_last = gh.run_model(model, x[order], lens[order], h0[:, order])               # row 3 as the only row of the second tile
    for a, b, f, l, o, g, gl in zip(alone, again, first, last, other_lens, big, big_last):
        assert np.array_equal(a, b)
        assert np.array_equal(a[0], f[0]) and np.array_equal(a[0], l[2]) and np.array_equal(a[0], o[1])
        assert np.array_equal(a[0], g[3]) and np.array_equal(a[0], gl[B - 1])


def test_chunks_of_a_large_batch_return_the_same_bits(lib, monkeypatch):
    from mdm_amd import gru_recogniser as gr
    model, _ = _model(lib, "red2", "trained")
    x, h0 = gh.make_input("red2", 79, 5, 4)
    lens = np.asarray([4, 1, 3, 2, 4])
    whole = gh.run_model(model, x, lens, h0)
    monkeypatch.setattr(gr, "ROW_CHUNK", 2)
    cut = gh.run_model(model, x, lens, h0)
    assert np.array_equal(whole[0], cut[0]) and np.array_equal(whole[1], cut[1])


def _native_call(lib, model, x, lens, h0, ws_fill=0, out_fill=0.0):
    m = model._model()
    B, T = x.shape[0], x.shape[3]
    need = lib.mdm_gru_cls_workspace_bytes(C.byref(m), B, T)
    assert need > 0
    ws = np.full(need, ws_fill, dtype=np.uint8)
    feat = np.full((B, m.mid), out_fill, dtype=np.float32)
    yhat = np.full((B, m.num_class), out_fill, dtype=np.float32)
    x, h0, lens = np.ascontiguousarray(x), np.ascontiguousarray(h0), np.ascontiguousarray(lens, dtype=np.int32)
    rc = lib.mdm_gru_cls_forward(C.byref(m), x.ctypes.data, lens.ctypes.data, h0.ctypes.data, feat.ctypes.data, yhat.ctypes.data, B, T,
                                 ws.ctypes.data, need, None)
    return rc, feat, yhat


@pytest.mark.parametrize("net", ["red1", "red2"])
def test_poison_in_workspace_and_outputs_does_not_reach_the_results(lib, net):
    """A NaN-filled (0xFF bytes) workspace and NaN-filled outputs: finite results, the bits of a run over zeros -- frames behind a
    row's length and the pad rows of the last tile are never read."""
    model, _ = _model(lib, net, "trained")
    x, h0 = gh.make_input(net, 80, R + 1, 5)
    lens = gh.make_lens("short", R + 1, 5, 80)
    rc0, f0, y0 = _native_call(lib, model, x, lens, h0)
    rc1, f1, y1 = _native_call(lib, model, x, lens, h0, ws_fill=0xFF, out_fill=np.nan)
    assert rc0 == 0 and rc1 == 0
    assert np.isfinite(f1).all() and np.isfinite(y1).all()
    assert np.array_equal(f0, f1) and np.array_equal(y0, y1)


def test_device_side_lengths_are_clamped_into_the_frames(lib):
    """The native call clamps lens to [1, T] (include/mdm_hip.h): 0 and -5 run one frame, T + 9 runs T frames."""
    model, _ = _model(lib, "red2", "trained")
    x, h0 = gh.make_input("red2", 81, 3, 4)
    rc, f, y = _native_call(lib, model, x, np.asarray([0, -5, 13]), h0)
    rc2, f2, y2 = _native_call(lib, model, x, np.asarray([1, 1, 4]), h0)
    assert rc == 0 and rc2 == 0 and np.array_equal(f, f2) and np.array_equal(y, y2)
