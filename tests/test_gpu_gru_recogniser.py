"""mdm_amd/gru_recogniser.py on the MI355X at full width (H = 128, two layers): the two fixtures of tests/golden/gru_recogniser_*.npz,
shapes around the 16-row tile against the fp64 restatement, the NTU-13 input (I = 54, 13 classes), row invariance across batches and
across a chunk boundary, NaN poison, and a call on a side stream.

Accuracy condition: max-abs error of features and of yhat against fp64 <= 4 x e_ref, e_ref the reference's own fp32 error pooled per
(net, regime, output) (tests/golden/PIN_REPORT_gru_recogniser.json; the reference tree is not needed here).  Every test prints its
figure before it asserts; tools/bench_gru_recogniser.py collects timings into profiles/r17a_gru_recogniser.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import gru_recogniser_helpers as gh
from helpers import memo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = gh.ROWS
FIXTURES = [n for n, c in gh.CASES.items() if c["fixture"]]
SHAPES = [n for n, c in gh.CASES.items() if c["net"] == "full" and not c["fixture"]]
NTU = [n for n, c in gh.CASES.items() if c["net"] == "ntu"]


def _model(net, regime, fid=False):
    weights = memo(("gru_w", net, regime), lambda: gh.build_weights(net, regime))
    return memo(("gru_gpu", net, regime, fid), lambda: gh.loaded_model(net, weights, DEV, fid=fid)), weights


def _check(tag, got, want, net, regime):
    ef, ey = gh.errors(got, want)
    bf, by = gh.bound(net, regime)
    print(f"[gru] {tag}: max-abs vs fp64 features = {ef:.3e} (bound {bf:.3e})  yhat = {ey:.3e} (bound {by:.3e})")
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[0].dtype == np.float32
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert ef <= bf and ey <= by


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_meets_the_accuracy_condition(name):
    c, g = gh.CASES[name], gh.load_fixture(name)
    x, lens, h0 = gh.case_input(name)
    assert np.array_equal(g["x"], x) and np.array_equal(g["lens"], lens) and np.array_equal(g["h0"], h0)      # the stored inputs are the seeded ones
    assert list(g["lens"]) == [60, 37, 1] and g["x"].shape == (3, 24, 3, 60)
    model, _ = _model(c["net"], c["regime"])
    got = gh.run_model(model, g["x"], g["lens"], g["h0"])
    _check(name, got, (g["fp64_features"], g["fp64_yhat"]), c["net"], c["regime"])
    # the classes the reference's own fp32 run predicts
    assert np.array_equal(got[1].argmax(1), g["ref_yhat"].argmax(1))
    # the two classes return the two outputs; device-side lengths (no host synchronisation) give the same bits
    fid, _ = _model(c["net"], c["regime"], fid=True)
    xt, ht = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["h0"]).to(DEV)
    lt = torch.from_numpy(g["lens"]).to(DEV)
    assert np.array_equal(model(xt, lt, ht).cpu().numpy(), got[1]) and np.array_equal(fid(xt, lt, ht).cpu().numpy(), got[0])


@pytest.mark.parametrize("name", SHAPES)
def test_shapes_against_the_fp64_restatement(name):
    """(1, 1); (1, 60); (R + 1, 7): a second tile of one row; (2 R + 1, 13) and (33, 5) ragged: three tiles, lengths 1 .. T."""
    c = gh.CASES[name]
    model, weights = _model("full", c["regime"])
    x, lens, h0 = gh.case_input(name)
    got = gh.run_model(model, x, lens, h0)
    assert got[0].shape == (c["B"], 30) and got[1].shape == (c["B"], 12)
    _check(name, got, gh.forward_fp64("full", weights, x, lens, h0), "full", c["regime"])


@pytest.mark.parametrize("name", NTU)
def test_ntu13_input_of_54_features_and_13_classes(name):
    """I = 54 is no multiple of 4: the frame loader zero-fills the k tile, W_ih's rows are read unaligned."""
    c = gh.CASES[name]
    model, weights = _model("ntu", c["regime"])
    x, lens, h0 = gh.case_input(name)
    got = gh.run_model(model, x, lens, h0)
    assert got[1].shape == (c["B"], 13)
    _check(name, got, gh.forward_fp64("ntu", weights, x, lens, h0), "ntu", c["regime"])


def test_row_invariance_is_bit_exact_across_batches_of_1_3_33_and_a_chunk_boundary(monkeypatch):
    from mdm_amd import gru_recogniser as gr
    model, _ = _model("full", "trained")
    B, T = 33, 9
    x, h0 = gh.make_input("full", 94, B, T)
    lens = gh.make_lens("ragged", B, T, 94)
    lens[5] = 6
    one = lambda idx, ln: gh.run_model(model, x[idx], np.asarray(ln), h0[:, idx])      # noqa: E731
    alone, again = one([5], [6]), one([5], [6])
    first, last = one([5, 0, 1], [6, 9, 1]), one([0, 1, 5], [1, 9, 6])
    big = gh.run_model(model, x, lens, h0)
    order = [i for i in range(B) if i != 5] + [5]
    big_last = gh.run_model(model, x[order], lens[order], h0[:, order])               # row 5 alone in the third tile
    monkeypatch.setattr(gr, "ROW_CHUNK", 20)                                          # chunks of 20 + 13: row 5 in the first, row 32 in the second
    cut = gh.run_model(model, x, lens, h0)
    for a, b, f, l, g, gl, c in zip(alone, again, first, last, big, big_last, cut):
        assert np.array_equal(a, b)
        assert np.array_equal(a[0], f[0]) and np.array_equal(a[0], l[2])
        assert np.array_equal(a[0], g[5]) and np.array_equal(a[0], gl[32])
        assert np.array_equal(g, c)


def test_poison_in_workspace_and_outputs_does_not_reach_the_results():
    """The native call over a 0xFF-filled (NaN) workspace and NaN-filled outputs: finite, and the bits of a call over zeros."""
    from mdm_amd import _native as nat
    model, _ = _model("full", "trained")
    lib, m = nat.load_native(), model._model()
    B, T = R + 1, 7
    xn, h0n = gh.make_input("full", 95, B, T)
    x, h0 = torch.from_numpy(xn).to(DEV), torch.from_numpy(h0n).to(DEV)
    lens = torch.from_numpy(gh.make_lens("short", B, T, 95).astype(np.int32)).to(DEV)
    need = lib.mdm_gru_cls_workspace_bytes(C.byref(m), B, T)
    assert need > 0
    out = []
    for ws_fill, out_fill in ((0, 0.0), (0xFF, float("nan"))):
        ws = torch.full((need,), ws_fill, dtype=torch.uint8, device=DEV)
        feat = torch.full((B, 30), out_fill, dtype=torch.float32, device=DEV)
        yhat = torch.full((B, 12), out_fill, dtype=torch.float32, device=DEV)
        lib.check(lib.mdm_gru_cls_forward(C.byref(m), x.data_ptr(), lens.data_ptr(), h0.data_ptr(), feat.data_ptr(), yhat.data_ptr(), B, T,
                                          ws.data_ptr(), need, torch.cuda.current_stream(DEV).cuda_stream), "mdm_gru_cls_forward")
        torch.cuda.synchronize()
        out.append((feat.cpu(), yhat.cpu()))
    print(f"[gru] poison: max |features| = {out[1][0].abs().max().item():.3f}  max |yhat| = {out[1][1].abs().max().item():.3f}")
    assert bool(torch.isfinite(out[1][0]).all()) and bool(torch.isfinite(out[1][1]).all())
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_call_on_a_side_stream_behind_a_call_on_the_default_stream():
    """One chain per device (include/mdm_hip.h CONCURRENCY): a call on a side stream right behind one on the default stream is ordered
    behind it and returns the default stream's bits."""
    model, _ = _model("full", "trained")
    xn, h0n = gh.make_input("full", 96, 3, 10)
    x, h0 = torch.from_numpy(xn).to(DEV), torch.from_numpy(h0n).to(DEV)
    lens = torch.tensor([10, 4, 1], device=DEV)
    base = model(x, lens, h0)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = model(x, lens, h0)
    side.synchronize()
    torch.cuda.synchronize()
    print(f"[gru] side stream: max |yhat| = {base.abs().max().item():.3f}, equal = {torch.equal(got, base)}")
    assert torch.equal(got, base)


def test_hidden_unit_none_draws_on_the_models_device():
    """`hidden_unit=None`: torch.randn(L, B, H, device=self.device), the reference's own call -- the same bits as passing that draw."""
    model, _ = _model("full", "trained")
    xn, _ = gh.make_input("full", 97, 2, 5)
    x, lens = torch.from_numpy(xn).to(DEV), torch.tensor([5, 2])
    torch.manual_seed(7)
    got = model(x, lens)
    torch.manual_seed(7)
    h0 = torch.randn(2, 2, 128, device=DEV)
    want = model(x, lens, h0)
    print(f"[gru] hidden_unit=None: max |yhat| = {got.abs().max().item():.3f}")
    assert torch.equal(got, want)
