"""mdm_amd/stgcn.py on the MI355X at full width: the four fixtures of tests/golden/stgcn_*.npz, the a2m net at shapes around the
9-tap window, the stride and the tile edges against the fp64 restatement, row invariance, NaN poison, and a call on a side stream.

Accuracy condition: max-abs error of features and of yhat against fp64 <= 4 x e_ref, e_ref = the reference's own fp32 error on that
case (tests/golden/PIN_REPORT_stgcn.json; the reference tree is not needed here).  Every test prints its figure before it asserts;
tools/bench_stgcn.py collects timings into profiles/r15a_stgcn.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import stgcn_helpers as sh
from helpers import memo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = [n for n, c in sh.CASES.items() if c["fixture"]]
SHAPES = ["a2m_trained_1x1", "a2m_trained_2x13", "a2m_trained_1x9", "a2m_trained_3x10", "a2m_trained_33x5"]


def _model(net, regime):
    weights = memo(("stgcn_w", net, regime), lambda: sh.build_weights(net, {"default": 101, "trained": 102}[regime], regime))
    return memo(("stgcn_gpu", net, regime), lambda: sh.loaded_model(net, weights, DEV)), weights


def _report(name, got, want):
    ef, ey = sh.errors(got, want)
    print(f"[stgcn] {name}: max-abs vs fp64 features = {ef:.3e} yhat = {ey:.3e}  e_ref = {sh.bound(name) / 4:.3e}  bound = {sh.bound(name):.3e}")
    return ef, ey


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_meets_the_accuracy_condition(name):
    c, g = sh.CASES[name], sh.load_fixture(name)
    model, _ = _model(c["net"], c["regime"])
    assert np.array_equal(g["x"], sh.case_input(name))           # the stored input is the seeded one
    got = sh.run_case(model, name, g["x"])
    ef, ey = _report(name, got, (g["fp64_features"], g["fp64_yhat"]))
    assert got[0].shape == g["fp64_features"].shape == (3, 256) and got[1].shape == g["fp64_yhat"].shape
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert ef <= sh.bound(name) and ey <= sh.bound(name)
    # the classes the reference's own fp32 run predicts
    assert np.array_equal(got[1].argmax(1), g["ref_yhat"].argmax(1))


@pytest.mark.parametrize("name", SHAPES)
def test_a2m_shapes_against_the_fp64_restatement(name):
    """(1, 1); (2, 13); (1, 9) and (3, 10) on both sides of the 9-tap window; (33, 5): 3,960 rows, no multiple of the tile height."""
    c = sh.CASES[name]
    model, weights = _model("a2m", "trained")
    x = sh.case_input(name)
    got = sh.run_case(model, name, x)
    ef, ey = _report(name, got, sh.forward_fp64("a2m", weights, x))
    assert got[0].shape == (c["N"], 256) and got[1].shape == (c["N"], 40)
    assert ef <= sh.bound(name) and ey <= sh.bound(name)


def test_row_invariance_is_bit_exact_across_batches_of_1_3_33():
    model, _ = _model("a2m", "trained")
    x = sh.make_input("a2m", 91, 33, 10)
    alone = sh.run_case(model, None, x[5:6])
    again = sh.run_case(model, None, x[5:6])
    three_first = sh.run_case(model, None, x[[5, 0, 1]])
    three_last = sh.run_case(model, None, x[[0, 1, 5]])
    big = sh.run_case(model, None, x)
    big_last = sh.run_case(model, None, x[[i for i in range(33) if i != 5] + [5]])
    for a, b, f, l, g, gl in zip(alone, again, three_first, three_last, big, big_last):
        assert np.array_equal(a, b)
        assert np.array_equal(a[0], f[0]) and np.array_equal(a[0], l[2])
        assert np.array_equal(a[0], g[5]) and np.array_equal(a[0], gl[32])


def test_poison_in_workspace_and_outputs_does_not_reach_the_results():
    """The native call over a 0xFF-filled (NaN) workspace and NaN-filled outputs: finite, and the bits of a call over zeros."""
    from mdm_amd import _native as nat
    model, _ = _model("a2m", "trained")
    lib, m = nat.load_native(), model._model()
    x = torch.from_numpy(sh.make_input("a2m", 92, 2, 13)).to(DEV)
    need = lib.mdm_stgcn_workspace_bytes(C.byref(m), 2, 13)
    assert need > 0
    out = []
    for ws_fill, out_fill in ((0, 0.0), (0xFF, float("nan"))):
        ws = torch.full((need,), ws_fill, dtype=torch.uint8, device=DEV)
        feat = torch.full((2, 256), out_fill, dtype=torch.float32, device=DEV)
        yhat = torch.full((2, 40), out_fill, dtype=torch.float32, device=DEV)
        lib.check(lib.mdm_stgcn_forward(C.byref(m), x.data_ptr(), feat.data_ptr(), yhat.data_ptr(), 2, 13, ws.data_ptr(), need,
                                        torch.cuda.current_stream(DEV).cuda_stream), "mdm_stgcn_forward")
        torch.cuda.synchronize()
        out.append((feat.cpu(), yhat.cpu()))
    assert bool(torch.isfinite(out[1][0]).all()) and bool(torch.isfinite(out[1][1]).all())
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_call_on_a_side_stream_behind_a_call_on_the_default_stream():
    """One chain per device (include/mdm_hip.h CONCURRENCY): a call on a side stream right behind one on the default stream is ordered
    behind it and returns the default stream's bits."""
    model, _ = _model("a2m", "trained")
    x = torch.from_numpy(sh.make_input("a2m", 93, 3, 10)).to(DEV)
    base = model({"output": x})
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = model({"output": x})
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(got["features"], base["features"]) and torch.equal(got["yhat"], base["yhat"])
