"""csrc/stgcn.h (mdm_stgcn_forward behind mdm_amd/stgcn.py) on the CPU wave emulator of tests/emu, on reduced nets: an a2m-like net
(V = 24, blocks 6->8 without residual, 8 identity, 8->16 stride 2 and 16->32 stride 1 with a convolutional residual, 32 identity)
and an unconstrained-like one (V = 15, 3 input channels) against the fp64 restatement; row invariance bit for bit; NaN poison in
the workspace and the outputs; the native refusals.

Bound: the accuracy condition of the GPU test -- max-abs error of features and of yhat against fp64 <= 4 x e_ref, e_ref being the
reference's own fp32 error on that very case (tests/golden/PIN_REPORT_stgcn.json: the reference ran the same reduced net)."""
import ctypes as C

import numpy as np
import pytest
import torch

from emu.emu_lib import emu
import stgcn_helpers as sh
from helpers import memo
from mdm_amd import _native as nat

EMU_CASES = [n for n in sh.CASES if n.startswith("red_")]


@pytest.fixture(scope="module")
def lib():
    return emu()


def _model(lib, net, regime):
    weights = memo(("stgcn_w", net, regime), lambda: sh.build_weights(net, {"default": 101, "trained": 102}[regime], regime))
    return memo(("stgcn_emu", net, regime), lambda: sh.loaded_model(net, weights, "cpu", lib)), weights


@pytest.mark.parametrize("name", EMU_CASES)
def test_emulated_case_meets_the_accuracy_condition(lib, name):
    """(N, T): (2, 13); (1, 1); (1, 8), (1, 9), (3, 10) on both sides of the 9-tap window, odd and even lengths under stride 2;
    (1, 5) and (1, 6) at V = 24: 120 and 144 rows, either side of two 64-row tiles."""
    c = sh.CASES[name]
    model, weights = _model(lib, c["net"], c["regime"])
    got = sh.run_case(model, name)
    want = sh.forward_fp64(c["net"], weights, sh.case_input(name))
    ef, ey = sh.errors(got, want)
    print(f"[stgcn] {name}: max-abs vs fp64 features = {ef:.3e} yhat = {ey:.3e}  e_ref = {sh.bound(name) / 4:.3e}  bound = {sh.bound(name):.3e}")
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[0].dtype == np.float32
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert ef <= sh.bound(name) and ey <= sh.bound(name)


def test_features_keep_the_references_squeeze(lib):
    model, _ = _model(lib, "red_a2m", "trained")
    one = model({"output": torch.from_numpy(sh.case_input("red_a2m_trained_1x9"))})
    two = model({"output": torch.from_numpy(sh.case_input("red_a2m_trained_2x13"))})
    assert one["features"].shape == (32,) and one["yhat"].shape == (1, 5)
    assert two["features"].shape == (2, 32) and two["yhat"].shape == (2, 5)


@pytest.mark.parametrize("net", ["red_a2m", "red_unc"])
def test_a_samples_bits_do_not_depend_on_the_batch(lib, net):
    """A sample alone, as row 0 and as the last row of a batch of 3, and the same call twice."""
    model, _ = _model(lib, net, "trained")
    x = sh.make_input(net, 77, 3, 10)
    alone = sh.run_case(model, None, x[1:2])
    again = sh.run_case(model, None, x[1:2])
    first = sh.run_case(model, None, x[[1, 0, 2]])
    last = sh.run_case(model, None, x[[0, 2, 1]])
    for a, b, f, l in zip(alone, again, first, last):
        assert np.array_equal(a, b)
        assert np.array_equal(a[0], f[0])
        assert np.array_equal(a[0], l[2])


def _native_call(lib, model, x, ws_fill=None, out_fill=None, ws_bytes=None):
    """mdm_stgcn_forward over numpy buffers; returns (rc, features, yhat)."""
    m = model._model()
    N, T = x.shape[0], x.shape[3]
    need = lib.mdm_stgcn_workspace_bytes(C.byref(m), N, T)
    assert need > 0
    ws = np.zeros(need, dtype=np.uint8)
    if ws_fill is not None:
        ws[:] = ws_fill
    feat = np.zeros((N, model.fcn.weight.shape[1]), dtype=np.float32)
    yhat = np.zeros((N, model.num_class), dtype=np.float32)
    if out_fill is not None:
        feat[:], yhat[:] = out_fill, out_fill
    x = np.ascontiguousarray(x)
    rc = lib.mdm_stgcn_forward(C.byref(m), x.ctypes.data, feat.ctypes.data, yhat.ctypes.data, N, T, ws.ctypes.data,
                               need if ws_bytes is None else ws_bytes, None)
    return rc, feat, yhat


@pytest.mark.parametrize("net", ["red_a2m", "red_unc"])
def test_poison_in_workspace_and_outputs_does_not_reach_the_results(lib, net):
    """A NaN-filled (0xFF bytes) workspace and NaN-filled outputs: finite results, bit-identical to a clean call."""
    model, _ = _model(lib, net, "trained")
    x = sh.make_input(net, 78, 2, 13)
    rc0, f0, y0 = _native_call(lib, model, x)
    rc1, f1, y1 = _native_call(lib, model, x, ws_fill=0xFF, out_fill=np.nan)
    assert rc0 == 0 and rc1 == 0
    assert np.isfinite(f1).all() and np.isfinite(y1).all()
    assert np.array_equal(f0, f1) and np.array_equal(y0, y1)


def test_short_workspace_and_bad_shapes_are_refused(lib):
    model, _ = _model(lib, "red_a2m", "trained")
    x = sh.make_input("red_a2m", 79, 1, 5)
    m = model._model()
    need = lib.mdm_stgcn_workspace_bytes(C.byref(m), 1, 5)
    assert need == 3 * 72 * 32 * 4 + 64                  # the widest buffer: 3 frames x 24 nodes behind the stride, 32 channels
    rc, _, _ = _native_call(lib, model, x, ws_bytes=need - 1)
    assert rc == -3 and b"workspace" in lib.lib.mdm_last_error()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    for N, T, word in ((0, 5, b"N must"), (1, 0, b"T must"), (1, 1 << 17, b"T must"), (1 << 20, 1 << 12, b"chunk")):
        assert lib.mdm_stgcn_workspace_bytes(C.byref(m), N, T) == 0
        assert word in lib.lib.mdm_last_error(), (N, T, lib.lib.mdm_last_error())
        assert lib.mdm_stgcn_forward(C.byref(m), p, p, p, N, T, p, 256, None) < 0
    assert lib.mdm_stgcn_workspace_bytes(None, 1, 5) == 0 and b"null model" in lib.lib.mdm_last_error()
    assert lib.mdm_stgcn_forward(C.byref(m), None, p, p, 1, 5, p, need, None) == -1 and b"null" in lib.lib.mdm_last_error()

    def broken(**over):
        """A copy of the model struct with one field of block 2 (or of the model) replaced."""
        blocks = (nat.MdmStgcnBlock * m.n_blocks)(*[m.blocks[i] for i in range(m.n_blocks)])
        mm = nat.MdmStgcnModel(blocks=blocks, in_scale=m.in_scale, in_shift=m.in_shift, fcn_w=m.fcn_w, fcn_b=m.fcn_b,
                               n_blocks=m.n_blocks, V=m.V, K=m.K, num_class=m.num_class)
        for k, v in over.items():
            if hasattr(mm, k):
                setattr(mm, k, v)
            else:
                setattr(blocks[2], k, v)
        return mm, blocks

    for over, word in ((dict(c_in=12), b"c_in must equal"), (dict(c_out=18), b"multiple of 4"), (dict(stride=0), b"stride"),
                       (dict(residual=1), b"identity residual"), (dict(residual=7), b"MDM_STGCN_RES"), (dict(tcn_w=None), b"tcn_w"),
                       (dict(res_w=m.blocks[2].res_w + 4), b"16-byte aligned"), (dict(n_blocks=17), b"n_blocks"), (dict(V=0), b"V must"),
                       (dict(K=9), b"K must"), (dict(num_class=0), b"num_class"), (dict(fcn_w=None), b"fcn_w")):
        mm, keep = broken(**over)
        assert lib.mdm_stgcn_workspace_bytes(C.byref(mm), 1, 5) == 0, over
        assert word in lib.lib.mdm_last_error(), (over, lib.lib.mdm_last_error())


def test_a_malformed_neighbour_table_does_not_leave_its_bounds(lib):
    """Counts beyond the lists' 8 entries and node indices outside [0, V) are clamped (include/mdm_hip.h): the call completes with
    finite results -- every read stays inside the lists and the sample's own V rows."""
    model, _ = _model(lib, "red_a2m", "trained")
    m = model._model()
    blocks = (nat.MdmStgcnBlock * m.n_blocks)(*[m.blocks[i] for i in range(m.n_blocks)])
    K, V = m.K, m.V
    idx = np.where(np.arange(K * V * nat.STGCN_MAX_NEIGHBOURS) % 2 == 0, 10 ** 6, -10 ** 6).astype(np.int32)
    cnt = np.full(K * V, 100, dtype=np.int32)
    blocks[1].nbr_idx, blocks[1].nbr_cnt = idx.ctypes.data, cnt.ctypes.data
    mm = nat.MdmStgcnModel(blocks=blocks, in_scale=m.in_scale, in_shift=m.in_shift, fcn_w=m.fcn_w, fcn_b=m.fcn_b,
                           n_blocks=m.n_blocks, V=V, K=K, num_class=m.num_class)
    x = sh.make_input("red_a2m", 80, 1, 6)
    need = lib.mdm_stgcn_workspace_bytes(C.byref(mm), 1, 6)
    ws = np.zeros(need, dtype=np.uint8)
    feat, yhat = np.zeros((1, 32), np.float32), np.zeros((1, 5), np.float32)
    rc = lib.mdm_stgcn_forward(C.byref(mm), x.ctypes.data, feat.ctypes.data, yhat.ctypes.data, 1, 6, ws.ctypes.data, need, None)
    assert rc == 0 and np.isfinite(feat).all() and np.isfinite(yhat).all()
