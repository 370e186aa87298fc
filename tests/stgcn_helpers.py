"""Checker of mdm_amd/stgcn.py: seeded weight builders, an fp64 numpy restatement of the ST-GCN forward pass written from its
definition, the case table, and the loaders of tests/golden/stgcn_*.npz and PIN_REPORT_stgcn.json (written by
tests/make_golden_stgcn.py from the reference's own modules).  Full weights are never stored (the a2m net has 3.1 M parameters):
weights and inputs are rebuilt from their seeds (numpy's legacy RandomState streams are frozen).

Restated (eval mode, one person, no mask):
  x [N, V, C, T] -> data_bn over the V C channels -> [N, C, T, V]
  per block: y = conv1x1(x) [N, K C_out, T, V];  g[n,c,t,w] = sum_k sum_v y[n,k,c,t,v] (A * importance)[k,v,w];  g = relu(BN(g));
             z = BN(conv9x1(g, stride s, zero padding 4));  x = relu(z + residual(x)),  residual = 0 | x | BN(conv1x1 stride s)
  features = mean over (T', V);  yhat = fcn(features)
"""
import json
import os
import pickle
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PIN_REPORT = os.path.join(GOLDEN, "PIN_REPORT_stgcn.json")
KEYS_FILE = os.path.join(GOLDEN, "stgcn_state_dict_keys.json")
GRAPH_FILE = os.path.join(GOLDEN, "stgcn_graph_A.npz")

# SMPL's kinematic tree (parent of joint i; public with the model): what kintree_table.pkl holds
SMPL_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]

# (c_in, c_out, stride, residual): the reduced nets of the emulator tests -- no residual, identity, strided convolutional residual,
# unstrided convolutional residual (c_in != c_out), identity
REDUCED_BLOCKS = ((None, 8, 1, False), (8, 8, 1, True), (8, 16, 2, True), (16, 32, 1, True), (32, 32, 1, True))

# net -> constructor facts.  `full` nets take the class's own block list.
NETS = {
    "a2m": dict(cls="STGCN", in_channels=6, num_class=40, layout="smpl", blocks=None),
    "unc": dict(cls="STGCNUnconstrained", in_channels=3, num_class=12, layout="openpose", blocks=None),
    "red_a2m": dict(cls="STGCN", in_channels=6, num_class=5, layout="smpl", blocks=REDUCED_BLOCKS),
    "red_unc": dict(cls="STGCNUnconstrained", in_channels=3, num_class=5, layout="openpose", blocks=REDUCED_BLOCKS),
}


def _case(net, regime, N, T, seed, fixture=False):
    return dict(net=net, regime=regime, N=N, T=T, seed=seed, wseed={"default": 101, "trained": 102}[regime], fixture=fixture)


CASES = {
    # full width, outputs stored (tests/golden/stgcn_{a2m,unc}_{default,trained}.npz)
    "a2m_default": _case("a2m", "default", 3, 60, 201, True),
    "a2m_trained": _case("a2m", "trained", 3, 60, 202, True),
    "unc_default": _case("unc", "default", 3, 60, 203, True),
    "unc_trained": _case("unc", "trained", 3, 60, 204, True),
    # full width a2m, trained regime: the report holds e_ref, the tests restate in fp64
    "a2m_trained_1x1": _case("a2m", "trained", 1, 1, 211),
    "a2m_trained_2x13": _case("a2m", "trained", 2, 13, 212),
    "a2m_trained_1x9": _case("a2m", "trained", 1, 9, 213),
    "a2m_trained_3x10": _case("a2m", "trained", 3, 10, 214),
    "a2m_trained_33x5": _case("a2m", "trained", 33, 5, 215),
}
EMU_SHAPES = [(2, 13), (1, 1), (1, 8), (1, 9), (3, 10), (1, 5), (1, 6)]
for _i, (_n, _t) in enumerate(EMU_SHAPES):
    CASES[f"red_a2m_trained_{_n}x{_t}"] = _case("red_a2m", "trained", _n, _t, 300 + _i)
CASES["red_a2m_default_2x13"] = _case("red_a2m", "default", 2, 13, 320)
CASES["red_unc_trained_2x13"] = _case("red_unc", "trained", 2, 13, 321)
CASES["red_unc_trained_1x9"] = _case("red_unc", "trained", 1, 9, 322)
CASES["red_unc_default_2x13"] = _case("red_unc", "default", 2, 13, 323)


# ---- the synthetic kintree file ------------------------------------------------------------------------------------------------------
_KINTREE = None


def kintree_path():
    """A kintree_table.pkl with SMPL's tree, in a temp dir of this process: row 0 the parents (the root's 2^32 - 1), row 1 the ids."""
    global _KINTREE
    if _KINTREE is None:
        d = tempfile.mkdtemp(prefix="stgcn_kintree_")
        kt = np.array([[p if p >= 0 else 2 ** 32 - 1 for p in SMPL_PARENTS], list(range(24))], dtype=np.uint32)
        _KINTREE = os.path.join(d, "kintree_table.pkl")
        with open(_KINTREE, "wb") as fh:
            pickle.dump(kt, fh)
    return _KINTREE


def graph_args(layout, strategy="spatial"):
    return {"layout": layout, "strategy": strategy, "kintree_path": kintree_path()}


# ---- models and weights -----------------------------------------------------------------------------------------------------------------
def make_model(net, device="cpu", native_lib=None):
    from mdm_amd import stgcn as sg
    f = NETS[net]
    kw = {}
    if f["blocks"] is not None:
        kw["_blocks"] = f["blocks"]
    if native_lib is not None:
        kw["_native_lib"] = native_lib
    return getattr(sg, f["cls"])(in_channels=f["in_channels"], num_class=f["num_class"], graph_args=graph_args(f["layout"]),
                                 edge_importance_weighting=True, device=device, **kw)


def state_shapes(net):
    """[(key, shape)] of the net's state dict, in its order."""
    return [(k, tuple(v.shape)) for k, v in make_model(net).state_dict().items()]


def build_weights(net, seed, regime):
    """A state dict of fp32 tensors.  "default": the values the modules start from (Conv2d: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for
    weight and bias; BatchNorm 1 / 0 with running statistics 0 / 1; edge importance 1).  "trained": the same convolutions 1.4x
    larger, random BatchNorm running statistics and affine terms, and edge importances in [0.5, 1.5] -- nothing a zero or a one
    would hide.  `A` is the graph's own."""
    assert regime in ("default", "trained")
    rs = np.random.RandomState(seed)
    model = make_model(net)
    sd = {}
    for key, t in model.state_dict().items():
        shape = tuple(t.shape)
        leaf = key.rsplit(".", 1)[-1]
        if key == "A":
            sd[key] = t.clone()
            continue
        if leaf == "num_batches_tracked":
            sd[key] = torch.zeros(shape, dtype=torch.long)
            continue
        if key.startswith("edge_importance."):
            a = rs.uniform(0.5, 1.5, shape) if regime == "trained" else np.ones(shape)
        elif len(shape) == 4:                                     # a convolution's weight
            k = 1.0 / np.sqrt(shape[1] * shape[2] * shape[3])
            a = rs.uniform(-k, k, shape) * (1.4 if regime == "trained" else 1.0)
            fan = k
        elif leaf == "bias" and (".conv." in key or ".tcn.2." in key or ".residual.0." in key or key == "fcn.bias"):
            a = rs.uniform(-fan, fan, shape)                      # (follows its weight in the state dict)
        elif leaf == "weight":                                    # BatchNorm gamma
            a = rs.uniform(0.5, 1.5, shape) if regime == "trained" else np.ones(shape)
        elif leaf == "bias":
            a = rs.normal(0.0, 0.2, shape) if regime == "trained" else np.zeros(shape)
        elif leaf == "running_mean":
            a = rs.normal(0.0, 0.3, shape) if regime == "trained" else np.zeros(shape)
        elif leaf == "running_var":
            a = rs.uniform(0.5, 1.5, shape) if regime == "trained" else np.ones(shape)
        else:
            raise KeyError(key)
        sd[key] = torch.from_numpy(np.asarray(a, dtype=np.float32))
    return sd


def make_input(net, seed, N, T):
    f = NETS[net]
    V = 24 if f["layout"] == "smpl" else 15
    return (np.random.RandomState(seed).standard_normal((N, V, f["in_channels"], T)) * 0.8).astype(np.float32)


def case_weights(name):
    c = CASES[name]
    return build_weights(c["net"], c["wseed"], c["regime"])


def case_input(name, draw=0):
    c = CASES[name]
    return make_input(c["net"], c["seed"] + 1000 * draw, c["N"], c["T"])


def loaded_model(net, weights, device="cpu", native_lib=None):
    m = make_model(net, device, native_lib)
    m.load_state_dict(weights)
    return m.to(device).eval()


# ---- fp64 restatement ------------------------------------------------------------------------------------------------------------------
def _bn64(x, sd, prefix, axis):
    shape = [1] * x.ndim
    shape[axis] = -1
    g, b, m, v = (sd[prefix + k].double().numpy().reshape(shape) for k in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / np.sqrt(v + 1e-5) * g + b


def net_blocks(net):
    from mdm_amd import stgcn as sg
    f = NETS[net]
    return f["blocks"] if f["blocks"] is not None else getattr(sg, f["cls"]).BLOCKS


def forward_fp64(net, sd, x):
    """(features [N, C_last], yhat [N, num_class]) in fp64, from the definition in this file's header."""
    x = np.asarray(x, dtype=np.float64)
    N, V, C, T = x.shape
    A32 = sd["A"].float()
    h = _bn64(x.reshape(N, V * C, T), sd, "data_bn.", 1).reshape(N, V, C, T).transpose(0, 2, 3, 1)       # [N, C, T, V]
    for b, (_, co, s, residual) in enumerate(net_blocks(net)):
        p = f"st_gcn_networks.{b}."
        ci = h.shape[1]
        A_b = (A32.double() * sd[f"edge_importance.{b}"].double()).numpy()
        K = A_b.shape[0]
        w = sd[p + "gcn.conv.weight"].double().numpy()[:, :, 0, 0]
        y = np.einsum("oc,nctv->notv", w, h) + sd[p + "gcn.conv.bias"].double().numpy()[None, :, None, None]
        g = np.einsum("nkctv,kvw->nctw", y.reshape(N, K, co, h.shape[2], V), A_b)
        g = np.maximum(_bn64(g, sd, p + "tcn.0.", 1), 0.0)
        Tin = g.shape[2]
        Tout = (Tin - 1) // s + 1
        gp = np.zeros((N, co, Tin + 8, V))
        gp[:, :, 4:4 + Tin] = g
        tw = sd[p + "tcn.2.weight"].double().numpy()[:, :, :, 0]
        z = np.zeros((N, co, Tout, V))
        for tap in range(9):
            z += np.einsum("oc,nctv->notv", tw[:, :, tap], gp[:, :, tap:tap + (Tout - 1) * s + 1:s])
        z = _bn64(z + sd[p + "tcn.2.bias"].double().numpy()[None, :, None, None], sd, p + "tcn.3.", 1)
        if not residual:
            r = 0.0
        elif ci == co and s == 1:
            r = h
        else:
            rw = sd[p + "residual.0.weight"].double().numpy()[:, :, 0, 0]
            r = np.einsum("oc,nctv->notv", rw, h[:, :, ::s]) + sd[p + "residual.0.bias"].double().numpy()[None, :, None, None]
            r = _bn64(r, sd, p + "residual.1.", 1)
        h = np.maximum(z + r, 0.0)
    feat = h.mean(axis=(2, 3))
    fw = sd["fcn.weight"].double().numpy()[:, :, 0, 0]
    return feat, feat @ fw.T + sd["fcn.bias"].double().numpy()[None, :]


# ---- fixtures and the report -------------------------------------------------------------------------------------------------------------
_REPORT = None


def pin_report():
    global _REPORT
    if _REPORT is None:
        with open(PIN_REPORT) as fh:
            _REPORT = json.load(fh)
    return _REPORT


def bound(name):
    """The accuracy condition: 4 x the reference's own fp32 error against fp64 on that case."""
    return 4 * pin_report()[name]["e_ref"]


def load_fixture(name):
    assert CASES[name]["fixture"]
    with np.load(os.path.join(GOLDEN, f"stgcn_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def run_case(model, name, x=None):
    """(features [N, C], yhat) as fp32 numpy from a model's forward over the case's input (the `squeeze()` undone)."""
    x = case_input(name) if x is None else x
    dev = model.fcn.weight.device
    batch = model({model.INPUT_KEY: torch.from_numpy(np.asarray(x)).to(dev)})
    return batch["features"].reshape(len(x), -1).cpu().numpy(), batch["yhat"].cpu().numpy()


def errors(got, want):
    """max-abs error of features and of yhat against the fp64 pair."""
    return tuple(float(np.abs(np.asarray(g, dtype=np.float64) - w).max()) for g, w in zip(got, want))
