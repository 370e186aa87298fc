"""Checker of mdm_amd/gru_recogniser.py: seeded weight builders, an fp64 numpy restatement of the recogniser written from its
equations, the case table, and the loaders of tests/golden/gru_recogniser_*.npz and PIN_REPORT_gru_recogniser.json (written by
tests/make_golden_gru_recogniser.py from the reference's own modules).  Weights are never stored: weights, inputs, lengths and
initial states are rebuilt from their seeds (numpy's legacy RandomState streams are frozen).

Restated (PyTorch's GRU, gates r | z | n; x [B, njoints, nfeats, T] read as [B, I, T]):
  per layer, from h = h0[layer], for every frame t:
      r = s(W_ir x_t + b_ir + W_hr h + b_hr)   z = s(W_iz x_t + b_iz + W_hz h + b_hz)   n = tanh(W_in x_t + b_in + r (W_hn h + b_hn))
      h = (1 - z) n + z h;   the layer's output at t is h, the next layer's x_t
  out[b] = the last layer's output at frame lengths[b] - 1;   features = tanh(linear1(out));   yhat = linear2(features)

Accuracy condition: max-abs error against this restatement <= 4 x e_ref, e_ref the reference's own fp32 error against fp64 on the
same weights, POOLED: the maximum over all cases of the same (net, regime, output) and three input draws per case.  A short case's
own e_ref is the maximum of a few dozen numbers and lies below what a different but valid summation order produces; the recurrence
is a contraction, its error saturates with T, so every (net, regime) has a T = 60 case that sets the level."""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PIN_REPORT = os.path.join(GOLDEN, "PIN_REPORT_gru_recogniser.json")
KEYS_FILE = os.path.join(GOLDEN, "gru_recogniser_state_dict_keys.json")
SEEDED_FILE = os.path.join(GOLDEN, "gru_recogniser_seeded.npz")
MID = 30
ROWS = 16                  # csrc/gru_recogniser.h GRU_SEQ_ROWS: the tile height built

# net -> constructor facts: (njoints, nfeats) of the input, hidden width, layers, classes
NETS = {
    "full": dict(joints=(24, 3), H=128, L=2, classes=12),        # HumanAct12: the published checkpoint's shape
    "ntu": dict(joints=(18, 3), H=128, L=2, classes=13),         # the reference's NTU-13 test(): I = 54, no multiple of 4
    "red1": dict(joints=(5, 2), H=32, L=1, classes=12),          # reduced nets of the emulator tests: I = 10
    "red2": dict(joints=(5, 2), H=32, L=2, classes=12),
    "red2c13": dict(joints=(5, 2), H=32, L=2, classes=13),
}
WSEED = {"default": 111, "trained": 112}


def _case(net, regime, B, T, lens, seed, fixture=False):
    return dict(net=net, regime=regime, B=B, T=T, lens=lens, seed=seed, fixture=fixture)


R = ROWS
CASES = {
    # full width, outputs stored (tests/golden/gru_recogniser_{default,trained}.npz); they also set their pool's level
    "full_default": _case("full", "default", 3, 60, [60, 37, 1], 401, True),
    "full_trained": _case("full", "trained", 3, 60, [60, 37, 1], 402, True),
    "ntu_trained_3x60": _case("ntu", "trained", 3, 60, [60, 37, 1], 421),
    "ntu_trained_5x13": _case("ntu", "trained", 5, 13, "ragged", 422),
}
# full width, both regimes: restated in fp64 by the tests
FULL_SHAPES = [(1, 1, "full"), (1, 60, "full"), (R + 1, 7, "full"), (2 * R + 1, 13, "ragged"), (33, 5, "ragged")]
for _regime in ("default", "trained"):
    for _i, (_b, _t, _lens) in enumerate(FULL_SHAPES):
        CASES[f"full_{_regime}_{_b}x{_t}"] = _case("full", _regime, _b, _t, _lens, 430 + 10 * len(CASES) + _i)
# reduced nets: (B, T, lengths).  "ragged": seeded, row 0 = 1 and the last row = T (a length-1 row beside a length-T row);
# "short": the rows of the LAST tile are all shorter than T
EMU_SHAPES = [(1, 1, "full"), (1, 2, "full"), (2, 13, "ragged"), (R, 5, "ragged"), (R + 1, 5, "short"), (2 * R + 1, 3, "ragged")]
for _net in ("red1", "red2"):
    for _regime in ("default", "trained"):
        for _i, (_b, _t, _lens) in enumerate(EMU_SHAPES):
            CASES[f"{_net}_{_regime}_{_b}x{_t}"] = _case(_net, _regime, _b, _t, _lens, 500 + 10 * len(CASES) + _i)
        # (not run on the emulator: the T = 60 case that sets the pool's level)
        CASES[f"{_net}_{_regime}_3x60"] = _case(_net, _regime, 3, 60, [60, 37, 1], 900 + len(CASES))
for _regime in ("default", "trained"):
    CASES[f"red2c13_{_regime}_2x13"] = _case("red2c13", _regime, 2, 13, "ragged", 950 + len(CASES))
    CASES[f"red2c13_{_regime}_3x60"] = _case("red2c13", _regime, 3, 60, [60, 37, 1], 970 + len(CASES))
EMU_CASES = [n for n, c in CASES.items() if n.startswith("red") and c["T"] < 60]
SEEDED = dict(net="red2", regime="trained", B=3, T=13, lens=[13, 6, 1], seed=991, torch_seed=1234)


# ---- models and weights -----------------------------------------------------------------------------------------------------------------
def input_size(net):
    j, f = NETS[net]["joints"]
    return j * f


def make_model(net, device="cpu", native_lib=None, fid=False):
    from mdm_amd import gru_recogniser as gr
    f = NETS[net]
    cls = gr.MotionDiscriminatorForFID if fid else gr.MotionDiscriminator
    kw = {} if native_lib is None else {"_native_lib": native_lib}
    return cls(input_size(net), f["H"], f["L"], device=device, output_size=f["classes"], **kw)


def state_shapes(net):
    return [(k, tuple(v.shape)) for k, v in make_model(net).state_dict().items()]


def build_weights(net, regime):
    """A state dict of fp32 tensors in the reference's key order.  "default": the modules' own U(-1/sqrt(fan), 1/sqrt(fan)) (fan = H
    for the GRU and linear1, 30 for linear2).  "trained": GRU and linear weights 2x larger, every bias N(0, 0.3) -- nothing a zero
    would hide."""
    assert regime in ("default", "trained")
    f = NETS[net]
    H, L, I = f["H"], f["L"], input_size(net)
    rs = np.random.RandomState(WSEED[regime] + 1000 * sorted(NETS).index(net))
    shapes = []
    for l in range(L):          # nn.GRU registers, per layer: weight_ih, weight_hh, bias_ih, bias_hh
        shapes += [(f"recurrent.weight_ih_l{l}", (3 * H, I if l == 0 else H), H), (f"recurrent.weight_hh_l{l}", (3 * H, H), H),
                   (f"recurrent.bias_ih_l{l}", (3 * H,), H), (f"recurrent.bias_hh_l{l}", (3 * H,), H)]
    shapes += [("linear1.weight", (MID, H), H), ("linear1.bias", (MID,), H), ("linear2.weight", (f["classes"], MID), MID),
               ("linear2.bias", (f["classes"],), MID)]
    sd = {}
    for key, shape, fan in shapes:
        k = 1.0 / np.sqrt(fan)
        if regime == "trained" and len(shape) == 1:
            a = rs.normal(0.0, 0.3, shape)
        else:
            a = rs.uniform(-k, k, shape) * (2.0 if regime == "trained" else 1.0)
        sd[key] = torch.from_numpy(np.asarray(a, dtype=np.float32))
    return sd


def loaded_model(net, weights, device="cpu", native_lib=None, fid=False):
    m = make_model(net, device, native_lib, fid)
    m.load_state_dict(weights)
    return m.to(device).eval()


def make_lens(kind, B, T, seed):
    if isinstance(kind, (list, tuple)):
        assert len(kind) == B
        return np.asarray(kind, dtype=np.int64)
    if kind == "full":
        return np.full(B, T, dtype=np.int64)
    rs = np.random.RandomState(seed + 77)
    lens = rs.randint(1, T + 1, size=B)
    if kind == "short":              # the rows of the last tile end in front of T; the first tile holds a full row
        assert B > ROWS and T > 1
        last = (B - 1) // ROWS * ROWS
        lens[last:] = rs.randint(1, T, size=B - last)
        lens[0] = T
    else:
        assert kind == "ragged"
        lens[0] = 1
        lens[-1] = T
    return lens.astype(np.int64)


def make_input(net, seed, B, T):
    """(x [B, njoints, nfeats, T], h0 [L, B, H]) fp32."""
    f = NETS[net]
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((B,) + f["joints"] + (T,)) * 0.8).astype(np.float32)
    h0 = rs.standard_normal((f["L"], B, f["H"])).astype(np.float32)
    return x, h0


def case_weights(name):
    c = CASES[name]
    return build_weights(c["net"], c["regime"])


def case_input(name, draw=0, attempt=None):
    """(x, lens, h0) of a case.  draw 1, 2: the further draws of e_ref.  A fixture's seed moves by `attempt` until every row's top-2
    margin holds (tests/make_golden_gru_recogniser.py); the report records the attempt that did."""
    c = CASES[name]
    if attempt is None:
        attempt = pin_report()["cases"][name].get("attempt", 0) if c["fixture"] else 0
    seed = c["seed"] + 1000 * draw + 100000 * attempt
    x, h0 = make_input(c["net"], seed, c["B"], c["T"])
    return x, make_lens(c["lens"], c["B"], c["T"], seed), h0


# ---- fp64 restatement ------------------------------------------------------------------------------------------------------------------
def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def forward_fp64(net, sd, x, lens, h0):
    """(features [B, 30], yhat [B, classes]) in fp64, from the equations in this file's header."""
    f = NETS[net]
    H = f["H"]
    x = np.asarray(x, dtype=np.float64)
    B, T = x.shape[0], x.shape[3]
    seq = x.reshape(B, -1, T).transpose(2, 0, 1)                     # [T, B, I]
    for l in range(f["L"]):
        w_ih, w_hh, b_ih, b_hh = (sd[f"recurrent.{k}_l{l}"].double().numpy() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
        h = np.asarray(h0[l], dtype=np.float64)
        outs = []
        for t in range(T):
            gi = seq[t] @ w_ih.T + b_ih
            gh = h @ w_hh.T + b_hh
            r = _sig(gi[:, :H] + gh[:, :H])
            z = _sig(gi[:, H:2 * H] + gh[:, H:2 * H])
            n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            h = (1.0 - z) * n + z * h
            outs.append(h)
        seq = np.stack(outs)
    out = seq[np.asarray(lens) - 1, np.arange(B)]
    feat = np.tanh(out @ sd["linear1.weight"].double().numpy().T + sd["linear1.bias"].double().numpy())
    return feat, feat @ sd["linear2.weight"].double().numpy().T + sd["linear2.bias"].double().numpy()


# ---- fixtures and the report -------------------------------------------------------------------------------------------------------------
_REPORT = None


def pin_report():
    global _REPORT
    if _REPORT is None:
        with open(PIN_REPORT) as fh:
            _REPORT = json.load(fh)
    return _REPORT


def pool_key(net, regime):
    return f"{net}/{regime}"


def bound(net, regime):
    """The accuracy condition: (4 x pooled e_ref of features, 4 x pooled e_ref of yhat)."""
    p = pin_report()["pooled"][pool_key(net, regime)]
    return 4 * p["e_ref_features"], 4 * p["e_ref_yhat"]


def case_bound(name):
    return bound(CASES[name]["net"], CASES[name]["regime"])


def load_fixture(name):
    assert CASES[name]["fixture"]
    with np.load(os.path.join(GOLDEN, f"gru_recogniser_{name.split('_', 1)[1]}.npz")) as z:
        return {k: z[k] for k in z.files}


def load_seeded():
    with np.load(SEEDED_FILE) as z:
        return {k: z[k] for k in z.files}


def run_model(model, x, lens, h0, lens_device=None):
    """(features, yhat) as fp32 numpy from one native call through the module (`run` returns both views' outputs)."""
    dev = model.linear1.weight.device
    lt = torch.from_numpy(np.asarray(lens))
    if lens_device is not None:
        lt = lt.to(lens_device)
    h = None if h0 is None else torch.from_numpy(np.asarray(h0)).to(dev)
    with torch.no_grad():
        feat, yhat = model.run(torch.from_numpy(np.asarray(x)).to(dev), lt, h)
    return feat.cpu().numpy(), yhat.cpu().numpy()


def errors(got, want):
    """max-abs error of features and of yhat against the fp64 pair."""
    return tuple(float(np.abs(np.asarray(g, dtype=np.float64) - w).max()) for g, w in zip(got, want))
