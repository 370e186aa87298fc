"""Checker of mdm_amd/evaluator.py: an fp64 numpy restatement of the evaluator's three networks, a deterministic weight builder, and
the loader of tests/golden/evaluator_*.npz (written by tests/make_golden_evaluator.py from the reference's own modules).

Restated, with the reference's lines:
  data_loaders/humanml/networks/modules.py:79-98    MovementConvEncoder: Conv1d(C, h, 4, 2, 1) - LeakyReLU(0.2) - Conv1d(h, o, 4, 2, 1) -
                                                    LeakyReLU(0.2) over the permuted input, then out_net (dropout: eval mode)
  modules.py:311-350                                TextEncoderBiGRUCo: input_emb(word_embs + pos_emb(pos_onehot)), packed BiGRU from the
                                                    learned `hidden`, cat(gru_last[0], gru_last[1]), output_net
  modules.py:353-386                                MotionEncoderBiGRUCo: the same without pos_emb
  torch.nn.GRU                                      r = s(W_ir x + b_ir + W_hr h + b_hr), z likewise, n = tanh(W_in x + b_in + r (W_hn h + b_hn)),
                                                    h' = (1 - z) n + z h; packed: the reverse direction starts at each row's last element
  networks/evaluator_wrapper.py:154-187             get_co_embeddings / get_motion_embeddings: argsort(m_lens)[::-1], m_lens // unit_length,
                                                    text_embedding[align_idx]
  data_loaders/humanml/utils/metrics.py:6-45        euclidean_distance_matrix, calculate_top_k (R-precision's boolean matrix)
"""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PIN_REPORT = os.path.join(GOLDEN, "PIN_REPORT_evaluator.json")
KEYS_FILE = os.path.join(GOLDEN, "evaluator_state_dict_keys.json")

FULL = dict(dim_pose=263, dim_word=300, dim_pos_ohot=15, dim_movement_enc_hidden=512, dim_movement_latent=512,
            dim_motion_hidden=1024, dim_text_hidden=512, dim_coemb_hidden=512)
# the narrowest widths the kernels take (hidden sizes are multiples of 256); the 259-feature gather of the first convolution is kept
REDUCED = dict(dim_pose=263, dim_word=300, dim_pos_ohot=15, dim_movement_enc_hidden=64, dim_movement_latent=32,
               dim_motion_hidden=256, dim_text_hidden=256, dim_coemb_hidden=64)
KIT_REDUCED = dict(REDUCED, dim_pose=251)
DIMS = {"full": FULL, "reduced": REDUCED}

# name -> what the fixture runs.  Weights and inputs are rebuilt from the seeds (numpy's legacy RandomState streams are frozen): even at
# the reduced widths the two GRUs alone are 6 MB of fp32, beyond what a committed file may hold, so every file carries outputs only.
FIXTURES = {
    "motion_b3_reduced": dict(kind="motion", dims="reduced", trained=False, seed=11, T=60, m_lens=[37, 60, 37]),
    "motion_b32_full_default": dict(kind="motion", dims="full", trained=False, seed=12, T=196,
                                    m_lens=[40 + (i * 61) % 157 for i in range(31)] + [196]),
    "motion_b32_full_trained": dict(kind="motion", dims="full", trained=True, seed=13, T=196,
                                    m_lens=[40 + (i * 61) % 157 for i in range(31)] + [196]),
    "motion_b5_short_reduced": dict(kind="motion", dims="reduced", trained=True, seed=14, T=200, m_lens=[200, 6, 133, 200, 81]),
    "text_b4_reduced": dict(kind="text", dims="reduced", trained=False, seed=15, L=22, cap_lens=[22, 9, 4, 1]),
    "text_b4_full": dict(kind="text", dims="full", trained=True, seed=16, L=22, cap_lens=[22, 9, 4, 1]),
    "co_b32_full": dict(kind="co", dims="full", trained=False, seed=17, T=196, L=22,
                        m_lens=[196 - (i * 37) % 150 for i in range(32)], cap_lens=sorted([3 + (i * 7) % 20 for i in range(32)], reverse=True)),
}


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def _shapes(dims):
    from mdm_amd import evaluator as ev
    d = dims
    return (ev.movement_encoder_shapes(d["dim_pose"] - 4, d["dim_movement_enc_hidden"], d["dim_movement_latent"]),
            ev.text_encoder_shapes(d["dim_word"], d["dim_pos_ohot"], d["dim_text_hidden"], d["dim_coemb_hidden"]),
            ev.motion_encoder_shapes(d["dim_movement_latent"], d["dim_motion_hidden"], d["dim_coemb_hidden"]))


def build_weights(seed, dims, trained=False):
    """(movement, text, motion) state dicts of fp32 tensors.  Default: the distributions the reference's modules start from
    (modules.py:27-32 xavier_normal_ weights and zero biases on Conv1d / Linear; nn.GRU's U(-1/sqrt(H), 1/sqrt(H)); LayerNorm 1 / 0;
    `hidden` ~ N(0, 1)).  trained=True ("trained-like"): the GRU matrices 4x larger, so that gates saturate and the recurrence keeps
    state, and non-zero biases / LayerNorm affine -- nothing a zero or a one would hide."""
    rs = np.random.RandomState(seed)
    out = []
    for shapes in _shapes(dims):
        sd = {}
        H = dict(shapes)["hidden"][-1] if "hidden" in dict(shapes) else None
        for key, shape in shapes:
            if key == "hidden":
                a = rs.standard_normal(shape)
            elif key.startswith("gru."):
                k = 1.0 / np.sqrt(H)
                a = rs.uniform(-k, k, shape)
                if trained and "weight" in key:
                    a = a * 4.0
            elif key.startswith("output_net.1."):
                a = np.ones(shape) if key.endswith("weight") else np.zeros(shape)
                if trained:
                    a = a + 0.1 * rs.standard_normal(shape)
            elif key.endswith("weight"):
                fan_out, fan_in = shape[0], shape[1]
                rf = int(np.prod(shape[2:])) if len(shape) > 2 else 1
                a = rs.standard_normal(shape) * np.sqrt(2.0 / ((fan_in + fan_out) * rf))
            else:
                a = 0.1 * rs.standard_normal(shape) if trained else np.zeros(shape)
            sd[key] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        out.append(sd)
    return tuple(out)


def make_motion_inputs(seed, B, T, dim_pose, m_lens):
    """Normalised-feature-like motions, zero beyond each length (the data loader pads with zeros)."""
    rs = np.random.RandomState(seed + 1000)
    x = rs.standard_normal((B, T, dim_pose)).astype(np.float32)
    for b, l in enumerate(m_lens):
        x[b, l:] = 0
    return x


def make_text_inputs(seed, B, L, dim_word, dim_pos, cap_lens):
    rs = np.random.RandomState(seed + 2000)
    w = (0.3 * rs.standard_normal((B, L, dim_word))).astype(np.float32)
    pos = np.zeros((B, L, dim_pos), np.float32)
    pos[np.arange(B)[:, None], np.arange(L)[None], rs.randint(0, dim_pos, (B, L))] = 1
    for b, l in enumerate(cap_lens):
        w[b, l:] = 0
        pos[b, l:] = 0
    return w, pos


def fixture_inputs(name):
    f = FIXTURES[name]
    d = DIMS[f["dims"]]
    out = {}
    if f["kind"] in ("motion", "co"):
        out["motions"] = make_motion_inputs(f["seed"], len(f["m_lens"]), f["T"], d["dim_pose"], f["m_lens"])
        out["m_lens"] = np.asarray(f["m_lens"], np.int64)
    if f["kind"] in ("text", "co"):
        out["word_embs"], out["pos_ohot"] = make_text_inputs(f["seed"], len(f["cap_lens"]), f["L"], d["dim_word"], d["dim_pos_ohot"],
                                                             f["cap_lens"])
        out["cap_lens"] = np.asarray(f["cap_lens"], np.int64)
    return out


def fixture_weights(name):
    f = FIXTURES[name]
    return build_weights(f["seed"], DIMS[f["dims"]], f["trained"])


def load_fixture(name):
    g = dict(np.load(os.path.join(GOLDEN, f"evaluator_{name}.npz")))
    return g


def pin_report():
    with open(PIN_REPORT) as fh:
        return json.load(fh)


# ---- fp64 restatement -----------------------------------------------------------------------------------------------------------------
def _np64(sd):
    return {k: np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, np.float64) for k, v in sd.items()}


def _leaky(x):
    return np.where(x > 0, x, 0.2 * x)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def conv1d_k4s2_fp64(x, w, b):
    """nn.Conv1d(C, O, 4, 2, 1) on channels-last x [B, T, C]: out[b, t, o] = b[o] + sum_{c, tap} w[o, c, tap] xpad[b, 2 t + tap, c]."""
    B, T, C = x.shape
    Tout = (T + 2 - 4) // 2 + 1
    xp = np.zeros((B, T + 2, C))
    xp[:, 1:T + 1] = x
    win = np.stack([xp[:, tap:tap + 2 * Tout:2] for tap in range(4)], axis=2)      # [B, Tout, 4, C]
    return np.einsum("btkc,ock->bto", win, w) + b


def movement_encoder_fp64(sd, inputs):
    sd = _np64(sd)
    x = np.asarray(inputs, np.float64)
    x = _leaky(conv1d_k4s2_fp64(x, sd["main.0.weight"], sd["main.0.bias"]))
    x = _leaky(conv1d_k4s2_fp64(x, sd["main.3.weight"], sd["main.3.bias"]))
    return x @ sd["out_net.weight"].T + sd["out_net.bias"]


def bigru_last_fp64(sd, emb, lens):
    """gru_last of nn.GRU(H, H, batch_first=True, bidirectional=True) over pack_padded_sequence(emb, lens): [2, B, H]."""
    B, _, H = emb.shape
    lens = np.asarray(lens)
    last = []
    for d, sfx in enumerate(("", "_reverse")):
        w_ih, w_hh = sd[f"gru.weight_ih_l0{sfx}"], sd[f"gru.weight_hh_l0{sfx}"]
        b_ih, b_hh = sd[f"gru.bias_ih_l0{sfx}"], sd[f"gru.bias_hh_l0{sfx}"]
        h = np.repeat(sd["hidden"][d], B, axis=0)                                     # hidden.repeat(1, num_samples, 1)
        for s in range(int(lens.max())):
            act = s < lens
            t = np.where(act, s if d == 0 else lens - 1 - s, 0)
            gi = emb[np.arange(B), t] @ w_ih.T + b_ih
            gh = h @ w_hh.T + b_hh
            r = _sigmoid(gi[:, :H] + gh[:, :H])
            z = _sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            h = np.where(act[:, None], (1 - z) * n + z * h, h)
        last.append(h)
    return np.stack(last)


def _output_net_fp64(sd, x):
    x = x @ sd["output_net.0.weight"].T + sd["output_net.0.bias"]
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    x = (x - mu) / np.sqrt(var + 1e-5) * sd["output_net.1.weight"] + sd["output_net.1.bias"]
    return _leaky(x) @ sd["output_net.3.weight"].T + sd["output_net.3.bias"]


def motion_encoder_fp64(sd, movements, lens):
    sd = _np64(sd)
    emb = np.asarray(movements, np.float64) @ sd["input_emb.weight"].T + sd["input_emb.bias"]
    last = bigru_last_fp64(sd, emb, lens)
    return _output_net_fp64(sd, np.concatenate([last[0], last[1]], -1))


def text_encoder_fp64(sd, word_embs, pos_ohot, cap_lens):
    sd = _np64(sd)
    pos = np.asarray(pos_ohot, np.float64) @ sd["pos_emb.weight"].T + sd["pos_emb.bias"]
    emb = (np.asarray(word_embs, np.float64) + pos) @ sd["input_emb.weight"].T + sd["input_emb.bias"]
    last = bigru_last_fp64(sd, emb, cap_lens)
    return _output_net_fp64(sd, np.concatenate([last[0], last[1]], -1))


def motion_embeddings_fp64(weights, motions, m_lens, unit_length=4):
    """get_motion_embeddings (evaluator_wrapper.py:175-187): rows in argsort(m_lens)[::-1] order."""
    movement, _, motion = weights
    m_lens = np.asarray(m_lens)
    align_idx = np.argsort(m_lens.tolist())[::-1].copy()
    mv = movement_encoder_fp64(movement, np.asarray(motions)[align_idx][..., :-4])
    return motion_encoder_fp64(motion, mv, m_lens[align_idx] // unit_length), align_idx


def co_embeddings_fp64(weights, word_embs, pos_ohot, cap_lens, motions, m_lens, unit_length=4):
    """get_co_embeddings (evaluator_wrapper.py:154-172) -> (text_embedding[align_idx], motion_embedding)."""
    me, align_idx = motion_embeddings_fp64(weights, motions, m_lens, unit_length)
    te = text_encoder_fp64(weights[1], word_embs, pos_ohot, cap_lens)
    return te[align_idx], me


def run_fp64(name):
    f, inp, w = FIXTURES[name], fixture_inputs(name), fixture_weights(name)
    if f["kind"] == "motion":
        return {"motion": motion_embeddings_fp64(w, inp["motions"], inp["m_lens"])[0]}
    if f["kind"] == "text":
        return {"text": text_encoder_fp64(w[1], inp["word_embs"], inp["pos_ohot"], inp["cap_lens"])}
    te, me = co_embeddings_fp64(w, inp["word_embs"], inp["pos_ohot"], inp["cap_lens"], inp["motions"], inp["m_lens"])
    return {"text": te, "motion": me}


# ---- metrics.py restated ----------------------------------------------------------------------------------------------------------
def euclidean_distance_matrix(m1, m2):
    """metrics.py:6-20."""
    d1 = -2 * np.dot(m1, m2.T)
    d2 = np.sum(np.square(m1), axis=1, keepdims=True)
    d3 = np.sum(np.square(m2), axis=1)
    return np.sqrt(d1 + d2 + d3)


def top_k_matrix(emb1, emb2, top_k=3):
    """calculate_R_precision(..., sum_all=False) of metrics.py:22-58: [N, top_k] booleans, 'the matching row is among the k nearest'."""
    dist = euclidean_distance_matrix(emb1, emb2)
    argmax = np.argsort(dist, axis=1)
    gt = np.arange(dist.shape[0])[:, None]
    bool_mat = argmax == gt
    correct, out = np.zeros(dist.shape[0], bool), []
    for i in range(top_k):
        correct = correct | bool_mat[:, i]
        out.append(correct.copy())
    return np.stack(out, axis=1)


def nearest_gap(emb1, emb2, top_k=3):
    """The smallest difference between consecutive sorted distances of a row, over the first top_k + 1 of every row: what rounding
    would have to exceed to change top_k_matrix."""
    d = np.sort(euclidean_distance_matrix(np.asarray(emb1, np.float64), np.asarray(emb2, np.float64)), axis=1)
    return float(np.diff(d[:, :top_k + 1], axis=1).min())


def make_wrapper(name_or_dims, weights, device, native_lib=None, dataset_name="humanml"):
    from mdm_amd.evaluator import EvaluatorMDMWrapper
    dims = DIMS[FIXTURES[name_or_dims]["dims"]] if isinstance(name_or_dims, str) else name_or_dims
    movement, text, motion = weights
    return EvaluatorMDMWrapper.from_state_dicts(movement, text, motion, dataset_name, device, dims=dims, _native_lib=native_lib)
