"""Checker of mdm_amd/clip_text.py: an fp64 numpy restatement of OpenAI CLIP's encode_text (clip/model.py), a deterministic weight
builder under OpenAI's state-dict keys, the OpenAI -> HF key map, a stub byte-pair encoder, and the loaders of
tests/golden/clip_text_*.npz and PIN_REPORT_clip_text.json (written by tests/make_golden_clip_text.py from HF transformers'
CLIPTextModelWithProjection with hidden_act="quick_gelu", the same network under other names).

Restated (clip/model.py CLIP.encode_text, ResidualAttentionBlock, QuickGELU):
  x = token_embedding[ids] + positional_embedding[:L]
  per block: x += out_proj(attn(ln_1(x))), causal mask, heads of width / heads, scores / sqrt(head width);
             x += c_proj(quick_gelu(c_fc(ln_2(x)))), quick_gelu(v) = v sigmoid(1.702 v);   LayerNorm eps 1e-5
  e[b] = ln_final(x)[b, argmax(ids[b])] @ text_projection
"""
import functools
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PIN_REPORT = os.path.join(GOLDEN, "PIN_REPORT_clip_text.json")
KEYS_FILE = os.path.join(GOLDEN, "clip_text_state_dict_keys.json")

FULL = dict(width=512, heads=8, layers=12, mlp=2048, embed=512, positions=77)          # ViT-B/32's text tower
REDUCED = dict(width=128, heads=2, layers=2, mlp=256, embed=64, positions=77)          # non-square: a transposed projection shows
CFGS = {"full": FULL, "reduced": REDUCED}
VOCAB = 66                  # words 0 .. 63, then SOT and EOT: EOT is the highest id, so upstream's argmax rule and HF's first-EOS
SOT, EOT = 64, 65           # rule pick the same row
SEED = 11
LN_EPS = 1e-5

FIXTURE_LENS = [22, 9, 2, 16]           # tokens per prompt with SOT and EOT, in a [4, 77] batch (22: humanml's context length)
FIXTURES = {f"{c}_{r}": dict(cfg=c, trained=(r == "trained")) for c in ("reduced", "full") for r in ("default", "trained")}

# cases without a file of their own: HF's fp32 output is not kept, its error against fp64 (e_ref) is, in the pin report
KEY_TILE_LS = [1, 2, 31, 32, 33, 63, 64, 65, 76, 77]
ROW_BS = [1, 4, 5, 9, 10, 19]
SWEEP = {}
for _L in KEY_TILE_LS:
    SWEEP[f"keytile_L{_L}"] = dict(cfg="reduced", trained=True, ids_seed=100 + _L, L=_L, lens=[_L, max(1, _L // 2), 1])
for _B in ROW_BS:
    SWEEP[f"rows_B{_B}"] = dict(cfg="reduced", trained=True, ids_seed=200 + _B, L=7, lens=[7] + [1 + (3 * i) % 7 for i in range(1, _B)])
SWEEP["proj_B65_L2"] = dict(cfg="reduced", trained=True, ids_seed=265, L=2, lens=[2 - (i % 3 == 1) for i in range(65)])
SWEEP["full_B1_L12"] = dict(cfg="full", trained=True, ids_seed=300, L=12, lens=[12])

_BLOCK = (("attn.in_proj_weight", "3w,w"), ("attn.in_proj_bias", "3w"), ("attn.out_proj.weight", "w,w"), ("attn.out_proj.bias", "w"),
          ("ln_1.weight", "w"), ("ln_1.bias", "w"), ("mlp.c_fc.weight", "m,w"), ("mlp.c_fc.bias", "m"),
          ("mlp.c_proj.weight", "w,m"), ("mlp.c_proj.bias", "w"), ("ln_2.weight", "w"), ("ln_2.bias", "w"))


def state_dict_shapes(cfg, vocab=VOCAB):
    """The text side of OpenAI CLIP's state dict, in its order (pinned at full size by tests/golden/clip_text_state_dict_keys.json)."""
    dims = {"w": cfg["width"], "3w": 3 * cfg["width"], "m": cfg["mlp"]}
    s = [("positional_embedding", (cfg["positions"], cfg["width"])), ("text_projection", (cfg["width"], cfg["embed"]))]
    for n in range(cfg["layers"]):
        s += [(f"transformer.resblocks.{n}.{k}", tuple(dims[d] for d in shape.split(","))) for k, shape in _BLOCK]
    return s + [("token_embedding.weight", (vocab, cfg["width"])), ("ln_final.weight", (cfg["width"],)), ("ln_final.bias", (cfg["width"],))]


def build_weights(seed, cfg, trained=False):
    """An OpenAI-keyed state dict of fp32 tensors from ONE np.random.RandomState(seed), keys in upstream's order; a value is drawn
    only where the regime uses one.  Default: matrices and embeddings 0.02 N(0, 1), biases 0, LayerNorm 1 / 0.  trained=True
    ("trained-like"): matrices N(0, 1) / sqrt(fan_in) with the q and k rows of in_proj doubled -- peaked softmax rows, so that a
    wrong mask or max shows --, embeddings 0.06 N, every bias 0.1 N, LayerNorm weight 1 + 0.2 N."""
    rs = np.random.RandomState(seed)
    w, sd = cfg["width"], {}
    for key, shape in state_dict_shapes(cfg):
        if key.endswith("bias"):
            a = 0.1 * rs.standard_normal(shape) if trained else np.zeros(shape)
        elif ".ln_" in key or key.startswith("ln_final"):
            a = 1.0 + 0.2 * rs.standard_normal(shape) if trained else np.ones(shape)
        elif key in ("positional_embedding", "token_embedding.weight"):
            a = (0.06 if trained else 0.02) * rs.standard_normal(shape)
        elif trained:
            a = rs.standard_normal(shape) / np.sqrt(shape[0] if key == "text_projection" else shape[1])
            if key.endswith("in_proj_weight"):
                a[:2 * w] *= 2.0
        else:
            a = 0.02 * rs.standard_normal(shape)
        sd[key] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return sd


@functools.lru_cache(maxsize=None)
def weights(cfg_name, trained):
    """The fixtures' and sweep cases' weights (seed 11), built once per process and left unchanged."""
    return build_weights(SEED, CFGS[cfg_name], trained)


_HF_BLOCK = {"attn.out_proj": "self_attn.out_proj", "ln_1": "layer_norm1", "mlp.c_fc": "mlp.fc1", "mlp.c_proj": "mlp.fc2",
             "ln_2": "layer_norm2"}


def hf_key_map(cfg):
    """OpenAI key -> the HF CLIPTextModelWithProjection key(s) it maps to: in_proj_* is q | k | v stacked, text_projection is
    text_projection.weight transposed, everything else one to one."""
    t = "text_model."
    m = {"positional_embedding": t + "embeddings.position_embedding.weight", "text_projection": "text_projection.weight (transposed)",
         "token_embedding.weight": t + "embeddings.token_embedding.weight",
         "ln_final.weight": t + "final_layer_norm.weight", "ln_final.bias": t + "final_layer_norm.bias"}
    for n in range(cfg["layers"]):
        h, o = f"{t}encoder.layers.{n}.", f"transformer.resblocks.{n}."
        for leaf in ("weight", "bias"):
            m[f"{o}attn.in_proj_{leaf}"] = " | ".join(f"{h}self_attn.{p}_proj.{leaf}" for p in "qkv")
            for ours, theirs in _HF_BLOCK.items():
                m[f"{o}{ours}.{leaf}"] = f"{h}{theirs}.{leaf}"
    return m


def hf_state_dict(sd, cfg):
    """The OpenAI-keyed `sd` under HF's keys, by hf_key_map."""
    out = {}
    for key, target in hf_key_map(cfg).items():
        if " | " in target:
            for name, part in zip(target.split(" | "), torch.chunk(sd[key], 3, 0)):
                out[name] = part.clone()
        elif target.endswith("(transposed)"):
            out[target.split()[0]] = sd[key].t().contiguous()
        else:
            out[target] = sd[key].clone()
    return out


def hf_model(cfg_name, trained):
    """HF's module over the seed-11 weights (needs the transformers package; builds from a bare config, no file, no network)."""
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    cfg = CFGS[cfg_name]
    hf_cfg = CLIPTextConfig(vocab_size=VOCAB, hidden_size=cfg["width"], intermediate_size=cfg["mlp"], projection_dim=cfg["embed"],
                            num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"], max_position_embeddings=cfg["positions"],
                            hidden_act="quick_gelu", layer_norm_eps=LN_EPS, attention_dropout=0.0, pad_token_id=0, bos_token_id=SOT,
                            eos_token_id=EOT)
    model = CLIPTextModelWithProjection(hf_cfg)
    model.load_state_dict(hf_state_dict(weights(cfg_name, trained), cfg))
    return model.eval()


def make_tokens(seed, B, L, lens):
    """SOT, random word ids in [0, 64), EOT at len - 1, zeros behind; EOT alone when len = 1.  -> [B, L] int64."""
    rs = np.random.RandomState(seed)
    ids = np.zeros((B, L), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rs.randint(0, SOT, n)
        ids[b, 0] = SOT
        ids[b, n - 1] = EOT
    return ids


def fixture_tokens():
    return make_tokens(SEED + 1, 4, 77, FIXTURE_LENS)


def sweep_inputs(name):
    c = SWEEP[name]
    return make_tokens(c["ids_seed"], len(c["lens"]), c["L"], c["lens"])


def load_fixture(name):
    return dict(np.load(os.path.join(GOLDEN, f"clip_text_{name}.npz")))


@functools.lru_cache(maxsize=None)
def pin_report():
    with open(PIN_REPORT) as fh:
        return json.load(fh)


def pooled_e_ref(cfg_name, trained):
    """The unit of the accuracy condition: the maximum of e_ref = max |HF fp32 - fp64| over every case of the same (config, regime).
    Pooled because one output is only B x embed numbers."""
    cases = [n for n, f in FIXTURES.items() if (f["cfg"], f["trained"]) == (cfg_name, trained)]
    cases += [n for n, c in SWEEP.items() if (c["cfg"], c["trained"]) == (cfg_name, trained)]
    return max(pin_report()[n]["e_ref"] for n in cases)


def state_dict_keys():
    with open(KEYS_FILE) as fh:
        return json.load(fh)


# ---- fp64 restatement -----------------------------------------------------------------------------------------------------------------
def _ln(x, g, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + LN_EPS) * g + b


def encode_text_fp64(sd, tokens, heads):
    """text_embed [B, embed] in fp64, over all L positions as upstream computes them."""
    w = {k: np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, np.float64) for k, v in sd.items()}
    ids = np.asarray(tokens)
    B, L = ids.shape
    W = w["token_embedding.weight"].shape[1]
    hd = W // heads
    x = w["token_embedding.weight"][ids] + w["positional_embedding"][:L][None]
    causal = np.triu(np.full((L, L), -np.inf), 1)
    n = 0
    while f"transformer.resblocks.{n}.ln_1.weight" in w:
        p = f"transformer.resblocks.{n}."

        def split(v):
            return v.reshape(B, L, heads, hd).transpose(0, 2, 1, 3)                # [B, H, L, hd]

        h = _ln(x, w[p + "ln_1.weight"], w[p + "ln_1.bias"])
        q, k, v = (split(t) for t in np.split(h @ w[p + "attn.in_proj_weight"].T + w[p + "attn.in_proj_bias"], 3, -1))
        s = (q / np.sqrt(hd)) @ k.transpose(0, 1, 3, 2) + causal
        s = np.exp(s - s.max(-1, keepdims=True))
        ctx = ((s / s.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(B, L, W)
        x = x + ctx @ w[p + "attn.out_proj.weight"].T + w[p + "attn.out_proj.bias"]
        u = _ln(x, w[p + "ln_2.weight"], w[p + "ln_2.bias"]) @ w[p + "mlp.c_fc.weight"].T + w[p + "mlp.c_fc.bias"]
        x = x + (u / (1.0 + np.exp(-1.702 * u))) @ w[p + "mlp.c_proj.weight"].T + w[p + "mlp.c_proj.bias"]
        n += 1
    x = _ln(x, w["ln_final.weight"], w["ln_final.bias"])
    return x[np.arange(B), ids.argmax(-1)] @ w["text_projection"]


def maxabs(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    return float(np.abs(got.astype(np.float64) - np.asarray(want, np.float64)).max())


class StubBpe:
    """The byte-pair encoder interface of mdm_amd.clip_text.tokenize over the 66-id vocabulary: "w17" -> 17."""
    sot, eot = SOT, EOT

    def encode(self, text):
        return [int(w[1:]) for w in text.split()]


def make_clip(cfg_name, trained, device, native_lib=None, dtype=None):
    """mdm_amd.clip_text.ClipText over the seed-11 weights of a config, with the stub encoder as its tokenizer."""
    from mdm_amd.clip_text import load_clip_text
    sd = weights(cfg_name, trained)
    if dtype is not None:
        sd = {k: v.to(dtype) for k, v in sd.items()}
    return load_clip_text(sd, tokenizer=StubBpe(), _native_lib=native_lib).to(device)


def check(label, cfg_name, trained, got, want):
    """The accuracy condition: max-abs error against fp64 <= 4 x the pooled e_ref; prints its figure before it asserts."""
    e_ref = pooled_e_ref(cfg_name, trained)
    err = maxabs(got, want)
    print(f"[clip text] {label}: max-abs vs fp64 = {err:.3e} (bound {4 * e_ref:.3e}, ratio {err / e_ref:.2f} e_ref)")
    assert tuple(got.shape) == tuple(np.shape(want)) and got.dtype == torch.float32
    assert err <= 4 * e_ref
