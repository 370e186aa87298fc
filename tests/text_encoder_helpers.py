"""Checker of mdm_amd/text_encoder.py: an fp64 numpy restatement of HF DistilBertModel as the reference's model/BERT/BERT_encoder.py
runs it (eval mode, fp32, dropout off), a deterministic weight builder, and the loaders of tests/golden/text_encoder_*.npz and
PIN_REPORT_text_encoder.json (written by tests/make_golden_text_encoder.py from the reference's own load_bert).

Restated (HF transformers models/distilbert/modeling_distilbert.py):
  Embeddings                  LN(word_embeddings[id] + position_embeddings[t]), eps 1e-12
  MultiHeadSelfAttention      q, k, v = x W^T + b; heads of dim / n_heads; softmax(q k^T / sqrt(head_dim)) over the keys the
                              attention mask keeps; out_lin
  TransformerBlock            x = sa_layer_norm(attn + x); x = output_layer_norm(lin2(gelu(lin1(x))) + x), gelu the erf form
"""
import functools
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PIN_REPORT = os.path.join(GOLDEN, "PIN_REPORT_text_encoder.json")
KEYS_FILE = os.path.join(GOLDEN, "text_encoder_state_dict_keys.json")

FULL = dict(dim=768, n_heads=12, hidden=3072, n_layers=6, max_pos=512)
REDUCED = dict(dim=128, n_heads=2, hidden=256, n_layers=2, max_pos=128)
CFGS = {"full": FULL, "reduced": REDUCED}
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(59)]
PAD, CLS, SEP = 0, 2, 3
SEED = 5
LN_EPS = 1e-12

# the four fixtures: B = 4 prompts of 31, 7, 1 and 18 words -> [CLS] words [SEP], padded to L = 33
FIXTURE_WORDS = [31, 7, 1, 18]
FIXTURE_LENS = [33, 9, 3, 20]
FIXTURES = {f"{c}_{r}": dict(cfg=c, trained=(r == "trained")) for c in ("reduced", "full") for r in ("default", "trained")}

# cases without a file of their own: the reference's fp32 output is not kept, its error against fp64 (e_ref) is, in the pin report
KEY_TILE_LS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128]
ROW_BS = [1, 4, 5, 9, 10, 19]
SWEEP = {}
for _L in KEY_TILE_LS:
    SWEEP[f"keytile_L{_L}"] = dict(cfg="reduced", trained=True, ids_seed=100 + _L, L=_L, lens=[_L, max(1, _L // 2), 1])
for _B in ROW_BS:
    SWEEP[f"rows_B{_B}"] = dict(cfg="reduced", trained=True, ids_seed=200 + _B, L=7, lens=[7] + [1 + (3 * i) % 7 for i in range(1, _B)])
SWEEP["full_B1_L12"] = dict(cfg="full", trained=True, ids_seed=300, L=12, lens=[12])


def state_dict_shapes(cfg, vocab=len(VOCAB)):
    """HF DistilBertModel's state-dict keys and shapes, in its order (pinned by tests/golden/text_encoder_state_dict_keys.json)."""
    d, h = cfg["dim"], cfg["hidden"]
    s = [("embeddings.word_embeddings.weight", (vocab, d)), ("embeddings.position_embeddings.weight", (cfg["max_pos"], d)),
         ("embeddings.LayerNorm.weight", (d,)), ("embeddings.LayerNorm.bias", (d,))]
    for n in range(cfg["n_layers"]):
        p = f"transformer.layer.{n}."
        for lin in ("q_lin", "k_lin", "v_lin", "out_lin"):
            s += [(p + f"attention.{lin}.weight", (d, d)), (p + f"attention.{lin}.bias", (d,))]
        s += [(p + "sa_layer_norm.weight", (d,)), (p + "sa_layer_norm.bias", (d,)),
              (p + "ffn.lin1.weight", (h, d)), (p + "ffn.lin1.bias", (h,)), (p + "ffn.lin2.weight", (d, h)), (p + "ffn.lin2.bias", (d,)),
              (p + "output_layer_norm.weight", (d,)), (p + "output_layer_norm.bias", (d,))]
    return s


def build_weights(seed, cfg, trained=False):
    """A DistilBertModel state dict of fp32 tensors from ONE np.random.RandomState(seed), keys in HF's order; a value is drawn only
    where the regime uses one.  Default (HF's init): matrices and embeddings 0.02 N(0, 1), biases 0, LayerNorm 1 / 0.
    trained=True ("trained-like"): matrices N(0, 1) / sqrt(fan_in) with q_lin and k_lin doubled -- peaked softmax rows, so that a
    wrong mask or max shows --, embeddings 0.06 N, every bias 0.1 N, LayerNorm weight 1 + 0.2 N."""
    rs = np.random.RandomState(seed)
    sd = {}
    for key, shape in state_dict_shapes(cfg):
        norm = "LayerNorm" in key or "layer_norm" in key
        if key.endswith("bias"):
            a = 0.1 * rs.standard_normal(shape) if trained else np.zeros(shape)
        elif norm:
            a = 1.0 + 0.2 * rs.standard_normal(shape) if trained else np.ones(shape)
        elif key.startswith("embeddings."):
            a = (0.06 if trained else 0.02) * rs.standard_normal(shape)
        elif trained:
            a = rs.standard_normal(shape) / np.sqrt(shape[1]) * (2.0 if ("q_lin" in key or "k_lin" in key) else 1.0)
        else:
            a = 0.02 * rs.standard_normal(shape)
        sd[key] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return sd


@functools.lru_cache(maxsize=None)
def weights(cfg_name, trained):
    """The fixtures' and sweep cases' weights (seed 5), built once per process and left unchanged."""
    return build_weights(SEED, CFGS[cfg_name], trained)


def make_ids(seed, B, L, lens):
    """[CLS], random word ids in [5, 64), [SEP] at len - 1, [PAD] behind; [CLS] alone when len = 1.  -> ids [B, L] int64, mask [B, L] bool."""
    rs = np.random.RandomState(seed)
    ids = np.full((B, L), PAD, np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rs.randint(5, len(VOCAB), n)
        ids[b, 0] = CLS
        if n > 1:
            ids[b, n - 1] = SEP
    return ids, np.arange(L)[None, :] < np.asarray(lens)[:, None]


def fixture_texts():
    """The four prompts of the fixtures (words of the 64-entry vocabulary, so the tokenizer maps a word to one id)."""
    rs = np.random.RandomState(SEED + 1)
    return [" ".join(f"w{i}" for i in rs.randint(0, 59, n)) for n in FIXTURE_WORDS]


def sweep_inputs(name):
    c = SWEEP[name]
    ids, mask = make_ids(c["ids_seed"], len(c["lens"]), c["L"], c["lens"])
    return ids, mask, list(c["lens"])


def load_fixture(name):
    return dict(np.load(os.path.join(GOLDEN, f"text_encoder_{name}.npz")))


def pin_report():
    with open(PIN_REPORT) as fh:
        return json.load(fh)


def state_dict_keys():
    with open(KEYS_FILE) as fh:
        return json.load(fh)


# ---- fp64 restatement -----------------------------------------------------------------------------------------------------------------
def _ln(x, g, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + LN_EPS) * g + b


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(x / np.sqrt(2.0))).numpy())


def encoder_fp64(sd, ids, lens, n_heads):
    """last_hidden_state [B, L, dim] in fp64.  Rows at or beyond a length hold what HF computes there (padded queries over the valid
    keys); the tests compare valid rows only."""
    w = {k: np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, np.float64) for k, v in sd.items()}
    ids = np.asarray(ids)
    B, L = ids.shape
    D = w["embeddings.word_embeddings.weight"].shape[1]
    hd = D // n_heads
    keep = np.arange(L)[None, :] < np.asarray(lens)[:, None]                      # [B, L] keys
    x = _ln(w["embeddings.word_embeddings.weight"][ids] + w["embeddings.position_embeddings.weight"][:L][None],
            w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"])
    n = 0
    while f"transformer.layer.{n}.ffn.lin1.weight" in w:
        p = f"transformer.layer.{n}."

        def lin(name, v):
            return v @ w[p + name + ".weight"].T + w[p + name + ".bias"]

        def heads(v):
            return v.reshape(B, L, n_heads, hd).transpose(0, 2, 1, 3)                # [B, H, L, hd]

        q, k, v = heads(lin("attention.q_lin", x)), heads(lin("attention.k_lin", x)), heads(lin("attention.v_lin", x))
        s = (q / np.sqrt(hd)) @ k.transpose(0, 1, 3, 2)
        s = np.where(keep[:, None, None, :], s, -np.inf)
        s = np.exp(s - s.max(-1, keepdims=True))
        ctx = ((s / s.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(B, L, D)
        x = _ln(lin("attention.out_lin", ctx) + x, w[p + "sa_layer_norm.weight"], w[p + "sa_layer_norm.bias"])
        x = _ln(lin("ffn.lin2", _gelu(lin("ffn.lin1", x))) + x, w[p + "output_layer_norm.weight"], w[p + "output_layer_norm.bias"])
        n += 1
    return x


def valid_maxabs(got, want, lens):
    """max |got - want| over the rows below each length; got / want [B, L, D]."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    keep = np.arange(got.shape[1])[None, :] < np.asarray(lens)[:, None]
    return float(np.abs(got.astype(np.float64) - np.asarray(want, np.float64))[keep].max())


def make_bert(cfg_name, trained, device, native_lib=None):
    """mdm_amd.text_encoder.BERT over the seed-5 weights of a config, without a tokenizer."""
    from mdm_amd.text_encoder import BERT
    return BERT.from_state_dict(weights(cfg_name, trained), n_heads=CFGS[cfg_name]["n_heads"], _native_lib=native_lib).to(device)


def encode(bert, ids, mask, token_major=False):
    return bert.encode_ids(torch.from_numpy(np.asarray(ids)), torch.from_numpy(np.asarray(mask)), token_major=token_major)


def synth_model_dir(path, cfg_name, trained):
    """A local HF model directory (tokenizer over the 64-entry vocabulary + DistilBertModel with the seed-5 weights) for the code
    paths that read one: the reference's load_bert and BERT.from_pretrained_dir.  Needs the transformers package; no network."""
    from transformers import BertTokenizerFast, DistilBertConfig, DistilBertModel
    cfg = CFGS[cfg_name]
    os.makedirs(path, exist_ok=True)
    vocab_file = os.path.join(path, "vocab.txt")
    with open(vocab_file, "w") as fh:
        fh.write("\n".join(VOCAB) + "\n")
    BertTokenizerFast(vocab_file=vocab_file, do_lower_case=True).save_pretrained(path)
    hf_cfg = DistilBertConfig(vocab_size=len(VOCAB), max_position_embeddings=cfg["max_pos"], n_layers=cfg["n_layers"],
                              n_heads=cfg["n_heads"], dim=cfg["dim"], hidden_dim=cfg["hidden"], dropout=0.1, attention_dropout=0.1,
                              activation="gelu", pad_token_id=PAD)
    model = DistilBertModel(hf_cfg)
    model.load_state_dict(weights(cfg_name, trained))
    model.save_pretrained(path)
    return path


class WordTokenizer:
    """The slice of HF's tokenizer interface BERT.tokenize uses -- tokenizer(texts, return_tensors="pt", padding=True) -> input_ids,
    attention_mask -- over the 64-entry vocabulary, one id per whitespace-separated word: for the tests that hand over y['text']
    where the transformers package may be absent."""

    def __call__(self, texts, return_tensors="pt", padding=True):
        assert return_tensors == "pt" and padding
        texts = [texts] if isinstance(texts, str) else list(texts)
        rows = [[CLS] + [VOCAB.index(w) if w in VOCAB else 1 for w in t.lower().split()] + [SEP] for t in texts]
        L = max(len(r) for r in rows)
        ids = torch.tensor([r + [PAD] * (L - len(r)) for r in rows], dtype=torch.int64)
        mask = torch.tensor([[1] * len(r) + [0] * (L - len(r)) for r in rows], dtype=torch.int64)
        return {"input_ids": ids, "attention_mask": mask}
