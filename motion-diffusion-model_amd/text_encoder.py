"""The DistilBERT text encoder of the `text_encoder_type='bert'` checkpoints on the HIP path: `load_bert` / `BERT` of
model/BERT/BERT_encoder.py (the memory of the trans_dec / DiP denoisers is DistilBERT's last_hidden_state of the prompts,
model/mdm.py:180-187).

`BERT.text_model` is a parameter container under HF DistilBertModel's own state-dict keys -- so `clip_model.text_model.*` of a
state dict written by the reference loads as it is -- and the arithmetic is csrc/text_encoder.h behind include/mdm_hip.h's
mdm_text_encode (exact fp32; no eager PyTorch forward, and no fall-back when the library is missing).  The tokenizer stays HF's, on
the host, read from a local directory only: nothing here reads an environment variable or opens a network connection."""
import torch
import torch.nn as nn

from . import _native as nat
from ._native_model import NativeModelMixin, _ParamContainer

MAX_WORD_PIECES = 128      # include/mdm_hip.h mdm_text_encode
HEAD_DIM = 64
LN_EPS = 1e-12             # DistilBERT's LayerNorm eps (HF configuration_distilbert / modeling_distilbert)

_LAYER_LINEARS = ("attention.q_lin", "attention.k_lin", "attention.v_lin", "attention.out_lin")


def distilbert_shapes(vocab, max_pos, dim, hidden, n_layers):
    """HF DistilBertModel's state dict, in its order."""
    s = [("embeddings.word_embeddings.weight", (vocab, dim)), ("embeddings.position_embeddings.weight", (max_pos, dim)),
         ("embeddings.LayerNorm.weight", (dim,)), ("embeddings.LayerNorm.bias", (dim,))]
    for n in range(n_layers):
        p = f"transformer.layer.{n}."
        for lin in _LAYER_LINEARS:
            s += [(p + lin + ".weight", (dim, dim)), (p + lin + ".bias", (dim,))]
        s += [(p + "sa_layer_norm.weight", (dim,)), (p + "sa_layer_norm.bias", (dim,)),
              (p + "ffn.lin1.weight", (hidden, dim)), (p + "ffn.lin1.bias", (hidden,)),
              (p + "ffn.lin2.weight", (dim, hidden)), (p + "ffn.lin2.bias", (dim,)),
              (p + "output_layer_norm.weight", (dim,)), (p + "output_layer_norm.bias", (dim,))]
    return s


class TextModel(_ParamContainer):
    """Parameters under DistilBertModel's state-dict keys and nothing else; there is no forward (BERT.encode_ids runs the HIP path)."""

    @property
    def device(self):
        return self.embeddings.word_embeddings.weight.device

    def forward(self, *a, **k):
        raise nat.MdmError("the text encoder's text_model is a parameter container: call BERT.forward / BERT.encode_ids (the HIP "
                           "path); there is no eager PyTorch forward")


def load_bert(model_path, _native_lib=None):
    """BERT_encoder.py:4-10."""
    bert = BERT(model_path, _native_lib=_native_lib)
    bert.eval()
    for p in bert.parameters():
        p.requires_grad = False
    return bert


class BERT(NativeModelMixin, nn.Module):
    """BERT_encoder.py:12-32: `.tokenizer`, `.text_model`, forward(texts) -> (last_hidden_state [B, L, dim] fp32, mask [B, L] bool)."""

    def __init__(self, modelpath=None, _native_lib=None):
        super().__init__()
        self._native_lib = _native_lib
        self.tokenizer = None
        self._ws = {}
        if modelpath is not None:
            self._init_from_dir(modelpath)

    # ---- constructors ---------------------------------------------------------------------------------------------------------
    def _init_from_dir(self, path):
        from transformers import AutoModel, AutoTokenizer      # lazily: only this constructor needs the package
        self.tokenizer = AutoTokenizer.from_pretrained(path, local_files_only=True)
        hf = AutoModel.from_pretrained(path, local_files_only=True)
        sd = {k: v.detach().float() for k, v in hf.state_dict().items()}
        n_heads = int(getattr(hf.config, "n_heads", 0)) or None
        del hf
        self._init_from_state_dict(sd, n_heads)

    def _init_from_state_dict(self, sd, n_heads):
        sd = {k: v for k, v in sd.items() if k != "embeddings.position_ids"}      # (a buffer older HF versions saved)
        try:
            vocab, dim = sd["embeddings.word_embeddings.weight"].shape
            max_pos = sd["embeddings.position_embeddings.weight"].shape[0]
            hidden = sd["transformer.layer.0.ffn.lin1.weight"].shape[0]
        except KeyError as e:
            raise ValueError(f"not a DistilBertModel state dict: {e.args[0]} is missing") from None
        n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.layer."))
        n_heads = int(n_heads) if n_heads is not None else dim // HEAD_DIM
        if dim != HEAD_DIM * n_heads or dim > 1024:
            raise ValueError(f"dim = {dim}, n_heads = {n_heads}: the attention kernel takes heads of {HEAD_DIM} (dim = 64 n_heads <= 1024)")
        if hidden % 4 or not 1 <= n_layers <= 16:
            raise ValueError(f"hidden = {hidden} (a multiple of 4) / n_layers = {n_layers} (1 to 16)")
        self.cfg = dict(vocab=int(vocab), max_pos=int(max_pos), dim=int(dim), hidden=int(hidden), n_layers=n_layers, n_heads=n_heads)
        self.text_model = TextModel(distilbert_shapes(vocab, max_pos, dim, hidden, n_layers))
        self.text_model.load_state_dict(sd)

    @classmethod
    def from_state_dict(cls, sd, tokenizer=None, n_heads=None, _native_lib=None):
        """The encoder over a DistilBertModel state dict (n_heads: dim // 64 when not given); `tokenizer` is any callable with HF's
        tokenizer interface, or None when only encode_ids is used."""
        self = cls(None, _native_lib=_native_lib)
        self.tokenizer = tokenizer
        self._init_from_state_dict({k: torch.as_tensor(v).detach().float() for k, v in sd.items()}, n_heads)
        self.eval()
        return self

    @classmethod
    def from_pretrained_dir(cls, path, _native_lib=None):
        """Tokenizer and weights from a local HF model directory (e.g. a copy of distilbert-base-uncased)."""
        return load_bert(path, _native_lib=_native_lib)

    # ---- native model ----------------------------------------------------------------------------------------------------------
    def _native_version(self):
        return self.text_model.version()

    def _build_native(self, keep):
        """The prepared weight tables (q | k | v stacked, 1/8 folded into the q rows -- a power of two: no bit changes) and the C
        structs over them."""
        sd = {k: v.detach().float() for k, v in self.text_model.state_dict().items()}
        c = self.cfg

        def own(t):          # own storage: 16-byte aligned, unaffected by later loads
            t = t.contiguous().clone()
            keep.append(t)
            return t.data_ptr()

        layers = (nat.MdmTextLayer * c["n_layers"])()
        for n in range(c["n_layers"]):
            p = f"transformer.layer.{n}."
            qkv_w = torch.cat([sd[p + "attention.q_lin.weight"] * 0.125, sd[p + "attention.k_lin.weight"], sd[p + "attention.v_lin.weight"]], 0)
            qkv_b = torch.cat([sd[p + "attention.q_lin.bias"] * 0.125, sd[p + "attention.k_lin.bias"], sd[p + "attention.v_lin.bias"]], 0)
            layers[n] = nat.MdmTextLayer(
                qkv_w=own(qkv_w), qkv_b=own(qkv_b), out_w=own(sd[p + "attention.out_lin.weight"]), out_b=own(sd[p + "attention.out_lin.bias"]),
                sa_ln_g=own(sd[p + "sa_layer_norm.weight"]), sa_ln_b=own(sd[p + "sa_layer_norm.bias"]),
                lin1_w=own(sd[p + "ffn.lin1.weight"]), lin1_b=own(sd[p + "ffn.lin1.bias"]),
                lin2_w=own(sd[p + "ffn.lin2.weight"]), lin2_b=own(sd[p + "ffn.lin2.bias"]),
                out_ln_g=own(sd[p + "output_layer_norm.weight"]), out_ln_b=own(sd[p + "output_layer_norm.bias"]))
        keep.append(layers)
        return nat.MdmTextModel(
            word_emb=own(sd["embeddings.word_embeddings.weight"]), pos_emb=own(sd["embeddings.position_embeddings.weight"]),
            emb_ln_g=own(sd["embeddings.LayerNorm.weight"]), emb_ln_b=own(sd["embeddings.LayerNorm.bias"]), layers=layers,
            n_layers=c["n_layers"], dim=c["dim"], n_heads=c["n_heads"], hidden=c["hidden"], vocab=c["vocab"], max_pos=c["max_pos"],
            ln_eps=LN_EPS)

    # ---- the encoder -----------------------------------------------------------------------------------------------------------
    def check_ids(self, input_ids, attention_mask):
        """Host-side refusals of encode_ids -> (ids [B, L] int64 on the host, lens list)."""
        if input_ids.dim() != 2 or tuple(attention_mask.shape) != tuple(input_ids.shape):
            raise ValueError(f"input_ids and attention_mask must be [B, L]; got {tuple(input_ids.shape)} and {tuple(attention_mask.shape)}")
        B, L = input_ids.shape
        if B < 1 or L < 1:
            raise ValueError("empty batch of prompts")
        if L > MAX_WORD_PIECES:
            raise ValueError(f"prompt longer than 128 word pieces ({L}): the text encoder's attention kernel keeps 128 keys")
        if L > self.cfg["max_pos"]:
            raise ValueError(f"prompt of {L} word pieces: the position table has {self.cfg['max_pos']} rows")
        ids = input_ids.detach().to("cpu", torch.int64)
        mask = attention_mask.detach().to("cpu").to(torch.bool)
        lens = mask.sum(dim=1)
        if not bool((mask == (torch.arange(L)[None, :] < lens[:, None])).all()) or int(lens.min()) < 1:
            raise ValueError("attention_mask must be a suffix mask (right-padded prompts) with at least one token per prompt")
        valid = ids[mask]
        if int(valid.min()) < 0 or int(valid.max()) >= self.cfg["vocab"]:
            raise ValueError(f"token id outside the vocabulary of {self.cfg['vocab']} entries")
        return ids, lens

    def encode_ids(self, input_ids, attention_mask, token_major=False):
        """input_ids, attention_mask [B, L] (what HF's tokenizer returns with padding=True) -> last_hidden_state [B, L, dim] fp32, or
        [L, B, dim] with token_major (the decoder's memory layout), on the parameters' device.  Rows behind a prompt's end are zeros."""
        ids, lens = self.check_ids(input_ids, attention_mask)
        B, L = ids.shape
        lib, model = self._lib(), self._model()
        dev = self.text_model.device
        stream = self._stream(lib, dev, "the text encoder's parameters")
        ids_dev = ids.to(torch.int32).contiguous().to(dev)
        lens_dev = lens.to(torch.int32).contiguous().to(dev)
        D = self.cfg["dim"]
        out = torch.empty((L, B, D) if token_major else (B, L, D), dtype=torch.float32, device=dev)
        ws, nbytes = self._workspace("mdm_text_workspace_bytes", model, B, L, dev=dev, stream=stream, cache=True)
        lib.check(lib.mdm_text_encode(nat.C.byref(model), ids_dev.data_ptr(), lens_dev.data_ptr(), out.data_ptr(), B, L, int(bool(token_major)),
                                      ws.data_ptr(), nbytes, stream), "mdm_text_encode")
        return out

    def tokenize(self, texts):
        """BERT_encoder.py:28 -> (input_ids, attention_mask), on the host."""
        if self.tokenizer is None:
            raise RuntimeError("this BERT has no tokenizer (built from a state dict): call encode_ids, or pass tokenizer=")
        enc = self.tokenizer(texts, return_tensors="pt", padding=True)
        return enc["input_ids"], enc["attention_mask"]

    def forward(self, texts):
        input_ids, attention_mask = self.tokenize(texts)
        out = self.encode_ids(input_ids, attention_mask)
        return out, attention_mask.to(device=out.device, dtype=torch.bool)
