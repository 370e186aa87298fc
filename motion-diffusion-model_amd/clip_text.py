"""The text tower of OpenAI CLIP on the HIP path: what `clip.load(...)[0].encode_text(clip.tokenize(texts))` gives the
`text_encoder_type='clip'` checkpoints (model/mdm.py:163-178), without the `clip` package.

`ClipText` is a parameter container under OpenAI's own state-dict keys, text side only -- so the text entries of the published
archive, or `clip_model.*` of a state dict written by the reference, load as they are -- and the arithmetic is csrc/clip_text.h behind
include/mdm_hip.h's mdm_clip_text_encode (exact fp32; no eager PyTorch forward, and no fall-back when the library is missing).  The
published weights are fp16-valued; they are widened to fp32, never rounded, so this path sees upstream's values.  The tokenizer stays
on the host, over any byte-pair encoder with `.encode(text) -> list[int]`, `.sot` and `.eot`; nothing here reads an environment
variable or opens a network connection."""
import os

import torch

from . import _native as nat
from ._native_model import NativeModelMixin, _ParamContainer

HEAD_DIM = 64
MAX_TOKENS = 128           # include/mdm_hip.h mdm_clip_text_encode
MAX_ROWS = 16384           # token rows (B L) per library call: 335 MB of workspace at ViT-B/32's widths
_EXACT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)       # every value of these is an fp32 value

_BLOCK = (("attn.in_proj_weight", "3w,w"), ("attn.in_proj_bias", "3w"), ("attn.out_proj.weight", "w,w"), ("attn.out_proj.bias", "w"),
          ("ln_1.weight", "w"), ("ln_1.bias", "w"), ("mlp.c_fc.weight", "m,w"), ("mlp.c_fc.bias", "m"),
          ("mlp.c_proj.weight", "w,m"), ("mlp.c_proj.bias", "w"), ("ln_2.weight", "w"), ("ln_2.bias", "w"))
# HF CLIPTextModelWithProjection's name of each one-to-one entry of a residual block (q | k | v are stacked into attn.in_proj_*)
_HF_BLOCK = {"attn.out_proj": "self_attn.out_proj", "ln_1": "layer_norm1", "mlp.c_fc": "mlp.fc1", "mlp.c_proj": "mlp.fc2",
             "ln_2": "layer_norm2"}


def clip_text_shapes(vocab, positions, width, layers, mlp, embed):
    """The text side of OpenAI CLIP's state dict (clip/model.py CLIP), in its order."""
    dims = {"w": width, "3w": 3 * width, "m": mlp}
    s = [("positional_embedding", (positions, width)), ("text_projection", (width, embed))]
    for n in range(layers):
        s += [(f"transformer.resblocks.{n}.{k}", tuple(dims[d] for d in shape.split(","))) for k, shape in _BLOCK]
    return s + [("token_embedding.weight", (vocab, width)), ("ln_final.weight", (width,)), ("ln_final.bias", (width,))]


def openai_from_hf(sd):
    """An HF CLIPTextModelWithProjection (or CLIPModel) state dict -> OpenAI's text-side keys; everything else is dropped."""
    t = "text_model."
    out = {"token_embedding.weight": sd[t + "embeddings.token_embedding.weight"],
           "positional_embedding": sd[t + "embeddings.position_embedding.weight"],
           "ln_final.weight": sd[t + "final_layer_norm.weight"], "ln_final.bias": sd[t + "final_layer_norm.bias"],
           "text_projection": sd["text_projection.weight"].t()}
    n = 0
    while f"{t}encoder.layers.{n}.layer_norm1.weight" in sd:
        h, o = f"{t}encoder.layers.{n}.", f"transformer.resblocks.{n}."
        for leaf in ("weight", "bias"):
            out[f"{o}attn.in_proj_{leaf}"] = torch.cat([sd[f"{h}self_attn.{p}_proj.{leaf}"] for p in "qkv"], 0)
            for ours, theirs in _HF_BLOCK.items():
                out[f"{o}{ours}.{leaf}"] = sd[f"{h}{theirs}.{leaf}"]
        n += 1
    return out


def hf_from_openai(sd):
    """The inverse of openai_from_hf over a text-side OpenAI state dict (what CLIPTextModelWithProjection.load_state_dict takes)."""
    t = "text_model."
    out = {t + "embeddings.token_embedding.weight": sd["token_embedding.weight"],
           t + "embeddings.position_embedding.weight": sd["positional_embedding"],
           t + "final_layer_norm.weight": sd["ln_final.weight"], t + "final_layer_norm.bias": sd["ln_final.bias"],
           "text_projection.weight": sd["text_projection"].t()}
    n = 0
    while f"transformer.resblocks.{n}.ln_1.weight" in sd:
        h, o = f"{t}encoder.layers.{n}.", f"transformer.resblocks.{n}."
        for leaf in ("weight", "bias"):
            for p, part in zip("qkv", torch.chunk(sd[f"{o}attn.in_proj_{leaf}"], 3, 0)):
                out[f"{h}self_attn.{p}_proj.{leaf}"] = part
            for ours, theirs in _HF_BLOCK.items():
                out[f"{h}{theirs}.{leaf}"] = sd[f"{o}{ours}.{leaf}"]
        n += 1
    return out


# ---- the tokenizer ------------------------------------------------------------------------------------------------------------------
def tokenize(bpe, texts, context_length=77, truncate=False):
    """clip.tokenize over `bpe` (.encode(text) -> list[int], .sot, .eot): [SOT] + bpe(text) + [EOT], zero-padded -> [B, context_length]
    int32 on the host.  Too long: cut with the last id made EOT when `truncate`, RuntimeError otherwise."""
    texts = [texts] if isinstance(texts, str) else list(texts)
    result = torch.zeros(len(texts), context_length, dtype=torch.int32)
    for i, text in enumerate(texts):
        tokens = [bpe.sot] + list(bpe.encode(text)) + [bpe.eot]
        if len(tokens) > context_length:
            if not truncate:
                raise RuntimeError(f"Input {text} is too long for context length {context_length}")
            tokens = tokens[:context_length]
            tokens[-1] = bpe.eot
        result[i, :len(tokens)] = torch.tensor(tokens, dtype=torch.int32)
    return result


class SimpleTokenizerBpe:
    """clip.simple_tokenizer.SimpleTokenizer (needs the `clip` package and the vocabulary file it ships)."""

    def __init__(self):
        from clip.simple_tokenizer import SimpleTokenizer
        self._tok = SimpleTokenizer()
        self.sot, self.eot = self._tok.encoder["<|startoftext|>"], self._tok.encoder["<|endoftext|>"]

    def encode(self, text):
        return self._tok.encode(text)


class HfClipBpe:
    """HF's CLIPTokenizer read from a LOCAL directory (vocab.json + merges.txt)."""

    def __init__(self, path):
        from transformers import CLIPTokenizer
        self._tok = CLIPTokenizer.from_pretrained(path, local_files_only=True)
        self.sot, self.eot = self._tok.bos_token_id, self._tok.eos_token_id

    def encode(self, text):
        return self._tok.encode(text, add_special_tokens=False)


# ---- the encoder --------------------------------------------------------------------------------------------------------------------
class ClipText(NativeModelMixin, _ParamContainer):
    """Parameters under OpenAI CLIP's text-side state-dict keys; `encode_text(tokens)` runs the HIP path and there is no eager forward."""

    def __init__(self, vocab, positions, width, layers, mlp, embed, tokenizer=None, _native_lib=None):
        heads = width // HEAD_DIM                            # clip/model.py build_model: transformer_heads = transformer_width // 64
        if width != HEAD_DIM * heads or not 64 <= width <= 1024:
            raise ValueError(f"width = {width}: the attention kernel takes heads of {HEAD_DIM} (width = 64 heads <= 1024)")
        if mlp % 4 or embed % 4 or mlp < 4 or embed < 4 or not 1 <= layers <= 32:
            raise ValueError(f"mlp = {mlp}, embed = {embed} (positive multiples of 4) / layers = {layers} (1 to 32)")
        super().__init__(clip_text_shapes(vocab, positions, width, layers, mlp, embed))
        self.cfg = dict(vocab=int(vocab), positions=int(positions), width=int(width), heads=heads, layers=int(layers), mlp=int(mlp),
                        embed=int(embed))
        self.tokenizer = tokenizer
        self._native_lib = _native_lib
        self._ws = {}

    @classmethod
    def from_state_dict(cls, sd, tokenizer=None, _native_lib=None):
        """The encoder over an OpenAI state dict (visual.*, logit_scale and the archive's scalar entries are ignored) or an HF one;
        frozen, in eval mode.  Values are widened to fp32 exactly: fp32, fp16 and bfloat16 are taken, anything else is refused."""
        sd = {k: torch.as_tensor(v).detach() for k, v in sd.items()}
        if any(k.startswith("text_model.") for k in sd):
            sd = openai_from_hf(sd)
        try:
            vocab, width = sd["token_embedding.weight"].shape
            positions, embed = sd["positional_embedding"].shape[0], sd["text_projection"].shape[1]
            mlp = sd["transformer.resblocks.0.mlp.c_fc.weight"].shape[0]
        except KeyError as e:
            raise ValueError(f"not a CLIP state dict: {e.args[0]} is missing") from None
        layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.resblocks."))
        self = cls(vocab, positions, width, layers, mlp, embed, tokenizer=tokenizer, _native_lib=_native_lib)
        own = {k: sd[k] for k, _ in self.shapes if k in sd}
        for k, v in own.items():
            if v.dtype not in _EXACT_DTYPES:
                raise ValueError(f"{k} is {v.dtype}: fp32, fp16 or bfloat16 weights widen to fp32 exactly, others would be rounded")
        self.load_state_dict(own)                            # (strict: a missing text-side key is named)
        self.eval()
        for p in self.parameters():
            p.requires_grad = False
        return self

    @property
    def device(self):
        return self.positional_embedding.device

    def forward(self, *a, **k):
        raise nat.MdmError("ClipText is a parameter container: call encode_text(tokens) (the HIP path); there is no eager PyTorch "
                           "forward and no image tower")

    # ---- native model ----------------------------------------------------------------------------------------------------------
    def _native_version(self):
        return self.version()

    def _build_native(self, keep):
        """The prepared tables (1/8 folded into the q rows -- a power of two: no bit changes --, the projection laid out
        [embed, width]) and the C structs over them."""
        sd = {k: v.detach().float() for k, v in self.state_dict().items()}
        c = self.cfg

        def own(t):          # own storage: 16-byte aligned, unaffected by later loads
            t = t.contiguous().clone()
            keep.append(t)
            return t.data_ptr()

        W = c["width"]
        layers = (nat.MdmClipTextLayer * c["layers"])()
        for n in range(c["layers"]):
            p = f"transformer.resblocks.{n}."
            qkv_w, qkv_b = sd[p + "attn.in_proj_weight"].clone(), sd[p + "attn.in_proj_bias"].clone()
            qkv_w[:W] *= 0.125
            qkv_b[:W] *= 0.125
            layers[n] = nat.MdmClipTextLayer(
                ln1_g=own(sd[p + "ln_1.weight"]), ln1_b=own(sd[p + "ln_1.bias"]), qkv_w=own(qkv_w), qkv_b=own(qkv_b),
                out_w=own(sd[p + "attn.out_proj.weight"]), out_b=own(sd[p + "attn.out_proj.bias"]),
                ln2_g=own(sd[p + "ln_2.weight"]), ln2_b=own(sd[p + "ln_2.bias"]),
                fc_w=own(sd[p + "mlp.c_fc.weight"]), fc_b=own(sd[p + "mlp.c_fc.bias"]),
                proj_w=own(sd[p + "mlp.c_proj.weight"]), proj_b=own(sd[p + "mlp.c_proj.bias"]))
        keep.append(layers)
        return nat.MdmClipTextModel(
            tok_emb=own(sd["token_embedding.weight"]), pos_emb=own(sd["positional_embedding"]), lnf_g=own(sd["ln_final.weight"]),
            lnf_b=own(sd["ln_final.bias"]), text_proj=own(sd["text_projection"].t()), layers=layers, n_layers=c["layers"], dim=W,
            n_heads=c["heads"], mlp=c["mlp"], vocab=c["vocab"], max_pos=c["positions"], embed=c["embed"])

    # ---- the encoder -----------------------------------------------------------------------------------------------------------
    def check_tokens(self, tokens):
        """Host-side refusals of encode_text -> (ids [B, max len] int32 on the host, lens [B] int32): len_b = argmax(ids[b]) + 1, the
        first occurrence of the row's maximum, upstream's rule for the EOT (the highest id of the vocabulary)."""
        tokens = torch.as_tensor(tokens)
        if tokens.dim() != 2 or tokens.is_floating_point() or tokens.dtype == torch.bool:
            raise ValueError(f"tokens must be [B, L] integer ids; got {tuple(tokens.shape)} {tokens.dtype}")
        B, L = tokens.shape
        if B < 1 or L < 1:
            raise ValueError("empty batch of prompts")
        if L > self.cfg["positions"]:
            raise ValueError(f"prompts of {L} tokens: the positional table has {self.cfg['positions']} rows")
        ids = tokens.detach().to("cpu", torch.int64)
        if int(ids.min()) < 0 or int(ids.max()) >= self.cfg["vocab"]:
            raise ValueError(f"token id outside the vocabulary of {self.cfg['vocab']} entries")
        lens = ids.argmax(dim=1) + 1
        if int(lens.max()) > MAX_TOKENS:
            raise ValueError(f"prompt longer than {MAX_TOKENS} tokens ({int(lens.max())}): the attention kernel keeps {MAX_TOKENS} keys")
        return ids[:, :int(lens.max())].to(torch.int32).contiguous(), lens.to(torch.int32)

    def encode_text(self, tokens):
        """tokens [B, L] integer ids as clip.tokenize makes them (zero behind each EOT), on the host or on a device -> text_embed
        [B, embed] fp32 on the parameters' device.  The library sees the rows up to the longest prompt's EOT and no further; a prompt's
        row does not depend on the batch, so batches beyond MAX_ROWS token rows go in chunks."""
        ids, lens = self.check_tokens(tokens)
        B, L = ids.shape
        lib, model = self._lib(), self._model()
        dev = self.device
        stream = self._stream(lib, dev, "the CLIP text encoder's parameters")
        ids_dev, lens_dev = ids.to(dev), lens.to(dev)
        out = torch.empty((B, self.cfg["embed"]), dtype=torch.float32, device=dev)
        step = max(1, MAX_ROWS // L)
        for b0 in range(0, B, step):
            n = min(step, B - b0)
            ws, nbytes = self._workspace("mdm_clip_text_workspace_bytes", model, n, L, dev=dev, stream=stream, cache=True)
            lib.check(lib.mdm_clip_text_encode(nat.C.byref(model), ids_dev[b0:b0 + n].data_ptr(), lens_dev[b0:b0 + n].data_ptr(),
                                               out[b0:b0 + n].data_ptr(), n, L, ws.data_ptr(), nbytes, stream), "mdm_clip_text_encode")
        return out

    def tokenize(self, texts, context_length=77, truncate=False):
        if self.tokenizer is None:
            raise RuntimeError("this ClipText has no tokenizer: pass tokenizer= (SimpleTokenizerBpe(), HfClipBpe(dir) or any object "
                               "with .encode, .sot and .eot), or call encode_text with token ids")
        return tokenize(self.tokenizer, texts, context_length=context_length, truncate=truncate)


def load_clip_text(source, tokenizer=None, _native_lib=None):
    """`source`: an OpenAI or HF state dict; a .pt file holding an OpenAI one; the published TorchScript archive (ViT-B-32.pt); or a
    local HF model directory.  `tokenizer`: see ClipText.tokenize; when None, the directory's own CLIPTokenizer, or for a file the
    `clip` package's SimpleTokenizer where it is importable.  The result is frozen and in eval mode."""
    if isinstance(source, dict):
        return ClipText.from_state_dict(source, tokenizer=tokenizer, _native_lib=_native_lib)
    path = os.fspath(source)
    if os.path.isdir(path):
        from transformers import CLIPTextModelWithProjection      # lazily: only this branch needs the package
        sd = CLIPTextModelWithProjection.from_pretrained(path, local_files_only=True).state_dict()
        if tokenizer is None and os.path.isfile(os.path.join(path, "vocab.json")):
            tokenizer = HfClipBpe(path)
    else:
        try:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        except RuntimeError:                                      # not a pickled state dict: the published TorchScript archive
            sd = torch.jit.load(path, map_location="cpu").state_dict()
        if tokenizer is None:
            try:
                tokenizer = SimpleTokenizerBpe()
            except ImportError:
                pass
    return ClipText.from_state_dict(sd, tokenizer=tokenizer, _native_lib=_native_lib)
