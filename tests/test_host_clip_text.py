"""Host side of mdm_amd/clip_text.py: the container's state-dict keys, the HF <-> OpenAI key map, exact widening, the tokenizer's
clip.tokenize semantics, the refusals of encode_text and of the C entry points (on the CPU emulation: no kernel is reached), the
ctypes view of the header's structs, and MDM's wiring."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import clip_text_helpers as ch
from helpers import ROOT
from mdm_amd import _native as nat
from mdm_amd import clip_text as ct


@pytest.fixture(scope="module")
def lib():
    from emu.emu_lib import emu
    return emu()


# ---- keys and loading -----------------------------------------------------------------------------------------------------------------
def test_container_keys_are_openai_clip_s_text_side():
    want = ch.state_dict_keys()
    clip = ct.ClipText(49408, 77, 512, 12, 2048, 512)
    got = {k: list(v.shape) for k, v in clip.state_dict().items()}
    assert list(got) == list(want) and got == {k: v["shape"] for k, v in want.items()}
    assert clip.cfg["heads"] == 8 and ct.ClipText(66, 77, 768, 1, 3072, 768).cfg["heads"] == 12      # ViT-L/14's text tower by shape
    assert {k: v["hf"] for k, v in want.items()} == ch.hf_key_map(ch.FULL)


def test_hf_and_openai_key_maps_round_trip():
    sd = ch.weights("reduced", True)
    hf = ct.hf_from_openai(sd)
    want = ch.hf_state_dict(sd, ch.REDUCED)
    assert sorted(hf) == sorted(want) and all(torch.equal(hf[k], want[k]) for k in want)
    back = ct.openai_from_hf(hf)
    assert sorted(back) == sorted(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    from_hf, from_openai = ct.load_clip_text(hf).state_dict(), ct.load_clip_text(sd).state_dict()
    assert list(from_hf) == list(from_openai) and all(torch.equal(from_hf[k], from_openai[k]) for k in from_hf)


def test_the_archive_s_other_entries_are_ignored_and_the_result_is_frozen():
    sd = dict(ch.weights("reduced", False))
    extra = {"visual.proj": torch.ones(4, 4), "visual.conv1.weight": torch.ones(2, 3, 4, 4), "logit_scale": torch.tensor(4.6),
             "input_resolution": torch.tensor(224), "context_length": torch.tensor(77), "vocab_size": torch.tensor(ch.VOCAB)}
    clip = ct.load_clip_text({**extra, **sd})
    assert list(clip.state_dict()) == [k for k, _ in ch.state_dict_shapes(ch.REDUCED)]
    assert not clip.training and not any(p.requires_grad for p in clip.parameters())
    assert clip.cfg == dict(vocab=ch.VOCAB, positions=77, width=128, heads=2, layers=2, mlp=256, embed=64)
    with pytest.raises(nat.MdmError, match="no eager PyTorch forward"):
        clip(torch.zeros(1, 3, dtype=torch.int64))
    missing = {k: v for k, v in sd.items() if k != "ln_final.bias"}
    with pytest.raises(RuntimeError, match="ln_final.bias"):
        ct.load_clip_text(missing)


def test_fp16_weights_load_to_exactly_their_widened_values(tmp_path):
    sd16 = {k: v.half() for k, v in ch.weights("reduced", True).items()}
    got = ct.load_clip_text(sd16).state_dict()
    assert all(got[k].dtype == torch.float32 and torch.equal(got[k], sd16[k].float()) for k in sd16)
    path = str(tmp_path / "clip_text.pt")
    torch.save(sd16, path)                                         # a .pt file holding an OpenAI state dict
    from_file = ct.load_clip_text(path, tokenizer=ch.StubBpe()).state_dict()
    assert all(torch.equal(from_file[k], got[k]) for k in got)
    with pytest.raises(ValueError, match="would be rounded"):
        ct.load_clip_text({k: v.double() for k, v in sd16.items()})


def test_prepared_tables_are_rebuilt_when_a_parameter_changes():
    clip = ch.make_clip("reduced", True, "cpu")
    first = clip._model()
    assert clip._model() is first
    with torch.no_grad():
        clip.ln_final.bias.add_(1.0)
    assert clip._model() is not first


# ---- the tokenizer --------------------------------------------------------------------------------------------------------------------
def test_tokenize_has_clip_tokenize_s_semantics():
    bpe = ch.StubBpe()
    got = ct.tokenize(bpe, ["w3 w14 w15", "w9", ""], context_length=8)
    assert got.dtype == torch.int32 and got.tolist() == [[64, 3, 14, 15, 65, 0, 0, 0], [64, 9, 65, 0, 0, 0, 0, 0], [64, 65, 0, 0, 0, 0, 0, 0]]
    assert ct.tokenize(bpe, "w1 w2").shape == (1, 77)                                # one string, the default context
    long = " ".join(f"w{i}" for i in range(30))
    cut = ct.tokenize(bpe, [long], context_length=22, truncate=True)[0].tolist()
    assert cut == [64] + list(range(20)) + [65]                                      # cut, and the last id becomes EOT
    with pytest.raises(RuntimeError, match="too long for context length 22"):
        ct.tokenize(bpe, [long], context_length=22)
    exact = " ".join(f"w{i}" for i in range(20))                                     # 22 ids with SOT and EOT: fits as it is
    assert ct.tokenize(bpe, [exact], context_length=22)[0].tolist() == cut
    texts = ["w5 w6 w7", long]
    t22, t77 = ct.tokenize(bpe, texts, 22, truncate=True), ct.tokenize(bpe, texts, 77, truncate=True)
    assert torch.equal(t77[0, :22], t22[0]) and not bool(t77[0, 22:].any())          # a short prompt: trailing zeros only
    clip = ch.make_clip("reduced", False, "cpu")
    assert torch.equal(clip.tokenize(texts, context_length=22, truncate=True), t22)
    clip.tokenizer = None
    with pytest.raises(RuntimeError, match="no tokenizer"):
        clip.tokenize(texts)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_encode_text_refuses_what_the_kernels_do_not_take(lib):
    clip = ch.make_clip("reduced", False, "cpu", native_lib=lib)
    tokens = torch.from_numpy(ch.make_tokens(1, 2, 8, [8, 5]))
    bad = tokens.clone()
    bad[0, 3] = ch.VOCAB
    with pytest.raises(ValueError, match="vocabulary"):
        clip.encode_text(bad)
    bad[0, 3] = -1
    with pytest.raises(ValueError, match="vocabulary"):
        clip.encode_text(bad)
    with pytest.raises(ValueError, match="positional table has 77 rows"):
        clip.encode_text(torch.from_numpy(ch.make_tokens(1, 1, 78, [78])))
    with pytest.raises(ValueError, match="empty batch"):
        clip.encode_text(torch.zeros(0, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="integer ids"):
        clip.encode_text(tokens.float())
    with pytest.raises(ValueError, match="integer ids"):
        clip.encode_text(tokens[0])
    with pytest.raises(ValueError, match="heads of 64"):
        ct.ClipText(66, 77, 96, 1, 256, 64)
    product = ch.make_clip("reduced", False, "cpu")                # the product library takes device parameters only
    if os.path.isfile(nat.LIB_PATH):
        with pytest.raises(nat.MdmError, match="cuda"):
            product.encode_text(tokens)


def _call(lib, model, B, L, ws_bytes=None, out=None, ids=True):
    tokens = np.zeros((B, max(L, 1)), np.int32)
    lens = np.ones(B, np.int32)
    need = lib.mdm_clip_text_workspace_bytes(C.byref(model), B, L)
    ws = np.zeros(max(need, 64) // 4 + 4, np.float32)
    out = np.zeros((max(B, 1), model.embed), np.float32) if out is None else out
    rc = lib.mdm_clip_text_encode(C.byref(model), tokens.ctypes.data if ids else None, lens.ctypes.data, out.ctypes.data, B, L,
                                  ws.ctypes.data, need if ws_bytes is None else ws_bytes, None)
    return need, rc, lib.mdm_last_error().decode()


def test_entry_points_validate_and_name_the_field(lib):
    model = ch.make_clip("reduced", True, "cpu", native_lib=lib)._model()

    def variant(**over):
        m = nat.MdmClipTextModel()
        C.memmove(C.byref(m), C.byref(model), C.sizeof(m))
        for k, v in over.items():
            setattr(m, k, v)
        return m

    floats = 2 * 5 * (6 * 128 + 256) + 2 * 128
    need, rc, _ = _call(lib, model, 2, 5)
    assert rc == 0 and need == floats * 4 + 64
    for m, B, L, code, word in [(model, 2, 129, -5, "L must be at most 128"), (model, 2, 78, -1, "L exceeds max_pos"),
                                (model, 0, 5, -1, "B must be at least 1"), (model, 2, 0, -1, "L must be at least 1"),
                                (variant(n_heads=3), 2, 5, -5, "dim must equal 64 * n_heads"),
                                (variant(dim=2048, n_heads=32), 2, 5, -5, "dim must be at most 1024"),
                                (variant(mlp=254), 2, 5, -5, "mlp"), (variant(embed=62), 2, 5, -5, "embed"),
                                (variant(tok_emb=None), 2, 5, -1, "null weight pointer tok_emb"),
                                (variant(text_proj=model.text_proj + 4), 2, 5, -1, "text_proj must be 16-byte aligned"),
                                (variant(layers=None), 2, 5, -1, "null layers"), (variant(n_layers=33), 2, 5, -5, "n_layers"),
                                (model, 1 << 20, 77, -5, "chunk the prompts")]:
        need, rc, msg = _call(lib, m, B, L)
        assert need == 0 and rc == code and word in msg, (B, L, need, rc, msg)
    assert lib.mdm_clip_text_workspace_bytes(None, 2, 5) == 0 and "null model" in lib.mdm_last_error().decode()
    layers = (nat.MdmClipTextLayer * 2)(model.layers[0], model.layers[1])
    layers[1].proj_b = layers[1].proj_b + 8
    need, rc, msg = _call(lib, variant(layers=layers), 2, 5)
    assert need == 0 and rc == -1 and "layers[1].proj_b" in msg and "aligned" in msg, msg
    need, rc, msg = _call(lib, model, 2, 5, ws_bytes=floats * 4)
    assert rc == -3 and "workspace_bytes" in msg, msg
    out = np.zeros(2 * 64 + 4, np.float32)
    _, rc, msg = _call(lib, model, 2, 5, out=out[1:])
    assert rc == -1 and "out_dev" in msg, msg
    _, rc, msg = _call(lib, model, 2, 5, ids=False)
    assert rc == -1 and "null ids_dev" in msg, msg


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def _header_struct(name):
    """[(member, 'ptr' | 'i32')] of `typedef struct <name> { ... }` in include/mdm_hip.h."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdm_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct " + name + r" \{(.*?)\}", src, flags=re.S).group(1)
    members = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const \w+\*|int32_t)\s+(.*)", decl, flags=re.S)
        members += [(n.strip(), "ptr" if m.group(1).endswith("*") else "i32") for n in m.group(2).split(",")]
    return members


@pytest.mark.parametrize("name, view", [("mdm_clip_text_layer", nat.MdmClipTextLayer), ("mdm_clip_text_model", nat.MdmClipTextModel)])
def test_ctypes_structs_match_the_header(name, view):
    members = _header_struct(name)
    assert [n for n, _ in members] == [n for n, _ in view._fields_]
    for (n, kind), (_, t) in zip(members, view._fields_):
        assert C.sizeof(t) == (8 if kind == "ptr" else 4), n
    raw = sum(8 if kind == "ptr" else 4 for _, kind in members)            # pointers first, then the int32s: padded to 8 at the end
    assert C.sizeof(view) == (raw + 7) // 8 * 8


def test_abi_version_stays_10_and_the_exports_are_declared(lib):
    assert lib.mdm_abi_version() == 10
    assert {"mdm_clip_text_workspace_bytes", "mdm_clip_text_encode"} <= set(nat.EXPORTED_SYMBOLS)


# ---- MDM's wiring ---------------------------------------------------------------------------------------------------------------------
def _mdm(**kargs):
    from mdm_amd import model_util
    args = model_util.default_args(layers=1, latent_dim=256)
    model, _ = model_util.create_model_and_diffusion(args, num_heads=4, ff_size=256, **kargs)
    return model


def test_mdm_attaches_a_clip_text_from_clip_model_path(tmp_path, lib):
    path = str(tmp_path / "clip_text.pt")
    torch.save(dict(ch.weights("reduced", True)), path)
    model = _mdm(clip_model_path=path, clip_dim=64)
    assert isinstance(model.clip_model, ct.ClipText) and not any(p.requires_grad for p in model.clip_model.parameters())
    names = {n for n, _ in model.named_parameters()}
    assert "clip_model.positional_embedding" in names and len(model.parameters_wo_clip()) == sum(not n.startswith("clip_model.") for n in names)
    # prompts through MDM.encode_text on the CPU emulation: context 22 (humanml), truncated, [1, B, embed]
    model.clip_model.tokenizer, model.clip_model._native_lib = ch.StubBpe(), lib
    texts = ["w3 w14 w15 w9", " ".join(f"w{i % 64}" for i in range(40))]
    got = model.encode_text(texts)
    tokens = ct.tokenize(ch.StubBpe(), texts, context_length=22, truncate=True)
    assert tuple(got.shape) == (1, 2, 64) and got.dtype == torch.float32
    ch.check("MDM.encode_text", "reduced", True, got[0], ch.encode_text_fp64(ch.weights("reduced", True), tokens.numpy(), 2))


def test_mdm_without_a_clip_path_behaves_as_before():
    model = _mdm()
    if model.clip_model is None:                                   # (no `clip` package here: the standing refusal)
        with pytest.raises(RuntimeError, match="CLIP is not available"):
            model.encode_text(["a person walks"])
    else:
        assert not isinstance(model.clip_model, ct.ClipText)
