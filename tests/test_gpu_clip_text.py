"""mdm_amd/clip_text.py on the MI355X: the four fixtures of tests/golden/clip_text_*.npz and every sweep case of the pin report (padded
lengths on both sides of each key-tile edge, the GEMMs' row edges, the projection's 64-row edge, one full-width prompt) against
the fp64 restatement; a prompt's row bit for bit alone, in any batch, at any padded length and whatever follows its EOT; poison;
and prompts through a trans_enc sampling loop.

Accuracy condition: max-abs error against fp64 <= 4 x e_ref, e_ref = HF CLIPTextModelWithProjection's own fp32 error pooled as the
maximum over the cases of the same (config, regime) (tests/golden/PIN_REPORT_clip_text.json, written by
tests/make_golden_clip_text.py): a different but equally long summation order and no more.  Every case prints its figure before it
asserts."""
import numpy as np
import pytest
import torch

import clip_text_helpers as ch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CLIPS = {}


def _clip(cfg_name, trained):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    if (cfg_name, trained) not in _CLIPS:
        _CLIPS[cfg_name, trained] = ch.make_clip(cfg_name, trained, DEV)
    return _CLIPS[cfg_name, trained]


def _encode(clip, tokens):
    return clip.encode_text(torch.from_numpy(np.asarray(tokens)))


@pytest.mark.parametrize("name", list(ch.FIXTURES))
def test_fixture_matches_fp64(name):
    f, g = ch.FIXTURES[name], ch.load_fixture(name)
    got = _encode(_clip(f["cfg"], f["trained"]), g["tokens"])
    assert got.device.type == "cuda"
    ch.check("gpu " + name, f["cfg"], f["trained"], got.cpu(), g["fp64"])


@pytest.mark.parametrize("name", list(ch.SWEEP))
def test_sweep_case_matches_fp64(name):
    """keytile_L*: B = 3 with lens [L, max(1, L // 2), 1] on both sides of every 32-key tile edge; rows_B*: 7 to 133 token rows (both
    GEMM tile heights and their edges); proj_B65_L2: 65 rows into the projection; full_B1_L12: one prompt at full width."""
    c = ch.SWEEP[name]
    tokens = ch.sweep_inputs(name)
    want = ch.encode_text_fp64(ch.weights(c["cfg"], True), tokens, ch.CFGS[c["cfg"]]["heads"])
    ch.check("gpu " + name, c["cfg"], True, _encode(_clip(c["cfg"], True), tokens).cpu(), want)


def test_a_prompt_gives_the_same_bits_alone_in_any_batch_and_whatever_follows_its_eot():
    """The length-9 prompt of the full-width fixture: alone at L = 9, as row 1 of the fixture (the library is handed L = 22, the
    longest prompt), as rows 0 and 3 of a permuted batch, beside a prompt of 77 ids (L = 77), and in a second identical call; with
    the ids behind every EOT replaced by other ids below EOT, no bit changes; one id in front of an EOT does change its row."""
    clip, g = _clip("full", True), ch.load_fixture("full_trained")
    tokens = g["tokens"]
    alone = _encode(clip, tokens[1:2, :9])[0]
    fix = _encode(clip, tokens)
    assert torch.equal(fix, _encode(clip, tokens)) and torch.equal(fix[1], alone)
    for row, order in ((0, [1, 0, 2, 3]), (3, [0, 3, 2, 1])):
        assert torch.equal(_encode(clip, tokens[order])[row], alone), row
    for L in (22, 77):               # (a neighbour of L ids pads this prompt to L)
        padded = ch.make_tokens(40 + L, 2, 77, [L, 9])
        padded[1, :9] = tokens[1, :9]
        assert torch.equal(_encode(clip, padded)[1], alone), L
    noisy = tokens.copy()
    behind = np.arange(77)[None, :] > tokens.argmax(-1)[:, None]
    noisy[behind] = np.random.RandomState(3).randint(0, ch.EOT, int(behind.sum()))
    assert torch.equal(_encode(clip, noisy), fix)
    changed = tokens.copy()
    changed[1, 4] = (changed[1, 4] + 1) % ch.SOT
    other = _encode(clip, changed)
    assert not torch.equal(other[1], fix[1]) and torch.equal(other[[0, 2, 3]], fix[[0, 2, 3]])


def test_chunked_batches_give_the_rows_of_one_call(monkeypatch):
    import mdm_amd.clip_text as ct
    clip, tokens = _clip("reduced", True), ch.sweep_inputs("rows_B19")
    whole = _encode(clip, tokens)
    monkeypatch.setattr(ct, "MAX_ROWS", 7 * 5)                     # chunks of 5 prompts: 5 + 5 + 5 + 4
    assert torch.equal(_encode(clip, tokens), whole)


def test_poison_in_workspace_and_output_does_not_reach_the_result(monkeypatch):
    """Workspace and `out` start as NaN: a finite result identical to the clean call."""
    import mdm_amd.clip_text as ct
    clip, g = _clip("full", True), ch.load_fixture("full_trained")
    clean = _encode(clip, g["tokens"])
    real_empty = torch.empty

    def poisoned_empty(*a, **k):
        t = real_empty(*a, **k)
        return t.fill_(0xFF) if t.dtype == torch.uint8 else (t.fill_(float("nan")) if t.is_floating_point() else t)

    monkeypatch.setattr(ct.torch, "empty", poisoned_empty)
    clip._ws = {}                                                   # (the cached workspace of the clean call)
    got = _encode(clip, g["tokens"])
    assert bool(torch.isfinite(got).all()) and torch.equal(got, clean)


# ---- inside a sampling loop ----------------------------------------------------------------------------------------------------------
E2E = dict(ch.FULL, layers=2)                                       # full width, reduced depth
TEXTS = ["w3 w14 w15 w9 w26 w5 w35", "w8", " ".join(f"w{(7 * i) % 64}" for i in range(30))]      # the last one is cut at context 22


def test_prompts_through_a_trans_enc_loop_and_a_side_stream():
    """A one-layer trans_enc text model with this encoder attached: p_sample_loop given y['text'] equals, bit for bit, the loop given
    y['text_embed'] = model.encode_text(texts); and an encode_text on a side stream right behind a loop returns what the default
    stream returns (one chain per device, include/mdm_hip.h CONCURRENCY)."""
    from helpers import make_pair, synth_state_dict, synth_y
    from mdm_amd.clip_text import load_clip_text
    assert torch.cuda.is_available(), "these tests need the MI355X"
    B, T, steps = 3, 40, 2
    model, diffusion = make_pair(synth_state_dict(seed=0, num_layers=1), steps, DEV, guided=False, precision="f16x3")
    model.clip_model = load_clip_text(ch.build_weights(ch.SEED, E2E, True), tokenizer=ch.StubBpe()).to(DEV)
    y = synth_y(B, T, seed=5, lengths=[T, T - 9, T - 20])
    y.pop("text_embed")
    y = {k: v.to(DEV) for k, v in y.items()}
    g = torch.Generator().manual_seed(8)
    seq = [torch.randn(B, 263, 1, T, generator=g).to(DEV) for _ in range(1 + steps)]

    def loop(extra):
        return diffusion.p_sample_loop(model, (B, 263, 1, T), clip_denoised=False, model_kwargs={"y": {**y, **extra}}, noise_sequence=seq)

    enc = model.encode_text(TEXTS)
    assert tuple(enc.shape) == (1, B, 512) and enc.dtype == torch.float32 and bool(torch.isfinite(enc).all())
    from_text = loop({"text": TEXTS})
    from_embed = loop({"text_embed": enc})
    assert bool(torch.isfinite(from_text).all()) and torch.equal(from_text, from_embed)

    tokens = model.clip_model.tokenize(TEXTS, context_length=22, truncate=True)
    assert (tokens.argmax(-1) + 1).tolist() == [9, 3, 22]
    base = model.clip_model.encode_text(tokens)
    assert torch.equal(base, enc[0])
    again = loop({"text": TEXTS})
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = model.clip_model.encode_text(tokens)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(again, from_text) and torch.equal(got, base)
