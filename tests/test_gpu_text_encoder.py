"""mdm_amd/text_encoder.py on the MI355X: the four fixtures of tests/golden/text_encoder_*.npz, every key-tile count of the attention
kernel and the GEMM's row-tile edges against the fp64 restatement, row invariance and poison bit for bit, the token-major layout,
and the encoder inside a trans_dec sampling loop.

Accuracy condition: max-abs error against fp64 over valid rows <= 4 x e_ref, e_ref = the reference's own fp32 error on the same case
(tests/golden/PIN_REPORT_text_encoder.json, from the reference's load_bert run by tests/make_golden_text_encoder.py): a different but
equally long summation order and no more.  Every case prints its figure before it asserts."""
import numpy as np
import pytest
import torch

import text_encoder_helpers as th

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_BERTS = {}


def _bert(cfg_name, trained):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    if (cfg_name, trained) not in _BERTS:
        _BERTS[cfg_name, trained] = th.make_bert(cfg_name, trained, DEV)
    return _BERTS[cfg_name, trained]


def _check(name, got, want, lens):
    got = got.cpu()
    err, bound = th.valid_maxabs(got, want, lens), 4 * th.pin_report()[name]["e_ref"]
    print(f"[text encoder] gpu {name}: max-abs vs fp64 over valid rows = {err:.3e} (bound {bound:.3e}, ratio {err / bound * 4:.2f} e_ref)")
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == torch.float32
    assert err <= bound
    keep = np.arange(got.shape[1])[None, :] < np.asarray(lens)[:, None]
    assert not bool(got[torch.from_numpy(~keep)].any())            # rows at or beyond a length: exactly zero


@pytest.mark.parametrize("name", list(th.FIXTURES))
def test_fixture_matches_fp64(name):
    f, g = th.FIXTURES[name], th.load_fixture(name)
    _check(name, th.encode(_bert(f["cfg"], f["trained"]), g["ids"], g["mask"]), g["fp64"], th.FIXTURE_LENS)


@pytest.mark.parametrize("name", [n for n in th.SWEEP if n.startswith("keytile")])
def test_key_tile_edges(name):
    """L on both sides of every 32-key tile edge, B = 3 with lens [L, max(1, L // 2), 1]; reduced width, trained-like weights."""
    ids, mask, lens = th.sweep_inputs(name)
    _check(name, th.encode(_bert("reduced", True), ids, mask),
           th.encoder_fp64(th.weights("reduced", True), ids, lens, th.REDUCED["n_heads"]), lens)


@pytest.mark.parametrize("name", [n for n in th.SWEEP if n.startswith("rows")] + ["full_B1_L12"])
def test_gemm_row_edges(name):
    """7 to 133 rows at the reduced width (both GEMM tile heights and their edges), and 12 rows at full width."""
    c = th.SWEEP[name]
    ids, mask, lens = th.sweep_inputs(name)
    _check(name, th.encode(_bert(c["cfg"], True), ids, mask),
           th.encoder_fp64(th.weights(c["cfg"], True), ids, lens, th.CFGS[c["cfg"]]["n_heads"]), lens)


def test_a_prompt_gives_the_same_bits_alone_and_in_any_batch():
    """The length-9 prompt of the full-width fixture: alone at L = 9, where the fixture has it (row 1), as row 0 and as row 3 of an
    L = 33 batch, and in an L = 128 batch; and twice the same call.  (A sharded DiP run changes the batch and its padded length.)"""
    bert, g = _bert("full", True), th.load_fixture("full_trained")
    p9 = g["ids"][1, :9]
    alone = th.encode(bert, p9[None], np.ones((1, 9), bool))[0]
    fix = th.encode(bert, g["ids"], g["mask"])
    assert torch.equal(fix, th.encode(bert, g["ids"], g["mask"]))
    assert torch.equal(fix[1, :9], alone)
    for row, order in ((0, [1, 0, 2, 3]), (3, [0, 3, 2, 1])):
        got = th.encode(bert, g["ids"][order], g["mask"][order])
        assert torch.equal(got[row, :9], alone), row
    ids, mask = th.make_ids(77, 2, 128, [128, 9])
    ids[1, :9] = p9
    assert torch.equal(th.encode(bert, ids, mask)[1, :9], alone)


def test_poison_in_workspace_output_and_padding_does_not_reach_the_output(monkeypatch):
    """Workspace and `out` start as NaN, and the ids behind the lengths are other valid ids: all finite, padded rows zero, valid rows
    bit-identical to the clean call."""
    import mdm_amd.text_encoder as te
    bert, g = _bert("full", True), th.load_fixture("full_trained")
    clean = th.encode(bert, g["ids"], g["mask"])
    real_empty = torch.empty

    def poisoned_empty(*a, **k):
        t = real_empty(*a, **k)
        return t.fill_(0xFF) if t.dtype == torch.uint8 else (t.fill_(float("nan")) if t.is_floating_point() else t)

    monkeypatch.setattr(te.torch, "empty", poisoned_empty)
    bert._ws = {}                                                   # (the cached workspace of the clean call)
    ids = g["ids"].copy()
    ids[~g["mask"]] = np.random.RandomState(3).randint(5, len(th.VOCAB), int((~g["mask"]).sum()))
    got = th.encode(bert, ids, g["mask"])
    assert bool(torch.isfinite(got).all())
    assert not bool(got[torch.from_numpy(~g["mask"]).to(DEV)].any())
    assert torch.equal(got, clean)


def test_token_major_is_the_permuted_result():
    bert, g = _bert("full", True), th.load_fixture("full_trained")
    got = th.encode(bert, g["ids"], g["mask"], token_major=True)
    assert tuple(got.shape) == (33, 4, 768)
    assert torch.equal(got, th.encode(bert, g["ids"], g["mask"]).permute(1, 0, 2))


# ---- inside a sampling loop ----------------------------------------------------------------------------------------------------------
E2E = dict(dim=768, n_heads=12, hidden=3072, n_layers=2, max_pos=128)      # full width, reduced depth
TEXTS = ["w3 w14 w15 w9 w26 w5 w35", "w8", "w9 w7 w9 w3 w23 w8 w46 w26 w43 w38 w32"]


def test_prompts_through_a_trans_dec_loop_and_a_side_stream():
    """A one-layer trans_dec model with this encoder attached: p_sample_loop given y['text'] equals, bit for bit, the loop given
    y['text_embed'] = model.encode_text(texts); and an encode_ids on a side stream right behind a loop returns what the default stream
    returns (one chain per device, include/mdm_hip.h CONCURRENCY)."""
    import decoder_helpers as dh
    from mdm_amd.text_encoder import BERT
    assert torch.cuda.is_available(), "these tests need the MI355X"
    B, C, P, steps = 3, 20, 40, 2
    model, diffusion = dh._model(dh._sd("plain", 512, 1024, "bert"), 512, 1024, C, "bert", steps, DEV, None, "f16x3")
    model.clip_model = BERT.from_state_dict(th.build_weights(th.SEED, E2E, True), tokenizer=th.WordTokenizer(), n_heads=12).to(DEV)
    y = dh._y("plain", B, C, P, [9, 3, 13], None, False, "bert", 0)
    y.pop("text_embed")
    y = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in y.items()}
    g = torch.Generator().manual_seed(8)
    seq = [torch.randn(B, 263, 1, P, generator=g).to(DEV) for _ in range(1 + steps)]

    def loop(extra):
        return diffusion.p_sample_loop(model, (B, 263, 1, P), clip_denoised=False, model_kwargs={"y": {**y, **extra}}, noise_sequence=seq)

    enc, pad = model.encode_text(TEXTS)
    assert tuple(enc.shape) == (13, B, 768) and pad.dtype == torch.bool and (~pad).sum(1).tolist() == [9, 3, 13]
    from_text = loop({"text": TEXTS})
    from_embed = loop({"text_embed": (enc, pad)})
    assert bool(torch.isfinite(from_text).all()) and torch.equal(from_text, from_embed)

    ids, mask = model.clip_model.tokenize(TEXTS)
    base = model.clip_model.encode_ids(ids, mask)
    again = loop({"text": TEXTS})
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = model.clip_model.encode_ids(ids, mask)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(again, from_text) and torch.equal(got, base)
