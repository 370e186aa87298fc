"""csrc/clip_text.h (mdm_clip_text_encode behind mdm_amd/clip_text.py) on the CPU wave emulator of tests/emu, at the reduced width:
the two reduced fixtures and five padded lengths around the key-tile edges against the fp64 restatement, and the invariance of a
prompt's row bit for bit.

Bound: the accuracy condition of the GPU test -- max-abs error against fp64 <= 4 x e_ref, e_ref being HF's own fp32 error pooled
over the cases of the same (config, regime) (tests/golden/PIN_REPORT_clip_text.json)."""
import numpy as np
import pytest
import torch

from emu.emu_lib import emu
import clip_text_helpers as ch


@pytest.fixture(scope="module")
def clip():
    return ch.make_clip("reduced", True, "cpu", native_lib=emu())


def _encode(clip, tokens):
    return clip.encode_text(torch.from_numpy(np.asarray(tokens)))


@pytest.mark.parametrize("name", ["reduced_default", "reduced_trained"])
def test_emulated_fixture_matches_fp64(name):
    f, g = ch.FIXTURES[name], ch.load_fixture(name)
    got = _encode(ch.make_clip("reduced", f["trained"], "cpu", native_lib=emu()), g["tokens"])
    ch.check(name, "reduced", f["trained"], got, g["fp64"])


@pytest.mark.parametrize("L", [1, 32, 33, 65, 77])
def test_emulated_key_tile_edges(clip, L):
    tokens = ch.sweep_inputs(f"keytile_L{L}")
    ch.check(f"keytile_L{L}", "reduced", True, _encode(clip, tokens), ch.encode_text_fp64(ch.weights("reduced", True), tokens, 2))


def test_a_prompt_gives_the_same_bits_alone_in_any_batch_and_whatever_follows_its_eot(clip):
    """The length-9 prompt of the fixture: alone at L = 9, as row 1 of the fixture (L = 77, the batch's longest prompt has 22 ids), as
    rows 0 and 3 of a permuted batch, padded to L = 22 and to L = 77, in a second identical call, and with the ids behind every EOT
    replaced by other ids below EOT.  One id in front of an EOT does change the row."""
    g = ch.load_fixture("reduced_trained")
    tokens = g["tokens"]
    p9 = tokens[1:2, :9]
    alone = _encode(clip, p9)[0]
    fix = _encode(clip, tokens)
    assert torch.equal(fix, _encode(clip, tokens)) and torch.equal(fix[1], alone)
    for row, order in ((0, [1, 0, 2, 3]), (3, [0, 3, 2, 1])):
        assert torch.equal(_encode(clip, tokens[order])[row], alone), row
    for L in (22, 77):               # (the library is handed the longest prompt's length: a neighbour of L ids pads this one to L)
        padded = ch.make_tokens(40 + L, 2, 77, [L, 9])
        padded[1, :9] = p9
        assert torch.equal(_encode(clip, padded)[1], alone), L
    noisy = tokens.copy()
    behind = np.arange(77)[None, :] > tokens.argmax(-1)[:, None]
    noisy[behind] = np.random.RandomState(3).randint(0, ch.EOT, int(behind.sum()))
    assert torch.equal(_encode(clip, noisy), fix)
    changed = tokens.copy()
    changed[1, 4] = (changed[1, 4] + 1) % ch.SOT
    other = _encode(clip, changed)
    assert not torch.equal(other[1], fix[1]) and torch.equal(other[[0, 2, 3]], fix[[0, 2, 3]])


def test_chunked_batches_give_the_rows_of_one_call(clip, monkeypatch):
    import mdm_amd.clip_text as ct
    tokens = ch.sweep_inputs("rows_B9")
    whole = _encode(clip, tokens)
    monkeypatch.setattr(ct, "MAX_ROWS", 7 * 4)                     # chunks of 4 prompts: 4 + 4 + 1
    assert torch.equal(_encode(clip, tokens), whole)
    ch.check("rows_B9", "reduced", True, whole, ch.encode_text_fp64(ch.weights("reduced", True), tokens, 2))
