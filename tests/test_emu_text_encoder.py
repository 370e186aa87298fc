"""csrc/text_encoder.h (mdm_text_encode behind mdm_amd/text_encoder.py) on the CPU wave emulator of tests/emu, at the reduced width:
the two reduced fixtures and three key-tile counts against the fp64 restatement, row invariance and poison bit for bit, the
token-major layout, and the entry points' refusals.

Bound: the accuracy condition of the GPU test -- max-abs error against fp64 over valid rows <= 4 x e_ref, e_ref being the
reference's own fp32 error on the same case (tests/golden/PIN_REPORT_text_encoder.json)."""
import ctypes as C

import numpy as np
import pytest
import torch

from emu.emu_lib import emu
import text_encoder_helpers as th
from mdm_amd import _native as nat


@pytest.fixture(scope="module")
def lib():
    return emu()


@pytest.fixture(scope="module")
def bert(lib):
    return th.make_bert("reduced", True, "cpu", native_lib=lib)


def _check(name, got, want, lens):
    err, bound = th.valid_maxabs(got, want, lens), 4 * th.pin_report()[name]["e_ref"]
    print(f"[text encoder] {name}: max-abs vs fp64 over valid rows = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    keep = np.arange(got.shape[1])[None, :] < np.asarray(lens)[:, None]
    assert not bool(got[torch.from_numpy(~keep)].any())            # rows at or beyond a length: exactly zero


@pytest.mark.parametrize("name", ["reduced_default", "reduced_trained"])
def test_emulated_fixture_matches_fp64(lib, name):
    g = th.load_fixture(name)
    b = th.make_bert("reduced", th.FIXTURES[name]["trained"], "cpu", native_lib=lib)
    got = th.encode(b, g["ids"], g["mask"])
    assert tuple(got.shape) == g["fp64"].shape and got.dtype == torch.float32
    _check(name, got, g["fp64"], th.FIXTURE_LENS)


@pytest.mark.parametrize("L", [1, 33, 65])
def test_emulated_key_tile_edges(bert, L):
    name = f"keytile_L{L}"
    ids, mask, lens = th.sweep_inputs(name)
    got = th.encode(bert, ids, mask)
    _check(name, got, th.encoder_fp64(th.weights("reduced", True), ids, lens, th.REDUCED["n_heads"]), lens)


def _prompt9():
    g = th.load_fixture("reduced_trained")
    return g, g["ids"][1, :9]


def test_a_prompt_gives_the_same_bits_alone_and_in_any_batch(bert):
    """The length-9 prompt of the fixture: alone at L = 9, as row 1 (where the fixture has it), as row 0 and as row 3 of an L = 33
    batch, and in an L = 128 batch; and twice the same call."""
    g, p9 = _prompt9()
    alone = th.encode(bert, p9[None], np.ones((1, 9), bool))[0]
    fix = th.encode(bert, g["ids"], g["mask"])
    assert torch.equal(fix, th.encode(bert, g["ids"], g["mask"]))
    assert torch.equal(fix[1, :9], alone)
    for row in (0, 3):
        order = [1, 0, 2, 3] if row == 0 else [0, 3, 2, 1]
        got = th.encode(bert, g["ids"][order], g["mask"][order])
        assert torch.equal(got[row, :9], alone), row
    ids, mask = th.make_ids(77, 2, 128, [128, 9])
    ids[1, :9] = p9
    assert torch.equal(th.encode(bert, ids, mask)[1, :9], alone)


def test_poison_in_workspace_output_and_padding_does_not_reach_the_output(bert, monkeypatch):
    """Workspace and `out` start as NaN, and the ids behind the lengths are other valid ids: all finite, padded rows zero, valid rows
    bit-identical to the clean call."""
    import mdm_amd.text_encoder as te
    g = th.load_fixture("reduced_trained")
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
    assert not bool(got[torch.from_numpy(~g["mask"])].any())
    assert torch.equal(got, clean)


def test_token_major_is_the_permuted_result(bert):
    g = th.load_fixture("reduced_trained")
    got = th.encode(bert, g["ids"], g["mask"], token_major=True)
    assert tuple(got.shape) == (33, 4, th.REDUCED["dim"])
    assert torch.equal(got, th.encode(bert, g["ids"], g["mask"]).permute(1, 0, 2))


# ---- the entry points' refusals --------------------------------------------------------------------------------------------------------
def _call(lib, model, B, L, ws_bytes=None, out=None):
    ids = np.zeros((B, max(L, 1)), np.int32)
    lens = np.ones(B, np.int32)
    need = lib.mdm_text_workspace_bytes(C.byref(model), B, L)
    ws = np.zeros(max(need, 64) // 4 + 4, np.float32)
    out = np.zeros((B, max(L, 1), model.dim), np.float32) if out is None else out
    rc = lib.mdm_text_encode(C.byref(model), ids.ctypes.data, lens.ctypes.data, out.ctypes.data, B, L, 0, ws.ctypes.data,
                             need if ws_bytes is None else ws_bytes, None)
    return need, rc, lib.mdm_last_error().decode()


def test_entry_points_validate_and_name_the_field(lib, bert):
    model = bert._model()

    def variant(**over):
        m = nat.MdmTextModel()
        C.memmove(C.byref(m), C.byref(model), C.sizeof(m))
        for k, v in over.items():
            setattr(m, k, v)
        return m

    need, rc, _ = _call(lib, model, 2, 5)
    assert rc == 0 and need == 2 * 5 * (5 * 128 + 256) * 4 + 64
    for m, L, code, word in [(model, 129, -5, "L must be at most 128"), (variant(max_pos=4), 5, -1, "max_pos"),
                             (variant(n_heads=3), 5, -5, "dim"), (variant(hidden=254), 5, -5, "hidden"),
                             (variant(word_emb=None), 5, -1, "word_emb"), (variant(pos_emb=model.pos_emb + 4), 5, -1, "pos_emb"),
                             (variant(n_layers=17), 5, -5, "n_layers")]:
        need, rc, msg = _call(lib, m, 2, L)
        assert need == 0 and rc == code and word in msg, (L, need, rc, msg)
    layers = (nat.MdmTextLayer * 2)(model.layers[0], model.layers[1])
    layers[1].lin2_b = layers[1].lin2_b + 8
    need, rc, msg = _call(lib, variant(layers=layers), 2, 5)
    assert need == 0 and rc == -1 and "layers[1].lin2_b" in msg and "aligned" in msg, msg
    need, rc, msg = _call(lib, model, 2, 5, ws_bytes=2 * 5 * (5 * 128 + 256) * 4)
    assert rc == -3 and "workspace_bytes" in msg, msg
    out = np.zeros(2 * 5 * 128 + 4, np.float32)
    _, rc, msg = _call(lib, model, 2, 5, out=out[1:])
    assert rc == -1 and "out_dev" in msg, msg
