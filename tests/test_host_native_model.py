"""mdm_amd/_native_model.py NativeModelMixin on the CPU emulator: the prepared-model cache and the workspace cache, once for the five
wrappers that keep a prepared model, each at the smallest widths its own host tests use."""
import pytest
import torch

import clip_text_helpers as ch
import evaluator_helpers as eh
import gru_recogniser_helpers as gh
import stgcn_helpers as sh
import text_encoder_helpers as th
from emu.emu_lib import emu


def _bert():
    m = th.make_bert("reduced", False, "cpu", emu())
    return m, m.text_model, lambda s: (s.word_emb, s.layers[0].qkv_w, s.layers[1].out_ln_b)


def _clip():
    m = ch.make_clip("reduced", False, "cpu", emu())
    return m, m, lambda s: (s.tok_emb, s.layers[0].qkv_w, s.text_proj)


def _stgcn():
    m = sh.loaded_model("red_a2m", sh.build_weights("red_a2m", 3, "trained"), "cpu", emu())
    # (computed tables; on the host fcn_w / fcn_b are views of the parameters, which keep their address)
    return m, m, lambda s: (s.in_scale, s.blocks[0].gcn_w, s.blocks[4].tcn_shift)


def _gru():
    m = gh.loaded_model("red2", gh.build_weights("red2", "trained"), "cpu", emu())
    return m, m, lambda s: (s.lin1_w, s.layers[0].w_ih, s.layers[1].b_hh)


def _evaluator():
    m = eh.make_wrapper(eh.REDUCED, eh.build_weights(3, eh.REDUCED), "cpu", emu())
    return m, m.text_encoder, lambda s: (s.conv1_w, s.motion.w_ih, s.text.o2_b)


WRAPPERS = {"BERT": _bert, "ClipText": _clip, "STGCN": _stgcn, "MotionDiscriminator": _gru, "EvaluatorMDMWrapper": _evaluator}
# The GRU recogniser's struct points at the parameters themselves where they are fp32, contiguous and 16-byte aligned (torch's host
# and device allocations are): a write in place keeps their addresses.  The other four own copies of their tables.
OWNS_COPIES = {"BERT", "ClipText", "STGCN", "EvaluatorMDMWrapper"}
CACHING = {"BERT": "mdm_text_workspace_bytes", "ClipText": "mdm_clip_text_workspace_bytes"}


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_prepared_model_is_cached_and_rebuilt_when_a_parameter_changes(name):
    obj, module, pointers = WRAPPERS[name]()
    first = obj._model()
    assert obj._model() is first                                        # two calls in a row: the same struct
    held = [obj._prepared]                                              # (kept alive: a rebuilt table cannot land on a freed address)
    before = pointers(first)
    assert all(before)

    key, param = next(iter(module.named_parameters()))
    for change in ("write", "load"):
        obj._ws = {"stale": None}
        if change == "write":
            with torch.no_grad():
                param.add_(1.0)
        else:
            sd = {k: v.clone() for k, v in module.state_dict().items()}
            sd[key] += 1.0
            module.load_state_dict(sd)
        again = obj._model()
        assert again is not first and again is not held[-1][1], change   # a rebuilt struct ...
        assert obj._ws == {}, change                                    # ... and the workspaces of the old one are gone
        after = pointers(again)
        assert all(after)
        if name in OWNS_COPIES:
            for old in held:
                assert not set(after) & set(pointers(old[1])), change   # over tables of its own
        else:
            assert after[0] == obj.linear1.weight.data_ptr()
        assert obj._model() is again
        held.append(obj._prepared)


@pytest.mark.parametrize("name", sorted(CACHING))
def test_a_ninth_workspace_shape_starts_the_cache_over(name):
    obj, _, _ = WRAPPERS[name]()
    model = obj._model()
    dev = torch.device("cpu")
    for L in range(1, 9):
        ws, nbytes = obj._workspace(CACHING[name], model, 1, L, dev=dev, stream=None, cache=True)
        assert ws.numel() == nbytes > 0 and len(obj._ws) == L
        assert obj._workspace(CACHING[name], model, 1, L, dev=dev, stream=None, cache=True)[0] is ws      # a hit: the same tensor
    assert (1, 8, "cpu", None) in obj._ws
    obj._workspace(CACHING[name], model, 1, 9, dev=dev, stream=None, cache=True)
    assert list(obj._ws) == [(1, 9, "cpu", None)]                       # the ninth distinct shape: exactly one entry
