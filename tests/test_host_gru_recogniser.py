"""mdm_amd/gru_recogniser.py without a device: the reference's state-dict keys and shapes, the checkpoint loaders, the refusals of the
module and of the native call (each with its message in mdm_last_error), the ABI version, and the build's scratch audit."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import gru_recogniser_helpers as gh
from emu.emu_lib import emu
from mdm_amd import _native as nat
from mdm_amd import gru_recogniser as gr


@pytest.mark.parametrize("net", ["full", "ntu"])
def test_state_dict_keys_and_shapes_are_the_references(net):
    with open(gh.KEYS_FILE) as fh:
        want = [(k, tuple(s)) for k, s in json.load(fh)[net]]
    assert len(want) == 12 and want[0][0] == "recurrent.weight_ih_l0" and want[0][1] == (384, gh.input_size(net))
    assert gh.state_shapes(net) == want
    weights = gh.build_weights(net, "trained")
    assert [(k, tuple(v.shape)) for k, v in weights.items()] == want
    gh.make_model(net).load_state_dict(weights)                   # strictly
    gh.make_model(net, fid=True).load_state_dict(weights)


def test_loaders_read_the_checkpoint_at_model_path(tmp_path, monkeypatch):
    weights = gh.build_weights("full", "trained")
    path = tmp_path / "humanact12_gru.tar"
    torch.save({"model": weights, "epoch": 3}, str(path))
    assert gr.model_path == "./assets/actionrecognition/humanact12_gru.tar"
    monkeypatch.setattr(gr, "model_path", str(path))
    clf, fid = gr.load_classifier(72, 12, "cpu"), gr.load_classifier_for_fid(72, 12, "cpu")
    assert type(clf) is gr.MotionDiscriminator and type(fid) is gr.MotionDiscriminatorForFID and isinstance(fid, gr.MotionDiscriminator)
    for m in (clf, fid):
        assert not m.training and m.hidden_size == 128 and m.hidden_layer == 2 and m.input_size == 72
        assert m.linear2.out_features == 12 and m.linear1.out_features == 30
        for k, v in m.state_dict().items():
            assert torch.equal(v, weights[k]), k
    assert clf.initHidden(5, 2).shape == (2, 5, 128)


def test_the_module_refuses_bad_arguments_by_name():
    m = gh.loaded_model("red2", gh.build_weights("red2", "trained"), "cpu", emu())
    x, lens, h0 = (torch.from_numpy(a) for a in gh.case_input("red2_trained_2x13"))
    with pytest.raises(ValueError, match="lengths"):
        m(x)                                                         # upstream fails on `None - 1`
    with pytest.raises(ValueError, match="lengths"):
        m(x, None, h0)
    for bad in ([0, 13], [1, 14], [-1, 5]):
        with pytest.raises(ValueError, match=r"\[1, 13\]"):
            m(x, torch.tensor(bad), h0)
    with pytest.raises(ValueError, match="integer"):
        m(x, torch.tensor([1.0, 2.0]), h0)
    with pytest.raises(ValueError, match="integer"):
        m(x, torch.tensor([1, 2, 3]), h0)
    with pytest.raises(ValueError, match="features"):
        m(torch.zeros(2, 6, 2, 13), lens, h0)
    with pytest.raises(ValueError, match="njoints"):
        m(torch.zeros(2, 10, 13), lens, h0)
    with pytest.raises(ValueError, match="hidden_unit"):
        m(x, lens, h0[:1])
    with pytest.raises(ValueError, match="hidden_layer"):
        gr.MotionDiscriminator(10, 32, 5, "cpu")


def test_product_path_has_no_fallback_without_the_library(monkeypatch, tmp_path):
    monkeypatch.setattr(nat, "_LIB", None)
    monkeypatch.setenv("MDM_HIP_LIB", str(tmp_path / "missing.so"))
    m = gh.loaded_model("red2", gh.build_weights("red2", "trained"))
    x, lens, h0 = (torch.from_numpy(a) for a in gh.case_input("red2_trained_2x13"))
    with pytest.raises(nat.MdmError, match="not found"):
        m(x, lens, h0)


def test_native_refusals_say_which_argument():
    lib = emu()
    assert lib.mdm_abi_version() == 10 == nat.ABI_VERSION
    model = gh.loaded_model("red2", gh.build_weights("red2", "trained"), "cpu", lib)
    m = model._model()
    err = lambda: lib.lib.mdm_last_error()      # noqa: E731
    B, T = 2, 5
    need = lib.mdm_gru_cls_workspace_bytes(C.byref(m), B, T)
    assert need == (B * T * 96 + B * T * 32 + B * 32) * 4 + 64
    buf = np.zeros(need // 4 + 8, dtype=np.float32)
    p = buf.ctypes.data
    assert p % 16 == 0
    call = lambda mm, x=p, l=p, h=p, f=p, y=p, b=B, t=T, ws=p, n=need: lib.mdm_gru_cls_forward(      # noqa: E731
        C.byref(mm), x, l, h, f, y, b, t, ws, n, None)

    assert lib.mdm_gru_cls_workspace_bytes(None, B, T) == 0 and b"null model" in err()
    for kw in (dict(x=None), dict(l=None), dict(h=None), dict(f=None), dict(y=None), dict(ws=None)):
        assert call(m, **kw) == -1 and b"null" in err(), kw
    for kw, word in ((dict(x=p + 2), b"x_dev must be 4-byte aligned"), (dict(h=p + 1), b"h0_dev must be 4-byte aligned"),
                     (dict(l=p + 2), b"lens_dev must be 4-byte aligned"), (dict(y=p + 3), b"yhat_dev must be 4-byte aligned")):
        assert call(m, **kw) == -1 and word in err(), (kw, err())
    for b, t, word in ((0, 5, b"B must"), (2, 0, b"T must"), (-1, 5, b"B must"), (2, 1 << 17, b"T must"), (1 << 20, 1 << 12, b"chunk")):
        assert lib.mdm_gru_cls_workspace_bytes(C.byref(m), b, t) == 0 and word in err(), (b, t, err())
        assert call(m, b=b, t=t) < 0 and word in err()
    assert call(m, n=need - 1) == -3 and b"workspace_bytes too small" in err()

    def broken(layer=None, **over):
        mm = nat.MdmGruClsModel.from_buffer_copy(m)
        for k, v in over.items():
            setattr(mm.layers[layer] if layer is not None else mm, k, v)
        return mm

    for mm, word in ((broken(num_layers=5), b"num_layers must be between 1 and 4"), (broken(num_layers=0), b"num_layers"),
                     (broken(hidden_size=48), b"hidden_size must be 128"), (broken(input_size=0), b"input_size"),
                     (broken(mid=65), b"mid must"), (broken(num_class=0), b"num_class must"),
                     (broken(lin1_w=None), b"null weight pointer lin1_w"), (broken(layer=1, w_hh=None), b"null weight pointer layers[1].w_hh"),
                     (broken(layer=0, w_ih=m.layers[0].w_ih + 4), b"layers[0].w_ih must be 16-byte aligned"),
                     (broken(lin2_b=m.lin2_b + 8), b"lin2_b must be 16-byte aligned")):
        assert lib.mdm_gru_cls_workspace_bytes(C.byref(mm), B, T) == 0 and word in err(), err()
        assert call(mm) < 0 and word in err()
    # a third layer's pointers are not looked at when num_layers is 2: the call over buffers of its own runs
    x, h0 = gh.make_input("red2", 5, B, T)
    lens = np.asarray([5, 2], dtype=np.int32)
    feat, yhat = np.zeros((B, 30), np.float32), np.zeros((B, 12), np.float32)
    assert m.layers[2].w_ih is None
    assert call(m, x=x.ctypes.data, l=lens.ctypes.data, h=h0.ctypes.data, f=feat.ctypes.data, y=yhat.ctypes.data) == 0
    assert np.isfinite(feat).all() and np.isfinite(yhat).all() and np.abs(yhat).max() > 0


def test_recurrence_and_tail_kernels_use_no_scratch():
    audit = os.path.join(gh.ROOT, "build", "resource_usage.txt")
    if not os.path.isfile(audit):
        return            # written by build(); a tree that has not been built has nothing to audit
    with open(audit) as fh:
        lines = [ln for ln in fh if "gru_seq_kernel" in ln or "gru_tail_kernel" in ln]
    assert any("gru_seq_kernelILi128" in ln for ln in lines) and any("gru_seq_kernelILi32" in ln for ln in lines)
    for ln in lines:
        assert re.search(r"\bscratch=0\b", ln), ln
