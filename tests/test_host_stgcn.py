"""mdm_amd/stgcn.py without a device: the reference's state-dict keys and shapes, Graph.A against the reference's own tensors for
every layout x strategy (tests/golden/stgcn_graph_A.npz), the T_out arithmetic, the refusals, and -- where the reference tree is at
hand -- its calculate_accuracy over this classifier on the emulator at reduced width."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import stgcn_helpers as sh
from mdm_amd import _native as nat
from mdm_amd import stgcn as sg


@pytest.mark.parametrize("net", ["a2m", "unc"])
def test_state_dict_keys_and_shapes_are_the_references(net):
    with open(sh.KEYS_FILE) as fh:
        want = [(k, tuple(s)) for k, s in json.load(fh)[net]]
    got = sh.state_shapes(net)
    assert len(want) > 100 if net == "a2m" else len(want) > 60
    assert got == want
    # ... and a state dict saved from one instance loads into another, strictly
    m = sh.make_model(net)
    m.load_state_dict(sh.build_weights(net, 5, "trained"))


def test_graph_A_equals_the_references_for_every_layout_and_strategy():
    with np.load(sh.GRAPH_FILE) as z:
        stored = {k: z[k] for k in z.files}
    assert len(stored) == len(sg.LAYOUTS) * len(sg.STRATEGIES) == 18
    for key, want in stored.items():
        layout, strategy = key.split("__")
        g = sg.Graph(layout=layout, strategy=strategy, kintree_path=sh.kintree_path())
        assert g.A.shape == want.shape and g.A.dtype == want.dtype, key
        assert np.array_equal(g.A, want), key
    # the unconstrained class builds its tree's 15-node `openpose`; the a2m class the 18-node one
    assert sh.make_model("unc").A.shape == (3, 15, 15)
    m = sg.STGCN(3, 4, {"layout": "openpose", "strategy": "uniform"}, True, "cpu")
    assert m.A.shape == (1, 18, 18)
    assert torch.equal(sh.make_model("a2m").A, torch.tensor(stored["smpl__spatial"], dtype=torch.float32))


def test_t_out_arithmetic():
    for s in (1, 2, 3, 4):
        for T in list(range(1, 40)) + [59, 60, 61, 157, 196]:
            want = torch.nn.functional.conv2d(torch.zeros(1, 1, T, 1), torch.zeros(1, 1, 9, 1), stride=(s, 1), padding=(4, 0)).shape[2]
            assert sg.t_out(T, s) == want == (T + 8 - 9) // s + 1
    # the a2m net: 60 -> 30 -> 15 frames; T = 1 stays 1
    t = 60
    for _, _, s, _ in sg.A2M_BLOCKS:
        t = sg.t_out(t, s)
    assert t == 15 and sg.t_out(sg.t_out(1, 2), 2) == 1


def test_refusals_name_what_is_not_implemented():
    m = sh.make_model("red_a2m")
    x = torch.zeros(2, 24, 6, 5)
    with pytest.raises(nat.MdmError, match="training mode"):
        m({"output": x})                                   # a fresh module is in training mode, as torch's are
    m.eval()
    with pytest.raises(nat.MdmError, match="M > 1"):
        m({"output": torch.zeros(2, 24, 6, 5, 2)})
    for bad in (torch.zeros(2, 23, 6, 5), torch.zeros(2, 24, 3, 5), torch.zeros(2, 24, 6), torch.zeros(2, 24, 6, 0)):
        with pytest.raises(ValueError, match="must"):
            m({"output": bad})
    with pytest.raises(KeyError):
        m({"x": x})                                        # the a2m class reads batch["output"]
    d = sg.STGCN(6, 5, sh.graph_args("smpl"), True, "cpu", dropout=0.5, _blocks=sh.REDUCED_BLOCKS)
    assert d.st_gcn_networks[0].tcn[4].p == 0 and d.st_gcn_networks[1].tcn[4].p == 0.5
    d.train()
    with pytest.raises(nat.MdmError, match="dropout"):
        d({"output": x})
    with pytest.raises(nat.MdmError, match="training"):
        d.compute_loss({"yhat": torch.zeros(2, 5), "y": torch.zeros(2, dtype=torch.long)})
    with pytest.raises(nat.MdmError, match="no eager PyTorch forward"):
        m.st_gcn_networks[0](x, m.A)
    with pytest.raises(TypeError, match="unexpected"):
        sg.STGCN(6, 5, sh.graph_args("smpl"), True, "cpu", t_kernel_size=3)
    with pytest.raises(NotImplementedError, match="layout"):
        sg.Graph(layout="coco")
    with pytest.raises(NotImplementedError, match="strategy"):
        sg.Graph(layout="openpose", strategy="other")
    # a dense A * importance does not fit the neighbour lists: refused by name, not truncated
    m.A.fill_(0.1)
    with pytest.raises(nat.MdmError, match="MDM_STGCN_MAX_NEIGHBOURS"):
        m._model()


def test_references_calculate_accuracy_runs_over_this_classifier_on_the_emulator():
    from oracle import ref_harness
    ref_root = ref_harness.REFERENCE_ROOT
    if not os.path.isfile(os.path.join(ref_root, "eval", "a2m", "stgcn", "accuracy.py")):
        pytest.skip("needs the upstream reference source tree (MDM_REFERENCE_ROOT), which the repository does not hold")
    from emu.emu_lib import emu
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_stgcn_accuracy", os.path.join(ref_root, "eval", "a2m", "stgcn", "accuracy.py"))
    acc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(acc)
    name = "red_a2m_trained_2x13"
    weights = sh.case_weights(name)
    clf = sh.loaded_model("red_a2m", weights, "cpu", emu())
    xs = [sh.case_input(name, d) for d in range(2)]
    want = [np.argmax(sh.forward_fp64("red_a2m", weights, x)[1], axis=1) for x in xs]
    loader = [{"output": torch.from_numpy(x), "y": torch.from_numpy(w)} for x, w in zip(xs, want)]
    accuracy, confusion = acc.calculate_accuracy(None, loader, 5, clf, "cpu")
    assert confusion.sum().item() == 4 and accuracy == 1.0         # labels = the fp64 restatement's own predictions
    assert loader[0]["features"].shape == (2, 32)
