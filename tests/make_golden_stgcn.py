"""Writes tests/golden/stgcn_{a2m,unc}_{default,trained}.npz, stgcn_graph_A.npz, stgcn_state_dict_keys.json and PIN_REPORT_stgcn.json.

Run on the CPU, with the reference checkout's path:   python tests/make_golden_stgcn.py /path/to/motion-diffusion-model

The reference's own eval/a2m/recognition/models/stgcn.py, eval/unconstrained/models/stgcn.py and their Graph classes are IMPORTED
here, at generation time only, fed a synthetic kintree_table.pkl (SMPL's public tree) and run in fp32 on the weights
tests/stgcn_helpers.py builds; the files hold data only.  Reduced nets are the reference's own instance with `st_gcn_networks`,
`edge_importance` and `fcn` swapped for narrower ones of the reference's own `st_gcn`, so the reference's forward still runs them.
Per case the report records
  fp64_agrees   the fp64 restatement of stgcn_helpers.py against the reference module run in .double(), to 1e-10 (asserted);
  e_ref         max |reference fp32 - fp64| over features and yhat, over the case's input and two further draws of the same shape:
                the unit of the accuracy condition of the tests."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import stgcn_helpers as sh  # noqa: E402

LAYOUTS_A2M = ("openpose", "smpl", "smpl_noglobal", "ntu-rgb+d", "ntu_edge")
STRATEGIES = ("uniform", "distance", "spatial")


def reference_model(ref, net, weights, dtype=torch.float32):
    f = sh.NETS[net]
    mod = ref["unc"] if f["cls"] == "STGCNUnconstrained" else ref["a2m"]
    m = mod.STGCN(in_channels=f["in_channels"], num_class=f["num_class"], graph_args=sh.graph_args(f["layout"]),
                  edge_importance_weighting=True, device="cpu")
    if f["blocks"] is not None:
        K = m.A.size(0)
        m.st_gcn_networks = torch.nn.ModuleList(
            mod.st_gcn(f["in_channels"] if ci is None else ci, co, (9, K), s, residual=res) for ci, co, s, res in f["blocks"])
        m.edge_importance = torch.nn.ParameterList([torch.nn.Parameter(torch.ones(m.A.size())) for _ in m.st_gcn_networks])
        m.fcn = torch.nn.Conv2d(f["blocks"][-1][1], f["num_class"], kernel_size=1)
    m.load_state_dict(weights)
    return m.to(dtype).eval()


def reference_run(model, key, x):
    with torch.no_grad():
        batch = model({key: torch.from_numpy(x).to(model.fcn.weight.dtype)})
    return batch["features"].reshape(x.shape[0], -1).numpy(), batch["yhat"].numpy()


def main(ref_root):
    sys.path.insert(0, ref_root)
    from eval.a2m.recognition.models import stgcn as ref_a2m
    from eval.a2m.recognition.models.stgcnutils import graph as graph_a2m
    from eval.unconstrained.models import stgcn as ref_unc
    from eval.unconstrained.models.stgcnutils import graph as graph_unc
    ref = {"a2m": ref_a2m, "unc": ref_unc}
    assert ref_a2m.st_gcn is not None and graph_a2m.Graph is not None
    torch.manual_seed(0)
    torch.set_num_threads(8)

    report = {}
    for name, c in sh.CASES.items():
        net = c["net"]
        key = "x" if sh.NETS[net]["cls"] == "STGCNUnconstrained" else "output"
        weights = sh.case_weights(name)
        m32 = reference_model(ref, net, weights)
        m64 = reference_model(ref, net, weights, torch.float64)
        e_feat = e_yhat = agree = 0.0
        for draw in range(3):
            x = sh.case_input(name, draw)
            got = reference_run(m32, key, x)
            dbl = reference_run(m64, key, x.astype(np.float64))
            f64 = sh.forward_fp64(net, weights, x)
            agree = max(agree, *sh.errors(dbl, f64))
            ef, ey = sh.errors(got, f64)
            e_feat, e_yhat = max(e_feat, ef), max(e_yhat, ey)
            if draw == 0:
                first = (got, f64)
        assert agree <= 1e-10, (name, agree)
        (ref_f, ref_y), (f64_f, f64_y) = first
        report[name] = {"e_ref": max(e_feat, e_yhat), "e_ref_features": e_feat, "e_ref_yhat": e_yhat, "fp64_agrees": True,
                        "fp64_vs_reference_double": agree, "shape": [c["N"], c["T"]],
                        "max_abs_features": float(np.abs(f64_f).max()), "max_abs_yhat": float(np.abs(f64_y).max())}
        if c["fixture"]:
            np.savez_compressed(os.path.join(sh.GOLDEN, f"stgcn_{name}.npz"), x=sh.case_input(name), ref_features=ref_f, ref_yhat=ref_y,
                                fp64_features=f64_f, fp64_yhat=f64_y)
        print(f"{name}: e_ref = {report[name]['e_ref']:.3e} (features {e_feat:.3e}, yhat {e_yhat:.3e})  restatement vs .double() = "
              f"{agree:.1e}  max|features| = {report[name]['max_abs_features']:.3f}  max|yhat| = {report[name]['max_abs_yhat']:.3f}", flush=True)

    # the A tensors of every layout x strategy of both copies (`openpose15`: what the unconstrained copy builds as `openpose`)
    graphs = {}
    for strategy in STRATEGIES:
        for layout in LAYOUTS_A2M:
            graphs[f"{layout}__{strategy}"] = graph_a2m.Graph(layout=layout, strategy=strategy, kintree_path=sh.kintree_path()).A
        graphs[f"openpose15__{strategy}"] = graph_unc.Graph(layout="openpose", strategy=strategy, kintree_path=sh.kintree_path()).A
        for layout in LAYOUTS_A2M[1:]:
            assert np.array_equal(graph_unc.Graph(layout=layout, strategy=strategy, kintree_path=sh.kintree_path()).A,
                                  graphs[f"{layout}__{strategy}"])
    np.savez_compressed(sh.GRAPH_FILE, **graphs)

    keys = {net: [[k, list(v.shape)] for k, v in reference_model(ref, net, sh.build_weights(net, 1, "default")).state_dict().items()]
            for net in ("a2m", "unc")}
    with open(sh.KEYS_FILE, "w") as fh:
        json.dump(keys, fh, indent=1)
    with open(sh.PIN_REPORT, "w") as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
    print("wrote", sh.PIN_REPORT)


if __name__ == "__main__":
    main(sys.argv[1])
