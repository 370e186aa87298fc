"""Writes tests/golden/gru_recogniser_{default,trained}.npz, gru_recogniser_seeded.npz, gru_recogniser_state_dict_keys.json and
PIN_REPORT_gru_recogniser.json.

Run on the CPU, with the reference checkout's path:   python tests/make_golden_gru_recogniser.py /path/to/motion-diffusion-model

The reference's own eval/a2m/action2motion/models.py is IMPORTED here, at generation time only, and both classes are run in fp32 on
the weights tests/gru_recogniser_helpers.py builds; the files hold data only.  Reduced nets are the reference's own class with
H = 32, I = 10, L in {1, 2}.  The reference's forward casts its input with `.float()`, so the `.double()` instance is driven through
its own submodules in forward's order (recurrent, the gather at lengths - 1, linear1, tanh, linear2).  The report records
  per case   fp64_agrees: the restatement of gru_recogniser_helpers.py against that double run, to 1e-10 (asserted); e_ref_features /
             e_ref_yhat: max |reference fp32 - fp64| over the case's input and two further draws of the same shape;
  pooled     per (net, regime): the maximum of the cases' e_ref per output -- the unit of the accuracy condition of the tests.
Fixture rows must be classifiable: the generator moves a fixture's seed until every row's top-2 margin in fp64 is >= 1e-3."""
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

import gru_recogniser_helpers as gh  # noqa: E402

MARGIN = 1e-3


def reference_model(ref, net, weights, fid=False, dtype=torch.float32):
    f = gh.NETS[net]
    cls = ref.MotionDiscriminatorForFID if fid else ref.MotionDiscriminator
    m = cls(gh.input_size(net), f["H"], f["L"], device="cpu", output_size=f["classes"])
    m.load_state_dict(weights)
    return m.to(dtype).eval()


def reference_run(m_cls, m_fid, x, lens, h0):
    """(features, yhat) of the reference's two classes in fp32; h0 None: hidden_unit=None (the caller has seeded torch)."""
    with torch.no_grad():
        xt, lt = torch.from_numpy(x), torch.from_numpy(lens)
        ht = None if h0 is None else torch.from_numpy(h0)
        return m_fid(xt, lt, ht).numpy(), m_cls(xt, lt, ht).numpy()


def reference_double(m64, x, lens, h0):
    with torch.no_grad():
        bs, T = x.shape[0], x.shape[3]
        seq = torch.from_numpy(x).double().reshape(bs, -1, T).permute(2, 0, 1)
        gru_o, _ = m64.recurrent(seq, torch.from_numpy(h0).double())
        out = gru_o[tuple(torch.stack((torch.from_numpy(lens) - 1, torch.arange(bs))))]
        lin1 = torch.tanh(m64.linear1(out))
        return lin1.numpy(), m64.linear2(lin1).numpy()


def margin(yhat):
    top = np.sort(yhat, axis=1)
    return float((top[:, -1] - top[:, -2]).min())


def main(ref_root):
    sys.path.insert(0, ref_root)
    from eval.a2m.action2motion import models as ref
    torch.set_num_threads(4)

    report, pooled = {}, {}
    for name, c in gh.CASES.items():
        net = c["net"]
        weights = gh.case_weights(name)
        m_cls, m_fid = reference_model(ref, net, weights), reference_model(ref, net, weights, fid=True)
        m64 = reference_model(ref, net, weights, dtype=torch.float64)
        attempt = 0
        while c["fixture"]:
            x, lens, h0 = gh.case_input(name, 0, attempt)
            if margin(gh.forward_fp64(net, weights, x, lens, h0)[1]) >= MARGIN:
                break
            attempt += 1
            assert attempt < 50, name
        e_feat = e_yhat = agree = 0.0
        for draw in range(3):
            x, lens, h0 = gh.case_input(name, draw, attempt)
            got = reference_run(m_cls, m_fid, x, lens, h0)
            f64 = gh.forward_fp64(net, weights, x, lens, h0)
            agree = max(agree, *gh.errors(reference_double(m64, x, lens, h0), f64))
            ef, ey = gh.errors(got, f64)
            e_feat, e_yhat = max(e_feat, ef), max(e_yhat, ey)
            if draw == 0:
                first = (x, lens, h0, got, f64)
        assert agree <= 1e-10, (name, agree)
        x, lens, h0, (ref_f, ref_y), (f64_f, f64_y) = first
        report[name] = {"e_ref_features": e_feat, "e_ref_yhat": e_yhat, "fp64_agrees": True, "fp64_vs_reference_double": agree,
                        "shape": [c["B"], c["T"]], "max_abs_features": float(np.abs(f64_f).max()),
                        "max_abs_yhat": float(np.abs(f64_y).max()), "top2_margin_fp64": margin(f64_y)}
        p = pooled.setdefault(gh.pool_key(net, c["regime"]), {"e_ref_features": 0.0, "e_ref_yhat": 0.0, "cases": []})
        p["e_ref_features"], p["e_ref_yhat"] = max(p["e_ref_features"], e_feat), max(p["e_ref_yhat"], e_yhat)
        p["cases"].append(name)
        if c["fixture"]:
            report[name]["attempt"] = attempt
            assert np.array_equal(ref_y.argmax(1), f64_y.argmax(1)), name
            np.savez_compressed(os.path.join(gh.GOLDEN, f"gru_recogniser_{c['regime']}.npz"), x=x, lens=lens, h0=h0, ref_features=ref_f,
                                ref_yhat=ref_y, fp64_features=f64_f, fp64_yhat=f64_y)
        print(f"{name}: e_ref features {e_feat:.3e} yhat {e_yhat:.3e}  restatement vs .double() = {agree:.1e}  max|features| = "
              f"{report[name]['max_abs_features']:.3f}  max|yhat| = {report[name]['max_abs_yhat']:.3f}  margin = "
              f"{report[name]['top2_margin_fp64']:.3e}", flush=True)

    # hidden_unit=None under a torch seed, on the CPU generator: the reference draws torch.randn(L, B, H) once per forward
    s = gh.SEEDED
    weights = gh.build_weights(s["net"], s["regime"])
    m_cls, m_fid = reference_model(ref, s["net"], weights), reference_model(ref, s["net"], weights, fid=True)
    x, _ = gh.make_input(s["net"], s["seed"], s["B"], s["T"])
    lens = np.asarray(s["lens"], dtype=np.int64)
    with torch.no_grad():
        torch.manual_seed(s["torch_seed"])
        ref_y = m_cls(torch.from_numpy(x), torch.from_numpy(lens)).numpy()
        torch.manual_seed(s["torch_seed"])
        ref_f = m_fid(torch.from_numpy(x), torch.from_numpy(lens)).numpy()
        torch.manual_seed(s["torch_seed"])
        h0 = torch.randn(gh.NETS[s["net"]]["L"], s["B"], gh.NETS[s["net"]]["H"]).numpy()
    f64_f, f64_y = gh.forward_fp64(s["net"], weights, x, lens, h0)
    ef, ey = gh.errors((ref_f, ref_y), (f64_f, f64_y))
    p = pooled[gh.pool_key(s["net"], s["regime"])]
    assert ef <= 4 * p["e_ref_features"] and ey <= 4 * p["e_ref_yhat"], (ef, ey)      # the draw IS torch.randn after the seed
    np.savez_compressed(gh.SEEDED_FILE, torch_seed=np.int64(s["torch_seed"]), x=x, lens=lens, ref_features=ref_f, ref_yhat=ref_y,
                        fp64_features=f64_f, fp64_yhat=f64_y)

    keys = {net: [[k, list(v.shape)] for k, v in reference_model(ref, net, gh.build_weights(net, "default")).state_dict().items()]
            for net in ("full", "ntu")}
    with open(gh.KEYS_FILE, "w") as fh:
        json.dump(keys, fh, indent=1)
    with open(gh.PIN_REPORT, "w") as fh:
        json.dump({"cases": report, "pooled": pooled}, fh, indent=1, sort_keys=True)
    for k, p in sorted(pooled.items()):
        print(f"pooled {k}: e_ref features {p['e_ref_features']:.3e} yhat {p['e_ref_yhat']:.3e} over {len(p['cases'])} cases")
    print("wrote", gh.PIN_REPORT)


if __name__ == "__main__":
    main(sys.argv[1])
