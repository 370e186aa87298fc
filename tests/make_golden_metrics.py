"""Writes tests/golden/metrics_{pr_65x65_d256,pr_130x130_d30,kid,stats,diversity}.npz and PIN_REPORT_metrics.json.

Run on the CPU, with the reference checkout's path:   python tests/make_golden_metrics.py /path/to/motion-diffusion-model

The reference's own eval/unconstrained/metrics/precision_recall.py, eval/unconstrained/metrics/kid.py, eval/a2m/action2motion/fid.py
and eval/a2m/action2motion/diversity.py are IMPORTED here, at generation time only, and run on the inputs tests/metrics_helpers.py
builds; the files hold data only.  (calculate_activation_statistics lives in eval/unconstrained/evaluate.py, whose imports need the
whole evaluation stack; it is np.mean(axis=0) and np.cov(rowvar=False) on the fp32 array, which is what runs here.)  The report records
  pr      per case: the `attempt` at which no row is fragile, the smallest margin and tau, and the reference's own fractions -- asserted
          equal to the fp64 oracle's;
  kid     per case: e_ref of mmd2 and var = max |reference on fp32 - restatement| over POOL_MIN subsets of the case's shape, and the
          restatement against the reference on float64 inputs, asserted <= 1e-10 relative;
  pooled  per (D, regime, m): the maximum of the cases' e_ref and the number of subset results behind it (>= 24)."""
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

import metrics_helpers as mh  # noqa: E402


def main(ref_root):
    sys.path.insert(0, ref_root)
    from eval.unconstrained.metrics import precision_recall as ref_pr
    from eval.unconstrained.metrics import kid as ref_kid
    from eval.a2m.action2motion import fid as ref_fid
    from eval.a2m.action2motion import diversity as ref_div
    torch.set_num_threads(4)
    report = {"pr": {}, "kid": {}, "pooled": {}}

    # ---- precision / recall
    for name, c in mh.PR_CASES.items():
        attempt = 0
        while True:
            A, B = mh.pr_input(name, attempt)
            m_ab, m_ba = mh.margins(A, B)[1], mh.margins(B, A)[1]
            if min(m_ab.min(), m_ba.min()) >= mh.tau(c["D"]):
                break
            attempt += 1
            assert attempt < 50, name
        in_a, in_b = mh.pr_oracle(A, B)                    # B's rows in A's manifold (precision), A's rows in B's (recall)
        ta, tb = torch.from_numpy(A), torch.from_numpy(B)
        ref_p, ref_r = ref_pr.manifold_estimate(ta, tb, mh.K), ref_pr.manifold_estimate(tb, ta, mh.K)
        assert ref_p == int(in_a.sum()) / len(B) and ref_r == int(in_b.sum()) / len(A), name
        report["pr"][name] = {"attempt": attempt, "min_margin": float(min(m_ab.min(), m_ba.min())), "tau": mh.tau(c["D"]),
                              "precision_ref": ref_p, "recall_ref": ref_r}
        if c["fixture"]:
            both_p, both_r = ref_pr.precision_and_recall(tb, ta)
            assert (both_p, both_r) == (ref_p, ref_r), name
            np.savez_compressed(os.path.join(mh.GOLDEN, f"metrics_pr_{name}.npz"), real=A, generated=B, ref_precision=np.float64(ref_p),
                                ref_recall=np.float64(ref_r), fp64_generated_in_real=in_a, fp64_real_in_generated=in_b)
        print(f"pr {name}: attempt {attempt}  margin {report['pr'][name]['min_margin']:.3e} (tau {mh.tau(c['D']):.3e})  precision "
              f"{ref_p:.4f} recall {ref_r:.4f}", flush=True)

    # ---- KID
    for name, c in mh.KID_CASES.items():
        g, r = mh.kid_input(name)
        kw = mh.REGIMES[c["regime"]]
        m = min(len(g), len(r))
        ig, ir = mh.kid_draw(name, S=max(mh.POOL_MIN, c["S"]), np_seed=c["seed"] + 555)
        f64 = mh.kid_fp64(g, r, ig, ir, **kw)
        e_mmd = e_var = agree = 0.0
        for s in range(len(ig)):
            got = ref_kid.polynomial_mmd(g[ig[s]], r[ir[s]], **kw, var_at_m=m)
            dbl = ref_kid.polynomial_mmd(g[ig[s]].astype(np.float64), r[ir[s]].astype(np.float64), **kw, var_at_m=m)
            e_mmd, e_var = max(e_mmd, abs(got[0] - f64[0][s])), max(e_var, abs(got[1] - f64[1][s]))
            agree = max(agree, abs(dbl[0] - f64[0][s]) / abs(f64[0][s]), abs(dbl[1] - f64[1][s]) / abs(f64[1][s]))
        assert agree <= 1e-10, (name, agree)
        report["kid"][name] = {"e_ref_mmd2": float(e_mmd), "e_ref_var": float(e_var), "fp64_vs_reference_double": float(agree),
                               "results": len(ig), "mmd2_range": [float(f64[0].min()), float(f64[0].max())],
                               "var_range": [float(f64[1].min()), float(f64[1].max())]}
        p = report["pooled"].setdefault(mh.pool_key(name), {"e_ref_mmd2": 0.0, "e_ref_var": 0.0, "results": 0, "cases": []})
        p["e_ref_mmd2"], p["e_ref_var"] = max(p["e_ref_mmd2"], float(e_mmd)), max(p["e_ref_var"], float(e_var))
        p["results"] += len(ig)
        p["cases"].append(name)
        print(f"kid {name}: e_ref mmd2 {e_mmd:.3e} var {e_var:.3e}  restatement vs double {agree:.1e}  mmd2 in "
              f"[{f64[0].min():.3f}, {f64[0].max():.3f}]", flush=True)
        if c["fixture"]:
            np.random.seed(c["seed"])
            ref_mmd2, ref_var = ref_kid.polynomial_mmd_averages(g, r, n_subsets=c["S"], subset_size=c["m"])
            ig, ir = mh.kid_draw(name)
            want = mh.kid_fp64(g, r, ig, ir)
            assert np.abs(ref_mmd2 - want[0]).max() <= 4 * e_mmd and np.abs(ref_var - want[1]).max() <= 4 * e_var      # the replayed draws ARE upstream's
            np.savez_compressed(os.path.join(mh.GOLDEN, "metrics_kid.npz"), g=g, r=r, np_seed=np.int64(c["seed"]), idx_g=ig, idx_r=ir,
                                ref_mmd2=ref_mmd2, ref_var=ref_var, fp64_mmd2=want[0], fp64_var=want[1])
    for p in report["pooled"].values():
        assert p["results"] >= mh.POOL_MIN

    # ---- statistics and FID: the reference's statements on the fp32 arrays
    x1, x2 = mh.make_features(65, 30, 5, 5101), mh.make_features(70, 30, 5, 5101, generated=True)
    s1, s2 = (np.mean(x1, axis=0), np.cov(x1, rowvar=False)), (np.mean(x2, axis=0), np.cov(x2, rowvar=False))
    f1, f2 = mh.stats_fp64(x1), mh.stats_fp64(x2)
    np.savez_compressed(os.path.join(mh.GOLDEN, "metrics_stats.npz"), x1=x1, x2=x2, ref_mu1=s1[0], ref_sigma1=s1[1], ref_mu2=s2[0],
                        ref_sigma2=s2[1], fp64_mu1=f1[0], fp64_sigma1=f1[1], fp64_mu2=f2[0], fp64_sigma2=f2[1],
                        ref_fid=np.float64(ref_fid.calculate_fid(s1, s2)), ref_fid_of_fp64=np.float64(ref_fid.calculate_fid(f1, f2)))

    # ---- diversity
    xd = mh.make_features(90, 256, 6, 5201)
    np.random.seed(5202)
    ref_d = ref_div.calculate_diversity(torch.from_numpy(xd))
    np.random.seed(5202)
    first, second = np.random.randint(0, len(xd), 200), np.random.randint(0, len(xd), 200)
    want = float(mh.pair_dist_fp64(xd, first, second).mean())
    assert abs(float(ref_d) - want) <= 1e-5 * want
    np.savez_compressed(os.path.join(mh.GOLDEN, "metrics_diversity.npz"), x=xd, np_seed=np.int64(5202), first=first, second=second,
                        ref_diversity=np.float64(float(ref_d)), fp64_diversity=np.float64(want))

    with open(mh.PIN_REPORT, "w") as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
    for k, p in sorted(report["pooled"].items()):
        print(f"pooled {k}: e_ref mmd2 {p['e_ref_mmd2']:.3e} var {p['e_ref_var']:.3e} over {p['results']} results")
    print("wrote", mh.PIN_REPORT)


if __name__ == "__main__":
    main(sys.argv[1])
