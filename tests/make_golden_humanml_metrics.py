"""Writes tests/golden/humanml_metrics_{case1,case5,diversity,multimodality,a2m}.npz and PIN_REPORT_humanml_metrics.json.

Run on the CPU, with the reference checkout's path:   python tests/make_golden_humanml_metrics.py /path/to/motion-diffusion-model

The reference's own data_loaders/humanml/utils/metrics.py, eval/a2m/action2motion/diversity.py and eval/a2m/stgcn/diversity.py are
IMPORTED here, at generation time only, and run on the inputs tests/humanml_metrics_helpers.py builds; the files hold data only.
The report records
  cases   per case: the `attempt` at which no row is fragile (for the two fixture cases: under the Gram-form margin too), the smallest
          margins, tau, the fp64 oracle's top-k counts and, where the reference can run (every group >= top_k), whether its summed
          top_k_mat equals them -- asserted for the fixture cases;
  e_ref   the reference's own relative error against the fp64 restatement, the maximum over POOL runs of the fixture's shape: the
          matching-score sum (its Gram form in fp32), diversity and multimodality (fp32 differences and norms), and the a2m floats
          (torch.dist sums accumulated in fp32)."""
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

import humanml_metrics_helpers as hh  # noqa: E402


def ref_loop(ref, text, motion, sizes):
    """eval_humanml.py's per-batch statements on the reference's functions: (summed top_k_mat, summed trace)."""
    topk, trace = 0, 0.0
    for b, e in hh.groups(sizes):
        dist_mat = ref.euclidean_distance_matrix(text[b:e], motion[b:e])
        trace += dist_mat.trace()
        topk = topk + ref.calculate_top_k(np.argsort(dist_mat, axis=1), top_k=hh.TOP_K).sum(axis=0)
    return np.asarray(topk, dtype=np.int64), float(trace)


def main(ref_root):
    sys.path.insert(0, ref_root)
    from data_loaders.humanml.utils import metrics as ref
    from eval.a2m.action2motion import diversity as ref_a2m
    from eval.a2m.stgcn import diversity as ref_stgcn
    torch.set_num_threads(4)
    report = {"cases": {}, "e_ref": {}}

    # ---- retrieval
    for name, c in hh.CASES.items():
        for attempt in range(hh.MAX_ATTEMPTS):
            text, motion = hh.case_input(name, attempt)
            bad, margin = hh.fragile_rows(text, motion, c["sizes"])
            bad_g, margin_g = hh.fragile_rows(text, motion, c["sizes"], gram=True) if c["fixture"] else (0, None)
            if bad == 0 and bad_g == 0:
                break
        else:
            raise AssertionError(f"case {name}: fragile rows in every one of {hh.MAX_ATTEMPTS} attempts")
        rank, diag, topk = hh.retrieval_fp64(text, motion, c["sizes"])
        entry = {"attempt": attempt, "min_margin": margin, "min_margin_gram": margin_g, "tau": hh.tau(c["D"]), "fp64_topk": topk.tolist(),
                 "rows": len(text)}
        if c["reference"]:
            ref_topk, ref_trace = ref_loop(ref, text, motion, c["sizes"])
            entry["reference_topk_equal"] = bool(np.array_equal(ref_topk, topk))
            entry["reference_has_nan"] = bool(np.isnan(ref_trace))
        if c["fixture"]:
            assert np.array_equal(ref_topk, topk), (name, ref_topk, topk)
            # the function under the reference's name says the same per group
            b, e = hh.groups(c["sizes"])[0]
            assert np.array_equal(ref.calculate_R_precision(text[b:e], motion[b:e], hh.TOP_K, sum_all=True),
                                  (rank[b:e, None] <= np.arange(hh.TOP_K)[None, :]).sum(axis=0))
            e_ref = 0.0
            for k in range(hh.POOL):
                tk, mk = hh.case_input(name, 1000 + k)
                want = hh.retrieval_fp64(tk, mk, c["sizes"])[1].sum()
                e_ref = max(e_ref, abs(ref_loop(ref, tk, mk, c["sizes"])[1] - want) / want)
            report["e_ref"][f"matching_case{name}"] = e_ref
            np.savez_compressed(os.path.join(hh.GOLDEN, f"humanml_metrics_case{name}.npz"), text=text, motion=motion,
                                sizes=np.array(c["sizes"], dtype=np.int64), ref_topk=ref_topk, ref_matching_sum=np.float64(ref_trace),
                                fp64_topk=topk, fp64_rank=rank, fp64_diag=diag, fp64_matching_sum=np.float64(diag.sum()))
        report["cases"][name] = entry
        print(f"case {name}: attempt {attempt}  margin {margin:.3e} (tau {hh.tau(c['D']):.3e})  top-k {topk.tolist()} of {len(text)}  "
              f"{ {k: v for k, v in entry.items() if k.startswith('reference')} }", flush=True)

    # ---- diversity and multimodality (humanml)
    for what, shape, times, fn in (("diversity", (80, 64), 30, ref.calculate_diversity), ("multimodality", (6, 8, 32), 5, ref.calculate_multimodality)):
        def restated(x, seed):
            np.random.seed(seed)
            n = x.shape[-2]
            first, second = np.random.choice(n, times, replace=False), np.random.choice(n, times, replace=False)
            x64 = x.astype(np.float64)
            return float(np.sqrt(((x64[..., first, :] - x64[..., second, :]) ** 2).sum(-1)).mean())
        e_ref = 0.0
        for k in range(hh.POOL + 1):
            x = hh.make_pair(int(np.prod(shape[:-1])), shape[-1], 5, 1.0, 8700 + 10 * k + len(shape))[1].reshape(shape)
            np.random.seed(8800 + k)
            got = float(fn(x, times))
            after = np.random.rand()
            want = restated(x, 8800 + k)
            e_ref = max(e_ref, abs(got - want) / want)
            if k == 0:
                np.savez_compressed(os.path.join(hh.GOLDEN, f"humanml_metrics_{what}.npz"), x=x, np_seed=np.int64(8800), times=np.int64(times),
                                    ref=np.float64(got), fp64=np.float64(want), rand_after=np.float64(after))
        report["e_ref"][what] = e_ref
        print(f"{what}: e_ref {e_ref:.3e} (relative, over {hh.POOL + 1} runs)", flush=True)

    # ---- a2m diversity / multimodality
    e_div = e_mm = 0.0
    for k in range(hh.POOL + 1):
        x, labels = hh.a2m_input(seed=8401 + 10 * k)
        seed = 8900 + k
        np.random.seed(seed)
        got_a = ref_a2m.calculate_diversity_multimodality(torch.from_numpy(x), torch.from_numpy(labels), 6)
        after = np.random.rand()
        got_s = ref_stgcn.calculate_diversity_multimodality(torch.from_numpy(x), torch.from_numpy(labels), 6, seed=seed)
        assert after == np.random.rand()
        want = hh.a2m_fp64(x, labels, 6, seed=seed)
        assert after == np.random.rand()                                        # the restated draw ends in the reference's state
        for got in (got_a, got_s):
            e_div, e_mm = max(e_div, abs(got[0] - want[0]) / want[0]), max(e_mm, abs(got[1] - want[1]) / want[1])
        if k == 0:
            first, second, pairs = hh.a2m_draw(labels, len(x), 6, seed=seed)
            np.savez_compressed(os.path.join(hh.GOLDEN, "humanml_metrics_a2m.npz"), x=x, labels=labels, num_labels=np.int64(6),
                                np_seed=np.int64(seed), ref_action2motion=np.array(got_a), ref_stgcn=np.array(got_s),
                                fp64_diversity=np.float64(want[0]), fp64_multimodality=np.float64(want[1]), first=first, second=second,
                                pairs=pairs, rand_after=np.float64(after))
    report["e_ref"]["a2m_diversity"], report["e_ref"]["a2m_multimodality"] = e_div, e_mm
    print(f"a2m: e_ref diversity {e_div:.3e} multimodality {e_mm:.3e}", flush=True)

    with open(hh.PIN_REPORT, "w") as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
    print("wrote", hh.PIN_REPORT)


if __name__ == "__main__":
    main(sys.argv[1])
