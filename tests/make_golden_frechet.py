"""Writes tests/golden/frechet_<case>.npz for the cases of tests/frechet_helpers.py and PIN_REPORT_frechet.json.

Run on the CPU, with the reference checkout's path:   python tests/make_golden_frechet.py /path/to/motion-diffusion-model

The reference's three copies of calculate_frechet_distance -- eval/a2m/action2motion/fid.py, eval/a2m/stgcn/fid.py and
data_loaders/humanml/utils/metrics.py -- are IMPORTED here, at generation time only, and run on the fp64 statistics of the inputs
frechet_helpers.make_sets builds; they must return the same float (recorded as `copies_agree`).  The files hold data only: the fp32
feature matrices x1, x2, their statistics mu1, sigma1, mu2, sigma2 (np.mean / np.cov of the promoted features), `ref` (the
reference's value), `alt` (numpy eigh on the formula of csrc/frechet.h), d = |ref - alt| and S = Tr sigma1 + Tr sigma2 + |mu1 - mu2|^2.
The report holds d / S, the rank of sigma1 and the tolerance the tests derive from them, per case."""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import frechet_helpers as fh  # noqa: E402

REF_MODULES = ("eval/a2m/action2motion/fid.py", "eval/a2m/stgcn/fid.py", "data_loaders/humanml/utils/metrics.py")


def _load(ref_root, rel):
    # by file: the three modules import numpy and scipy only, their packages' __init__ files the whole evaluation stack
    spec = importlib.util.spec_from_file_location("ref_" + rel.replace("/", "_")[:-3], os.path.join(ref_root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_root):
    refs = [_load(ref_root, rel) for rel in REF_MODULES]
    report = {}
    for name, (D, N, seed) in fh.CASES.items():
        x1, x2 = fh.make_sets(D, N, seed)
        (mu1, s1), (mu2, s2) = fh.stats_fp64(x1), fh.stats_fp64(x2)
        values = [float(m.calculate_frechet_distance(mu1, s1, mu2, s2)) for m in refs]
        agree = values[0] == values[1] == values[2]
        assert agree, (name, values)
        ref, alt = values[0], fh.frechet_eigh(mu1, s1, mu2, s2)[0]
        d, S = abs(ref - alt), fh.scale_of(mu1, s1, mu2, s2)
        np.savez_compressed(os.path.join(fh.GOLDEN, f"frechet_{name}.npz"), x1=x1, x2=x2, mu1=mu1, sigma1=s1, mu2=mu2, sigma2=s2,
                            ref=np.float64(ref), alt=np.float64(alt), d=np.float64(d), S=np.float64(S))
        report[name] = {"D": D, "N": N, "seed": seed, "ref": ref, "alt": alt, "d_over_S": d / S, "S": S, "copies_agree": bool(agree),
                        "rank_sigma1": int(np.linalg.matrix_rank(s1)), "bound_over_S": fh.bound(d, S) / S}
        print(f"{name}: ref {ref:.12g}  d / S {d / S:.3e}  bound / S {fh.bound(d, S) / S:.3e}  rank {report[name]['rank_sigma1']} of {D}", flush=True)
    with open(fh.PIN_REPORT, "w") as fh_out:
        json.dump(report, fh_out, indent=1, sort_keys=True)
    print("wrote", fh.PIN_REPORT)


if __name__ == "__main__":
    main(sys.argv[1])
