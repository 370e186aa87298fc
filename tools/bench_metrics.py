"""Measures mdm_amd/metrics.py on one MI355X at the unconstrained evaluation's size (N = 1000 features of D = 256 per set) and writes
profiles/r18a_metrics.md:
  * precision_and_recall, calculate_kid (100 subsets of 1000), calculate_activation_statistics and calculate_diversity: per call, the
    device span (HIP events) and the host wall time ending in a synchronise -- median / min / max of --calls calls after two warm calls;
  * next to each, the host path a user runs today, timed once in the same session on the same features.  With --reference PATH (a
    checkout of the reference) these are the reference's own functions; without it -- the reference tree is not part of this
    repository -- they are this tool's restatements on the same library calls (one torch.norm per pair of device rows and
    np.partition; sklearn's polynomial_kernel on fp32 subsets and numpy sums; np.mean / np.cov of the array brought to the host; 200
    torch.dist calls), and the note says which ran.  The host precision / recall runs at --pr-rows rows (default 250) and is scaled
    by (N / rows)^2: it issues 3 N^2 tiny launches with a host round trip each;
  * the accuracy figures of the same session: every KID, precision / recall, statistics and distance case of tests/metrics_helpers.py.
There is no speed gate: the note is the record.

    python tools/bench_metrics.py [--calls 10] [--pr-rows 250] [--reference PATH] [--out profiles/r18a_metrics.md]

With --frechet it measures the two FID paths instead and writes profiles/r19a_frechet.md: `calculate_fid` (the host path: the device
statistics copied to the host, scipy's sqrtm) against `calculate_fid_device(check=False)` followed by one synchronise, interleaved
call by call, at D = 30, 256 and 512; per D the sweeps both solves used, the launches the call enqueues, the host time of the
enqueue alone, and the same call on diagonal statistics, where every launch behind the first sweep returns at once (the price of the
sweeps that are enqueued and not needed).

    python tools/bench_metrics.py --frechet [--calls 10] [--out profiles/r19a_frechet.md]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import metrics_helpers as mh  # noqa: E402

DEV = "cuda:0"
N, D = 1000, 256


# ---- the host path, restated on the reference's library calls (used when no reference checkout is given) --------------------------------
def host_manifold_estimate(A, B, k):
    A, B = list(A), list(B)
    radius = []
    for a in A:
        d = np.zeros(len(A))
        for i, a2 in enumerate(A):
            d[i] = torch.norm(a - a2, 2)
        radius.append(np.partition(d, k)[k])
    n = 0
    for b in B:
        for a2, r in zip(A, radius):
            if torch.norm(b - a2, 2) <= r:
                n += 1
                break
    return n / len(B)


def host_precision_and_recall(generated, real):
    return host_manifold_estimate(real, generated, 3), host_manifold_estimate(generated, real, 3)


def host_kid(real, generated, n_subsets=100, subset_size=1000):
    from sklearn.metrics.pairwise import polynomial_kernel
    m = min(len(real), len(generated))
    replace = subset_size < len(real)
    out = np.zeros(n_subsets)
    for i in range(n_subsets):
        X = real[np.random.choice(len(real), subset_size, replace=replace)]
        Y = generated[np.random.choice(len(generated), subset_size, replace=replace)]
        Kxx, Kyy, Kxy = polynomial_kernel(X), polynomial_kernel(Y), polynomial_kernel(X, Y)
        s = Kxx.shape[0]
        rx, ry = Kxx.sum(1) - np.diagonal(Kxx), Kyy.sum(1) - np.diagonal(Kyy)
        out[i] = (rx.sum() + ry.sum()) / (s * (s - 1)) - 2 * Kxy.sum(0).sum() / (s * s)
        # (the variance estimate's further sums, which kid.py takes too: squares of the three matrices and four dot products)
        _ = (Kxx.ravel() @ Kxx.ravel(), Kyy.ravel() @ Kyy.ravel(), Kxy.ravel() @ Kxy.ravel(), rx @ Kxy.sum(1), ry @ Kxy.sum(0), m)
    return out.mean(), out.std()


def host_statistics(x):
    a = x.cpu().detach().numpy()
    return np.mean(a, axis=0), np.cov(a, rowvar=False)


def host_diversity(x):
    first, second = np.random.randint(0, len(x), 200), np.random.randint(0, len(x), 200)
    total = 0
    for i, j in zip(first, second):
        total += torch.dist(x[i, :], x[j, :])
    return total / 200


def timed(fn, calls, warm=2):
    """(device span ms, wall ms) as (median, min, max) each."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return [(statistics.median(v), min(v), max(v)) for v in (dev, wall)]


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


FRECHET_SIZES = ((30, 1000), (256, 1000), (512, 4000))      # (D, N): the GRU recogniser's, the ST-GCN's and the HumanML3D evaluator's widths


def frechet_launches(D):
    """Kernel launches mdm_frechet_distance enqueues at D (csrc/frechet_api.h)."""
    n = (D + 1) & ~1
    solve = 2 if n <= 64 else 1 + 30 * (n - 1) + 1
    return 2 + solve + 1 + 2 + 1 + solve + 1


def spread(v):
    return f"{statistics.median(v):.3f} | {min(v):.3f} | {max(v):.3f}"


def frechet_main(a):
    import frechet_helpers as fh
    from mdm_amd import _native as nat
    from mdm_amd import metrics as M
    lib = nat.load_native()
    out = a.out if a.out else os.path.join(ROOT, "profiles", "r19a_frechet.md")
    lines = ["# r19a — the Frechet distance on the device (csrc/frechet.h) against the host path, on the MI355X", "",
             f"Device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Written by `tools/bench_metrics.py --frechet`.", "",
             f"Per D: seeded anisotropic Gaussians (tests/frechet_helpers.py make_sets), statistics from `calculate_activation_statistics` "
             f"on the device; two warm calls of each path, then {a.calls} calls of each, interleaved host / device call by call.  `host`: "
             "`calculate_fid` on the device statistics (copy to the host included, scipy sqrtm).  `device`: "
             "`calculate_fid_device(check=False)` and one synchronise; `enqueue` is the host time of that call before the synchronise; "
             "`diagonal`: the same call on diagonal covariances, where no sweep rotates and all launches behind sweep 0 return at once.", "",
             "| D | N | host ms median | min | max | device ms median | min | max | enqueue ms median | min | max | diagonal ms median | min | max "
             "| sweeps | launches | host / device | abs(device - host) / S |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for D, N in FRECHET_SIZES:
        x1, x2 = fh.make_sets(D, N, 8200 + D)
        s1 = M.calculate_activation_statistics(torch.from_numpy(x1).to(DEV))
        s2 = M.calculate_activation_statistics(torch.from_numpy(x2).to(DEV))
        dg1, dg2 = (s1[0], torch.diag(torch.diagonal(s1[1])).contiguous()), (s2[0], torch.diag(torch.diagonal(s2[1])).contiguous())
        host_np = [t.cpu().numpy() for t in (*s1, *s2)]
        _, sw = fh.raw_call(lib, DEV, *host_np)
        for _ in range(2):
            ref = M.calculate_fid(s1, s2)
            got = M.calculate_fid_device(s1, s2, check=False)
            M.calculate_fid_device(dg1, dg2, check=False)
        torch.cuda.synchronize()
        host, dev, enq, diag = [], [], [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            ref = M.calculate_fid(s1, s2)
            host.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            got = M.calculate_fid_device(s1, s2, check=False)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            dev.append((time.perf_counter() - t0) * 1e3)
            enq.append((t1 - t0) * 1e3)
            t0 = time.perf_counter()
            M.calculate_fid_device(dg1, dg2, check=False)
            torch.cuda.synchronize()
            diag.append((time.perf_counter() - t0) * 1e3)
        S = fh.scale_of(*host_np)
        lines.append(f"| {D} | {N} | {spread(host)} | {spread(dev)} | {spread(enq)} | {spread(diag)} | {sw.tolist()} | {frechet_launches(D)} | "
                     f"{statistics.median(host) / statistics.median(dev):.2f} x | {abs(got.item() - ref) / S:.2e} |")
    lines += ["", "Not measured: per-kernel times (no traced run) and the share of any peak.  No speed gate applies; the option is off by "
              "default.", ""]
    with open(out, "w") as fh_out:
        fh_out.write("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--pr-rows", type=int, default=250)
    ap.add_argument("--reference", default=None, help="a checkout of the reference: time its own functions instead of the restatements")
    ap.add_argument("--out", default=None, help="default: profiles/r18a_metrics.md (with --frechet: profiles/r19a_frechet.md)")
    ap.add_argument("--frechet", action="store_true", help="measure the two FID paths instead (profiles/r19a_frechet.md)")
    a = ap.parse_args()
    assert torch.cuda.is_available()
    if a.frechet:
        return frechet_main(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "r18a_metrics.md")
    from mdm_amd import metrics as M

    if a.reference:
        sys.path.insert(0, a.reference)
        from eval.unconstrained.metrics.precision_recall import precision_and_recall as ref_pr
        from eval.unconstrained.metrics.kid import calculate_kid as ref_kid
        from eval.a2m.action2motion.diversity import calculate_diversity as ref_div
        which = "the reference's own functions"
    else:
        ref_pr, ref_kid, ref_div = host_precision_and_recall, host_kid, host_diversity
        which = "this tool's restatements of the reference's functions on the same library calls (no reference checkout was given)"

    real_n, gen_n = mh.make_features(N, D, 8, 8101), mh.make_features(N, D, 8, 8101, generated=True)
    real, gen = torch.from_numpy(real_n).to(DEV), torch.from_numpy(gen_n).to(DEV)
    rows = []

    # precision / recall: the host path at --pr-rows rows, scaled by (N / rows)^2
    (dm, dl, dh), (wm, wl, wh) = timed(lambda: M.precision_and_recall(gen, real), a.calls)
    pr = M.precision_and_recall(gen, real)
    small = M.precision_and_recall(gen[:a.pr_rows], real[:a.pr_rows])
    host_ms, host_pr = once(lambda: ref_pr(gen[:a.pr_rows], real[:a.pr_rows]))
    scale = (N / a.pr_rows) ** 2
    rows.append(("precision_and_recall", dm, dl, dh, wm, wl, wh, host_ms * scale,
                 f"host: {host_ms / 1e3:.1f} s at N = {a.pr_rows}, scaled by {scale:.0f}; at that N both return {small} / {tuple(host_pr)}; "
                 f"N = 1000: {pr}"))
    # KID
    np.random.seed(1)
    (dm, dl, dh), (wm, wl, wh) = timed(lambda: M.calculate_kid(real, gen), a.calls)
    np.random.seed(2)
    kid = M.calculate_kid(real, gen)
    np.random.seed(2)
    host_ms, host_kid_v = once(lambda: ref_kid(real_n, gen_n))
    rows.append(("calculate_kid (100 x 1000)", dm, dl, dh, wm, wl, wh, host_ms,
                 f"same seed: {kid[0]:.9f} ({kid[1]:.3e}) / host fp32 {host_kid_v[0]:.9f} ({host_kid_v[1]:.3e})"))
    # statistics
    (dm, dl, dh), (wm, wl, wh) = timed(lambda: M.calculate_activation_statistics(gen), a.calls)
    mu, sigma = M.calculate_activation_statistics(gen)
    host_ms, (hmu, hsigma) = once(lambda: host_statistics(gen))
    f64 = mh.stats_fp64(gen_n)
    rows.append(("calculate_activation_statistics", dm, dl, dh, wm, wl, wh, host_ms,
                 f"max-abs vs fp64: sigma {np.abs(sigma.cpu().numpy() - f64[1]).max():.2e} / host {np.abs(hsigma - f64[1]).max():.2e} "
                 f"(np.mean / np.cov after .cpu(): the statement of evaluate.py)"))
    # diversity
    np.random.seed(3)
    (dm, dl, dh), (wm, wl, wh) = timed(lambda: M.calculate_diversity(gen), a.calls)
    np.random.seed(4)
    div = M.calculate_diversity(gen)
    np.random.seed(4)
    host_ms, host_div = once(lambda: ref_div(gen))
    rows.append(("calculate_diversity", dm, dl, dh, wm, wl, wh, host_ms, f"same seed: {div.item():.6f} / host {float(host_div):.6f}"))

    lines = ["# r18a — the metrics of the unconstrained evaluation (csrc/metrics.h) on the MI355X", "",
             f"Device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Written by `tools/bench_metrics.py`.", "",
             f"## Timings at N = {N} features per set, D = {D}", "",
             f"HIP path: {a.calls} calls after two warm calls; `device` is the span between HIP events around the call, `wall` a host clock "
             "around the call and a synchronise (it includes the host's random draws, index uploads and result copies).  Host path: "
             f"{which}, timed ONCE in the same session.", "",
             "| function | device ms median | min | max | wall ms median | min | max | host path ms | wall speed-up | note |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, dm, dl, dh, wm, wl, wh, host_ms, note in rows:
        lines.append(f"| `{name}` | {dm:.3f} | {dl:.3f} | {dh:.3f} | {wm:.3f} | {wl:.3f} | {wh:.3f} | {host_ms:.1f} | {host_ms / wm:.0f} x | {note} |")
    lines += ["", "Not measured: per-kernel times (no traced run), the share of any peak, the host path more than once (its spread is unknown), "
              "and the host precision / recall at N = 1000 (scaled from the smaller run as stated).  No speed gate applies.", "",
              "## Accuracy in the same session", "",
              "KID: max-abs error of mmd2 / var per case against the fp64 restatement, next to the pooled e_ref of the reference's own fp32 "
              "run (`tests/golden/PIN_REPORT_metrics.json`); the bound is 4 x e_ref.", "",
              "| case | mmd2 error | e_ref | error / e_ref | var error | e_ref | error / e_ref |", "|---|---|---|---|---|---|---|"]
    for name, c in mh.KID_CASES.items():
        g, r = mh.kid_input(name)
        ig, ir = mh.kid_draw(name)
        want = mh.kid_fp64(g, r, ig, ir, **mh.REGIMES[c["regime"]])
        np.random.seed(c["seed"])
        got = M.polynomial_mmd_averages(torch.from_numpy(g).to(DEV), torch.from_numpy(r).to(DEV), n_subsets=c["S"], subset_size=c["m"],
                                        **mh.REGIMES[c["regime"]])
        bm, bv = mh.kid_bound(name)
        em, ev = np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max()
        lines.append(f"| {name} | {em:.3e} | {bm / 4:.3e} | {4 * em / bm:.3f} | {ev:.3e} | {bv / 4:.3e} | {4 * ev / bv:.3f} |")
    lines += ["", "Precision / recall: radius^2 against fp64 (bound: relative (D + 4) 2^-24), membership bitmaps against the fp64 oracle.", "",
              "| case | radius^2 relative error | bound | bitmaps equal | precision, recall (= the reference's floats) |", "|---|---|---|---|---|"]
    for name, c in mh.PR_CASES.items():
        A, B = mh.pr_input(name)
        in_a, in_b = mh.pr_oracle(A, B)
        ta, tb = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
        ra, rb = M.knn_radii(ta, 3), M.knn_radii(tb, 3)
        e = max(mh.rel_err(ra.cpu().numpy(), mh.radii2_fp64(A)), mh.rel_err(rb.cpu().numpy(), mh.radii2_fp64(B)))
        eq = np.array_equal(M.manifold_members(ta, ra, tb)[0].cpu().numpy().astype(bool), in_a) and \
            np.array_equal(M.manifold_members(tb, rb, ta)[0].cpu().numpy().astype(bool), in_b)
        rep = mh.pin_report()["pr"][name]
        same = (M.manifold_estimate(ta, tb, 3), M.manifold_estimate(tb, ta, 3)) == (rep["precision_ref"], rep["recall_ref"])
        lines.append(f"| {name} | {e:.3e} | {mh.rel_bound(c['D']):.3e} | {'yes' if eq else 'NO'} | {rep['precision_ref']:.4f}, "
                     f"{rep['recall_ref']:.4f}: {'equal' if same else 'DIFFERENT'} |")
    lines.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
