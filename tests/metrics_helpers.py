"""Checker of mdm_amd/metrics.py: the case tables, seeded input generators, fp64 restatements in numpy written from the metrics'
equations, the decision margin of precision / recall, and the loaders of tests/golden/metrics_*.npz and PIN_REPORT_metrics.json
(written by tests/make_golden_metrics.py from the reference's own functions).

Inputs.  I.i.d. Gaussian features in 256 dimensions are useless for precision / recall (distances concentrate: 0.0 / 1.0), so the
features have a low intrinsic dimension: Z [N, q] P [q, D] + 0.02 noise, clamped at 0 (the ST-GCN's features follow a ReLU), q = 4 .. 8;
the "generated" set has latent coordinate 0 shifted by 0.7 and scaled by 0.8.

Decision margin.  tau = 4 (D + 4) 2^-24: four times the worst-case relative rounding of a D-term fp32 sum of squares.  In fp64, with
r(a') the k-NN radius and d(b, a') the distance, a row b is ROBUST if some a' has (r - d) / r >= tau (it is inside, whatever the
rounding) or every a' has that ratio <= -tau (it is outside); any other row is FRAGILE.  Every P/R case must have zero fragile rows:
a condition on the inputs (the seed moves until it holds; `attempt` in the table below), asserted again by `pr_oracle`.  Under it the
membership bitmaps equal the fp64 oracle's exactly.

Restated (kid.py, the `unbiased` estimator): K = (gamma X Y^T + coef0)^degree; with Kt the matrices without their diagonals,
  mmd2 = (sum Kt_XX + sum Kt_YY) / (m (m - 1)) - 2 sum K_XY / m^2, and the variance estimate from zeta1 / zeta2 of `mmd_fp64`.

Bounds: radius^2 and pair distances relative (D + 4) 2^-24; mu / sigma max-abs (N + 8) 2^-52 4 max|x|^2 (both from the arithmetic);
mmd2 / var per subset 4 x e_ref, e_ref the reference's own error (fp32 sklearn kernel + numpy sums) against the restatement, pooled as
the maximum over >= 24 subset results per (D, regime, m) -- finer than per (D, regime): var scales with m, so a pool across subset
sizes would let the smallest m set the bound of all."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PIN_REPORT = os.path.join(GOLDEN, "PIN_REPORT_metrics.json")
T = 64                     # csrc/metrics.h MET_TILE: the row / column tile of every pair kernel
K = 3                      # precision_and_recall's k
U32 = 2.0 ** -24


def rel_bound(D):
    return (D + 4) * U32


def tau(D):
    return 4 * rel_bound(D)


def stats_bound(x):
    N = x.shape[0]
    return (N + 8) * 2.0 ** -52 * 4 * float(np.abs(x).max()) ** 2


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def make_features(N, D, q, seed, generated=False):
    """[N, D] fp32.  The projection P depends on (D, q, seed) only, so a real and a generated set of one seed share it."""
    P = np.random.RandomState(seed).standard_normal((q, D)) / np.sqrt(q)
    rs = np.random.RandomState(seed + (500001 if generated else 1))
    Z = rs.standard_normal((N, q))
    if generated:
        Z[:, 0] = 0.8 * Z[:, 0] + 0.7
    return np.maximum(Z @ P + 0.02 * rs.standard_normal((N, D)), 0.0).astype(np.float32)


def _pr(NA, NB, D, q, seed, fixture=False):
    return dict(NA=NA, NB=NB, D=D, q=q, seed=seed, fixture=fixture)


# name -> A is the real set [NA, D], B the generated set [NB, D].  N: k + 1, T - 1, T, T + 1, 2 T + 1; NA != NB; D = 256, 30, 1.
PR_CASES = {
    "4x4_d256": _pr(K + 1, K + 1, 256, 4, 1101),
    "63x63_d256": _pr(T - 1, T - 1, 256, 6, 1102),
    "64x64_d30": _pr(T, T, 30, 5, 1103),
    "65x65_d256": _pr(T + 1, T + 1, 256, 8, 1104, fixture=True),
    "129x63_d256": _pr(2 * T + 1, T - 1, 256, 6, 1105),
    "63x129_d30": _pr(T - 1, 2 * T + 1, 30, 4, 1106),
    "130x130_d30": _pr(130, 130, 30, 5, 1107, fixture=True),
    "65x65_d1": _pr(T + 1, T + 1, 1, 4, 1108),
    "129x129_d1": _pr(2 * T + 1, 2 * T + 1, 1, 4, 1109),
}
EMU_PR_CASES = ["4x4_d256", "63x63_d256", "64x64_d30", "129x63_d256", "63x129_d30", "65x65_d1"]


def pr_input(name, attempt=None):
    """(A = real, B = generated) of a case; the seed moves by `attempt` (the pin report's) until no row is fragile."""
    c = PR_CASES[name]
    if attempt is None:
        attempt = pin_report()["pr"][name]["attempt"]
    seed = c["seed"] + 100000 * attempt
    return make_features(c["NA"], c["D"], c["q"], seed), make_features(c["NB"], c["D"], c["q"], seed, generated=True)


def _kid(Ng, Nr, D, m, S, seed, regime="deg3", fixture=False):
    return dict(Ng=Ng, Nr=Nr, D=D, m=m, S=S, seed=seed, regime=regime, fixture=fixture)


REGIMES = {"deg3": {}, "deg2": dict(degree=2, gamma=0.05, coef0=0.5)}
# m: 3, T - 1, T + 1, 2 T + 1; S: 1 and 5; m < Ng: sampling with replacement (duplicated rows in a subset); m == Ng == Nr: without.
KID_CASES = {
    "m3_d256": _kid(40, 37, 256, 3, 5, 2101),
    "m63_d256": _kid(63, 63, 256, T - 1, 1, 2102),                    # without replacement
    "m65_d256": _kid(90, 80, 256, T + 1, 5, 2103),
    "m129_d256": _kid(129, 129, 256, 2 * T + 1, 1, 2104),             # without replacement
    "m3_d30": _kid(20, 25, 30, 3, 1, 2105),
    "m63_d30": _kid(100, 70, 30, T - 1, 5, 2106),
    "m65_d30": _kid(65, 65, 30, T + 1, 1, 2107),                      # without replacement
    "m129_d30": _kid(150, 140, 30, 2 * T + 1, 5, 2108),
    "m65_d30_deg2": _kid(80, 90, 30, T + 1, 5, 2109, regime="deg2"),
    "m3_d1": _kid(9, 9, 1, 3, 5, 2110),
    "m65_d1": _kid(70, 66, 1, T + 1, 1, 2111),
    "m129_d1": _kid(129, 129, 1, 2 * T + 1, 5, 2112),                 # without replacement
    "fixture": _kid(70, 70, 256, 33, 8, 2113, fixture=True),
}
EMU_KID_CASES = ["m3_d30", "m63_d30", "m65_d30", "m129_d30", "m65_d30_deg2", "m3_d1", "m65_d1"]
POOL_MIN = 24


def kid_input(name):
    c = KID_CASES[name]
    return make_features(c["Ng"], c["D"], 6, c["seed"]), make_features(c["Nr"], c["D"], 6, c["seed"], generated=True)


def kid_draw(name, S=None, np_seed=None):
    """The index tables [S, m] of a case, drawn as kid.py draws them: g then r per subset, on numpy's global generator."""
    c = KID_CASES[name]
    S = c["S"] if S is None else S
    np.random.seed(c["seed"] if np_seed is None else np_seed)
    replace = c["m"] < c["Ng"]
    ig, ir = [], []
    for _ in range(S):
        ig.append(np.random.choice(c["Ng"], c["m"], replace=replace))
        ir.append(np.random.choice(c["Nr"], c["m"], replace=replace))
    return np.stack(ig), np.stack(ir)


def pool_key(name):
    c = KID_CASES[name]
    return f"D{c['D']}/{c['regime']}/m{c['m']}"


STATS_CASES = {"65x256": (T + 1, 256, 3101), "129x30": (2 * T + 1, 30, 3102), "2x1": (2, 1, 3103), "33x17": (33, 17, 3104)}
EMU_STATS_CASES = ["129x30", "2x1", "33x17"]
DIST_CASES = {"200_d256": (65, 256, 200, 4101), "257_d30": (40, 30, 257, 4102), "1_d1": (5, 1, 1, 4103)}      # (N, D, P, seed)


def stats_input(name):
    N, D, seed = STATS_CASES[name]
    return make_features(N, D, 5, seed)


def dist_input(name):
    N, D, P, seed = DIST_CASES[name]
    rs = np.random.RandomState(seed + 7)
    first, second = rs.randint(0, N, P), rs.randint(0, N, P)
    if P > 3:
        second[3] = first[3]                 # a pair of one row with itself: exactly 0
    return make_features(N, D, 5, seed), first, second


# ---- fp64 restatements ------------------------------------------------------------------------------------------------------------------
def dist2_fp64(A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    return ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)


def radii2_fp64(A, k=K):
    """The (k+1)-th smallest squared distance of every row, self included."""
    return np.sort(dist2_fp64(A, A), axis=1)[:, k]


def margins(A, B, k=K):
    """(member [NB] bool, margin [NB]): per row of B the fp64 decision and how far it is from flipping -- max over a' of (r - d) / r
    for a member, min over a' of -(r - d) / r for a non-member.  A zero radius (k + 1 equal rows) is exact: d == 0 is inside."""
    r = np.sqrt(radii2_fp64(A, k))[None, :]
    d = np.sqrt(dist2_fp64(B, A))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(r > 0, (r - d) / r, np.where(d == 0, np.inf, -np.inf))
    best = ratio.max(axis=1)
    member = best >= 0
    return member, np.where(member, best, -best)


def pr_oracle(A, B, k=K):
    """(members of B in A's manifold, members of A in B's manifold) in fp64, with the zero-fragile-rows condition asserted."""
    out = []
    for X, Y in ((A, B), (B, A)):
        member, margin = margins(X, Y, k)
        assert (margin >= tau(X.shape[1])).all(), f"fragile rows: smallest margin {margin.min():.3e} < tau {tau(X.shape[1]):.3e}"
        out.append(member)
    return out


def poly_kernel_fp64(X, Y, degree=3, gamma=None, coef0=1):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    gamma = 1.0 / X.shape[1] if gamma is None else gamma
    return (gamma * (X @ Y.T) + coef0) ** degree


def mmd_fp64(X, Y, var_at_m, degree=3, gamma=None, coef0=1):
    """(mmd2, var) of two code matrices [m, D] in fp64: the unbiased MMD^2 estimate of the polynomial kernel and the estimate of its
    variance at var_at_m samples (Sutherland et al., arXiv:1611.04488, appendix; the form kid.py evaluates)."""
    Kxx, Kyy, Kxy = (poly_kernel_fp64(a, b, degree, gamma, coef0) for a, b in ((X, X), (Y, Y), (X, Y)))
    m = Kxx.shape[0]
    dx, dy = np.diagonal(Kxx), np.diagonal(Kyy)
    rx, ry = Kxx.sum(1) - dx, Kyy.sum(1) - dy                   # row sums without the diagonal
    c0, c1 = Kxy.sum(0), Kxy.sum(1)
    sx, sy, sxy = rx.sum(), ry.sum(), Kxy.sum()
    mmd2 = (sx + sy) / (m * (m - 1)) - 2 * sxy / (m * m)
    x2, y2, xy2 = (Kxx ** 2).sum() - (dx ** 2).sum(), (Kyy ** 2).sum() - (dy ** 2).sum(), (Kxy ** 2).sum()
    dots = rx @ c1 + ry @ c0
    common = (sx ** 2 + sy ** 2) / (m * (m - 1)) ** 2 + 2 * sxy ** 2 / m ** 4
    zeta1 = ((rx @ rx - x2 + ry @ ry - y2) / (m * (m - 1) * (m - 2)) - common + (c1 @ c1 + c0 @ c0 - 2 * xy2) / (m * m * (m - 1))
             - 2 * dots / (m * m * (m - 1)) + 2 * (sx + sy) * sxy / (m ** 3 * (m - 1)))
    zeta2 = ((x2 + y2) / (m * (m - 1)) - common + 2 * xy2 / (m * m) - 4 * dots / (m * m * (m - 1))
             + 4 * (sx + sy) * sxy / (m ** 3 * (m - 1)))
    v = var_at_m
    return mmd2, 4 * (v - 2) / (v * (v - 1)) * zeta1 + 2 / (v * (v - 1)) * zeta2


def kid_fp64(g, r, idx_g, idx_r, **kernel_args):
    """(mmd2 [S], var [S]) of the subsets of the index tables, var_at_m = min(len) as polynomial_mmd_averages sets it."""
    m = min(len(g), len(r))
    out = [mmd_fp64(g[a], r[b], m, **kernel_args) for a, b in zip(idx_g, idx_r)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def stats_fp64(x):
    x = np.asarray(x, dtype=np.float64)
    return x.mean(axis=0), np.atleast_2d(np.cov(x, rowvar=False))


def pair_dist_fp64(x, first, second):
    x = np.asarray(x, dtype=np.float64)
    return np.sqrt(((x[first] - x[second]) ** 2).sum(-1))


# ---- fixtures and the report -------------------------------------------------------------------------------------------------------------
_REPORT = None


def pin_report():
    global _REPORT
    if _REPORT is None:
        with open(PIN_REPORT) as fh:
            _REPORT = json.load(fh)
    return _REPORT


def kid_bound(name):
    """(4 x pooled e_ref of mmd2, 4 x pooled e_ref of var) of the case's (D, regime, m)."""
    p = pin_report()["pooled"][pool_key(name)]
    assert p["results"] >= POOL_MIN
    return 4 * p["e_ref_mmd2"], 4 * p["e_ref_var"]


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, f"metrics_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def rel_err(got, want):
    """max relative error; a wanted 0 must be met exactly."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == 0, 0.0, np.inf))
    return float(e.max())


# ---- the checks both backends run (the emulator on host tensors, the MI355X on cuda tensors; mdm_amd.metrics is bound by the file) ------
def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def check_pr_case(name, dev):
    """radius^2 within the relative bound; both membership bitmaps equal the fp64 oracle's; the fractions equal the reference's floats."""
    from mdm_amd import metrics as M
    c, rep = PR_CASES[name], pin_report()["pr"][name]
    A, B = pr_input(name)
    in_a, in_b = pr_oracle(A, B)
    for X, Y, want_members, ref in ((A, B, in_a, rep["precision_ref"]), (B, A, in_b, rep["recall_ref"])):
        r2 = M.knn_radii(_t(X, dev), K)
        e = rel_err(r2.cpu().numpy(), radii2_fp64(X))
        print(f"[metrics] pr {name}: radius^2 rel err {e:.3e} (bound {rel_bound(c['D']):.3e})")
        assert r2.dtype.is_floating_point and r2.shape == (len(X),) and e <= rel_bound(c["D"])
        member, count = M.manifold_members(_t(X, dev), r2, _t(Y, dev))
        assert np.array_equal(member.cpu().numpy().astype(bool), want_members)
        assert int(count.item()) == int(want_members.sum())
        assert M.manifold_estimate(_t(X, dev), _t(Y, dev), K) == ref
    if c["NA"] == c["NB"]:
        assert M.precision_and_recall(_t(B, dev), _t(A, dev)) == (rep["precision_ref"], rep["recall_ref"])


def check_kid_case(name, dev):
    """mmd2 and var of every subset within 4 x e_ref of the restatement, through polynomial_mmd_averages under the case's seed."""
    from mdm_amd import metrics as M
    c, kw = KID_CASES[name], REGIMES[KID_CASES[name]["regime"]]
    g, r = kid_input(name)
    ig, ir = kid_draw(name)
    want = kid_fp64(g, r, ig, ir, **kw)
    np.random.seed(c["seed"])
    got = M.polynomial_mmd_averages(_t(g, dev), _t(r, dev), n_subsets=c["S"], subset_size=c["m"], **kw)
    bm, bv = kid_bound(name)
    em, ev = float(np.abs(got[0] - want[0]).max()), float(np.abs(got[1] - want[1]).max())
    print(f"[metrics] kid {name}: mmd2 err {em:.3e} (bound {bm:.3e})  var err {ev:.3e} (bound {bv:.3e})")
    assert got[0].dtype == got[1].dtype == np.float64 and got[0].shape == got[1].shape == (c["S"],)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert em <= bm and ev <= bv
    if c["m"] < c["Ng"]:
        assert any(len(set(row)) < len(row) for row in ig) or c["m"] == 3      # sampling with replacement: duplicated rows in a subset
    return got


def check_stats_case(name, dev):
    from mdm_amd import metrics as M
    x = stats_input(name)
    mu, sigma = M.calculate_activation_statistics(_t(x, dev))
    wm, ws = stats_fp64(x)
    em, es = float(np.abs(mu.cpu().numpy() - wm).max()), float(np.abs(sigma.cpu().numpy() - ws).max())
    print(f"[metrics] stats {name}: mu err {em:.3e} sigma err {es:.3e} (bound {stats_bound(x):.3e})")
    assert mu.dtype == sigma.dtype and str(mu.dtype) == "torch.float64" and sigma.shape == (x.shape[1], x.shape[1])
    assert em <= stats_bound(x) and es <= stats_bound(x)
    assert np.array_equal(sigma.cpu().numpy(), sigma.cpu().numpy().T)


def check_dist_case(name, dev):
    from mdm_amd import metrics as M
    x, first, second = dist_input(name)
    dist, mean = M.gather_dist(_t(x, dev), first, second)
    want = pair_dist_fp64(x, first, second)
    e = rel_err(dist.cpu().numpy(), want)
    print(f"[metrics] dist {name}: rel err {e:.3e} (bound {rel_bound(x.shape[1]):.3e})")
    assert e <= rel_bound(x.shape[1])
    # the mean is the fp64 mean of the returned fp32 values, up to the rounding of P fp64 additions
    again = dist.cpu().numpy().astype(np.float64).mean()
    assert abs(float(mean.item()) - again) <= (len(first) + 2) * 2.0 ** -52 * abs(again)
    assert mean.dim() == 0 and str(mean.dtype) == "torch.float64"


def duplicates_input(D=30, N=T + 6):
    """A: row 5 repeated K + 1 times (rows 5, 17, T, T + 3: two tiles).  B: row 0 equals it, row 1 is at distance 1e-3 from it and
    far from everything else, the other rows are A's row 0 shifted far away."""
    A = make_features(N, D, 5, 6101) + 1.0
    A[5] += 50.0                              # the repeated row, far from every other row
    for i in (17, T, T + 3):
        A[i] = A[5]
    B = np.stack([A[5], A[5], A[0] + 500.0, A[1] - 500.0]).astype(np.float32)
    B[1, 0] += 1e-3
    return A.astype(np.float32), B


def check_duplicates(dev):
    from mdm_amd import metrics as M
    A, B = duplicates_input()
    r2 = M.knn_radii(_t(A, dev), K).cpu().numpy()
    for i in (5, 17, T, T + 3):
        assert r2[i] == 0.0                                        # exactly: direct differences of equal rows
    assert (np.delete(r2, [5, 17, T, T + 3]) > 0).all()
    assert float(np.sqrt(dist2_fp64(B[1:2], A).min())) > 0.9e-3
    member, count = M.manifold_members(_t(A, dev), _t(r2, dev), _t(B, dev))
    assert member.cpu().numpy().tolist() == [1, 0, 0, 0] and int(count.item()) == 1


def check_pair_invariance(dev):
    """radius^2 of a row: the same bits after a permutation of A, with far-away rows in front (the row lands in another tile) and
    in a repeated call."""
    from mdm_amd import metrics as M
    for D in (256, 30):
        A = make_features(T + 9, D, 6, 6201)
        base = M.knn_radii(_t(A, dev), K).cpu().numpy()
        assert np.array_equal(base, M.knn_radii(_t(A, dev), K).cpu().numpy())
        perm = np.random.RandomState(6202).permutation(len(A))
        assert np.array_equal(base[perm], M.knn_radii(_t(A[perm], dev), K).cpu().numpy())
        far = (make_features(T - 3, D, 6, 6203) + 1000.0).astype(np.float32)
        moved = M.knn_radii(_t(np.concatenate([far, A]), dev), K).cpu().numpy()
        assert np.array_equal(base, moved[len(far):])
        # k is a run-time value: every k from 1 to 7 against the oracle's order statistics
        d2 = np.sort(dist2_fp64(A, A), axis=1)
        for k in range(1, 8):
            assert rel_err(M.knn_radii(_t(A, dev), k).cpu().numpy(), d2[:, k]) <= rel_bound(D)


def check_subset_independence(dev):
    """mmd2 / var of a subset: the same bits alone and as subset 3 of 5; and per SUBSET_CHUNK."""
    from mdm_amd import metrics as M
    g, r = kid_input("m65_d30")
    ig, ir = kid_draw("m65_d30", S=5, np_seed=6301)
    five = M._poly_mmd(_t(g, dev), _t(r, dev), ig, ir, 3, None, 1, 65)
    alone = M._poly_mmd(_t(g, dev), _t(r, dev), ig[3:4], ir[3:4], 3, None, 1, 65)
    assert five[0][3] == alone[0][0] and five[1][3] == alone[1][0]
    old = M.SUBSET_CHUNK
    try:
        M.SUBSET_CHUNK = 2
        cut = M._poly_mmd(_t(g, dev), _t(r, dev), ig, ir, 3, None, 1, 65)
    finally:
        M.SUBSET_CHUNK = old
    assert np.array_equal(five[0], cut[0]) and np.array_equal(five[1], cut[1])


def raw_calls(lib, dev, stream, ws_fill, out_fill):
    """All five native calls at shapes with a partial tile, on workspaces filled with `ws_fill` bytes and outputs pre-filled with
    `out_fill`: every output as numpy."""
    import torch
    A, B = pr_input("63x129_d30")
    g, r = kid_input("m65_d30")
    ig, ir = kid_draw("m65_d30", S=2, np_seed=6401)
    D, m = 30, 65

    def ws(kind, rows, subsets=1):
        n = lib.mdm_metrics_workspace_bytes(kind, rows, subsets)
        assert n > 0
        return torch.full((n,), ws_fill, dtype=torch.uint8, device=dev), n

    def out(shape, dtype):
        if dtype in (torch.uint8, torch.int32):
            return torch.full(shape, 0x7F if out_fill != 0 else 0, dtype=dtype, device=dev)
        return torch.full(shape, out_fill, dtype=dtype, device=dev)

    a, b, gt, rt = _t(A, dev), _t(B, dev), _t(g, dev), _t(r, dev)
    igt, irt = _t(ig.astype(np.int32), dev), _t(ir.astype(np.int32), dev)
    r2, member, count = out((len(A),), torch.float32), out((len(B),), torch.uint8), out((), torch.int32)
    w, n = ws(0, len(A))
    assert lib.mdm_knn_radius(a.data_ptr(), len(A), D, K, r2.data_ptr(), w.data_ptr(), n, stream) == 0
    w1, n = ws(1, len(B))
    assert lib.mdm_manifold_members(a.data_ptr(), r2.data_ptr(), len(A), b.data_ptr(), len(B), D, member.data_ptr(), count.data_ptr(),
                                    w1.data_ptr(), n, stream) == 0
    first, second = _t(np.arange(40, dtype=np.int32), dev), _t(np.arange(40, dtype=np.int32)[::-1].copy(), dev)
    dist, mean = out((40,), torch.float32), out((), torch.float64)
    w2, n = ws(2, len(A))
    assert lib.mdm_gather_dist(a.data_ptr(), len(A), D, first.data_ptr(), second.data_ptr(), 40, dist.data_ptr(), mean.data_ptr(),
                               w2.data_ptr(), n, stream) == 0
    mmd2, var = out((2,), torch.float64), out((2,), torch.float64)
    w3, n = ws(3, m, 2)
    assert lib.mdm_poly_mmd(gt.data_ptr(), len(g), rt.data_ptr(), len(r), D, igt.data_ptr(), irt.data_ptr(), 2, m, 1.0 / D, 1.0, 3, 65,
                            mmd2.data_ptr(), var.data_ptr(), w3.data_ptr(), n, stream) == 0
    mu, sigma = out((D,), torch.float64), out((D, D), torch.float64)
    w4, n = ws(4, len(A))
    assert lib.mdm_feature_stats(a.data_ptr(), len(A), D, mu.data_ptr(), sigma.data_ptr(), w4.data_ptr(), n, stream) == 0
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(r2=r2, member=member, count=count, dist=dist, mean=mean, mmd2=mmd2, var=var, mu=mu,
                                                sigma=sigma).items()}


def check_poison(lib, dev, stream):
    """A 0xFF-filled workspace and NaN-filled outputs: finite results, the bits of a run over zeros (which is also the determinism
    check of every output: two calls, the same bits)."""
    clean = raw_calls(lib, dev, stream, 0, 0.0)
    dirty = raw_calls(lib, dev, stream, 0xFF, float("nan"))
    for k in clean:
        assert np.isfinite(dirty[k]).all(), k
        assert np.array_equal(clean[k], dirty[k]), k
    return clean


def check_fixtures(dev):
    """The reference's own runs (tests/golden/metrics_*.npz): its precision / recall floats exactly; its KID subsets under its seed;
    its statistics, FID and diversity."""
    from mdm_amd import metrics as M
    for name in ("65x65_d256", "130x130_d30"):
        z = load_fixture(f"pr_{name}")
        got = M.precision_and_recall(_t(z["generated"], dev), _t(z["real"], dev))
        assert got == (float(z["ref_precision"]), float(z["ref_recall"]))
        assert 0.0 < got[0] < 1.0 and 0.0 < got[1] < 1.0 and got[0] != got[1]
    z = load_fixture("kid")
    np.random.seed(int(z["np_seed"]))
    mmd2, var = M.polynomial_mmd_averages(_t(z["g"], dev), _t(z["r"], dev), n_subsets=8, subset_size=33)
    after = np.random.rand()
    np.random.seed(int(z["np_seed"]))
    ig, ir = kid_draw("fixture")
    assert np.array_equal(ig, z["idx_g"]) and np.array_equal(ir, z["idx_r"]) and after == np.random.rand()
    bm, bv = kid_bound("fixture")
    em, ev = float(np.abs(mmd2 - z["fp64_mmd2"]).max()), float(np.abs(var - z["fp64_var"]).max())
    print(f"[metrics] kid fixture: mmd2 err {em:.3e} (bound {bm:.3e}) var err {ev:.3e} (bound {bv:.3e}); vs the reference's fp32 run "
          f"{np.abs(mmd2 - z['ref_mmd2']).max():.3e} {np.abs(var - z['ref_var']).max():.3e}")
    assert em <= bm and ev <= bv
    z = load_fixture("stats")
    s1, s2 = M.calculate_activation_statistics(_t(z["x1"], dev)), M.calculate_activation_statistics(_t(z["x2"], dev))
    for (mu, sigma), x, wm, ws in ((s1, z["x1"], z["fp64_mu1"], z["fp64_sigma1"]), (s2, z["x2"], z["fp64_mu2"], z["fp64_sigma2"])):
        assert np.abs(mu.cpu().numpy() - wm).max() <= stats_bound(x) and np.abs(sigma.cpu().numpy() - ws).max() <= stats_bound(x)
    fid = M.calculate_fid(s1, s2)
    print(f"[metrics] fid fixture: {fid:.9f}  the reference on its fp32 statistics {float(z['ref_fid']):.9f}  on fp64 {float(z['ref_fid_of_fp64']):.9f}")
    assert abs(fid - float(z["ref_fid_of_fp64"])) <= 1e-9 * abs(float(z["ref_fid_of_fp64"]))
    assert abs(fid - float(z["ref_fid"])) <= 1e-4 * abs(float(z["ref_fid"]))         # (the reference's mean is an fp32 sum)
    z = load_fixture("diversity")
    np.random.seed(int(z["np_seed"]))
    div = M.calculate_diversity(_t(z["x"], dev))
    assert div.dim() == 0 and div.device == _t(z["x"], dev).device
    assert abs(float(div.item()) - float(z["fp64_diversity"])) <= rel_bound(256) * float(z["fp64_diversity"])
    assert abs(float(div.item()) - float(z["ref_diversity"])) <= 1e-5 * float(z["ref_diversity"])
