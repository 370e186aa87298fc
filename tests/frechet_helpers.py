"""Checker of mdm_amd.metrics.frechet_distance_device (csrc/frechet.h behind mdm_frechet_distance): the case table, the seeded input
generator, the loaders of tests/golden/frechet_*.npz and PIN_REPORT_frechet.json (written by tests/make_golden_frechet.py from the
reference's own calculate_frechet_distance), and the checks the emulator and the MI355X both run.

Inputs.  N samples of an anisotropic Gaussian in D dimensions (per-axis scales exp(N(0, 1)), a mean shift; the second set mixed by
I + 0.3 G / sqrt(D)), fp32.  The statistics are np.mean(axis=0) and np.cov(rowvar=False) of the features promoted to fp64 (on the fp32
array np.mean adds in fp32 and the reference then forms |mu1 - mu2|^2 in fp32: 1e-7 of it, which is not what this test is about).

Tolerance.  Per case `ref` is the reference's value (scipy sqrtm), `alt` numpy's eigh on  Tr sqrtm(S1 S2) = sum sqrt(eig(S^T S2 S)),
d = |ref - alt| the disagreement of these two independent fp64 evaluations -- about 1e-13 S at full rank, 1e-9 S when N < D, where the
problem takes square roots of eigenvalues at rounding level -- and S = Tr S1 + Tr S2 + |mu1 - mu2|^2.  The device value must lie
within max(100 d, 1e-11 S) of `ref`: a correct third algorithm stands within a few d; a dropped or mis-paired rotation moves the value
by 1e-6 S and more; the floor covers D <= 3, where d is 0 or an ulp.  Every check prints |got - ref| / S, d / S and the sweeps first.

D: 1, 2, 3 (an odd D has a pad pair), 15, 16, 17 (the MFMA tile edge), 30 (the GRU recogniser), 33 with N = 20 (rank-deficient: the
floor of the rotation criterion, rounding-level negative eigenvalues clamped), 64 and 65 (the last D of the one-launch form and the
first of the launch-per-round form, odd as well)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PIN_REPORT = os.path.join(GOLDEN, "PIN_REPORT_frechet.json")
SMALL_MAX = 64             # csrc/frechet.h FR_SMALL_MAX: n = D rounded up to even; n <= 64 is one launch per solve
MAX_SWEEPS = 30            # FR_MAX_SWEEPS: also what sweeps2 holds for a solve that did not converge
EPS = 2.0 ** -52

# name -> (D, N, seed)
CASES = {"d1": (1, 10, 7101), "d2": (2, 10, 7102), "d3": (3, 10, 7103), "d15": (15, 40, 7115), "d16": (16, 40, 7116),
         "d17": (17, 40, 7117), "d30": (30, 100, 7130), "d33_n20": (33, 20, 7133), "d64": (64, 200, 7164), "d65": (65, 200, 7165)}


def make_sets(D, N, seed):
    """(x1, x2) fp32 [N, D]."""
    rs = np.random.RandomState(seed)
    scale = np.exp(rs.standard_normal(D))
    x1 = rs.standard_normal((N, D)) * scale + rs.standard_normal(D)
    mix = np.eye(D) + 0.3 * rs.standard_normal((D, D)) / np.sqrt(D)
    x2 = (rs.standard_normal((N, D)) * scale) @ mix + 0.1
    return x1.astype(np.float32), x2.astype(np.float32)


def stats_fp64(x):
    x = np.asarray(x, dtype=np.float64)
    return x.mean(axis=0), np.atleast_2d(np.cov(x, rowvar=False))


def scale_of(mu1, s1, mu2, s2):
    return float(np.trace(s1) + np.trace(s2) + (mu1 - mu2) @ (mu1 - mu2))


def frechet_eigh(mu1, s1, mu2, s2):
    """`alt`: the formula of csrc/frechet.h in numpy -- (distance, sum of the roots)."""
    w, V = np.linalg.eigh((s1 + s1.T) / 2)
    S = V * np.sqrt(np.maximum(w, 0.0))
    M = S.T @ ((s2 + s2.T) / 2) @ S
    lam = np.linalg.eigvalsh((M + M.T) / 2)
    root = float(np.sqrt(np.maximum(lam, 0.0)).sum())
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2 * root), root


def bound(d, S):
    return max(100.0 * d, 1e-11 * S)


_REPORT = None


def pin_report():
    global _REPORT
    if _REPORT is None:
        with open(PIN_REPORT) as fh:
            _REPORT = json.load(fh)
    return _REPORT


_FIX = {}


def load_case(name):
    """The fixture of a case, loaded once and shared (read-only): x1, x2, mu1, sigma1, mu2, sigma2, ref, alt, d, S."""
    if name not in _FIX:
        with np.load(os.path.join(GOLDEN, f"frechet_{name}.npz")) as z:
            _FIX[name] = {k: z[k] for k in z.files}
        for v in _FIX[name].values():
            v.setflags(write=False)
    return _FIX[name]


def stats_of(name):
    z = load_case(name)
    return z["mu1"], z["sigma1"], z["mu2"], z["sigma2"]


# ---- the native call on raw buffers (the test-only path: it reads result4 and sweeps2) -------------------------------------------------
def _t(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(dev)      # (the fixtures are shared and read-only)


def raw_call(lib, dev, mu1, s1, mu2, s2, ws_fill=0, stream=None):
    """(result4, sweeps2) as numpy arrays from mdm_frechet_distance on a workspace filled with `ws_fill` bytes."""
    import torch
    D = len(mu1)
    n = lib.mdm_frechet_workspace_bytes(D)
    assert n > 0
    ws = torch.full((n,), ws_fill, dtype=torch.uint8, device=dev)
    res = torch.full((4,), float("nan"), dtype=torch.float64, device=dev)
    sw = torch.full((2,), -1, dtype=torch.int32, device=dev)
    args = [_t(np.asarray(a, dtype=np.float64), dev) for a in (mu1, s1, mu2, s2)]
    if stream is None and str(dev).startswith("cuda"):
        stream = torch.cuda.current_stream().cuda_stream
    rc = lib.mdm_frechet_distance(args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), args[3].data_ptr(), D, res.data_ptr(),
                                  sw.data_ptr(), ws.data_ptr(), n, stream)
    assert rc == 0, lib.mdm_last_error()
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()
    return res.cpu().numpy(), sw.cpu().numpy()


def form_of(D):
    return "small" if ((D + 1) & ~1) <= SMALL_MAX else "round"


# ---- the checks both backends run (mdm_amd.metrics is bound to its library by the test file) -------------------------------------------
def check_case(name, lib, dev):
    """The module's value and the raw call's within the rule of `ref`; the solves converged, in the form the case claims."""
    from mdm_amd import metrics as M
    z = load_case(name)
    D = CASES[name][0]
    mu1, s1, mu2, s2 = stats_of(name)
    ref, d, S = float(z["ref"]), float(z["d"]), float(z["S"])
    res, sw = raw_call(lib, dev, mu1, s1, mu2, s2)
    got = M.frechet_distance_device(_t(mu1, dev), _t(s1, dev), _t(mu2, dev), _t(s2, dev))
    print(f"[frechet] {name}: |got - ref| / S {abs(res[0] - ref) / S:.3e}  d / S {d / S:.3e}  bound / S {bound(d, S) / S:.3e}  sweeps "
          f"{sw.tolist()}  ({form_of(D)} form)  min/max w {res[2]:.3e} lambda {res[3]:.3e}")
    assert got.dim() == 0 and str(got.dtype) == "torch.float64" and str(got.device).startswith(str(dev).split(":")[0])
    assert float(got.item()) == res[0]                                    # the module returns the call's [0], the same bits
    assert abs(res[0] - ref) <= bound(d, S)
    assert 0 <= sw[0] < MAX_SWEEPS and 0 <= sw[1] < MAX_SWEEPS
    assert form_of(D) == ("small" if D <= 64 else "round")
    if D == 1:
        assert sw.tolist() == [0, 0]                                      # one pair, with the pad: nothing to rotate
    if D >= 15:
        assert sw[0] >= 2                                                 # (a dense matrix is not diagonal after one sweep)
    assert abs(res[1] - frechet_eigh(mu1, s1, mu2, s2)[1]) <= bound(d, S)
    return res, sw


def check_solve_alone(name, lib, dev):
    """Each eigen-solve on its own.  sigma2 = I: M = S^T S = diag(max(w, 0)) up to rounding, so the second solve only clears rounding-level
    elements (two sweeps at the most) and [1] = sum sqrt(w) -- compared with numpy's under |sqrt a - sqrt b| <= sqrt|a - b| per eigenvalue.  sigma2 = sigma1:
    M = diag(w^2), whose roots add up to the eigenvalue sum, so [1] = Tr sigma1 to D 2^-50 Tr (each of ~10 D rotations per diagonal
    element moves the trace by an ulp of it at most, with either sign)."""
    mu1, s1, _, _ = stats_of(name)
    D = len(mu1)
    tr = float(np.trace(s1))
    res, sw = raw_call(lib, dev, mu1, s1, mu1, np.eye(D))
    w = np.linalg.eigvalsh(s1)
    want = float(np.sqrt(np.maximum(w, 0.0)).sum())
    slack = D * np.sqrt(D * 2.0 ** -50 * np.abs(w).max())
    print(f"[frechet] {name} alone: sum sqrt(w) err {abs(res[1] - want):.3e} (slack {slack:.3e})  sweeps {sw.tolist()}")
    assert abs(res[1] - want) <= slack and sw[0] < MAX_SWEEPS and sw[1] <= 2
    res2, sw2 = raw_call(lib, dev, mu1, s1, mu1, s1)
    print(f"[frechet] {name} twice: |sum w - Tr| / Tr {abs(res2[1] - tr) / tr:.3e} (bound {D * 2.0 ** -50:.3e})  sweeps {sw2.tolist()}")
    assert abs(res2[1] - tr) <= D * 2.0 ** -50 * tr
    assert sw2[0] == sw[0] and sw2[1] < MAX_SWEEPS


def check_identical(name, lib, dev):
    mu1, s1, _, _ = stats_of(name)
    S = 2 * float(np.trace(s1))
    res, sw = raw_call(lib, dev, mu1, s1, mu1, s1)
    print(f"[frechet] {name} identical: |fid| / S {abs(res[0]) / S:.3e}  sweeps {sw.tolist()}")
    assert abs(res[0]) <= 1e-11 * S


def check_zero_sigma1(name, lib, dev):
    """sigma1 = 0: a singular product without an eps retry -- finite, |mu1 - mu2|^2 + Tr sigma2 up to the order of D additions."""
    mu1, s1, mu2, s2 = stats_of(name)
    D = len(mu1)
    res, sw = raw_call(lib, dev, mu1, np.zeros_like(s1), mu2, s2)
    want = float((mu1 - mu2) @ (mu1 - mu2) + np.trace(s2))
    print(f"[frechet] {name} sigma1 = 0: {res[0]:.12g} want {want:.12g}  sweeps {sw.tolist()}")
    assert np.isfinite(res[0]) and abs(res[0] - want) <= (D + 2) * EPS * want and res[1] == 0.0 and sw[0] == 0


def asymmetric_pair(name):
    """(sigma, sigma + K): sigma the fixture's covariance rounded to multiples of 2^-20, K antisymmetric in multiples of 2^-20, so
    that every (s_ij + k_ij) + (s_ji + k_ji) is exact and equals s_ij + s_ji."""
    _, s1, _, _ = stats_of(name)
    q = np.round(s1 * 2.0 ** 20) / 2.0 ** 20
    q = (q + q.T) / 2
    k = np.triu(np.random.RandomState(7301).randint(-2 ** 18, 2 ** 18, s1.shape), 1) / 2.0 ** 20
    return q, q + k - k.T


def check_asymmetric(name, lib, dev):
    mu1, _, mu2, s2 = stats_of(name)
    q, a = asymmetric_pair(name)
    assert not np.array_equal(a, a.T) and np.array_equal((a + a.T) / 2, q)
    for first in (True, False):
        sym = raw_call(lib, dev, mu1, q, mu2, s2) if first else raw_call(lib, dev, mu2, s2, mu1, q)
        asym = raw_call(lib, dev, mu1, a, mu2, s2) if first else raw_call(lib, dev, mu2, s2, mu1, a)
        assert np.array_equal(sym[0], asym[0]) and np.array_equal(sym[1], asym[1]) and np.isfinite(sym[0]).all()


def check_not_psd(name, dev):
    """sigma2 negated: the product has no positive eigenvalue.  check=True refuses it as upstream refuses an imaginary root;
    check=False returns the clamped value."""
    import pytest
    from mdm_amd import metrics as M
    mu1, s1, mu2, s2 = stats_of(name)
    t = [_t(a, dev) for a in (mu1, s1, mu2, -s2)]
    with pytest.raises(ValueError, match="Imaginary component"):
        M.frechet_distance_device(*t, check=True)
    got = float(M.frechet_distance_device(*t, check=False).item())
    top = float((mu1 - mu2) @ (mu1 - mu2) + np.trace(s1) - np.trace(s2))
    print(f"[frechet] {name} sigma2 negated: clamped value {got:.9g}  (without any root {top:.9g})")
    assert np.isfinite(got) and got <= top + 1e-11 * abs(top)


def check_poison(name, lib, dev):
    """A 0xFF-filled workspace: the bits of a run over zeros, twice (which is also the determinism check)."""
    mu1, s1, mu2, s2 = stats_of(name)
    clean = raw_call(lib, dev, mu1, s1, mu2, s2, 0)
    dirty = raw_call(lib, dev, mu1, s1, mu2, s2, 0xFF)
    assert np.isfinite(clean[0]).all()
    assert np.array_equal(clean[0], dirty[0]) and np.array_equal(clean[1], dirty[1])
    return clean
