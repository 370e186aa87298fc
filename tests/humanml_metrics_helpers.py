"""Checker of mdm_amd/humanml_metrics.py, mdm_amd/humanml_eval.py and mdm_amd/a2m_metrics.py: the case tables, seeded inputs, fp64
restatements in numpy written from the metrics' equations, the fragile-row condition, the loaders of
tests/golden/humanml_metrics_*.npz and PIN_REPORT_humanml_metrics.json (written by tests/make_golden_humanml_metrics.py from the
reference's own functions), and the checks both backends run (the emulator on host tensors, the MI355X on cuda tensors).

Inputs.  I.i.d. Gaussian embeddings retrieve nothing, so text and motion share a low-rank latent (metrics_helpers.make_features'
recipe without the clamp): text = Z P + 0.02 e, motion = (Z + s e') P + 0.02 e'', Z [N, q], P [q, D] / sqrt(q).  At s = 1 about a third
of the rows retrieve their own motion first.

Fragile rows.  tau = 4 (D + 4) 2^-24 (metrics_helpers.tau).  Row i of a group is FRAGILE if some j != i of the group has
|d2_ij - d2_ii| < tau max(d2_ij, d2_ii) in fp64: rounding could then move its rank.  Every case has zero fragile rows, a condition on
the inputs (the seed moves by `attempt`, recorded in the pin report, until it holds), asserted again by `retrieval_oracle`; under it
`rank` equals the fp64 oracle's exactly.  The two fixture cases hold the same inequality with max(...) replaced by
|q_i|^2 + |c_i|^2 + |c_j|^2, the scale of the reference's Gram-form rounding; under that the reference's summed top_k_mat equals ours.

Bounds.  diag, matrix entries, pair distances: relative (D + 4) 2^-24 against fp64.  diag_sum and the means: the fp64 sum of the
returned fp32 values to (n + 2) 2^-52 relative.  diag_sum, the means and the a2m floats against the reference's value: 4 x e_ref, e_ref
the reference's own error against the restatement (Gram form in fp32; fp32 accumulation in the a2m sums), pooled as the maximum
relative error over POOL runs of the fixture's shape.  topk_count, confusion and pred: exact."""
import json
import os

import numpy as np

from metrics_helpers import T, U32, dist2_fp64, pair_dist_fp64, rel_bound, rel_err, tau      # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PIN_REPORT = os.path.join(GOLDEN, "PIN_REPORT_humanml_metrics.json")
TOP_K = 3
POOL = 24
MAX_ATTEMPTS = 32


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def make_pair(N, D, q, s, seed):
    """(text, motion) [N, D] fp32 on one latent."""
    P = np.random.RandomState(seed).standard_normal((q, D)) / np.sqrt(q)
    rs = np.random.RandomState(seed + 1)
    Z = rs.standard_normal((N, q))
    text = Z @ P + 0.02 * rs.standard_normal((N, D))
    motion = (Z + s * rs.standard_normal((N, q))) @ P + 0.02 * rs.standard_normal((N, D))
    return text.astype(np.float32), motion.astype(np.float32)


def _case(sizes, D, s, q, seed, fixture=False, reference=True):
    return dict(sizes=sizes, D=D, s=s, q=q, seed=seed, fixture=fixture, reference=reference)


# group sizes at every edge of the 64-row tile and of top_k, mixed inside one call; D = 512 (eight feature chunks), 30 and 1
CASES = {
    "1": _case([32, 32, 32], 512, 1.0, 6, 8101, fixture=True),
    "2": _case([32, 32, 7], 512, 1.0, 5, 8102),
    "3": _case([3, 31, 33], 512, 1.0, 7, 8103),
    "4": _case([64, 65], 512, 1.0, 8, 8104),
    "5": _case([63, 4, 32], 512, 1.5, 6, 8105, fixture=True),
    "6": _case([65, 129], 30, 0.8, 4, 8106),
    "7": _case([32, 32], 1, 0.3, 4, 8107),
    "8": _case([129], 512, 1.0, 6, 8108),
    "9": _case([1, 2, 1], 30, 1.0, 4, 8109, reference=False),       # groups below top_k: the reference raises; fp64 oracle only
}
DIST_MATRIX_CASES = {"63x129_d30": (63, 129, 30, 8201), "129x63_d30": (129, 63, 30, 8202), "65x65_d512": (65, 65, 512, 8203),
                     "5x3_d1": (5, 3, 1, 8204)}
CONFUSION_CASES = {"1_c12": (1, 12, 8301), "63_c40": (63, 40, 8302), "65_c12": (65, 12, 8303), "257_c40": (257, 40, 8304),
                   "65_c1": (65, 1, 8305), "257_c12": (257, 12, 8306)}


def case_input(name, attempt=None):
    c = CASES[name]
    if attempt is None:
        attempt = pin_report()["cases"][name]["attempt"]
    return make_pair(sum(c["sizes"]), c["D"], c["q"], c["s"], c["seed"] + 100000 * attempt)


def dist_matrix_input(name):
    NA, NB, D, seed = DIST_MATRIX_CASES[name]
    a, _ = make_pair(NA, D, 5, 1.0, seed)
    _, b = make_pair(NB, D, 5, 1.0, seed)
    b[1] = a[2]                                  # equal rows: exactly 0 (the Gram form gives a rounding-sized number or nan)
    return a, b


def confusion_input(name):
    """(yhat [N, C], labels [N]): scores on a grid of 8 values (equal maxima in most rows); where N allows, one row with a NaN in
    front of its maximum, one with two NaNs, and two labels out of range (-1 and C)."""
    N, C, seed = CONFUSION_CASES[name]
    rs = np.random.RandomState(seed)
    yhat = (rs.randint(0, 8, (N, C)) / 4.0 - 1.0).astype(np.float32)
    labels = rs.randint(0, C, N).astype(np.int32)
    if N >= 8:
        yhat[3, C // 2] = np.nan
        yhat[5, C - 1] = np.nan
        yhat[5, 0] = np.nan if C > 1 else yhat[5, 0]
        labels[2], labels[N - 1] = -1, C
    return yhat, labels


# ---- fp64 restatements ------------------------------------------------------------------------------------------------------------------
def groups(sizes):
    o = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(o[i]), int(o[i + 1])) for i in range(len(sizes))]


def fragile_rows(text, motion, sizes, gram=False):
    """The number of fragile rows, and the smallest margin |d2_ij - d2_ii| / scale over all rows."""
    D = text.shape[1]
    n_bad, smallest = 0, np.inf
    for b, e in groups(sizes):
        if e - b < 2:
            continue
        d2 = dist2_fp64(text[b:e], motion[b:e])
        dii = np.diagonal(d2)[:, None]
        if gram:
            q2 = (text[b:e].astype(np.float64) ** 2).sum(1)
            c2 = (motion[b:e].astype(np.float64) ** 2).sum(1)
            scale = q2[:, None] + c2[:, None] + c2[None, :]
        else:
            scale = np.maximum(d2, dii)
        with np.errstate(divide="ignore", invalid="ignore"):
            margin = np.where(scale > 0, np.abs(d2 - dii) / scale, np.inf)
        np.fill_diagonal(margin, np.inf)
        n_bad += int((margin < tau(D)).any(axis=1).sum())
        smallest = min(smallest, float(margin.min()))
    return n_bad, smallest


def retrieval_fp64(text, motion, sizes, top_k=TOP_K):
    """(rank [N], diag [N], topk_count [top_k]) in fp64: rank by the stable rule."""
    rank, diag = np.zeros(len(text), dtype=np.int64), np.zeros(len(text))
    for b, e in groups(sizes):
        d2 = dist2_fp64(text[b:e], motion[b:e])
        dii = np.diagonal(d2)
        j, i = np.meshgrid(np.arange(e - b), np.arange(e - b))
        rank[b:e] = ((d2 < dii[:, None]) | ((d2 == dii[:, None]) & (j < i))).sum(axis=1)
        diag[b:e] = np.sqrt(dii)
    return rank, diag, np.array([(rank <= k).sum() for k in range(top_k)], dtype=np.int64)


def retrieval_oracle(text, motion, sizes, top_k=TOP_K):
    n_bad, smallest = fragile_rows(text, motion, sizes)
    assert n_bad == 0, f"{n_bad} fragile rows: smallest margin {smallest:.3e} < tau {tau(text.shape[1]):.3e}"
    return retrieval_fp64(text, motion, sizes, top_k)


def host_retrieval_loop(batches, top_k=TOP_K):
    """What the host loop of the evaluation script does with each batch of (text, motion) embeddings, restated in numpy on the
    library calls it makes: both tensors to the host, the Gram-form distance matrix in fp32, its trace, an argsort per row and the
    cumulative top-k hits.  (summed top-k counts, summed trace, rows); tools/bench_humanml_metrics.py times it."""
    topk, trace, rows = np.zeros(top_k, dtype=np.int64), 0.0, 0
    for text, motion in batches:
        a, b = text.cpu().numpy(), motion.cpu().numpy()
        dist = np.sqrt(-2 * np.dot(a, b.T) + np.sum(np.square(a), axis=1, keepdims=True) + np.sum(np.square(b), axis=1))
        trace += dist.trace()
        hit = np.argsort(dist, axis=1)[:, :top_k] == np.arange(len(a))[:, None]
        topk += (np.cumsum(hit, axis=1) > 0).sum(axis=0)
        rows += len(a)
    return topk, trace, rows


def argmax_rule(yhat):
    """The lowest index among equal maxima; a NaN counts as the maximum and the first NaN wins."""
    pred = np.zeros(len(yhat), dtype=np.int64)
    for n, row in enumerate(yhat):
        nans = np.flatnonzero(np.isnan(row))
        pred[n] = nans[0] if len(nans) else int(np.flatnonzero(row == row.max())[0])
    return pred


def confusion_fp64(yhat, labels, C):
    pred = argmax_rule(yhat)
    conf, bad = np.zeros((C, C), dtype=np.int64), 0
    for lab, p in zip(labels, pred):
        if 0 <= lab < C:
            conf[lab, p] += 1
        else:
            bad += 1
    return pred, conf, bad


def a2m_draw(labels, num_motions, num_labels, seed=None, unconstrained=False, times=(200, 20)):
    """The index sequence of diversity.py calculate_diversity_multimodality on numpy's global generator, restated: 200 + 200 uniform
    indices; then, until every label that appears has had 20 pairs: a first index (drawn again if its label's quota is spent), then
    second indices until one has the first's label."""
    if seed is not None:
        np.random.seed(seed)
    first, second = np.random.randint(0, num_motions, times[0]), np.random.randint(0, num_motions, times[0])
    pairs = []
    if not unconstrained:
        left = {int(lab): times[1] for lab in set(labels.tolist())}
        while any(v > 0 for v in left.values()):
            i = np.random.randint(0, num_motions)
            if left[int(labels[i])] <= 0:
                continue
            j = np.random.randint(0, num_motions)
            while labels[j] != labels[i]:
                j = np.random.randint(0, num_motions)
            left[int(labels[i])] -= 1
            pairs.append((i, j))
    return first, second, np.array(pairs, dtype=np.int64).reshape(-1, 2)


def a2m_fp64(x, labels, num_labels, seed=None, unconstrained=False):
    first, second, pairs = a2m_draw(labels, len(x), num_labels, seed, unconstrained)
    div = float(pair_dist_fp64(x, first, second).mean())
    if unconstrained:
        return div, float("nan")
    return div, float(pair_dist_fp64(x, pairs[:, 0], pairs[:, 1]).sum() / (20 * num_labels))


def a2m_input(N=96, D=64, num_labels=6, seed=8401):
    """Activations with a class structure; label num_labels - 1 does not appear (its quota stays zero)."""
    rs = np.random.RandomState(seed)
    labels = rs.randint(0, num_labels - 1, N).astype(np.int64)
    centres = rs.standard_normal((num_labels, D))
    return (centres[labels] + 0.5 * rs.standard_normal((N, D))).astype(np.float32), labels


# ---- fixtures and the report -------------------------------------------------------------------------------------------------------------
_REPORT = None


def pin_report():
    global _REPORT
    if _REPORT is None:
        with open(PIN_REPORT) as fh:
            _REPORT = json.load(fh)
    return _REPORT


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, f"humanml_metrics_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def sum_bound(n):
    return (n + 2) * 2.0 ** -52


# ---- the checks both backends run (mdm_amd.metrics.NATIVE_LIB is bound by the calling file) ---------------------------------------------
def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def check_retrieval_case(name, dev):
    """rank and topk_count equal the fp64 oracle's; diag within the relative bound; diag_sum is the fp64 sum of the returned diag;
    the reference-named functions say the same per group."""
    import torch
    from mdm_amd import humanml_metrics as H
    c = CASES[name]
    text, motion = case_input(name)
    want_rank, want_diag, want_topk = retrieval_oracle(text, motion, c["sizes"])
    rank, diag, topk, diag_sum = H.retrieval(_t(text, dev), _t(motion, dev), c["sizes"], TOP_K)
    e = rel_err(_np(diag), want_diag)
    again = _np(diag).astype(np.float64).sum()
    print(f"[humanml_metrics] case {name}: topk {_np(topk).tolist()} of {len(text)}  diag rel err {e:.3e} (bound {rel_bound(c['D']):.3e})  "
          f"diag_sum {float(diag_sum.item()):.9f} vs fp64 sum of diag {again:.9f}")
    assert rank.dtype == torch.int32 and diag.dtype == torch.float32 and topk.dtype == torch.int64 and diag_sum.dtype == torch.float64
    assert rank.device == diag.device == topk.device == diag_sum.device == _t(text, dev).device and diag_sum.dim() == 0
    assert np.array_equal(_np(rank), want_rank)
    assert np.array_equal(_np(topk), want_topk)
    assert e <= rel_bound(c["D"])
    assert abs(float(diag_sum.item()) - again) <= sum_bound(len(text)) * abs(again)
    if name == "1":
        assert 0 < want_topk[0] < want_topk[2] < len(text)                     # away from 0 and from 1
    # the reference's names, per group: R-precision as a boolean matrix and as sums, the matching score as a vector and as a sum
    for b, e_ in groups(c["sizes"])[:2]:
        tk = H.calculate_R_precision(_t(text[b:e_], dev), _t(motion[b:e_], dev), TOP_K)
        assert tk.dtype == torch.bool and tuple(tk.shape) == (e_ - b, TOP_K)
        assert np.array_equal(_np(tk), want_rank[b:e_, None] <= np.arange(TOP_K)[None, :])
        sums = H.calculate_R_precision(_t(text[b:e_], dev), _t(motion[b:e_], dev), TOP_K, sum_all=True)
        assert np.array_equal(_np(sums), _np(tk).sum(axis=0))
        if e_ - b >= TOP_K:
            order = np.argsort(dist2_fp64(text[b:e_], motion[b:e_]), axis=1, kind="stable")
            assert np.array_equal(_np(H.calculate_top_k(_t(order, dev), TOP_K)), _np(tk))
    ms = H.calculate_matching_score(_t(text, dev), _t(motion, dev))
    assert np.array_equal(_np(ms), _np(diag))                                  # the same bits in other groups
    total = H.calculate_matching_score(_t(text, dev), _t(motion, dev), sum_all=True)
    assert float(total.item()) == float(diag_sum.item())


def check_dist_matrix_case(name, dev):
    from mdm_amd import humanml_metrics as H
    a, b = dist_matrix_input(name)
    out = _np(H.euclidean_distance_matrix(_t(a, dev), _t(b, dev)))
    want = np.sqrt(dist2_fp64(a, b))
    e = rel_err(out, want)
    print(f"[humanml_metrics] dist matrix {name}: rel err {e:.3e} (bound {rel_bound(a.shape[1]):.3e})")
    assert out.shape == (len(a), len(b)) and out.dtype == np.float32 and np.isfinite(out).all()
    assert out[2, 1] == 0.0 and e <= rel_bound(a.shape[1])


def check_confusion_case(name, dev):
    import torch
    from mdm_amd import a2m_metrics as A
    N, C, _ = CONFUSION_CASES[name]
    yhat, labels = confusion_input(name)
    want_pred, want_conf, want_bad = confusion_fp64(yhat, labels, C)
    assert np.array_equal(want_pred, torch.from_numpy(yhat).max(dim=1).indices.numpy())          # the rule IS torch.max's on the CPU
    pred, conf, bad = A.confusion(_t(yhat, dev), _t(labels, dev), C)
    print(f"[humanml_metrics] confusion {name}: trace {int(np.trace(want_conf))} of {int(want_conf.sum())}, bad {want_bad}")
    assert conf.dtype == torch.int64 and pred.dtype == torch.int32
    assert np.array_equal(_np(pred), want_pred) and np.array_equal(_np(conf), want_conf) and int(bad.item()) == want_bad
    assert want_bad == (2 if N >= 8 else 0)


def check_confusion_accumulates(dev):
    """One call on 257 rows and three accumulating calls on its parts: the same matrix, predictions and bad count."""
    from mdm_amd import a2m_metrics as A
    yhat, labels = confusion_input("257_c12")
    pred, conf, bad = A.confusion(_t(yhat, dev), _t(labels, dev), 12)
    m = b = None
    parts = []
    for lo, hi in ((0, 1), (1, 66), (66, 257)):
        p, m, b = A.confusion(_t(yhat[lo:hi], dev), _t(labels[lo:hi], dev), 12, m, b)
        parts.append(_np(p))
    assert np.array_equal(np.concatenate(parts), _np(pred)) and np.array_equal(_np(m), _np(conf)) and int(b.item()) == int(bad.item()) == 2


def check_group_invariance(dev):
    """A group's rank / diag: the same bits alone, as part of a many-group call, behind other groups (another workgroup, another
    row offset, rows no longer 16-byte aligned relative to a tile) and in a repeated call."""
    from mdm_amd import humanml_metrics as H
    for D in (512, 30):
        text, motion = make_pair(70, D, 6, 1.0, 8501)
        alone = H.retrieval(_t(text, dev), _t(motion, dev), [70], TOP_K)
        again = H.retrieval(_t(text, dev), _t(motion, dev), [70], TOP_K)
        ft, fm = make_pair(37, D, 6, 1.0, 8502)
        both_t, both_m = np.concatenate([ft, text, ft[:5]]), np.concatenate([fm, motion, fm[:5]])
        many = H.retrieval(_t(both_t, dev), _t(both_m, dev), [3, 34, 70, 5], TOP_K)
        for k in (0, 1):
            assert np.array_equal(_np(alone[k]), _np(again[k]))
            assert np.array_equal(_np(alone[k]), _np(many[k])[37:107])
        assert np.array_equal(_np(alone[2]), _np(again[2])) and float(alone[3].item()) == float(again[3].item())
        # the first 34-row group of `many` alone
        sub = H.retrieval(_t(both_t[3:37], dev), _t(both_m[3:37], dev), [34], TOP_K)
        assert np.array_equal(_np(sub[0]), _np(many[0])[3:37]) and np.array_equal(_np(sub[1]), _np(many[1])[3:37])


def check_ties(dev):
    """Equal candidate rows rank by the tie rule (the lower index first); diag is exactly 0 where q_i == c_i."""
    from mdm_amd import humanml_metrics as H
    text, motion = make_pair(70, 30, 5, 1.0, 8601)
    motion[10] = text[10]                       # q_10 == c_10: distance 0, rank 0
    motion[20] = motion[66] = motion[3]         # three equal candidates, in two column tiles
    text[3] = text[20] = text[66] = motion[3] + 0.01        # their queries: equally far from all three, far nearer than any other
    rank, diag, topk, _ = H.retrieval(_t(text, dev), _t(motion, dev), [70], TOP_K)
    rank, diag = _np(rank), _np(diag)
    assert diag[10] == 0.0 and rank[10] == 0
    assert (rank[3], rank[20], rank[66]) == (0, 1, 2)
    assert diag[3] == diag[20] == diag[66] > 0
    want = retrieval_fp64(text, motion, [70])
    assert np.array_equal(rank[[3, 10, 20, 66]], want[0][[3, 10, 20, 66]])
    # groups below top_k: every row is a hit from the group's size on
    r, _, tk, _ = H.retrieval(_t(text[:4], dev), _t(motion[:4], dev), [1, 2, 1], TOP_K)
    assert _np(r).max() <= 1 and _np(tk)[1:].tolist() == [4, 4]
    full = H.calculate_R_precision(_t(text[:2], dev), _t(motion[:2], dev), TOP_K)
    assert _np(full)[:, 1:].all()


def raw_calls(lib, dev, stream, ws_fill, out_fill):
    """The three native calls at shapes with partial tiles, on workspaces filled with `ws_fill` bytes and outputs pre-filled with
    `out_fill` (the confusion matrix and `bad` are the call's inputs: zeros): every output as numpy."""
    import torch
    from mdm_amd import _native as nat
    text, motion = case_input("6")
    sizes, D = CASES["6"]["sizes"], CASES["6"]["D"]
    N = len(text)
    K = nat.METRICS_KINDS

    def ws(kind, rows):
        n = lib.mdm_metrics_workspace_bytes(kind, rows, 1)
        assert n > 0
        return torch.full((n,), ws_fill, dtype=torch.uint8, device=dev), n

    def out(shape, dtype):
        if not dtype.is_floating_point:
            return torch.full(shape, 0x7F if out_fill != 0 else 0, dtype=dtype, device=dev)
        return torch.full(shape, out_fill, dtype=dtype, device=dev)

    q, c = _t(text, dev), _t(motion, dev)
    off = _t(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), dev)
    rank, diag, topk, dsum = out((N,), torch.int32), out((N,), torch.float32), out((TOP_K,), torch.int64), out((), torch.float64)
    w, n = ws(K["retrieval_ranks"], N)
    assert lib.mdm_retrieval_ranks(q.data_ptr(), c.data_ptr(), N, D, off.data_ptr(), len(sizes), max(sizes), TOP_K, rank.data_ptr(),
                                   diag.data_ptr(), topk.data_ptr(), dsum.data_ptr(), w.data_ptr(), n, stream) == 0
    a, b = (_t(x, dev) for x in dist_matrix_input("63x129_d30"))
    mat = out((63, 129), torch.float32)
    w1, n = ws(K["dist_matrix"], 63)
    assert lib.mdm_dist_matrix(a.data_ptr(), 63, b.data_ptr(), 129, 30, mat.data_ptr(), w1.data_ptr(), n, stream) == 0
    yhat, labels = (_t(x, dev) for x in confusion_input("65_c12"))
    pred = out((65,), torch.int32)
    conf, bad = torch.zeros(12, 12, dtype=torch.int64, device=dev), torch.zeros((), dtype=torch.int32, device=dev)
    w2, n = ws(K["confusion"], 65)
    assert lib.mdm_confusion(yhat.data_ptr(), labels.data_ptr(), 65, 12, pred.data_ptr(), conf.data_ptr(), bad.data_ptr(), w2.data_ptr(),
                             n, stream) == 0
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()
    return {k: _np(v) for k, v in dict(rank=rank, diag=diag, topk=topk, dsum=dsum, mat=mat, pred=pred, conf=conf, bad=bad).items()}


def check_poison(lib, dev, stream):
    """0xFF workspaces and NaN / 0x7F outputs: finite results with the bits of a run over zeros (two calls: the same bits)."""
    clean = raw_calls(lib, dev, stream, 0, 0.0)
    dirty = raw_calls(lib, dev, stream, 0xFF, float("nan"))
    for k in clean:
        assert np.isfinite(dirty[k]).all(), k
        assert np.array_equal(clean[k], dirty[k]), k
    assert np.array_equal(clean["rank"], retrieval_oracle(*case_input("6"), CASES["6"]["sizes"])[0])
    return clean


def check_fixtures(dev):
    """The reference's own runs (tests/golden/humanml_metrics_*.npz): its summed top_k_mat exactly, its matching score, diversity,
    multimodality and a2m floats within 4 x e_ref, and numpy's generator in the reference's state after each draw."""
    from mdm_amd import a2m_metrics as A
    from mdm_amd import humanml_metrics as H
    rep = pin_report()
    for name in ("1", "5"):
        z = load_fixture(f"case{name}")
        sizes = [int(s) for s in z["sizes"]]
        _, _, topk, diag_sum = H.retrieval(_t(z["text"], dev), _t(z["motion"], dev), sizes, TOP_K)
        bound = 4 * rep["e_ref"][f"matching_case{name}"] * float(z["fp64_matching_sum"])
        err = abs(float(diag_sum.item()) - float(z["ref_matching_sum"]))
        print(f"[humanml_metrics] fixture case {name}: topk {_np(topk).tolist()} (reference {z['ref_topk'].tolist()})  matching sum vs the "
              f"reference {err:.3e} (bound {bound:.3e})")
        assert np.array_equal(_np(topk), z["ref_topk"]) and np.array_equal(_np(topk), z["fp64_topk"])
        assert err <= bound
    for what, call in (("diversity", lambda x, t: H.calculate_diversity(x, t)), ("multimodality", lambda x, t: H.calculate_multimodality(x, t))):
        z = load_fixture(what)
        np.random.seed(int(z["np_seed"]))
        got = call(_t(z["x"], dev), int(z["times"]))
        after = np.random.rand()
        bound = 4 * rep["e_ref"][what] * float(z["fp64"])
        err = abs(float(got.item()) - float(z["ref"]))
        print(f"[humanml_metrics] fixture {what}: {float(got.item()):.9f} vs the reference {err:.3e} (bound {bound:.3e})")
        assert got.dim() == 0 and str(got.dtype) == "torch.float64" and got.device == _t(z["x"], dev).device
        assert after == float(z["rand_after"])
        assert abs(float(got.item()) - float(z["fp64"])) <= rel_bound(z["x"].shape[-1]) * float(z["fp64"]) and err <= bound
    z = load_fixture("a2m")
    for variant, kw in (("action2motion", {}), ("stgcn", {"seed": int(z["np_seed"])})):
        np.random.seed(int(z["np_seed"]))
        div, mm = A.calculate_diversity_multimodality(_t(z["x"], dev), _t(z["labels"], dev), int(z["num_labels"]), **kw)
        after = np.random.rand()
        bd, bm = 4 * rep["e_ref"]["a2m_diversity"] * float(z["fp64_diversity"]), 4 * rep["e_ref"]["a2m_multimodality"] * float(z["fp64_multimodality"])
        ed, em = abs(div - float(z[f"ref_{variant}"][0])), abs(mm - float(z[f"ref_{variant}"][1]))
        print(f"[humanml_metrics] fixture a2m {variant}: diversity vs the reference {ed:.3e} (bound {bd:.3e})  multimodality {em:.3e} (bound {bm:.3e})")
        assert isinstance(div, float) and isinstance(mm, float) and after == float(z["rand_after"])
        assert ed <= bd and em <= bm
        assert abs(div - float(z["fp64_diversity"])) <= rel_bound(z["x"].shape[1]) * div
        assert abs(mm - float(z["fp64_multimodality"])) <= rel_bound(z["x"].shape[1]) * mm
    np.random.seed(int(z["np_seed"]))
    div, mm = A.calculate_diversity_multimodality(_t(z["x"], dev), None, int(z["num_labels"]), unconstrained=True)
    assert div == A.calculate_diversity_multimodality(_t(z["x"], dev), _t(z["labels"], dev), int(z["num_labels"]), seed=int(z["np_seed"]))[0]
    assert np.isnan(mm)


# ---- the evaluation loop and the accuracy on stub loaders ---------------------------------------------------------------------------------
class StubWrapper:
    """An eval_wrapper whose embeddings are the batch's own tensors; it records the order of the calls."""

    def __init__(self):
        self.calls = []

    def get_co_embeddings(self, word_embs, pos_ohot, cap_lens, motions, m_lens):
        self.calls.append(("co", int(word_embs.shape[0])))
        return word_embs, motions

    def get_motion_embeddings(self, motions, m_lens):
        self.calls.append(("motion", int(motions.shape[0])))
        return motions


def stub_loaders(dev, D=30):
    """(gt loader, vald loader, mm loader, their numpy data): batches in the reference's tuple layout."""
    def loader(text, motion, sizes):
        return [(_t(text[b:e], dev), None, None, None, _t(motion[b:e], dev), None, None) for b, e in groups(sizes)]
    gt_sizes, gen_sizes = [32, 32, 32], [32, 32, 7]
    gt = make_pair(sum(gt_sizes), D, 5, 0.6, 8701)
    gen = make_pair(sum(gen_sizes), D, 5, 1.2, 8702)
    mm = make_pair(6 * 8, D, 5, 1.0, 8703)[1].reshape(6, 8, D)
    mm_loader = [(_t(mm[i:i + 1], dev), _t(np.full((1, 8), 40, dtype=np.int64), dev)) for i in range(6)]
    return loader(*gt, gt_sizes), loader(*gen, gen_sizes), mm_loader, dict(gt=gt, gen=gen, mm=mm, gt_sizes=gt_sizes, gen_sizes=gen_sizes)


def check_evaluation(dev, tmp_path, capsys):
    """evaluation() with two replications and multimodality on stub loaders: the order of the wrapper's calls, the printed lines
    (stdout and the log file say the same), and every entry of the returned dictionary against the fp64 restatements under the same
    seed."""
    from mdm_amd import humanml_eval as E
    from mdm_amd import metrics as M
    gt_loader, gen_loader, mm_loader, d = stub_loaders(dev)
    wrapper = StubWrapper()
    log = os.path.join(str(tmp_path), "eval.log")
    np.random.seed(8704)
    capsys.readouterr()
    got = E.evaluation(wrapper, gt_loader, {"vald": lambda: (gen_loader, mm_loader)}, log, replication_times=2, diversity_times=20,
                       mm_num_times=5, run_mm=True)
    after = np.random.rand()
    out = capsys.readouterr().out.splitlines()
    one = [("co", 32)] * 3 + [("co", 32), ("co", 32), ("co", 7)] + [("motion", 32)] * 3 + [("motion", 8)] * 6
    assert wrapper.calls == one + one
    with open(log) as fh:
        logged = fh.read().splitlines()
    plain = [line for line in out if not line.startswith("Time: ") and not line.startswith("========== Evaluating")]
    assert plain == [line for line in logged if not line.startswith("Time: ")]
    assert [line for line in out if line.startswith("=====")][:6] == [
        "==================== Replication 0 ====================", "========== Evaluating Matching Score ==========",
        "========== Evaluating FID ==========", "========== Evaluating Diversity ==========",
        "========== Evaluating MultiModality ==========", "==================== Replication 1 ===================="]
    assert sum(line.startswith("Time: ") for line in out) == 8 and out.count("!!! DONE !!!") == 2
    # the restatements, with the draws replayed in the loop's order
    want = {}
    for key, name in (("gt", "ground truth"), ("gen", "vald")):
        text, motion = d[key]
        rank, diag, topk = retrieval_oracle(text, motion, d[key + "_sizes"])
        want["Matching Score_" + name] = diag.sum() / len(text)
        want["R_precision_" + name] = topk / len(text)
    np.random.seed(8704)
    div = {"ground truth": [], "vald": []}
    mmv = []
    for _ in range(2):
        for key, name in (("gt", "ground truth"), ("gen", "vald")):
            x = d[key][1]
            first, second = np.random.choice(len(x), 20, replace=False), np.random.choice(len(x), 20, replace=False)
            div[name].append(pair_dist_fp64(x, first, second).mean())
        first, second = np.random.choice(8, 5, replace=False), np.random.choice(8, 5, replace=False)
        x64 = d["mm"].astype(np.float64)
        mmv.append(np.sqrt(((x64[:, first] - x64[:, second]) ** 2).sum(-1)).mean())
    assert after == np.random.rand()
    want["Diversity_ground truth"], want["Diversity_vald"], want["MultiModality_vald"] = np.mean(div["ground truth"]), np.mean(div["vald"]), np.mean(mmv)
    print(f"[humanml_metrics] evaluation: {got}")
    assert sorted(got) == sorted(list(want) + ["FID_ground truth", "FID_vald"])
    for k, w in want.items():
        if k.startswith("R_precision"):
            assert isinstance(got[k], np.ndarray) and np.array_equal(got[k], w), k
        else:
            assert isinstance(got[k], np.float64) and abs(got[k] - w) <= rel_bound(30) * w, k
    stats = [M.calculate_activation_statistics(_t(d[key][1], dev)) for key in ("gt", "gen")]
    assert got["FID_vald"] == M.calculate_frechet_distance(*stats[0], *stats[1]) and got["FID_vald"] > 1e-3
    assert abs(got["FID_ground truth"]) < 1e-6
    r = want["R_precision_vald"]
    assert "---> [vald] R_precision: (top 1): %.4f (top 2): %.4f (top 3): %.4f " % tuple(r) in logged
    assert "---> [vald](top 1) Mean: %.4f CInt: 0.0000;(top 2) Mean: %.4f CInt: 0.0000;(top 3) Mean: %.4f CInt: 0.0000;" % tuple(r) in logged
    assert f"---> [ground truth] Matching Score: {got['Matching Score_ground truth']:.4f}" in logged
    assert [line for line in logged if line.endswith("Summary ==========")] == [
        "========== %s Summary ==========" % n for n in ("Matching Score", "R_precision", "FID", "Diversity", "MultiModality")]


def check_accuracy(dev):
    """calculate_accuracy in both calling conventions: the confusion matrix of three batches and trace / sum as upstream divides
    them; a label out of range is an error."""
    import torch
    from mdm_amd import a2m_metrics as A
    yhat, labels = confusion_input("257_c12")
    good = labels.copy()
    good[2], good[-1] = 3, 4

    def loader(lab):
        return [{"output_xyz": _t(yhat[lo:hi], dev), "lengths": None, "y": _t(lab[lo:hi].astype(np.int64), dev)}
                for lo, hi in ((0, 100), (100, 101), (101, 257))]
    _, want_conf, _ = confusion_fp64(yhat, good, 12)
    want_acc = (torch.trace(torch.from_numpy(want_conf)) / torch.sum(torch.from_numpy(want_conf))).item()
    for style, classifier in (("action2motion", lambda x, lengths: x), ("stgcn", lambda batch: {"yhat": batch["output_xyz"]})):
        acc, conf = A.calculate_accuracy(None, loader(good), 12, classifier, dev, style=style)
        assert isinstance(acc, float) and acc == want_acc and 0.0 < acc < 1.0
        assert conf.dtype == torch.int64 and conf.device.type == "cpu" and np.array_equal(conf.numpy(), want_conf)
    acc, _ = A.calculate_accuracy_stgcn(None, loader(good), 12, lambda batch: {"yhat": batch["output_xyz"]}, dev)
    assert acc == want_acc
    try:
        A.calculate_accuracy(None, loader(labels), 12, lambda x, lengths: x, dev)
    except ValueError as err:
        assert "2 labels" in str(err)
    else:
        raise AssertionError("labels out of range were accepted")
