"""The metrics of the unconstrained HumanAct12 evaluation on the HIP path, under the reference's names and signatures:
`precision_and_recall` / `manifold_estimate` (eval/unconstrained/metrics/precision_recall.py), `polynomial_mmd_averages` /
`polynomial_mmd` / `calculate_kid` (eval/unconstrained/metrics/kid.py), `calculate_activation_statistics`
(eval/unconstrained/evaluate.py), `calculate_fid` (eval/a2m/action2motion/fid.py) and `calculate_diversity`
(eval/a2m/action2motion/diversity.py).  The features stay on the device: the arithmetic is csrc/metrics.h behind include/mdm_hip.h's
mdm_knn_radius, mdm_manifold_members, mdm_gather_dist, mdm_poly_mmd and mdm_feature_stats (no torch.norm / sklearn call, and no
fall-back when the library is missing).  What stays on the host: the random draws (numpy's global generator, in upstream's order, so
a seeded run uses upstream's subsets and pairs) and, by default, `calculate_fid`'s matrix square root of a D x D matrix (scipy:
`calculate_frechet_distance` is upstream's host formula, bit for bit).  The option: `frechet_distance_device` / `calculate_fid_device`
evaluate the same distance on the device in fp64 (csrc/frechet.h behind mdm_frechet_distance: two Jacobi eigen-solves and two MFMA
products instead of sqrtm) and return a device scalar; the evaluation loops take them on request (`unconstrained_eval`: `fid_on_device=True`; `humanml_eval`:
the module switch `FID_ON_DEVICE`).

Differences from upstream: precision / recall compare squared distances (fp32, direct differences) with squared radii instead of
`torch.norm` values with fp64 copies of them; KID forms the Gram products in fp32 and everything behind them in fp64 (upstream: fp32
throughout); the statistics are fp64 from the first addition (upstream: numpy on fp32 arrays); `calculate_diversity` returns an fp64
scalar tensor.  `NATIVE_LIB` is None for the product library; the emulator tests bind theirs."""
import numpy as np
import torch

from . import _native as nat
from ._native_model import native_stream

NATIVE_LIB = None
SUBSET_CHUNK = 256         # KID subsets per native call: bounds the workspace and the grid (a subset's result does not depend on the call)
KNN_K = 3                  # precision_and_recall's k
DIVERSITY_TIMES = 200
KID_SUBSETS, KID_SUBSET_SIZE = 100, 1000


def _lib():
    return NATIVE_LIB if NATIVE_LIB is not None else nat.load_native()


def _features(x, name):
    """A feature matrix as an fp32, contiguous [N, D] tensor on its own device."""
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.dim() != 2:
        raise ValueError(f"{name} must be a feature matrix [N, D], got {tuple(t.shape)}")
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name} must hold at least one row and one feature, got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def _same_width(a, b, name_a, name_b):
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"{name_a} has {a.shape[1]} features, {name_b} has {b.shape[1]}")
    if a.device != b.device:
        raise ValueError(f"{name_a} is on {a.device}, {name_b} on {b.device}")


def _workspace(lib, kind, rows, subsets, dev):
    nbytes = lib.mdm_metrics_workspace_bytes(nat.METRICS_KINDS[kind], rows, subsets)
    if nbytes == 0:
        lib.check(-1, "mdm_metrics_workspace_bytes")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _indices(idx, n, name, dev):
    """A host index array as an int32 device tensor; the entries must lie in [0, n) (the native call trusts them)."""
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise ValueError(f"{name} must lie in [0, {n}), got {int(idx.min())} .. {int(idx.max())}")
    return torch.from_numpy(idx.astype(np.int32)).to(dev)


# ---- precision / recall ---------------------------------------------------------------------------------------------------------------
def knn_radii(A_features, k):
    """radius2 [N] fp32: the squared distance from every row of A to its k-th nearest other row (self is neighbour 0)."""
    lib = _lib()
    a = _features(A_features, "A_features")
    stream = native_stream(lib, a, "A_features")
    ws, nbytes = _workspace(lib, "knn_radius", a.shape[0], 1, a.device)
    radius2 = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    lib.check(lib.mdm_knn_radius(a.data_ptr(), a.shape[0], a.shape[1], int(k), radius2.data_ptr(), ws.data_ptr(), nbytes, stream),
              "mdm_knn_radius")
    return radius2


def manifold_members(A_features, radius2, B_features):
    """(member [NB] uint8, count 0-dim int32): which rows of B lie within the radius of some row of A."""
    lib = _lib()
    a, b = _features(A_features, "A_features"), _features(B_features, "B_features")
    _same_width(a, b, "A_features", "B_features")
    stream = native_stream(lib, a, "A_features")
    r2 = radius2.detach().to(device=a.device, dtype=torch.float32).contiguous()
    if tuple(r2.shape) != (a.shape[0],):
        raise ValueError(f"radius2 must be [{a.shape[0]}] (one per row of A_features), got {tuple(r2.shape)}")
    ws, nbytes = _workspace(lib, "manifold_members", b.shape[0], 1, a.device)
    member = torch.empty(b.shape[0], dtype=torch.uint8, device=a.device)
    count = torch.empty((), dtype=torch.int32, device=a.device)
    lib.check(lib.mdm_manifold_members(a.data_ptr(), r2.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1], member.data_ptr(),
                                       count.data_ptr(), ws.data_ptr(), nbytes, stream), "mdm_manifold_members")
    return member, count


def manifold_estimate(A_features, B_features, k):
    """The fraction of B's rows inside the k-NN manifold of A, as upstream's Python float n / len(B)."""
    a, b = _features(A_features, "A_features"), _features(B_features, "B_features")
    _, count = manifold_members(a, knn_radii(a, k), b)
    return int(count.item()) / b.shape[0]


def precision_and_recall(generated_features, real_features):
    k = KNN_K
    data_num = min(len(generated_features), len(real_features))
    if data_num <= 0:
        return None
    generated = _features(generated_features, "generated_features")[:data_num]
    real = _features(real_features, "real_features")[:data_num]
    _same_width(generated, real, "generated_features", "real_features")
    precision = manifold_estimate(real, generated, k)
    recall = manifold_estimate(generated, real, k)
    return precision, recall


# ---- KID --------------------------------------------------------------------------------------------------------------------------------
def _poly_mmd(g, r, idx_g, idx_r, degree, gamma, coef0, var_at_m):
    """(mmd2 [S], var [S]) float64 numpy arrays for the index tables idx_g, idx_r [S, m] (host)."""
    lib = _lib()
    _same_width(g, r, "codes_g", "codes_r")
    stream = native_stream(lib, g, "codes_g")
    S, m = idx_g.shape
    D = g.shape[1]
    if degree != int(degree) or int(degree) < 1:
        raise ValueError(f"degree must be a positive integer, got {degree}")
    gamma = 1.0 / D if gamma is None else float(gamma)
    ig, ir = _indices(idx_g, g.shape[0], "the subset indices of codes_g", g.device), _indices(idx_r, r.shape[0], "the subset indices of codes_r", g.device)
    mmd2 = torch.empty(S, dtype=torch.float64, device=g.device)
    var = torch.empty(S, dtype=torch.float64, device=g.device)
    chunk = min(S, SUBSET_CHUNK)
    ws, nbytes = _workspace(lib, "poly_mmd", m, chunk, g.device)
    for s0 in range(0, S, chunk):
        n = min(chunk, S - s0)
        lib.check(lib.mdm_poly_mmd(g.data_ptr(), g.shape[0], r.data_ptr(), r.shape[0], D, ig[s0:s0 + n].data_ptr(), ir[s0:s0 + n].data_ptr(),
                                   n, m, gamma, float(coef0), int(degree), int(var_at_m), mmd2[s0:s0 + n].data_ptr(),
                                   var[s0:s0 + n].data_ptr(), ws.data_ptr(), nbytes, stream), "mdm_poly_mmd")
    return mmd2.cpu().numpy(), var.cpu().numpy()


def polynomial_mmd_averages(codes_g, codes_r, n_subsets=50, subset_size=1000, ret_var=True, output=None, **kernel_args):
    """kid.py polynomial_mmd_averages: the same np.random.choice calls in the same order (g then r per subset), all subsets in one
    native call per SUBSET_CHUNK.  `output` (upstream's progress-bar stream) is accepted and unused."""
    g, r = _features(codes_g, "codes_g"), _features(codes_r, "codes_r")
    unknown = set(kernel_args) - {"degree", "gamma", "coef0"}
    if unknown:
        raise TypeError(f"polynomial_mmd_averages got unexpected kernel arguments {sorted(unknown)}")
    m = min(g.shape[0], r.shape[0])
    choice = np.random.choice
    replace = subset_size < len(g)
    idx_g = np.empty((n_subsets, subset_size), dtype=np.int64)
    idx_r = np.empty((n_subsets, subset_size), dtype=np.int64)
    for i in range(n_subsets):
        idx_g[i] = choice(len(g), subset_size, replace=replace)
        idx_r[i] = choice(len(r), subset_size, replace=replace)
    mmds, vars_ = _poly_mmd(g, r, idx_g, idx_r, kernel_args.get("degree", 3), kernel_args.get("gamma"), kernel_args.get("coef0", 1), m)
    return (mmds, vars_) if ret_var else mmds


def polynomial_mmd(codes_g, codes_r, degree=3, gamma=None, coef0=1, var_at_m=None, ret_var=True):
    """kid.py polynomial_mmd on all rows of both code matrices (equally many): (mmd2, var) as numpy float64 scalars."""
    g, r = _features(codes_g, "codes_g"), _features(codes_r, "codes_r")
    if g.shape[0] != r.shape[0]:
        raise ValueError(f"codes_g and codes_r must hold equally many rows, got {g.shape[0]} and {r.shape[0]}")
    m = g.shape[0]
    idx = np.arange(m, dtype=np.int64)[None]
    mmd2, var = _poly_mmd(g, r, idx, idx, degree, gamma, coef0, m if var_at_m is None else var_at_m)
    return (mmd2[0], var[0]) if ret_var else mmd2[0]


def calculate_kid(real_activations, generated_activations, n_subsets=KID_SUBSETS, subset_size=KID_SUBSET_SIZE):
    kid_values = polynomial_mmd_averages(real_activations, generated_activations, n_subsets=n_subsets, subset_size=subset_size)
    return kid_values[0].mean(), kid_values[0].std()


# ---- FID --------------------------------------------------------------------------------------------------------------------------------
def calculate_activation_statistics(activations):
    """(mu [D], sigma [D, D]) as fp64 tensors on the activations' device: np.mean(axis=0) and np.cov(rowvar=False)."""
    lib = _lib()
    x = _features(activations, "activations")
    stream = native_stream(lib, x, "activations")
    N, D = x.shape
    ws, nbytes = _workspace(lib, "feature_stats", N, 1, x.device)
    mu = torch.empty(D, dtype=torch.float64, device=x.device)
    sigma = torch.empty(D, D, dtype=torch.float64, device=x.device)
    lib.check(lib.mdm_feature_stats(x.data_ptr(), N, D, mu.data_ptr(), sigma.data_ptr(), ws.data_ptr(), nbytes, stream), "mdm_feature_stats")
    return mu, sigma


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """||mu1 - mu2||^2 + Tr(sigma1 + sigma2 - 2 sqrt(sigma1 sigma2)) on the host (the matrix is D x D); a singular product is retried
    with eps on both diagonals, an imaginary part beyond 1e-3 on the root's diagonal is an error."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(_host(mu1)), np.atleast_1d(_host(mu2))
    sigma1, sigma2 = np.atleast_2d(_host(sigma1)), np.atleast_2d(_host(sigma2))
    if mu1.shape != mu2.shape:
        raise ValueError(f"the mean vectors have different lengths: {mu1.shape} and {mu2.shape}")
    if sigma1.shape != sigma2.shape:
        raise ValueError(f"the covariances have different dimensions: {sigma1.shape} and {sigma2.shape}")
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    tr_covmean = np.trace(covmean)
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr_covmean


def calculate_fid(statistics_1, statistics_2):
    return calculate_frechet_distance(statistics_1[0], statistics_1[1], statistics_2[0], statistics_2[1])


IMAG_TOL = 1e-3            # upstream's np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3)


def frechet_distance_device(mu1, sigma1, mu2, sigma2, check=True):
    """The Frechet distance as a 0-dim fp64 tensor on the inputs' device, from fp64 device statistics (what
    `calculate_activation_statistics` returns): Tr sqrtm(sigma1 sigma2) = sum sqrt(eig(S^T sigma2 S)), S S^T = sigma1, by two symmetric
    eigen-solves in one native call.  Both covariances count by their symmetric parts; negative eigenvalues are clamped to 0.
    check=True reads the call's result block (one synchronisation) and raises ValueError when a solve did not converge, when the result is not finite or when the
    product has a negative eigenvalue with sqrt(-lambda_min) > 1e-3 -- upstream's "Imaginary component" refusal, tested on the bound
    sqrt(-lambda_min / lambda_max) sum sqrt(lambda) >= sqrt(-lambda_min) the block allows.  check=False touches nothing on the host: a
    solve that did not converge returns NaN."""
    lib = _lib()
    names = ("mu1", "sigma1", "mu2", "sigma2")
    for name, t in zip(names, (mu1, sigma1, mu2, sigma2)):
        if not torch.is_tensor(t):
            if lib.path.endswith(nat.LIB_NAME):
                raise nat.MdmError(f"the MI355X HIP path needs {name} on a cuda (ROCm) device; got a {type(t).__name__} on the host")
            raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    mu1, mu2 = (t.detach().reshape(-1) if t.dim() == 0 else t.detach() for t in (mu1, mu2))
    sigma1, sigma2 = (t.detach().reshape(1, 1) if t.dim() == 0 else t.detach() for t in (sigma1, sigma2))
    if mu1.shape != mu2.shape:
        raise ValueError(f"the mean vectors have different lengths: {tuple(mu1.shape)} and {tuple(mu2.shape)}")
    if sigma1.shape != sigma2.shape:
        raise ValueError(f"the covariances have different dimensions: {tuple(sigma1.shape)} and {tuple(sigma2.shape)}")
    D = mu1.shape[0] if mu1.dim() == 1 else -1
    if D < 1 or tuple(sigma1.shape) != (D, D):
        raise ValueError(f"mu1 must be [D] and sigma1 [D, D], got {tuple(mu1.shape)} and {tuple(sigma1.shape)}")
    stream = native_stream(lib, mu1, "mu1")
    args = []
    for name, t in zip(names, (mu1, sigma1, mu2, sigma2)):
        if t.device != mu1.device:
            raise ValueError(f"{name} is on {t.device}, mu1 on {mu1.device}")
        if t.dtype != torch.float64:
            raise ValueError(f"{name} must be float64 (calculate_activation_statistics returns it), got {t.dtype}")
        args.append(t.contiguous())
    nbytes = lib.mdm_frechet_workspace_bytes(D)
    if nbytes == 0:
        lib.check(-1, "mdm_frechet_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mu1.device)
    result = torch.empty(4, dtype=torch.float64, device=mu1.device)
    sweeps = torch.empty(2, dtype=torch.int32, device=mu1.device)
    lib.check(lib.mdm_frechet_distance(args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), args[3].data_ptr(), D, result.data_ptr(),
                                       sweeps.data_ptr(), ws.data_ptr(), nbytes, stream), "mdm_frechet_distance")
    if check:
        r, sw = result.cpu().numpy(), sweeps.cpu().numpy()
        if sw.max() >= nat.FRECHET_MAX_SWEEPS:
            raise ValueError(f"the eigen-solves of sigma1 / of the product ran {sw.tolist()} sweeps: no convergence within "
                             f"{nat.FRECHET_MAX_SWEEPS} (non-finite statistics?)")
        if not np.isfinite(r[0]):
            raise ValueError(f"the Frechet distance is not finite ({r[0]}): the statistics hold a value that is not finite")
        imag = np.inf if r[3] == -np.inf else (np.sqrt(-r[3]) * r[1] if r[3] < 0 else 0.0)
        if not imag <= IMAG_TOL:
            raise ValueError(f"Imaginary component {imag}: sigma1 sigma2 has a negative eigenvalue (min / max = {r[3]:.3e})")
    return result[0]


def calculate_fid_device(statistics_1, statistics_2, check=True):
    return frechet_distance_device(statistics_1[0], statistics_1[1], statistics_2[0], statistics_2[1], check=check)


# ---- diversity --------------------------------------------------------------------------------------------------------------------------
def gather_dist(activations, first_indices, second_indices):
    """(dist [P] fp32, mean 0-dim fp64) of the rows' pair distances, on the activations' device."""
    lib = _lib()
    x = _features(activations, "activations")
    stream = native_stream(lib, x, "activations")
    first = _indices(first_indices, x.shape[0], "first_indices", x.device)
    second = _indices(second_indices, x.shape[0], "second_indices", x.device)
    if first.dim() != 1 or first.shape != second.shape or first.numel() < 1:
        raise ValueError(f"first_indices and second_indices must be equally long 1-D arrays, got {tuple(first.shape)} and {tuple(second.shape)}")
    P = first.numel()
    ws, nbytes = _workspace(lib, "gather_dist", x.shape[0], 1, x.device)
    dist = torch.empty(P, dtype=torch.float32, device=x.device)
    mean = torch.empty((), dtype=torch.float64, device=x.device)
    lib.check(lib.mdm_gather_dist(x.data_ptr(), x.shape[0], x.shape[1], first.data_ptr(), second.data_ptr(), P, dist.data_ptr(),
                                  mean.data_ptr(), ws.data_ptr(), nbytes, stream), "mdm_gather_dist")
    return dist, mean


def calculate_diversity(activations):
    """diversity.py calculate_diversity: upstream's two np.random.randint draws in upstream's order, one native call."""
    num_motions = len(activations)
    first_indices = np.random.randint(0, num_motions, DIVERSITY_TIMES)
    second_indices = np.random.randint(0, num_motions, DIVERSITY_TIMES)
    return gather_dist(activations, first_indices, second_indices)[1]
