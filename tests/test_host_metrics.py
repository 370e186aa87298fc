"""mdm_amd/metrics.py without a device: the refusals of the native calls (each with its message in mdm_last_error, before any launch)
and of the module (ValueErrors that name the argument), the order of the np.random draws against the reference's functions under a
seed (recorded in tests/golden/metrics_*.npz; no native library needed), upstream's truncation to min(len), calculate_fid against the
reference's value on the same statistics, and the product path's refusal of host tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_helpers as mh
from emu.emu_lib import emu
from mdm_amd import _native as nat
from mdm_amd import metrics as M


@pytest.fixture()
def lib():
    M.NATIVE_LIB = emu()
    yield M.NATIVE_LIB
    M.NATIVE_LIB = None


def _bufs():
    x = np.zeros((8, 4), dtype=np.float32)
    out = np.zeros(64, dtype=np.float64)
    idx = np.zeros((2, 4), dtype=np.int32)
    ws = np.zeros(4096, dtype=np.uint8)
    return x, out, idx, ws


def test_native_calls_refuse_bad_arguments_with_a_message(lib):
    x, out, idx, ws = _bufs()
    px, po, pi, pw, n = x.ctypes.data, out.ctypes.data, idx.ctypes.data, ws.ctypes.data, ws.nbytes
    err = lambda: lib.mdm_last_error().decode()      # noqa: E731
    K, EINVAL, ENOSPC, EUNSUP = nat.METRICS_KINDS, -1, -3, -5
    # workspace sizes
    assert lib.mdm_metrics_workspace_bytes(K["knn_radius"], 8, 1) == 64
    assert lib.mdm_metrics_workspace_bytes(K["poly_mmd"], 65, 5) == 64 + 5 * 2 * 2 * 16 * 8
    assert lib.mdm_metrics_workspace_bytes(9, 8, 1) == 0 and "kind" in err()
    assert lib.mdm_metrics_workspace_bytes(K["poly_mmd"], 0, 1) == 0 and "rows" in err()
    assert lib.mdm_metrics_workspace_bytes(K["poly_mmd"], 8, 0) == 0 and "subsets" in err()
    assert lib.mdm_metrics_workspace_bytes(K["poly_mmd"], 1 << 20, 1 << 12) == 0 and "2^31" in err()
    # mdm_knn_radius: null pointers, k outside 1 .. 7, N < k + 1, D < 1, rows * D >= 2^31, a short or missing workspace
    assert lib.mdm_knn_radius(None, 8, 4, 3, po, pw, n, None) == EINVAL and "null a_dev" in err()
    assert lib.mdm_knn_radius(px, 8, 4, 3, None, pw, n, None) == EINVAL and "null radius2_dev" in err()
    for k in (0, 8, -1):
        assert lib.mdm_knn_radius(px, 8, 4, k, po, pw, n, None) == EINVAL and "between 1 and 7" in err()
    assert lib.mdm_knn_radius(px, 3, 4, 3, po, pw, n, None) == EINVAL and "k + 1" in err()
    assert lib.mdm_knn_radius(px, 8, 0, 3, po, pw, n, None) == EINVAL and "D must be at least 1" in err()
    assert lib.mdm_knn_radius(px, 1 << 16, 1 << 15, 3, po, pw, n, None) == EUNSUP and "2^31" in err()
    assert lib.mdm_knn_radius(px, 8, 4, 3, po, None, n, None) == EINVAL and "null workspace_dev" in err()
    assert lib.mdm_knn_radius(px, 8, 4, 3, po, pw, 63, None) == ENOSPC and "workspace_bytes too small" in err()
    assert lib.mdm_knn_radius(px + 2, 8, 4, 3, po, pw, n, None) == EINVAL and "aligned" in err()
    # mdm_manifold_members
    assert lib.mdm_manifold_members(px, None, 8, px, 8, 4, po, po, pw, n, None) == EINVAL and "null radius2_dev" in err()
    assert lib.mdm_manifold_members(px, po, 8, None, 8, 4, po, po, pw, n, None) == EINVAL and "null b_dev" in err()
    assert lib.mdm_manifold_members(px, po, 8, px, 0, 4, po, po, pw, n, None) == EINVAL and "b_dev must hold" in err()
    assert lib.mdm_manifold_members(px, po, 8, px, 8, 4, None, po, pw, n, None) == EINVAL and "null member_dev" in err()
    assert lib.mdm_manifold_members(px, po, 8, px, 8, 4, po, None, pw, n, None) == EINVAL and "null count_dev" in err()
    assert lib.mdm_manifold_members(px, po, 8, px, 8, 4, po, po, pw, 8, None) == ENOSPC
    # mdm_gather_dist
    assert lib.mdm_gather_dist(px, 8, 4, None, pi, 4, po, po, pw, n, None) == EINVAL and "null first_dev" in err()
    assert lib.mdm_gather_dist(px, 8, 4, pi, pi, 0, po, po, pw, n, None) == EINVAL and "P must be at least 1" in err()
    assert lib.mdm_gather_dist(px, 8, 4, pi, pi, 4, po, None, pw, n, None) == EINVAL and "null mean_dev" in err()
    assert lib.mdm_gather_dist(px, 8, 4, pi, pi, 4, po, po + 4, pw, n, None) == EINVAL and "8-byte aligned" in err()
    # mdm_poly_mmd: m < 3, degree < 1, S < 1, var_at_m < 2, a short workspace
    call = lambda **o: lib.mdm_poly_mmd(*[{**dict(g=px, Ng=8, r=px, Nr=8, D=4, ig=pi, ir=pi, S=2, m=4, gamma=0.25, coef0=1.0, degree=3,      # noqa: E731
                                                  var=8, mmd2=po, v=po + 64, ws=pw, n=n, stream=None), **o}[k]
                                          for k in ("g", "Ng", "r", "Nr", "D", "ig", "ir", "S", "m", "gamma", "coef0", "degree", "var", "mmd2",
                                                    "v", "ws", "n", "stream")])
    assert call(m=2) == EINVAL and "m must be at least 3" in err()
    assert call(degree=0) == EINVAL and "degree must be at least 1" in err()
    assert call(S=0) == EINVAL and "S must be at least 1" in err()
    assert call(var=1) == EINVAL and "var_at_m" in err()
    assert call(D=0) == EINVAL and "D must be at least 1" in err()
    assert call(ig=None) == EINVAL and "null idx_g_dev" in err()
    assert call(r=None) == EINVAL and "null r_dev" in err()
    assert call(mmd2=None) == EINVAL and "null mmd2_dev" in err()
    assert call(n=64) == ENOSPC and "workspace_bytes too small" in err()
    assert call(S=1 << 12, m=1 << 20) < 0 and "2^31" in err()
    assert call() == 0                                                        # (the same arguments, unharmed, run)
    # mdm_feature_stats
    assert lib.mdm_feature_stats(px, 1, 4, po, po + 64, pw, n, None) == EINVAL and "N must be at least 2" in err()
    assert lib.mdm_feature_stats(px, 8, 4, None, po, pw, n, None) == EINVAL and "null mu_dev" in err()
    assert lib.mdm_feature_stats(px, 8, 4, po, None, pw, n, None) == EINVAL and "null sigma_dev" in err()
    assert lib.mdm_feature_stats(px, 8, 1 << 16, po, po, pw, n, None) == EUNSUP and "D * D" in err()
    assert lib.mdm_abi_version() == 10


def test_the_module_refuses_bad_arguments_by_name(lib):
    a, b = torch.zeros(8, 4), torch.zeros(8, 5)
    with pytest.raises(ValueError, match="A_features"):
        M.knn_radii(torch.zeros(8), 3)
    with pytest.raises(ValueError, match="B_features has 5"):
        M.manifold_members(a, torch.zeros(8), b)
    with pytest.raises(ValueError, match="radius2"):
        M.manifold_members(a, torch.zeros(7), a)
    with pytest.raises(ValueError, match="real_features has 5"):
        M.precision_and_recall(a, b)
    with pytest.raises(ValueError, match="codes_r"):
        M.polynomial_mmd_averages(a, torch.zeros(8, 4, 1), n_subsets=1, subset_size=4)
    with pytest.raises(ValueError, match="equally many rows"):
        M.polynomial_mmd(a, torch.zeros(7, 4))
    with pytest.raises(ValueError, match="degree"):
        M.polynomial_mmd(a, a, degree=2.5)
    with pytest.raises(TypeError, match="kernel arguments"):
        M.polynomial_mmd_averages(a, a, n_subsets=1, subset_size=4, sigma=1.0)
    with pytest.raises(ValueError, match="activations"):
        M.calculate_activation_statistics(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match=r"first_indices must lie in \[0, 8\)"):
        M.gather_dist(a, [0, 8], [0, 1])
    with pytest.raises(ValueError, match="second_indices"):
        M.gather_dist(a, [0, 1], [-1, 1])
    # the ABI's refusals arrive as MdmError with the library's message
    with pytest.raises(nat.MdmError, match="between 1 and 7"):
        M.knn_radii(a, 8)
    with pytest.raises(nat.MdmError, match="k \\+ 1"):
        M.knn_radii(a[:3], 3)
    with pytest.raises(nat.MdmError, match="m must be at least 3"):
        M.polynomial_mmd_averages(a, a, n_subsets=1, subset_size=2)
    with pytest.raises(nat.MdmError, match="N must be at least 2"):
        M.calculate_activation_statistics(a[:1])
    assert M.precision_and_recall(a[:0], a) is None                       # upstream: "there is no data"


def test_product_path_refuses_host_tensors(monkeypatch):
    """With the product library bound, features on the host are an error -- not a silent CPU computation."""
    class Product:
        path = "/somewhere/" + nat.LIB_NAME
    monkeypatch.setattr(M, "NATIVE_LIB", Product())
    for call in (lambda: M.knn_radii(torch.zeros(8, 4), 3), lambda: M.calculate_activation_statistics(torch.zeros(8, 4)),
                 lambda: M.calculate_diversity(torch.zeros(8, 4)), lambda: M.polynomial_mmd(torch.zeros(8, 4), torch.zeros(8, 4)),
                 lambda: M.precision_and_recall(np.zeros((8, 4), dtype=np.float32), np.zeros((8, 4), dtype=np.float32))):
        with pytest.raises(nat.MdmError, match="cuda"):
            call()


def test_random_draws_are_upstreams_in_upstreams_order(monkeypatch):
    """polynomial_mmd_averages: choice(len(g)) then choice(len(r)) per subset with upstream's `replace`; calculate_diversity: two
    randint draws of 200.  The tables recorded beside the reference's run under the same seed are what reaches the native call, and
    the generator ends where upstream's ends.  No native library: the native layer is replaced by a recorder."""
    seen = {}

    def fake_mmd(g, r, idx_g, idx_r, degree, gamma, coef0, var_at_m):
        seen.update(idx_g=idx_g.copy(), idx_r=idx_r.copy(), kernel=(degree, gamma, coef0), var_at_m=var_at_m)
        return np.zeros(len(idx_g)), np.ones(len(idx_g))

    def fake_dist(x, first, second):
        seen.update(first=np.asarray(first).copy(), second=np.asarray(second).copy())
        return None, torch.zeros((), dtype=torch.float64)

    monkeypatch.setattr(M, "_poly_mmd", fake_mmd)
    monkeypatch.setattr(M, "gather_dist", fake_dist)
    z = mh.load_fixture("kid")
    np.random.seed(int(z["np_seed"]))
    mmds, vars_ = M.polynomial_mmd_averages(z["g"], z["r"], n_subsets=8, subset_size=33)
    assert np.array_equal(seen["idx_g"], z["idx_g"]) and np.array_equal(seen["idx_r"], z["idx_r"])
    assert seen["kernel"] == (3, None, 1) and seen["var_at_m"] == 70 and mmds.shape == vars_.shape == (8,)
    assert len(set(z["idx_g"][0])) < 33                                      # 33 of 70 with replacement
    after = np.random.rand()
    np.random.seed(int(z["np_seed"]))
    for _ in range(8):
        np.random.choice(70, 33, replace=True), np.random.choice(70, 33, replace=True)
    assert after == np.random.rand()
    # subset_size == len: without replacement, every subset a permutation; ret_var=False returns the mmds alone
    np.random.seed(5)
    only = M.polynomial_mmd_averages(z["g"], np.concatenate([z["r"], z["r"][:5]]), n_subsets=2, subset_size=70, ret_var=False, degree=2, gamma=0.5, coef0=0)
    assert isinstance(only, np.ndarray) and only.shape == (2,) and seen["kernel"] == (2, 0.5, 0) and seen["var_at_m"] == 70
    assert sorted(seen["idx_g"][1]) == list(range(70)) and len(set(seen["idx_r"][1])) == 70 and seen["idx_r"].max() > 69
    np.random.seed(5)
    assert np.array_equal(seen["idx_g"][0], np.random.choice(70, 70, replace=False))
    # calculate_kid: 100 subsets of 1000, (real, generated) in upstream's argument order, (mean, std)
    np.random.seed(6)
    kid = M.calculate_kid(np.zeros((1001, 2), dtype=np.float32), np.zeros((1200, 2), dtype=np.float32))
    assert seen["idx_g"].shape == (100, 1000) and kid == (0.0, 0.0) and seen["idx_g"].max() == 1000 and seen["idx_r"].max() > 1100
    assert seen["var_at_m"] == 1001
    # diversity
    d = mh.load_fixture("diversity")
    np.random.seed(int(d["np_seed"]))
    M.calculate_diversity(d["x"])
    assert np.array_equal(seen["first"], d["first"]) and np.array_equal(seen["second"], d["second"]) and len(seen["first"]) == 200


def test_precision_and_recall_truncates_to_the_shorter_set(lib):
    """Upstream cuts both sets to min(len) rows before anything else."""
    A, B = mh.pr_input("63x129_d30")                      # real 63, generated 129
    got = M.precision_and_recall(torch.from_numpy(B), torch.from_numpy(A))
    cut = torch.from_numpy(B[:63])
    assert got == (M.manifold_estimate(torch.from_numpy(A), cut, 3), M.manifold_estimate(cut, torch.from_numpy(A), 3))
    in_a, in_b = mh.margins(A, B[:63])[0], mh.margins(B[:63], A)[0]
    assert got == (int(in_a.sum()) / 63, int(in_b.sum()) / 63)


def test_calculate_fid_is_the_references_value_on_the_same_statistics():
    """The host formula on the statistics the reference's run recorded returns the reference's float, bit for bit -- from numpy
    arrays and from tensors; a singular product stays finite; a complex root beyond 1e-3 is refused."""
    z = mh.load_fixture("stats")
    s1, s2 = (z["ref_mu1"], z["ref_sigma1"]), (z["ref_mu2"], z["ref_sigma2"])
    assert M.calculate_fid(s1, s2) == float(z["ref_fid"])
    t1, t2 = tuple(torch.from_numpy(a) for a in s1), tuple(torch.from_numpy(a) for a in s2)
    assert M.calculate_fid(t1, t2) == float(z["ref_fid"])
    assert M.calculate_fid((z["fp64_mu1"], z["fp64_sigma1"]), (z["fp64_mu2"], z["fp64_sigma2"])) == float(z["ref_fid_of_fp64"])
    assert abs(M.calculate_fid(s1, s1)) < 1e-6
    with pytest.raises(ValueError, match="different lengths"):
        M.calculate_frechet_distance(np.zeros(3), np.eye(3), np.zeros(4), np.eye(4))
    with pytest.raises(ValueError, match="different dimensions"):
        M.calculate_frechet_distance(np.zeros(3), np.eye(3), np.zeros(3), np.eye(4))
    # a singular product (zero covariances) still yields a finite distance
    zero = np.zeros((2, 2))
    assert np.isfinite(M.calculate_frechet_distance(np.zeros(2), zero, np.zeros(2), zero))
    rot = np.array([[0.0, -1.0], [1.0, 0.0]])                                 # sqrtm(rot . I) has eigenvalues exp(+- i pi / 4)
    neg = np.array([[-1.0, 0.0], [0.0, 1.0]])
    with pytest.raises(ValueError, match="Imaginary component"):
        M.calculate_frechet_distance(np.zeros(2), neg, np.zeros(2), np.eye(2))
    assert np.isfinite(M.calculate_frechet_distance(np.zeros(2), rot, np.zeros(2), np.eye(2)))


def test_unconstrained_eval_keeps_upstreams_constants():
    from mdm_amd import unconstrained_eval as ue
    import inspect
    assert ue.ACT_REC_MODEL_PATH == "./assets/actionrecognition/humanact12_gru_modi_struct.pth.tar"
    assert ue.DATASET_PATH == "./dataset/HumanAct12Poses/humanact12_unconstrained_modi_struct.npy"
    p = inspect.signature(ue.evaluate_unconstrained_metrics).parameters
    assert list(p)[:3] == ["generated_motions", "device", "fast"] and p["kid_subsets"].default == 100 and p["kid_subset_size"].default == 1000
    assert ue.BATCH_SIZE == 64 and ue.ROOT_JOINT == 8
    m = np.arange(2 * 15 * 3 * 4, dtype=np.float32).reshape(2, 15, 3, 4)
    c = ue.centre_root(m)
    assert torch.equal(c, torch.from_numpy(m - m[:, 8:9])) and (c[:, 8] == 0).all()
    with pytest.raises(ValueError, match="motions"):
        ue.centre_root(np.zeros((2, 15, 3)))
