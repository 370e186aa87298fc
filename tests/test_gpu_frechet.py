"""mdm_amd.metrics.frechet_distance_device (csrc/frechet.h) on the MI355X: the fixture cases of tests/frechet_helpers.py against the
reference's own value; D = 256 and 512 (the ST-GCN's and the HumanML3D evaluator's widths; full rank and N < D) against the host
formula on the same device statistics -- `calculate_frechet_distance` is pinned to the reference bit for bit by
tests/test_host_metrics.py, and the reference tree is not needed here -- with d from numpy's eigh on the spot; bit-identity across
calls, streams, workspace contents and a graph replay; and evaluate_unconstrained_metrics with fid_on_device=True.

One rule for every value (frechet_helpers): within max(100 d, 1e-11 S) of the reference's, d the disagreement of two independent fp64
evaluations, S = Tr sigma1 + Tr sigma2 + |mu1 - mu2|^2.  Every test prints |got - ref| / S, d / S and the sweeps before it asserts;
tools/bench_metrics.py collects the timings into profiles/r19a_frechet.md."""
import numpy as np
import pytest
import torch

import frechet_helpers as fh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from mdm_amd import _native as nat
    return nat.load_native()


@pytest.mark.parametrize("name", list(fh.CASES))
def test_case_is_within_the_rule_of_the_references_value(name):
    fh.check_case(name, _lib(), DEV)


@pytest.mark.parametrize("name", ["d3", "d30", "d33_n20", "d65"])
def test_each_eigen_solve_on_its_own_keeps_the_trace(name):
    fh.check_solve_alone(name, _lib(), DEV)


@pytest.mark.parametrize("name", ["d1", "d30", "d33_n20", "d65"])
def test_identical_statistics_have_distance_zero(name):
    fh.check_identical(name, _lib(), DEV)


def test_a_zero_covariance_is_finite_without_a_retry():
    for name in ("d3", "d30", "d65"):
        fh.check_zero_sigma1(name, _lib(), DEV)


def test_an_asymmetric_input_counts_by_its_symmetric_part():
    for name in ("d17", "d65"):
        fh.check_asymmetric(name, _lib(), DEV)


def test_a_covariance_that_is_not_psd_is_refused_or_clamped():
    for name in ("d30", "d65"):
        fh.check_not_psd(name, DEV)


@pytest.mark.parametrize("D,N", [(256, 1000), (512, 4000), (512, 300)])
def test_evaluator_widths_against_the_host_formula_on_the_same_statistics(D, N):
    from mdm_amd import metrics as M
    x1, x2 = fh.make_sets(D, N, 7400 + D + N)
    s1 = M.calculate_activation_statistics(torch.from_numpy(x1).to(DEV))
    s2 = M.calculate_activation_statistics(torch.from_numpy(x2).to(DEV))
    host = [t.cpu().numpy() for t in (*s1, *s2)]
    ref = float(M.calculate_fid(s1, s2))
    alt = fh.frechet_eigh(host[0], host[1], host[2], host[3])[0]
    d, S = abs(ref - alt), fh.scale_of(host[0], host[1], host[2], host[3])
    res, sw = fh.raw_call(_lib(), DEV, host[0], host[1], host[2], host[3])
    got = M.calculate_fid_device(s1, s2)
    print(f"[frechet] D {D} N {N}: |got - ref| / S {abs(res[0] - ref) / S:.3e}  d / S {d / S:.3e}  bound / S {fh.bound(d, S) / S:.3e}  "
          f"sweeps {sw.tolist()}  ref {ref:.9g}")
    assert got.is_cuda and got.dim() == 0 and float(got.item()) == res[0]
    assert abs(res[0] - ref) <= fh.bound(d, S)
    assert 2 <= sw[0] < fh.MAX_SWEEPS and 2 <= sw[1] < fh.MAX_SWEEPS


def test_two_calls_a_side_stream_and_a_poisoned_workspace_give_the_same_bits():
    lib = _lib()
    for name in ("d30", "d65"):
        main = fh.check_poison(name, lib, DEV)                           # zeros, then 0xFF: two calls, the same bits
        side = torch.cuda.Stream(device=DEV)
        mu1, s1, mu2, s2 = fh.stats_of(name)
        with torch.cuda.stream(side):
            other = fh.raw_call(lib, DEV, mu1, s1, mu2, s2, 0xFF, stream=side.cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(main[0], other[0]) and np.array_equal(main[1], other[1])


def test_a_captured_call_replays_the_eager_bits():
    """check=False touches nothing on the host, so the call (3911 launches at D = 65) is captured into a graph after one warm-up
    call; the replay returns the eager call's bits."""
    from mdm_amd import metrics as M
    t = [torch.from_numpy(np.array(a)).to(DEV) for a in fh.stats_of("d65")]
    eager = M.frechet_distance_device(*t, check=False).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = M.frechet_distance_device(*t, check=False)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    print(f"[frechet] graph replay {out.item():.12g}  eager {eager.item():.12g}")
    assert out.item() == eager.item() and np.isfinite(eager.item())


def test_evaluate_unconstrained_metrics_with_the_fid_on_the_device(tmp_path):
    """The synthetic motions of tests/test_gpu_metrics.py's end-to-end test: with fid_on_device=True the FID is the device function's
    on the same statistics and stands within the rule of the default path's; every other entry is unchanged."""
    import stgcn_helpers as sh
    from mdm_amd import metrics as M
    from mdm_amd import unconstrained_eval as ue
    weights = sh.build_weights("unc", 102, "trained")
    model_path, data_path = str(tmp_path / "stgcn.pth.tar"), str(tmp_path / "dataset.npy")
    torch.save(weights, model_path)
    rs = np.random.RandomState(7101)
    generated = (rs.standard_normal((12, 15, 3, 20)) * 0.8).astype(np.float32)
    dataset = (rs.standard_normal((12, 16, 3, 20)) * 0.8 + 0.1).astype(np.float32)
    np.save(data_path, dataset)
    out = {}
    for on in (False, True):
        np.random.seed(7102)
        out[on] = ue.evaluate_unconstrained_metrics(generated, torch.device(DEV), True, act_rec_model_path=model_path, dataset_path=data_path,
                                                    kid_subsets=3, kid_subset_size=12, fid_on_device=on)
    model = ue.initialize_model(torch.device(DEV), model_path)
    gen_f, _ = ue.compute_features(model, ue.centre_root(generated), torch.device(DEV))
    real_f, _ = ue.compute_features(model, ue.centre_root(dataset[:, :15]), torch.device(DEV))
    s1, s2 = M.calculate_activation_statistics(gen_f), M.calculate_activation_statistics(real_f)
    host = [t.cpu().numpy() for t in (*s1, *s2)]
    d, S = abs(out[False]["fid"] - fh.frechet_eigh(*host)[0]), fh.scale_of(*host)
    print(f"[frechet] end to end: device {out[True]['fid']:.12g} host {out[False]['fid']:.12g}  |diff| / S "
          f"{abs(out[True]['fid'] - out[False]['fid']) / S:.3e}  d / S {d / S:.3e}")
    assert isinstance(out[True]["fid"], float) and out[True]["fid"] == M.calculate_fid_device(s1, s2).item()
    assert abs(out[True]["fid"] - out[False]["fid"]) <= fh.bound(d, S)
    assert {k: v for k, v in out[True].items() if k != "fid"} == {k: v for k, v in out[False].items() if k != "fid"}
