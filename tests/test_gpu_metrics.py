"""mdm_amd/metrics.py and mdm_amd/unconstrained_eval.py on the MI355X: every case of tests/metrics_helpers.py -- tile edges in N
(k + 1, T - 1, T, T + 1, 2 T + 1; NA != NB), D = 256, 30 and 1, KID subsets of 3, T - 1, T + 1 and 2 T + 1 rows with and without
replacement, degree 3 and 2 -- the duplicated rows, pair and subset invariance bit for bit, poison, a side stream, the fixtures of the
reference's own run, and evaluate_unconstrained_metrics end to end on synthetic motions.

Bounds (tests/metrics_helpers.py): radius^2 and distances relative (D + 4) 2^-24 against fp64; membership bitmaps and the precision /
recall floats exact (zero fragile rows: a condition on the inputs); mu / sigma max-abs (N + 8) 2^-52 4 max|x|^2; mmd2 / var within
4 x e_ref, the reference's own error pooled per (D, regime, m) (tests/golden/PIN_REPORT_metrics.json; the reference tree is not needed
here).  Every test prints its figures before it asserts; tools/bench_metrics.py collects timings into profiles/r18a_metrics.md."""
import numpy as np
import pytest
import torch

import metrics_helpers as mh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from mdm_amd import _native as nat
    return nat.load_native()


@pytest.mark.parametrize("name", list(mh.PR_CASES))
def test_precision_recall_case_equals_the_oracle_and_the_reference(name):
    mh.check_pr_case(name, DEV)


@pytest.mark.parametrize("name", [n for n in mh.KID_CASES if n != "fixture"])
def test_kid_case_meets_the_accuracy_condition(name):
    mh.check_kid_case(name, DEV)


@pytest.mark.parametrize("name", list(mh.STATS_CASES))
def test_statistics_case_meets_the_bound(name):
    mh.check_stats_case(name, DEV)


@pytest.mark.parametrize("name", list(mh.DIST_CASES))
def test_pair_distances_and_their_mean(name):
    mh.check_dist_case(name, DEV)


def test_duplicated_rows_have_radius_zero_and_decide_exactly():
    mh.check_duplicates(DEV)


def test_a_rows_radius_does_not_depend_on_where_the_row_stands():
    mh.check_pair_invariance(DEV)


def test_a_subsets_result_does_not_depend_on_the_other_subsets():
    mh.check_subset_independence(DEV)


def test_poison_determinism_and_a_side_stream():
    """0xFF workspaces and NaN outputs: the bits of a run over zeros (two calls: the same bits of every output); then the same calls
    on a side stream behind the default stream's: the default stream's bits."""
    lib = _lib()
    main = mh.check_poison(lib, DEV, torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        other = mh.raw_calls(lib, DEV, side.cuda_stream, 0xFF, float("nan"))
    torch.cuda.synchronize()
    for k in main:
        assert np.array_equal(main[k], other[k]), k


def test_fixtures_of_the_references_own_run():
    mh.check_fixtures(DEV)


def test_evaluate_unconstrained_metrics_end_to_end(tmp_path):
    """12 synthetic motions [12, 15, 3, 20] against a 12-motion synthetic dataset file (16 joints, as the real file), the
    unconstrained ST-GCN at full width on seeded weights, kid_subsets=3, kid_subset_size=12, fast=False: every entry of the dictionary
    equals the module functions on the features the recogniser returns (fid: the host formula on the returned statistics, bit for
    bit).  The wiring, not the network (tests/test_gpu_stgcn.py pins that)."""
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
    kept = generated.copy()

    np.random.seed(7102)
    got = ue.evaluate_unconstrained_metrics(generated, torch.device(DEV), False, act_rec_model_path=model_path, dataset_path=data_path,
                                            kid_subsets=3, kid_subset_size=12)
    assert np.array_equal(generated, kept)                                     # the caller's motions are not centred in place
    assert sorted(got) == ["diversity_gen", "diversity_gt", "fid", "kid", "precision", "recall"]

    model = ue.initialize_model(torch.device(DEV), model_path)
    assert type(model).__name__ == "STGCNUnconstrained" and not model.training
    gen_f, gen_y = ue.compute_features(model, ue.centre_root(generated), torch.device(DEV))
    real_f, _ = ue.compute_features(model, ue.centre_root(dataset[:, :15]), torch.device(DEV))
    assert gen_f.shape == (12, 256) and gen_y.shape == (12, 12) and gen_f.is_cuda
    centred = generated - generated[:, 8:9]
    assert torch.equal(ue.centre_root(generated), torch.from_numpy(centred))
    np.random.seed(7102)
    fid = M.calculate_fid(M.calculate_activation_statistics(gen_f), M.calculate_activation_statistics(real_f))
    kid = M.calculate_kid(real_f, gen_f, n_subsets=3, subset_size=12)
    div_gt, div_gen = M.calculate_diversity(real_f), M.calculate_diversity(gen_f)
    precision, recall = M.precision_and_recall(gen_f, real_f)
    print(f"[metrics] end to end: {got}")
    assert got["fid"] == fid and np.isfinite(fid)
    assert got["kid"] == kid[0] and np.isfinite(kid[0])
    assert got["diversity_gen"] == div_gen.item() and got["diversity_gt"] == div_gt.item()
    assert got["precision"] == precision and got["recall"] == recall and 0.0 <= precision <= 1.0 and 0.0 <= recall <= 1.0
    # fast=True skips precision / recall only
    np.random.seed(7102)
    fast = ue.evaluate_unconstrained_metrics(generated, torch.device(DEV), True, act_rec_model_path=model_path, dataset_path=data_path,
                                             kid_subsets=3, kid_subset_size=12)
    assert fast["precision"] is None and fast["recall"] is None
    assert {k: v for k, v in fast.items() if k not in ("precision", "recall")} == {k: v for k, v in got.items() if k not in ("precision", "recall")}
