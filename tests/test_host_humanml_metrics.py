"""mdm_amd/humanml_metrics.py, mdm_amd/a2m_metrics.py and mdm_amd/humanml_eval.py without a device: the refusals of the three native
calls (each with its message in mdm_last_error, before any launch) and of the modules (ValueErrors that name the argument), ABI 10
with the additive exports declared, kind 9 still unknown, a corrupt offset table (clamped on the device side: wrong ranks, no access
out of bounds), the a2m index sequence against the reference's recorded draws with numpy's generator in the reference's state, and
evaluation()'s call sequence and printed lines on stub loaders through the emulator."""
import numpy as np
import pytest
import torch

import humanml_metrics_helpers as hh
from emu.emu_lib import emu
from mdm_amd import _native as nat
from mdm_amd import a2m_metrics as A
from mdm_amd import humanml_metrics as H
from mdm_amd import metrics as M


@pytest.fixture()
def lib():
    M.NATIVE_LIB = emu()
    yield M.NATIVE_LIB
    M.NATIVE_LIB = None


def test_abi_is_still_10_and_the_exports_are_declared(lib):
    assert lib.mdm_abi_version() == 10 and nat.ABI_VERSION == 10
    for name in ("mdm_retrieval_ranks", "mdm_dist_matrix", "mdm_confusion"):
        assert name in nat.EXPORTED_SYMBOLS and callable(getattr(lib, name))
    assert (nat.METRICS_KINDS["retrieval_ranks"], nat.METRICS_KINDS["dist_matrix"], nat.METRICS_KINDS["confusion"]) == (5, 6, 7)
    with open(hh.os.path.join(hh.ROOT, "include", "mdm_hip.h")) as fh:
        header = fh.read()
    for line in ("#define MDM_ABI_VERSION 10", "#define MDM_METRICS_RETRIEVAL_RANKS 5", "#define MDM_METRICS_DIST_MATRIX 6",
                 "#define MDM_METRICS_CONFUSION 7", "int mdm_retrieval_ranks(", "int mdm_dist_matrix(", "int mdm_confusion("):
        assert line in header, line
    for kind in (5, 6, 7):
        assert lib.mdm_metrics_workspace_bytes(kind, 8, 1) == 64
    assert lib.mdm_metrics_workspace_bytes(9, 8, 1) == 0 and "kind" in lib.mdm_last_error().decode()
    assert lib.mdm_metrics_workspace_bytes(8, 8, 1) == 0 and lib.mdm_metrics_workspace_bytes(5, 0, 1) == 0


def test_native_calls_refuse_bad_arguments_with_a_message(lib):
    x = np.zeros((8, 4), dtype=np.float32)
    out = np.zeros(64, dtype=np.float64)
    off = np.array([0, 8], dtype=np.int32)
    ws = np.zeros(4096, dtype=np.uint8)
    px, po, pf, pw, n = x.ctypes.data, out.ctypes.data, off.ctypes.data, ws.ctypes.data, ws.nbytes
    err = lambda: lib.mdm_last_error().decode()      # noqa: E731
    EINVAL, ENOSPC, EUNSUP = -1, -3, -5
    names = ("q", "c", "N", "D", "off", "groups", "rows", "top_k", "rank", "diag", "topk", "dsum", "ws", "n", "stream")
    base = dict(q=px, c=px, N=8, D=4, off=pf, groups=1, rows=8, top_k=3, rank=po, diag=po + 64, topk=po + 128, dsum=po + 256, ws=pw, n=n,
                stream=None)
    call = lambda **o: lib.mdm_retrieval_ranks(*[{**base, **o}[k] for k in names])      # noqa: E731
    for arg, text in (("q", "null q_dev"), ("c", "null c_dev"), ("off", "null group_offsets_dev"), ("rank", "null rank_dev"),
                      ("diag", "null diag_dev"), ("topk", "null topk_count_dev"), ("dsum", "null diag_sum_dev"), ("ws", "null workspace_dev")):
        assert call(**{arg: None}) == EINVAL and text in err(), arg
    assert call(q=px + 2) == EINVAL and "aligned" in err()
    assert call(topk=po + 4) == EINVAL and "8-byte aligned" in err()
    assert call(groups=0) == EINVAL and "n_groups must be at least 1" in err()
    assert call(rows=0) == EINVAL and "max_group_rows must be at least 1" in err()
    for k in (0, 17, -1):
        assert call(top_k=k) == EINVAL and "between 1 and 16" in err()
    assert call(N=0) == EINVAL and "at least one row" in err()
    assert call(D=0) == EINVAL and "D must be at least 1" in err()
    assert call(N=1 << 16, D=1 << 15) == EUNSUP and "2^31" in err()
    assert call(n=63) == ENOSPC and "workspace_bytes too small" in err()
    assert call() == 0                                                        # (the same arguments, unharmed, run)
    # mdm_dist_matrix
    assert lib.mdm_dist_matrix(None, 8, px, 8, 4, po, pw, n, None) == EINVAL and "null a_dev" in err()
    assert lib.mdm_dist_matrix(px, 8, None, 8, 4, po, pw, n, None) == EINVAL and "null b_dev" in err()
    assert lib.mdm_dist_matrix(px, 8, px, 0, 4, po, pw, n, None) == EINVAL and "b_dev must hold" in err()
    assert lib.mdm_dist_matrix(px, 8, px, 8, 4, None, pw, n, None) == EINVAL and "null out_dev" in err()
    assert lib.mdm_dist_matrix(px, 1 << 16, px, 1 << 15, 1, po, pw, n, None) == EUNSUP and "NA * NB" in err()
    assert lib.mdm_dist_matrix(px, 8, px, 8, 4, po, pw, 8, None) == ENOSPC
    # mdm_confusion
    assert lib.mdm_confusion(None, pf, 8, 4, po, po + 64, po + 32, pw, n, None) == EINVAL and "null yhat_dev" in err()
    assert lib.mdm_confusion(px, None, 8, 4, po, po + 64, po + 32, pw, n, None) == EINVAL and "null labels_dev" in err()
    assert lib.mdm_confusion(px, pf, 8, 4, None, po + 64, po + 32, pw, n, None) == EINVAL and "null pred_dev" in err()
    assert lib.mdm_confusion(px, pf, 8, 4, po, None, po + 32, pw, n, None) == EINVAL and "null confusion_dev" in err()
    assert lib.mdm_confusion(px, pf, 8, 4, po, po + 64, None, pw, n, None) == EINVAL and "null bad_dev" in err()
    assert lib.mdm_confusion(px, pf, 8, 0, po, po + 64, po + 32, pw, n, None) == EINVAL and "C must be at least 1" in err()
    assert lib.mdm_confusion(px, pf, 1 << 16, 1 << 15, po, po + 64, po + 32, pw, n, None) == EUNSUP and "2^31" in err()
    assert lib.mdm_confusion(px, pf, 8, 4, po, po + 68, po + 32, pw, n, None) == EINVAL and "8-byte aligned" in err()
    assert lib.mdm_abi_version() == 10


def test_a_corrupt_offset_table_is_clamped(lib):
    """Offsets below 0, beyond N, descending, and groups larger than max_group_rows: the call runs, every rank it writes is a count
    within a group of at most max_group_rows rows, and rows outside every clamped group keep their bytes."""
    text, motion = hh.make_pair(70, 30, 5, 1.0, 8801)
    q, c = torch.from_numpy(text), torch.from_numpy(motion)
    ws = torch.zeros(64, dtype=torch.uint8)
    for table, rows in (([-5, 1000, 3], 70), ([0, 70], 16), ([60, 20, 1 << 30, -(1 << 30)], 70), ([0, 10, 20], 0x7FFFFFFF)):
        off = torch.tensor(table, dtype=torch.int32)
        rank = torch.full((70,), -7, dtype=torch.int32)
        diag = torch.full((70,), -1.0)
        topk, dsum = torch.zeros(3, dtype=torch.int64), torch.zeros((), dtype=torch.float64)
        assert lib.mdm_retrieval_ranks(q.data_ptr(), c.data_ptr(), 70, 30, off.data_ptr(), len(table) - 1, rows, 3, rank.data_ptr(),
                                       diag.data_ptr(), topk.data_ptr(), dsum.data_ptr(), ws.data_ptr(), 64, None) == 0
        written = rank != -7
        assert ((rank[written] >= 0) & (rank[written] < min(rows, 70))).all() and (diag[written] >= 0).all() and (diag[~written] == -1.0).all()
    assert written[:20].all() and not written[20:].any()                      # the last table: rows 0 .. 19 in two groups


def test_the_modules_refuse_bad_arguments_by_name(lib):
    a, b = torch.zeros(8, 4), torch.zeros(8, 5)
    with pytest.raises(ValueError, match="motion has 5"):
        H.retrieval(a, b, [8])
    with pytest.raises(ValueError, match="motion 7"):
        H.retrieval(a, a[:7], [8])
    with pytest.raises(ValueError, match="add up to 7"):
        H.retrieval(a, a, [3, 4])
    with pytest.raises(ValueError, match="positive"):
        H.retrieval(a, a, [8, 0])
    with pytest.raises(ValueError, match="integers"):
        H.retrieval(a, a, [4.5, 3.5])
    with pytest.raises(ValueError, match="integers"):
        H.retrieval(a, a, [])
    for k in (0, 17, 2.5):
        with pytest.raises(ValueError, match="top_k"):
            H.retrieval(a, a, [8], k)
    with pytest.raises(ValueError, match="matrix2 has 5"):
        H.euclidean_distance_matrix(a, b)
    with pytest.raises(ValueError, match="matrix1"):
        H.euclidean_distance_matrix(torch.zeros(8), a)
    with pytest.raises(IndexError):
        H.calculate_top_k(torch.zeros(2, 2, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="diversity_times"):
        H.calculate_diversity(a, 8)
    with pytest.raises(ValueError, match="multimodality_times"):
        H.calculate_multimodality(torch.zeros(3, 4, 5), 4)
    with pytest.raises(ValueError, match="num_per_sent"):
        H.calculate_multimodality(a, 2)
    with pytest.raises(ValueError, match="labels holds 7"):
        A.calculate_diversity_multimodality(a, torch.zeros(7, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 3\)"):
        A.calculate_diversity_multimodality(a, torch.full((8,), 3), 3)
    with pytest.raises(ValueError, match="yhat has 4 classes"):
        A.confusion(a, torch.zeros(8, dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="labels holds 7"):
        A.confusion(a, torch.zeros(7, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="confusion_matrix must be"):
        A.confusion(a, torch.zeros(8, dtype=torch.int64), 4, torch.zeros(4, 4), torch.zeros((), dtype=torch.int32))
    with pytest.raises(ValueError, match="style"):
        A.calculate_accuracy(None, [], 4, None, "cpu", style="gru")
    with pytest.raises(ValueError, match="no batch"):
        A.calculate_accuracy(None, [], 4, None, "cpu")
    # upstream's re-exports are mdm_amd.metrics' functions
    assert H.calculate_activation_statistics is M.calculate_activation_statistics and H.calculate_frechet_distance is M.calculate_frechet_distance


def test_product_path_refuses_host_tensors(monkeypatch):
    """With the product library bound, features on the host are an error -- not a silent CPU computation."""
    class Product:
        path = "/somewhere/" + nat.LIB_NAME
    monkeypatch.setattr(M, "NATIVE_LIB", Product())
    x = torch.zeros(8, 4)
    for call in (lambda: H.retrieval(x, x, [8]), lambda: H.euclidean_distance_matrix(x, x), lambda: H.calculate_matching_score(x, x),
                 lambda: H.calculate_diversity(x, 3), lambda: A.confusion(x, torch.zeros(8, dtype=torch.int64), 4),
                 lambda: A.calculate_diversity_multimodality(x, torch.zeros(8, dtype=torch.int64), 2)):
        with pytest.raises(nat.MdmError, match="cuda"):
            call()


def test_a2m_index_sequence_is_the_references(monkeypatch):
    """calculate_diversity_multimodality: the two randint vectors, then the quota loop with its rejection draws, as the restatement
    that was checked against the reference's own run draws them (tests/golden/humanml_metrics_a2m.npz records that run's pairs and the
    np.random.rand() that followed it).  The native layer is replaced by a recorder."""
    seen = []

    def fake(x, first, second):
        seen.append((np.asarray(first).copy(), np.asarray(second).copy()))
        return None, torch.ones((), dtype=torch.float64)
    monkeypatch.setattr(M, "gather_dist", fake)
    z = hh.load_fixture("a2m")
    x, labels = torch.from_numpy(z["x"]), torch.from_numpy(z["labels"])
    for kw in ({}, {"seed": int(z["np_seed"])}):
        seen.clear()
        np.random.seed(0 if kw else int(z["np_seed"]))
        div, mm = A.calculate_diversity_multimodality(x, labels, int(z["num_labels"]), **kw)
        assert np.random.rand() == float(z["rand_after"])
        assert len(seen) == 2
        assert np.array_equal(seen[0][0], z["first"]) and np.array_equal(seen[0][1], z["second"])
        assert np.array_equal(seen[1][0], z["pairs"][:, 0]) and np.array_equal(seen[1][1], z["pairs"][:, 1])
        # five of six labels appear: 100 pairs, divided by 20 * 6
        assert len(z["pairs"]) == 100 and div == 1.0 and mm == 100 / 120
        assert (z["labels"][z["pairs"][:, 0]] == z["labels"][z["pairs"][:, 1]]).all()
    # unconstrained: no label is read, no second call, nan
    seen.clear()
    np.random.seed(int(z["np_seed"]))
    div, mm = A.calculate_diversity_multimodality(x, None, int(z["num_labels"]), unconstrained=True)
    assert len(seen) == 1 and np.array_equal(seen[0][0], z["first"]) and div == 1.0 and np.isnan(mm)


def test_humanml_draws_are_upstreams_in_upstreams_order(monkeypatch):
    """calculate_diversity / calculate_multimodality: two np.random.choice(replace=False) draws each; the pairs that reach the native
    call are the replayed draws, flattened per sentence for multimodality; the generator ends in the reference's state."""
    seen = {}

    def fake(x, first, second):
        seen.update(rows=tuple(x.shape), first=np.asarray(first).copy(), second=np.asarray(second).copy())
        return None, torch.zeros((), dtype=torch.float64)
    monkeypatch.setattr(H, "gather_dist", fake)
    z = hh.load_fixture("diversity")
    np.random.seed(int(z["np_seed"]))
    H.calculate_diversity(torch.from_numpy(z["x"]), int(z["times"]))
    assert np.random.rand() == float(z["rand_after"])
    np.random.seed(int(z["np_seed"]))
    first, second = np.random.choice(80, 30, replace=False), np.random.choice(80, 30, replace=False)
    assert np.array_equal(seen["first"], first) and np.array_equal(seen["second"], second) and len(set(first)) == 30
    z = hh.load_fixture("multimodality")
    np.random.seed(int(z["np_seed"]))
    H.calculate_multimodality(torch.from_numpy(z["x"]), int(z["times"]))
    assert np.random.rand() == float(z["rand_after"])
    np.random.seed(int(z["np_seed"]))
    first, second = np.random.choice(8, 5, replace=False), np.random.choice(8, 5, replace=False)
    assert seen["rows"] == (48, 32) and len(seen["first"]) == 30
    assert np.array_equal(seen["first"], (np.arange(6)[:, None] * 8 + first[None]).reshape(-1))
    assert np.array_equal(seen["second"], (np.arange(6)[:, None] * 8 + second[None]).reshape(-1))


def test_evaluation_call_sequence_and_printed_lines(lib, tmp_path, capsys):
    hh.check_evaluation("cpu", tmp_path, capsys)


def test_calculate_accuracy_both_calling_conventions(lib):
    hh.check_accuracy("cpu")


def test_humanml_eval_keeps_upstreams_signatures():
    import inspect
    from mdm_amd import humanml_eval as E
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert sig(E.evaluate_matching_score) == ["eval_wrapper", "motion_loaders", "file"]
    assert sig(E.evaluate_fid) == ["eval_wrapper", "groundtruth_loader", "activation_dict", "file"]
    assert sig(E.evaluate_diversity) == ["activation_dict", "file", "diversity_times"]
    assert sig(E.evaluate_multimodality) == ["eval_wrapper", "mm_motion_loaders", "file", "mm_num_times"]
    assert sig(E.get_metric_statistics) == ["values", "replication_times"]
    assert sig(E.evaluation) == ["eval_wrapper", "gt_loader", "eval_motion_loaders", "log_file", "replication_times", "diversity_times",
                                 "mm_num_times", "run_mm", "eval_platform"]
    assert sig(H.calculate_R_precision) == ["embedding1", "embedding2", "top_k", "sum_all"]
    assert sig(H.calculate_matching_score) == ["embedding1", "embedding2", "sum_all"]
    assert sig(H.calculate_diversity) == ["activation", "diversity_times"] and sig(H.calculate_multimodality) == ["activation", "multimodality_times"]
    assert sig(A.calculate_diversity_multimodality) == ["activations", "labels", "num_labels", "seed", "unconstrained"]
    assert sig(A.calculate_accuracy)[:5] == ["model", "motion_loader", "num_labels", "classifier", "device"]
    mean, ci = E.get_metric_statistics(np.array([1.0, 3.0]), 2)
    assert mean == 2.0 and ci == 1.96 * 1.0 / np.sqrt(2)
