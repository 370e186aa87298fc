"""mdm_amd/humanml_metrics.py, mdm_amd/a2m_metrics.py and mdm_amd/humanml_eval.py on the MI355X: every case of
tests/humanml_metrics_helpers.py -- group sizes at the edges of the 64-row tile and of top_k, mixed inside one call, D = 512, 30 and 1;
the distance matrix with NA != NB; argmax + confusion with equal maxima, NaNs and labels out of range, in one call and accumulated --
group invariance bit for bit, the tie rule, poison, a side stream, the fixtures of the reference's own run, and evaluation() end to
end on stub loaders.

Bounds (tests/humanml_metrics_helpers.py): ranks, top-k counts, predictions and confusion matrices exact (zero fragile rows: a
condition on the inputs); distances relative (D + 4) 2^-24 against fp64; sums to (n + 2) 2^-52 of the fp64 sum of the returned
values; the reference's values within 4 x e_ref (tests/golden/PIN_REPORT_humanml_metrics.json; the reference tree is not needed
here).  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import humanml_metrics_helpers as hh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from mdm_amd import _native as nat
    return nat.load_native()


@pytest.mark.parametrize("name", list(hh.CASES))
def test_retrieval_case_equals_the_oracle(name):
    hh.check_retrieval_case(name, DEV)


@pytest.mark.parametrize("name", list(hh.DIST_MATRIX_CASES))
def test_distance_matrix_case_meets_the_bound(name):
    hh.check_dist_matrix_case(name, DEV)


@pytest.mark.parametrize("name", list(hh.CONFUSION_CASES))
def test_confusion_case_is_exact(name):
    hh.check_confusion_case(name, DEV)


def test_confusion_accumulates_over_calls():
    hh.check_confusion_accumulates(DEV)


def test_a_groups_result_does_not_depend_on_where_the_group_stands():
    hh.check_group_invariance(DEV)


def test_equal_candidates_rank_by_the_tie_rule_and_equal_rows_are_at_distance_zero():
    hh.check_ties(DEV)


def test_poison_determinism_and_a_side_stream():
    """0xFF workspaces and NaN / 0x7F outputs: the bits of a run over zeros; then the same calls on a side stream behind the default
    stream's: the default stream's bits."""
    lib = _lib()
    main = hh.check_poison(lib, DEV, torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        other = hh.raw_calls(lib, DEV, side.cuda_stream, 0xFF, float("nan"))
    torch.cuda.synchronize()
    for k in main:
        assert np.array_equal(main[k], other[k]), k


def test_fixtures_of_the_references_own_run():
    hh.check_fixtures(DEV)


def test_evaluation_end_to_end_on_stub_loaders(tmp_path, capsys):
    hh.check_evaluation(DEV, tmp_path, capsys)


def test_calculate_accuracy_both_calling_conventions():
    hh.check_accuracy(DEV)
