"""csrc/humanml_metrics.h (mdm_retrieval_ranks, mdm_dist_matrix, mdm_confusion behind mdm_amd/humanml_metrics.py and
mdm_amd/a2m_metrics.py) on the CPU wave emulator of tests/emu: every case of tests/humanml_metrics_helpers.py -- group sizes at the
edges of the 64-row tile and of top_k, mixed inside one call, D = 512, 30 and 1 -- under the bounds of the GPU test: ranks, top-k counts,
predictions and confusion matrices exact (zero fragile rows), distances relative (D + 4) 2^-24 against fp64, sums to (n + 2) 2^-52
of the fp64 sum of the returned values, and the reference's own values (tests/golden/humanml_metrics_*.npz) within 4 x its own error."""
import pytest

from emu.emu_lib import emu
import humanml_metrics_helpers as hh

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def lib():
    from mdm_amd import metrics as M
    M.NATIVE_LIB = emu()
    yield M.NATIVE_LIB
    M.NATIVE_LIB = None


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


def test_poison_in_workspace_and_outputs_does_not_reach_the_results(lib):
    hh.check_poison(lib, DEV, None)


def test_fixtures_of_the_references_own_run():
    hh.check_fixtures(DEV)
