"""csrc/metrics.h (mdm_knn_radius, mdm_manifold_members, mdm_gather_dist, mdm_poly_mmd, mdm_feature_stats behind mdm_amd/metrics.py) on
the CPU wave emulator of tests/emu: the cases of tests/metrics_helpers.py at reduced sizes -- every pair kernel sees one, two and
three tiles (N, m = 3 / 4, 63, 64, 65, 129), D = 30 (no multiple of 4 or of the k chunk), 1, and 256 where a second feature chunk
matters -- under the bounds of the GPU test: radius^2 and distances relative (D + 4) 2^-24 against fp64, membership bitmaps and the
precision / recall floats exact (zero fragile rows), mu / sigma max-abs (N + 8) 2^-52 4 max|x|^2, mmd2 / var within 4 x the
reference's own pooled error (tests/golden/PIN_REPORT_metrics.json holds the pools of these shapes)."""
import pytest

from emu.emu_lib import emu
import metrics_helpers as mh

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def lib():
    from mdm_amd import metrics as M
    M.NATIVE_LIB = emu()
    yield M.NATIVE_LIB
    M.NATIVE_LIB = None


@pytest.mark.parametrize("name", mh.EMU_PR_CASES)
def test_precision_recall_case_equals_the_oracle_and_the_reference(name):
    mh.check_pr_case(name, DEV)


@pytest.mark.parametrize("name", mh.EMU_KID_CASES)
def test_kid_case_meets_the_accuracy_condition(name):
    mh.check_kid_case(name, DEV)


@pytest.mark.parametrize("name", mh.EMU_STATS_CASES)
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


def test_poison_in_workspace_and_outputs_does_not_reach_the_results(lib):
    mh.check_poison(lib, DEV, None)


def test_fixtures_of_the_references_own_run():
    mh.check_fixtures(DEV)
