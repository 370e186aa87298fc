"""csrc/frechet.h (mdm_frechet_distance behind mdm_amd.metrics.frechet_distance_device) on the CPU wave emulator of tests/emu: every
case of tests/frechet_helpers.py -- D = 1, 2, 3, 15, 16, 17, 30, 33 with 20 samples, 64 and 65 -- against the reference's own value
under the rule max(100 d, 1e-11 S); each eigen-solve on its own; identical statistics, a zero covariance, an asymmetric input and a
covariance that is not positive semi-definite; and, at D = 65, the launch-per-round form's early return."""
import numpy as np
import pytest

from emu.emu_lib import emu
import frechet_helpers as fh

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def lib():
    from mdm_amd import metrics as M
    M.NATIVE_LIB = emu()
    yield M.NATIVE_LIB
    M.NATIVE_LIB = None


@pytest.mark.parametrize("name", list(fh.CASES))
def test_case_is_within_the_rule_of_the_references_value(lib, name):
    fh.check_case(name, lib, DEV)


@pytest.mark.parametrize("name", ["d2", "d3", "d17", "d30", "d33_n20", "d64", "d65"])
def test_each_eigen_solve_on_its_own_keeps_the_trace(lib, name):
    fh.check_solve_alone(name, lib, DEV)


@pytest.mark.parametrize("name", ["d1", "d3", "d30", "d33_n20"])
def test_identical_statistics_have_distance_zero(lib, name):
    fh.check_identical(name, lib, DEV)


@pytest.mark.parametrize("name", ["d3", "d30"])
def test_a_zero_covariance_is_finite_without_a_retry(lib, name):
    fh.check_zero_sigma1(name, lib, DEV)


@pytest.mark.parametrize("name", ["d17", "d30"])
def test_an_asymmetric_input_counts_by_its_symmetric_part(lib, name):
    fh.check_asymmetric(name, lib, DEV)


@pytest.mark.parametrize("name", ["d3", "d30"])
def test_a_covariance_that_is_not_psd_is_refused_or_clamped(name):
    fh.check_not_psd(name, DEV)


def test_the_round_form_returns_early_and_ignores_what_the_workspace_held(lib):
    """D = 65: 30 sweeps of 65 launches are enqueued per solve; the solve ends after sweeps2 < 30 of them, and a workspace filled
    with 0xFF (counters, thresholds, both ping-pong buffers) gives the bits of one filled with zeros."""
    res, sw = fh.check_poison("d65", lib, DEV)
    assert fh.form_of(65) == "round" and 2 <= sw[0] < fh.MAX_SWEEPS and 2 <= sw[1] < fh.MAX_SWEEPS
    z = fh.load_case("d65")
    assert abs(res[0] - float(z["ref"])) <= fh.bound(float(z["d"]), float(z["S"]))


def test_the_small_form_ignores_what_the_workspace_held(lib):
    for name in ("d3", "d64"):
        fh.check_poison(name, lib, DEV)


def test_statistics_that_are_not_finite_give_nan_not_a_number(lib):
    """A NaN in sigma1 (small form and round form) reaches the result as NaN, and check=True says so."""
    import torch
    from mdm_amd import metrics as M
    for name in ("d3", "d65"):
        mu1, s1, mu2, s2 = fh.stats_of(name)
        bad = s1.copy()
        bad[0, 0] = np.nan
        res, sw = fh.raw_call(lib, DEV, mu1, bad, mu2, s2)
        assert np.isnan(res[0]) and np.isnan(res[1])
        with pytest.raises(ValueError):
            M.frechet_distance_device(*[torch.from_numpy(np.array(a)) for a in (mu1, bad, mu2, s2)])
