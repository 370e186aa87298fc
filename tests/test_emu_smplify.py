"""csrc/smplify.h and csrc/smplify_api.h on the CPU emulation of the HIP kernels (tests/emu): the value and gradient of both fitting
losses against the float64 oracle at T = 1, F - 1, F, F + 1 and 2 F + 1 frames (F = 32 frames per workgroup) with every operand
regime of tests/smplify_helpers.py, the exact properties, the optimiser at a short horizon and one whole fit at T = 3.  Every test
prints its figures before it asserts; tests/test_gpu_smplify.py runs the same checks on the MI355X."""
import numpy as np
import pytest

import smplify_helpers as H
from emu.emu_lib import emu


@pytest.fixture(scope="module")
def bench():
    return H.Bench(emu(), "cpu")


@pytest.mark.parametrize("T,kind", H.CASES)
@pytest.mark.parametrize("stage", [1, 2])
def test_value_and_gradient_against_the_float64_oracle(bench, stage, T, kind):
    H.check_value_grad(bench, stage, T, kind, "emu")


@pytest.mark.parametrize("stage", [1, 2])
def test_a_frames_terms_and_gradient_do_not_depend_on_where_it_stands(bench, stage):
    H.check_position_invariance(bench, stage, "emu")


def test_two_calls_poisoned_workspace_and_outputs_give_the_same_bits(bench):
    H.check_determinism_and_poison(bench, "emu")


def test_a_nan_in_the_joints_is_refused_and_nothing_is_written(bench):
    H.check_nan_is_refused(bench, "emu")


def test_a_nan_the_first_pass_does_not_see_is_reported_behind_the_evaluation(bench):
    H.check_late_nan_is_reported(bench, "emu")


def test_two_fits_and_a_poisoned_workspace_give_the_same_bits(bench):
    H.check_fit_repetition_and_poison(bench, "emu")


def test_argument_checks(bench):
    nat, lib = bench.nat, bench.lib
    import ctypes as C
    call = nat.MdmSmplifyCall()
    assert lib.mdm_smplify_workspace_bytes(C.byref(bench.model), C.byref(call), 0) == 0 and b"T must be at least 1" in lib.mdm_last_error()
    assert lib.mdm_smplify_workspace_bytes(C.byref(bench.model), C.byref(nat.MdmSmplifyCall(history=129)), 4) == 0
    assert b"history" in lib.mdm_last_error()
    inp = H.fixture("value_grad")
    ws, nbytes = bench.workspace(call, 3)
    x = bench.to(H.flat(2, inp, 3))
    args = [C.byref(bench.model), C.byref(call), 2, x.data_ptr(), None, x.data_ptr(), None, None, x.data_ptr(), x.data_ptr(), 3,
            x.data_ptr(), x.data_ptr(), None, (C.c_float * 3)(), ws.data_ptr(), nbytes - 1, None]
    assert lib.mdm_smplify_value_grad(*args) == -3 and b"workspace_bytes too small" in lib.mdm_last_error()
    args[2] = 3
    assert lib.mdm_smplify_value_grad(*args) == -1 and b"stage must be 1 or 2" in lib.mdm_last_error()


@pytest.mark.parametrize("T", [3, H.F + 1])
def test_the_optimiser_at_a_short_horizon(bench, T):
    got = H.check_short_horizon(bench, T, "emu")
    H.check_fit_outputs(got, H.fixture("fit_short_T%d" % T)["j3d"])


def test_the_whole_fit_at_three_frames_and_its_result_as_initial_values(bench):
    got = H.check_whole_fit(bench, 3, "emu")
    # the result as init_params-style initial values: runs, and does not get worse
    fx = H.fixture("fit_full_T3")
    again = bench.fit(fx["j3d"], H.conf_of("ones"), H.short_call(bench.nat), init=(got["pose"], got["betas"]))
    print(f"[smplify emu] restarted from the result: final loss {again['stats'][5]:.6e} (was {got['stats'][5]:.6e})")
    assert np.isfinite(again["pose"]).all() and again["stats"][5] <= got["stats"][5] * (1 + 1e-3)
