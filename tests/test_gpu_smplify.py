"""mdm_amd/simplify_loc2rot.py and csrc/smplify.h on the MI355X: the checks of tests/test_emu_smplify.py on the device -- value and
gradient against the float64 oracle within 4 x e_ref at T = 1, F - 1, F, F + 1, 2 F + 1, the exact properties (position, repetition,
poison, a side stream, a refused NaN), the optimiser at a short horizon, whole fits at T = 3 and T = 8 -- and joints2smpl end to end
into Rotation2xyzFull.  Every test prints its figures before it asserts; tools/bench_smplify.py collects the timings."""
import numpy as np
import pytest
import torch

import smplify_helpers as H
import smpl_mesh_helpers as smh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def bench():
    from mdm_amd import _native as nat
    return H.Bench(nat.load_native(), DEV)


@pytest.mark.parametrize("T,kind", H.CASES)
@pytest.mark.parametrize("stage", [1, 2])
def test_value_and_gradient_against_the_float64_oracle(bench, stage, T, kind):
    H.check_value_grad(bench, stage, T, kind, "gpu")


@pytest.mark.parametrize("stage", [1, 2])
def test_a_frames_terms_and_gradient_do_not_depend_on_where_it_stands(bench, stage):
    H.check_position_invariance(bench, stage, "gpu")


def test_poison_determinism_and_a_side_stream(bench):
    main = H.check_determinism_and_poison(bench, "gpu")
    side = torch.cuda.Stream(device=DEV)
    inp = H.fixture("value_grad")
    with torch.cuda.stream(side):
        other = {stage: bench.value_grad(stage, inp, H.conf_of("foot"), H.F + 1, poison=0xFF, fill=float("nan"), stream=side.cuda_stream)
                 for stage in (1, 2)}
    torch.cuda.synchronize()
    for stage in (1, 2):
        assert H.outputs_equal(main[stage], other[stage]), stage


def test_a_nan_in_the_joints_is_refused_and_nothing_is_written(bench):
    H.check_nan_is_refused(bench, "gpu")


def test_a_nan_the_first_pass_does_not_see_is_reported_behind_the_evaluation(bench):
    H.check_late_nan_is_reported(bench, "gpu")


def test_two_fits_and_a_poisoned_workspace_give_the_same_bits(bench):
    H.check_fit_repetition_and_poison(bench, "gpu")


def test_a_capturing_stream_is_refused(bench):
    import ctypes as C
    call = bench.nat.MdmSmplifyCall()
    inp = H.fixture("value_grad")
    ws, nbytes = bench.workspace(call, 3)
    x = bench.to(H.flat(2, inp, 3))
    j3d, conf, pres = bench.to(inp["j3d"][:3]), bench.to(H.conf_of("ones")), bench.to(inp["preserve"][:3])
    grad, terms = torch.zeros(255, device=DEV), torch.zeros(3, 6, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = bench.lib.mdm_smplify_value_grad(C.byref(bench.model), C.byref(call), 2, x.data_ptr(), None, pres.data_ptr(), None, None,
                                              j3d.data_ptr(), conf.data_ptr(), 3, grad.data_ptr(), terms.data_ptr(), None,
                                              (C.c_float * 3)(), ws.data_ptr(), nbytes, side.cuda_stream)
        msg = bench.lib.mdm_last_error().decode()
        grad.zero_()                  # (so that the capture is not empty)
    torch.cuda.synchronize()
    assert rc == -5 and "cannot be captured" in msg, (rc, msg)


@pytest.mark.parametrize("T", [3, H.F + 1])
def test_the_optimiser_at_a_short_horizon(bench, T):
    got = H.check_short_horizon(bench, T, "gpu")
    H.check_fit_outputs(got, H.fixture("fit_short_T%d" % T)["j3d"])


@pytest.mark.parametrize("T", [3, 8])
def test_the_whole_fit(bench, T):
    H.check_whole_fit(bench, T, "gpu")


def test_joints2smpl_end_to_end_into_the_mesh_path(tmp_path):
    """visualize/vis_utils.py:24-39 on the synthetic model: joints2smpl(num_frames, device_id).joint2smpl(joints) -> thetas ->
    Rotation2xyzFull.  The 'smpl' joints of the fitted thetas (the existing kernel) equal the fit's own model joints to float32 accuracy
    and lie within the fit distance of the input joints,
    the vertices come out finite, the dictionary has the reference's shapes, and its entries run as initial values."""
    from mdm_amd import simplify_loc2rot as s2r
    from mdm_amd.smpl_mesh import Rotation2xyzFull
    fields, extra, ids, _maps = smh.fixture_model()
    model_path, extra_path = smh.write_model_files(tmp_path, fields, extra)
    gmm_path = H.write_gmm(tmp_path / "prior")
    fx = H.fixture("fit_full_T8")
    T = 8
    fit = s2r.joints2smpl(num_frames=T, device_id=0, smpl_model_path=model_path, gmm_path=gmm_path, mean_params=H.mean_params())
    thetas, opt = fit.joint2smpl(fx["j3d"])
    assert tuple(thetas.shape) == (1, 25, 6, T) and thetas.is_cuda
    assert tuple(opt["pose"].shape) == (72,) and tuple(opt["betas"].shape) == (T, 10) and tuple(opt["cam"].shape) == (T, 1, 3)
    r2x = Rotation2xyzFull(device=torch.device(DEV), model_path=model_path, extra_regressor_path=extra_path, vertex_joint_ids=ids)
    kw = dict(mask=None, pose_rep="rot6d", translation=True, glob=True, vertstrans=True, beta=0, glob_rot=None, get_rotations_back=False)
    # (vis_utils passes betas=None: the mesh is the mean shape's.  The joints are compared at the fitted betas.)
    joints = r2x(thetas, jointstype="smpl", betas=opt["betas"], **kw)                      # [1, 24, 3, T], root-relative + translation
    verts = r2x(thetas, jointstype="vertices", betas=None, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(verts).all() and tuple(verts.shape) == (1, fields["v_template"].shape[0], 3, T)
    mesh = joints[0].permute(2, 0, 1).cpu().numpy().astype(np.float64)                      # [T, 24, 3]
    # the mesh path pins the root to thetas' row 24 (the input root): out[t, k] = (p_k - p_0)_t + j3d[t, 0] - j3d[0, 0]
    assert np.abs(mesh[:, 0] - (fx["j3d"][:, 0].astype(np.float64) - fx["j3d"][0, 0])).max() <= 1e-6
    mesh_rel = mesh - mesh[:, :1]
    # (1) the thetas and the tail kernel: the existing kernel's root-relative joints of the fitted thetas are the fit's own model
    # joints, root-relative, to float32 accuracy -- two float32 chains of at most 9 rotations over O(1) offsets, whose rotation
    # matrices come by two routes (batch_rodrigues there, quaternion -> rot6d -> Gram-Schmidt here): the project's SMPL bar, 1e-5
    fit_joints = fit.last_fit["joints"].cpu().numpy().astype(np.float64)
    err = float(np.abs(mesh_rel - (fit_joints - fit_joints[:, :1])).max())
    # (2) the fit distance: with the pinning undone by the fit's own root (model root + camera), the mesh path's joints lie within
    # the issue's bound -- the ensemble's worst + 4 x its spread -- of the input joints
    cam = opt["cam"].cpu().numpy().astype(np.float64)                                       # [T, 1, 3]
    placed = mesh_rel[:, :22] + (fit_joints[:, :1] + cam)
    dist = float(np.linalg.norm(placed - fx["j3d"], axis=-1).max())
    bound = float(fx["dist_worst"]) + H.FACTOR * float(fx["dist_spread"])
    print(f"[smplify gpu] end to end: mesh path's root-relative joints against the fit's own: max-abs {err:.3e} (bound {smh.TOL:.0e}); worst "
          f"distance to the input joints {dist * 1e3:.2f} mm (bound {bound * 1e3:.2f} mm); stats {fit.last_stats}")
    assert err <= smh.TOL, err
    assert dist <= bound, dist
    again, _ = s2r.joints2smpl(num_frames=T, device_id=0, smpl_model_path=model_path, gmm_path=gmm_path, mean_params=H.mean_params(),
                               num_smplify_iters=4).joint2smpl(fx["j3d"], init_params=dict(pose=fit.last_fit["pose"], betas=opt["betas"],
                                                                                           cam=opt["cam"]))
    assert torch.isfinite(again).all()
