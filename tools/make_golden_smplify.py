"""Fixture generator: tests/golden/smplify_*.npz and PIN_REPORT_smplify.json -- the REFERENCE's own SMPLify code
(visualize/joints2smpl/src/smplify.py SMPLify3D and guess_init_3d, customloss.py body_fitting_loss_3d and camera_fitting_loss_3d,
prior.py MaxMixturePrior, imported unmodified from the reference checkout) on synthetic inputs: SMPL's 24-joint tree on the
48-vertex model of tools/make_golden_smpl.py, a random 8 x 69 mixture written as gmm_08.pkl into a temporary directory, targets made
from random poses and betas plus a translation and 5 mm of noise (tests/smplify_helpers.py states all three).

`smplx` is replaced in sys.modules by a stand-in whose model object returns `.joints` from a differentiable torch RESTATEMENT of smplx
0.1.28 (SMPL.forward's joint regression, lbs.batch_rodrigues, lbs.batch_rigid_transform): the fixtures pin the reference's SMPLify
code, not a run of smplx itself, and the pin report says so.  The reference hard-codes its step() counts (10 and num_iters); the short
horizon runs it with fewer through the `range` its module looks up, nothing of its text changed.

    smplify_prior.npz          MaxMixturePrior's float32 buffers on the synthetic mixture
    smplify_value_grad.npz     65 frames of inputs; the reference's float32 per-frame losses, totals and autograd gradients
    smplify_linesearch.npz     (t, f, g.d) sequences of torch's own _strong_wolfe on one-dimensional objectives, float64 and float32 tensors
    smplify_fit_short_T*.npz   stage1_calls = stage2_calls = 1, num_iters = 4: the reference's pose, betas, camera; nine runs
    smplify_fit_full_T*.npz    num_iters = 150: final loss, worst joint-to-target distance, evaluations; nine runs
    PIN_REPORT_smplify.json    e_ref of every yardstick (tests/smplify_helpers.py)

    MDM_REFERENCE_ROOT=<reference checkout> python tools/make_golden_smplify.py [out_dir]
"""
import builtins
import json
import math
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_smpl as base                      # noqa: E402
import smplify_helpers as H                          # noqa: E402

NOTE = dict(smplx="restated (smplx 0.1.28 SMPL.forward's joints, lbs.batch_rodrigues, lbs.batch_rigid_transform), not a run of smplx",
            smpl_model="synthetic: SMPL's 24-joint tree, %d vertices (tests/golden/smpl_mesh_model.npz)" % base.NUM_VERTS,
            prior="synthetic 8 x 69 mixture, SPD covariances with eigenvalues in [0.01, 0.5] (tests/smplify_helpers.synthetic_gmm)",
            step_calls="the short horizon limits the reference's step() loops through the `range` its module looks up")
TWINS = (1, -1, 2, -2, 3, -3, 4, -4)


class StandInSMPL(nn.Module):
    """What SMPLify3D needs of an smplx SMPL model: called with axis-angle global_orient / body_pose and betas, it returns `.joints`
    (the 24 posed joints) and a placeholder `.vertices`; `faces_tensor` exists.  float32, differentiable."""

    def __init__(self, fields):
        super().__init__()
        f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)       # noqa: E731
        self.register_buffer("v_template", f32(fields["v_template"]))
        self.register_buffer("shapedirs", f32(fields["shapedirs"][:, :, :10]))
        self.register_buffer("J_regressor", f32(fields["J_regressor"]))
        parents = torch.tensor(np.asarray(fields["kintree_table"][0]).astype(np.int64))
        parents[0] = -1
        self.register_buffer("parents", parents)
        self.faces_tensor = torch.zeros(1, 3, dtype=torch.long)
        self.calls = 0

    def forward(self, global_orient=None, body_pose=None, betas=None, **kwargs):
        self.calls += 1
        T = betas.shape[0]
        v_shaped = self.v_template + base.blend_shapes(betas, self.shapedirs)
        J = base.vertices2joints(self.J_regressor, v_shaped)
        full_pose = torch.cat([global_orient, body_pose], dim=1)
        rot_mats = H.batch_rodrigues(full_pose.view(-1, 3)).view(T, -1, 3, 3)
        joints, _ = base.batch_rigid_transform(rot_mats, J, self.parents)
        return types.SimpleNamespace(joints=joints, vertices=torch.zeros(T, 1, 3))


def install(tmp):
    sys.dont_write_bytecode = True
    if base.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, base.REFERENCE_ROOT)
    sys.modules["smplx"] = types.ModuleType("smplx")
    from visualize.joints2smpl.src import config, smplify          # the reference's own modules
    config.GMM_MODEL_DIR = tmp
    return smplify


def value_grad_fixture(ref, model, prior, out_dir, report):
    inp = H.value_grad_inputs()
    tab = H.tables64(H.model_fields())
    pr = dict(means=prior.means.numpy().astype(np.float64), prec=prior.precisions.numpy().astype(np.float64),
              nlw=-np.log(prior.nll_weights.numpy().astype(np.float64).reshape(8)))
    winners, margin = H.check_input_conditions(inp, pr)
    t32 = lambda k, grad=False: torch.tensor(inp[k], requires_grad=grad)       # noqa: E731
    arrays = dict(inp)
    report["value_grad"] = dict(winning_components=winners, smallest_margin=margin)
    # step 1
    go, cam = t32("go", True), torch.tensor(inp["cam"][:, None], requires_grad=True)
    body, betas, j3d = t32("body"), t32("betas"), t32("j3d")
    cam_est = torch.tensor(inp["cam_est"][:, None])
    mj = model(global_orient=go, body_pose=body, betas=betas).joints
    total = ref.camera_fitting_loss_3d(mj, cam, cam_est, j3d, "AMASS")
    total.backward()
    frames = np.array([float(ref.camera_fitting_loss_3d(mj[f:f + 1], cam[f:f + 1], cam_est[f:f + 1], j3d[f:f + 1], "AMASS")) for f in range(H.NF)],
                      np.float32)
    g = torch.cat([go.grad.reshape(-1), cam.grad.reshape(-1)]).numpy()
    with torch.no_grad():      # guess_init_3d on the same joints: the start of a fit
        arrays["s1_guess"] = ref.guess_init_3d(mj, j3d, "AMASS").numpy()
    arrays.update(s1_frames=frames, s1_grad=g, s1_total=np.float32(float(total)))
    f64, g64, _ = H.oracle(1, inp, None, H.NF, tab, pr)
    ev, eg = H.errors_against_oracle(1, frames, H.per_frame_grad(1, g, H.NF), f64, H.per_frame_grad(1, g64, H.NF))
    for kind in ("ones", "foot"):
        report["value_grad"]["stage1_" + kind] = dict(value=ev, grad=eg)
    # step 2, both confidence vectors
    for kind in ("ones", "foot"):
        conf = torch.tensor(H.conf_of(kind))
        body, betas, go = t32("body", True), t32("betas", True), t32("go", True)
        cam = torch.tensor(inp["cam"][:, None], requires_grad=True)
        preserve = t32("preserve")
        mj = model(global_orient=go, body_pose=body, betas=betas).joints[:, :22]
        kw = dict(joints3d_conf=conf, joint_loss_weight=600.0, pose_preserve_weight=5.0, use_collision=False)
        total = ref.body_fitting_loss_3d(body, preserve, betas, mj, cam, j3d, prior, **kw)
        total.backward()
        frames = np.array([float(ref.body_fitting_loss_3d(body[f:f + 1], preserve[f:f + 1], betas[f:f + 1], mj[f:f + 1], cam[f:f + 1],
                                                          j3d[f:f + 1], prior, **kw)) for f in range(H.NF)], np.float32)
        g = torch.cat([body.grad.reshape(-1), betas.grad.reshape(-1), go.grad.reshape(-1), cam.grad.reshape(-1)]).numpy()
        arrays.update({"s2_%s_frames" % kind: frames, "s2_%s_grad" % kind: g, "s2_%s_total" % kind: np.float32(float(total))})
        f64, g64, _ = H.oracle(2, inp, H.conf_of(kind), H.NF, tab, pr)
        ev, eg = H.errors_against_oracle(2, frames, H.per_frame_grad(2, g, H.NF), f64, H.per_frame_grad(2, g64, H.NF))
        report["value_grad"]["stage2_" + kind] = dict(value=ev, grad=eg)
    np.savez_compressed(os.path.join(out_dir, "smplify_value_grad.npz"), meta=json.dumps(NOTE), **arrays)
    print("value_grad", report["value_grad"])


def linesearch_fixture(out_dir, report):
    """torch's own _strong_wolfe on one-dimensional float64 objectives phi(t) along d = [1]: the steps it asks for, in order."""
    from torch.optim.lbfgs import _strong_wolfe
    cases = {   # name: (phi, dphi, t0, max_ls)
        "quadratic_overshoot": (lambda t: (t - 0.3) ** 2, lambda t: 2 * (t - 0.3), 1.0, 25),
        "quartic_bracket": (lambda t: -t + 5 * t ** 4, lambda t: -1 + 20 * t ** 3, 1.0, 25),
        "wiggle": (lambda t: -t + 0.3 * math.sin(8 * t) + 0.5 * t * t, lambda t: -1 + 2.4 * math.cos(8 * t) + t, 0.9, 25),
        "extrapolate": (lambda t: -math.log1p(t) + 0.01 * t * t, lambda t: -1 / (1 + t) + 0.02 * t, 1e-3, 25),
        "extrapolate_cut": (lambda t: -math.log1p(t) + 0.01 * t * t, lambda t: -1 / (1 + t) + 0.02 * t, 1e-3, 3),
        "flat_bottom": (lambda t: (t - 0.5) ** 4 - 0.0625, lambda t: 4 * (t - 0.5) ** 3, 2.0, 25),
        "steep_wall": (lambda t: -t + math.exp(20 * (t - 0.4)) - math.exp(-8.0), lambda t: -1 + 20 * math.exp(20 * (t - 0.4)), 0.5, 25),
        "accept_first": (lambda t: (t - 1.0) ** 2, lambda t: 2 * (t - 1.0), 1.0, 25),
    }
    names, rows = [], []
    # float64 tensors: every scalar of the search is a double.  float32 tensors: g . d and max|d| are 0-dim float32 tensors as in a
    # fit (f and the first step stay Python floats), and what torch derives from them is rounded to float
    for dtype, suffix in ((torch.float64, ""), (torch.float32, "_f32")):
        for name, (phi, dphi, t0, max_ls) in cases.items():
            log = []

            def obj(x, t, d):
                tt = float(t)
                g = torch.tensor([dphi(tt)], dtype=dtype)
                log.append((tt, phi(tt), float(g.dot(d))))
                return phi(tt), g
            d = torch.ones(1, dtype=dtype)
            g0 = torch.tensor([dphi(0.0)], dtype=dtype)
            f_new, _g, t, n = _strong_wolfe(obj, [torch.zeros(1, dtype=dtype)], t0, d, phi(0.0), g0, g0.dot(d), max_ls=max_ls)
            assert n == len(log)
            row = np.full((3, 32), np.nan)
            row[:, :n] = np.array(log).T
            names.append(name + suffix)
            rows.append(dict(seq=row, head=np.array([t0, phi(0.0), float(g0.dot(d)), float(max_ls), float(n), float(t), float(f_new),
                                                     float(dtype == torch.float32)])))
            print("linesearch", name + suffix, n, float(t))
    np.savez_compressed(os.path.join(out_dir, "smplify_linesearch.npz"), names=np.array(names), seq=np.stack([r["seq"] for r in rows]),
                        head=np.stack([r["head"] for r in rows]),
                        meta=json.dumps(dict(source="torch.optim.lbfgs._strong_wolfe of torch " + torch.__version__ + ", float64 and (names ending in _f32) float32 tensors",
                                             head="t0, f0, gtd0, max_ls, evaluations, final t, final f, float32 tensors; d = [1], tolerance_change 1e-9")))
    report["linesearch"] = dict(cases=names, evaluations=[int(r["head"][4]) for r in rows])


def run_reference(ref, fields, j3d, num_iters, calls=None):
    """SMPLify3D.__call__ as joints2smpl.joint2smpl drives it; `calls` = (step-1, step-2) step() counts, None: the reference's own."""
    T = j3d.shape[0]
    model = StandInSMPL(fields)
    fit = ref.SMPLify3D(smplxmodel=model, batch_size=T, joints_category="AMASS", num_iters=num_iters, device=torch.device("cpu"))
    pose0, shape0 = H.mean_params()
    init_pose = torch.from_numpy(pose0).unsqueeze(0).repeat(T, 1)
    init_betas = torch.from_numpy(shape0).unsqueeze(0).repeat(T, 1)
    if calls is not None:
        left = list(calls)
        ref.range = lambda n: builtins.range(left.pop(0))
    try:
        _v, joints, pose, betas, cam, loss = fit(init_pose, init_betas, torch.zeros(1, 3), torch.from_numpy(j3d), conf_3d=torch.ones(22))
    finally:
        if calls is not None:
            del ref.range
    dist = float(torch.linalg.norm(joints[:, :22] + cam.detach() - torch.from_numpy(j3d), dim=-1).max())
    return dict(pose=pose.numpy().astype(np.float64), betas=betas.numpy().astype(np.float64), cam=cam.detach().numpy().reshape(T, 3).astype(np.float64),
                joints=joints.numpy(), loss=float(loss), evals=model.calls - 2, dist=dist)


def twins_of(j3d):
    return [j3d] + [(j3d * np.float32(1.0 + k * 2.0 ** -23)).astype(np.float32) for k in TWINS]


def short_fixture(ref, fields, T, out_dir, report):
    j3d = H.fit_targets(T, seed=100 + T)
    runs = [run_reference(ref, fields, t, 4, calls=(1, 1)) for t in twins_of(j3d)]
    e = {k: max(float(np.abs(r[k] - runs[0][k]).max()) for r in runs[1:]) for k in ("pose", "betas", "cam")}
    assert all(v > 0 for v in e.values()), e
    np.savez_compressed(os.path.join(out_dir, "smplify_fit_short_T%d.npz" % T), j3d=j3d, pose=runs[0]["pose"], betas=runs[0]["betas"],
                        cam=runs[0]["cam"], final_loss=runs[0]["loss"], ref_evals=runs[0]["evals"], meta=json.dumps(NOTE),
                        **{"e_ref_" + k: v for k, v in e.items()})
    report["fit_short_T%d" % T] = dict(e_ref=e, evals=[r["evals"] for r in runs], final_loss=runs[0]["loss"])
    print("fit_short", T, report["fit_short_T%d" % T])


def full_fixture(ref, fields, T, out_dir, report):
    for seed in range(200 + T, 260 + T):
        j3d = H.fit_targets(T, seed=seed)
        runs = [run_reference(ref, fields, t, 150) for t in twins_of(j3d)]
        losses = np.array([r["loss"] for r in runs])
        spread = float((losses.max() - losses.min()) / losses.min())
        print("fit_full", T, "seed", seed, "losses", losses, "spread", spread, "evals", [r["evals"] for r in runs])
        if spread < 1e-3:
            break
    else:
        raise AssertionError("no seed with an ensemble spread below 1e-3")
    dists = np.array([r["dist"] for r in runs])
    np.savez_compressed(os.path.join(out_dir, "smplify_fit_full_T%d.npz" % T), j3d=j3d, final_loss=runs[0]["loss"], loss_spread=spread,
                        dist_worst=float(dists.max()), dist_spread=float(dists.max() - dists.min()), ref_evals_min=min(r["evals"] for r in runs),
                        ref_evals_max=max(r["evals"] for r in runs), pose=runs[0]["pose"], betas=runs[0]["betas"], cam=runs[0]["cam"],
                        meta=json.dumps(NOTE))
    report["fit_full_T%d" % T] = dict(seed=seed, losses=losses.tolist(), loss_spread=spread, dists=dists.tolist(),
                                      evals=[r["evals"] for r in runs])


def main(out_dir):
    torch.set_num_threads(1)
    fields = H.model_fields()
    report = dict(note=NOTE, factor=H.FACTOR)
    with tempfile.TemporaryDirectory() as tmp:
        H.write_gmm(tmp)
        ref = install(tmp)
        prior = ref.MaxMixturePrior(prior_folder=tmp, num_gaussians=8, dtype=torch.float32)
        np.savez_compressed(os.path.join(out_dir, "smplify_prior.npz"), means=prior.means.numpy(), precisions=prior.precisions.numpy(),
                            nll_weights=prior.nll_weights.numpy(), gmm_seed=H.GMM_SEED, meta=json.dumps(NOTE))
        value_grad_fixture(ref, StandInSMPL(fields), prior, out_dir, report)
        linesearch_fixture(out_dir, report)
        for T in (3, H.F + 1):
            short_fixture(ref, fields, T, out_dir, report)
        for T in (3, 8):
            full_fixture(ref, fields, T, out_dir, report)
    with open(os.path.join(out_dir, "PIN_REPORT_smplify.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    return report


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden"))
