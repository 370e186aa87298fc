"""Fixture generator: tests/golden/smpl_mesh_*.npz -- the REFERENCE's own full SMPL transform (model/rotation2xyz.py,
model/smpl.py, utils/rotation_conversions.py, imported unmodified from the reference checkout through tools/make_golden_smpl.py's
`_install`) on that tool's 48-vertex synthetic SMPL model, over every jointstype, every pose_rep, glob=False, translation=False,
vertstrans=False, beta, betas and get_rotations_back.

As there, `smplx` is a RESTATEMENT (smplx 0.1.28 SMPLLayer.forward / lbs / batch_rigid_transform), not a run of smplx; its
vertex-joint selector is the first 21 synthetic vertices.  Every file's metadata says so.

    smpl_mesh_model.npz        the model (float32-exact fields), the selector ids, J_regressor_extra, the reference's index maps
    smpl_mesh_<case>.npz       x, mask, betas, the call's arguments, the reference's output (and rotations, when asked back)
    PIN_REPORT_smpl_mesh.json  per case: max-abs of the reference's float32 output against the float64 restatement of
                               tests/smpl_mesh_helpers.py, and the output's magnitude.  The generator refuses a case on which the
                               reference alone is off by more than 5e-6: the tests hold this project to 1e-5.

    MDM_REFERENCE_ROOT=<reference checkout> python tools/make_golden_smpl_mesh.py [out_dir]
"""
import json
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_smpl as base                      # noqa: E402
import smpl_mesh_helpers as H                        # noqa: E402

REF_BOUND = 5e-6
SEL_IDS = list(range(21))
DEFAULT = dict(pose_rep="rot6d", translation=True, glob=True, jointstype="vertices", vertstrans=True, beta=0, glob_rot=None,
               get_rotations_back=False)
# name: (B, T, x seed, lengths or None (no mask) or "full", samples whose first frame is masked, betas: None / "frames" / "one", call)
CASES = {
    "vertices_rot6d_B2_T60": (2, 60, 11, [60, 23], [1], None, {}),                                   # vis_utils.py:33-40's call
    "vertices_rot6d_B1_T196": (1, 196, 12, "full", [], None, {}),
    "smpl_rotvec_B2_T60": (2, 60, 13, [41, 60], [0], None, dict(pose_rep="rotvec", jointstype="smpl")),
    "a2m_rot6d_B2_T60": (2, 60, 14, [60, 37], [1], None, dict(jointstype="a2m")),                    # a2m models.py:85-113's call
    "a2mpl_rotmat_B2_T60": (2, 60, 15, [17, 60], [], None, dict(pose_rep="rotmat", jointstype="a2mpl")),
    "vibe_rotquat_B2_T60": (2, 60, 16, None, [], None, dict(pose_rep="rotquat", jointstype="vibe")),
    "vertices_globfalse_back_B2_T60": (2, 60, 17, [60, 30], [1], None, dict(glob=False, glob_rot=[0.3, -0.2, 0.1],
                                                                            get_rotations_back=True)),
    "a2m_notranslation_B2_T60": (2, 60, 18, [55, 60], [0], None, dict(jointstype="a2m", translation=False)),
    "vibe_novertstrans_B2_T60": (2, 60, 19, [60, 12], [], None, dict(jointstype="vibe", vertstrans=False)),
    "vertices_beta_B2_T60": (2, 60, 20, [60, 44], [1], None, dict(beta=1.5)),
    "smpl_rotquat_betas_frames_back_B2_T60": (2, 60, 21, [33, 60], [0], "frames", dict(pose_rep="rotquat", jointstype="smpl",
                                                                                       get_rotations_back=True)),
    "a2m_betas_one_B1_T196": (1, 196, 22, [150], [0], "one", dict(jointstype="a2m")),
    # both sides of axis_angle_to_quaternion's small-angle branch (smpl_mesh_helpers.with_small_angles), and a glob_rot of zeros
    "vertices_rotvec_smallangle_globzero_back_B2_T60": (2, 60, 23, [60, 40], [1], None, dict(
        pose_rep="rotvec", glob=False, glob_rot=[0.0, 0.0, 0.0], get_rotations_back=True, _small_angles=True)),
}


def f32_exact(model):
    """Round every float field to float32 (kept as float64): the reference loads the pickle into float32 tensors anyway, and the
    shared fixture file then stores the fields in half the space without losing a bit."""
    return {k: (np.asarray(v, np.float32).astype(np.float64) if np.asarray(v).dtype.kind == "f" else v) for k, v in model.items()}


def main(out_dir):
    model = f32_exact(base.synthetic_smpl(seed=0))
    g = np.random.default_rng(1)
    extra = g.random((9, base.NUM_VERTS))
    extra = (extra / extra.sum(1, keepdims=True)).astype(np.float32).astype(np.float64)
    note = dict(smplx="restated (smplx 0.1.28 SMPLLayer.forward / lbs / batch_rigid_transform), not a pinned run of smplx; its "
                      "VertexJointSelector is the first 21 synthetic vertices",
                smpl_model="synthetic: SMPL's 24-joint tree, %d vertices, dense J_regressor and weights" % base.NUM_VERTS)
    report = {}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "SMPL_NEUTRAL.pkl"), "wb") as f:
            pickle.dump(model, f, protocol=2)
        np.save(os.path.join(tmp, "J_regressor_extra.npy"), extra)
        Rotation2xyz = base._install(tmp)
        r2x = Rotation2xyz(device="cpu", dataset="humanact12")
        ref_maps = {k: np.asarray(v) for k, v in r2x.smpl_model.maps.items()}
        np.savez_compressed(os.path.join(out_dir, "smpl_mesh_model.npz"),
                            **{k: np.asarray(model[k], np.float32) for k in ("v_template", "J_regressor", "shapedirs", "posedirs", "weights")},
                            kintree_table=model["kintree_table"], vertex_joint_ids=np.array(SEL_IDS), J_regressor_extra=extra.astype(np.float32),
                            **{"map_" + k: v for k, v in ref_maps.items()}, meta=json.dumps(note))
        for name, (B, T, seed, lengths, first_masked, betas_kind, over) in CASES.items():
            call = dict(DEFAULT, **over)
            small = call.pop("_small_angles", False)
            xn = H.make_x(B, T, call["pose_rep"], call["glob"], call["translation"], seed)
            x = torch.from_numpy(H.with_small_angles(xn) if small else xn)
            if lengths is None:
                mask = None
            elif lengths == "full":
                mask = torch.ones(B, T, dtype=torch.bool)
            else:
                mask = base.ragged_mask(B, T, lengths, first_masked)
            n_valid = B * T if mask is None else int(mask.sum())
            bg = np.random.default_rng(seed + 100)
            betas = None if betas_kind is None else torch.from_numpy(
                bg.normal(0, 1.0, (n_valid if betas_kind == "frames" else 1, 10)).astype(np.float32))
            # a [1, 10] betas is the fixture's INPUT; the restated SMPLLayer (like lbs itself) does not broadcast it over the frames,
            # so the reference is handed the same row once per valid frame
            ref_betas = betas.expand(n_valid, 10).contiguous() if betas_kind == "one" else betas
            with torch.no_grad():
                got = r2x(x=x, mask=mask, betas=ref_betas, **call)
            want = H.smpl_full_fp64(x.numpy(), None if mask is None else mask.numpy(), model, SEL_IDS, extra,
                                    betas=None if betas is None else betas.numpy(), **call)
            arrays = dict(x=x.numpy(), mask=(mask.numpy() if mask is not None else np.zeros(0, bool)), has_mask=mask is not None,
                          betas=(betas.numpy() if betas is not None else np.zeros(0, np.float32)), has_betas=betas is not None,
                          call=json.dumps(call), meta=json.dumps(dict(note, call="model/rotation2xyz.py Rotation2xyz.__call__",
                                                         betas=("the stored [1, 10] row was handed to the reference once per valid frame"
                                                                if betas_kind == "one" else "as stored"))))
            if call["get_rotations_back"]:
                out, rotations, global_orient = got
                w_out, w_rot, w_go = want
                arrays.update(rotations=rotations.numpy(), global_orient=global_orient.numpy())
                rot_err = max(float(np.abs(rotations.numpy() - w_rot).max()), float(np.abs(global_orient.numpy() - w_go).max()))
            else:
                out, w_out, rot_err = got, want, 0.0
            assert out.dtype == torch.float32 and torch.isfinite(out).all() and out.shape == w_out.shape, name
            err = float(np.abs(out.numpy().astype(np.float64) - w_out).max())
            report[name] = dict(B=B, T=T, points=int(out.shape[1]), absmax=float(out.abs().max()), reference_fp32_vs_fp64=err,
                                reference_rotations_fp32_vs_fp64=rot_err, bound=REF_BOUND)
            print(name, report[name])
            assert err <= REF_BOUND and rot_err <= REF_BOUND, (name, err, rot_err)
            arrays["out"] = out.numpy()
            path = os.path.join(out_dir, "smpl_mesh_" + name + ".npz")
            np.savez_compressed(path, **arrays)
            assert os.path.getsize(path) <= 300 * 1024, (name, os.path.getsize(path))
    with open(os.path.join(out_dir, "PIN_REPORT_smpl_mesh.json"), "w") as f:
        json.dump(dict(note=note, bound=REF_BOUND, cases=report), f, indent=1, sort_keys=True)
        f.write("\n")
    return report


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden"))
