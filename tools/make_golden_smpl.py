"""Fixture generator: tests/golden/smpl_joints_*.npz -- the REFERENCE's own SMPL transform (model/rotation2xyz.py, model/smpl.py,
utils/rotation_conversions.py, imported unmodified from the reference checkout) on a small synthetic SMPL model with SMPL's real
24-joint kinematic tree, called with the arguments of sample/generate.py:167-171 / eval/a2m/stgcn_eval.py:55.

What is NOT on a build machine is replaced in sys.modules:
  * `smplx` (SMPLLayer, lbs.vertices2joints): a RESTATEMENT of smplx 0.1.28's SMPLLayer.forward -> lbs -> batch_rigid_transform
    below (pose2rot=False, transl=None).  The fixtures pin the reference's rotation2xyz / smpl.py / rotation_conversions code, not
    a run of smplx itself; the metadata of every file says so.  smplx's vertex-joint selector (21 extra joints picked by SMPL-H
    vertex ids) is stood in for by the first 21 synthetic vertices: those joints do not enter the 'smpl' output.
  * `clip`, as oracle/ref_harness.py does.
utils/config.py's SMPL paths are pointed at a temporary directory holding the synthetic SMPL_NEUTRAL.pkl and J_regressor_extra.npy.

    MDM_REFERENCE_ROOT=<reference checkout> python tools/make_golden_smpl.py [out_dir]
"""
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("MDM_REFERENCE_ROOT", "/root/reference")
# SMPL's kinematic tree (kintree_table[0] of the official model files; the root's entry is 2**32 - 1 there)
SMPL_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
NUM_VERTS = 48


def synthetic_smpl(seed=0, V=NUM_VERTS):
    """A few dozen vertices in SMPL's layout of fields: v_template [V, 3], J_regressor [24, V] (non-negative rows summing to 1),
    kintree_table [2, 24], shapedirs [V, 3, 10], posedirs [V, 3, 207], weights [V, 24], f."""
    g = np.random.default_rng(seed)
    reg = g.random((24, V)) * (g.random((24, V)) < 0.3)
    reg[np.arange(24), g.integers(0, V, 24)] += 1.0
    reg /= reg.sum(1, keepdims=True)
    kin = np.array([[2 ** 32 - 1] + SMPL_PARENTS[1:], list(range(24))], dtype=np.int64)
    w = g.random((V, 24))
    return dict(v_template=g.uniform(-0.9, 0.9, (V, 3)), J_regressor=reg, kintree_table=kin,
                shapedirs=g.normal(0, 0.01, (V, 3, 10)), posedirs=g.normal(0, 0.01, (V, 3, 207)),
                weights=w / w.sum(1, keepdims=True), f=g.integers(0, V, (2 * V, 3)).astype(np.int64))


# ---- restatement of smplx 0.1.28 (smplx/lbs.py, SMPLLayer.forward with pose2rot=False) ------------------------------------
def vertices2joints(J_regressor, vertices):
    return torch.einsum("bik,ji->bjk", [vertices, J_regressor])


def blend_shapes(betas, shape_disps):
    return torch.einsum("bl,mkl->bmk", [betas, shape_disps])


def transform_mat(R, t):
    return torch.cat([F.pad(R, [0, 0, 0, 1]), F.pad(t, [0, 0, 0, 1], value=1)], dim=2)


def batch_rigid_transform(rot_mats, joints, parents):
    joints = torch.unsqueeze(joints, dim=-1)
    rel_joints = joints.clone()
    rel_joints[:, 1:] -= joints[:, parents[1:]]
    transforms_mat = transform_mat(rot_mats.reshape(-1, 3, 3), rel_joints.reshape(-1, 3, 1)).reshape(-1, joints.shape[1], 4, 4)
    transform_chain = [transforms_mat[:, 0]]
    for i in range(1, parents.shape[0]):
        transform_chain.append(torch.matmul(transform_chain[parents[i]], transforms_mat[:, i]))
    transforms = torch.stack(transform_chain, dim=1)
    posed_joints = transforms[:, :, :3, 3]
    joints_homogen = F.pad(joints, [0, 0, 0, 1])
    rel_transforms = transforms - F.pad(torch.matmul(transforms, joints_homogen), [3, 0, 0, 0, 0, 0, 0, 0])
    return posed_joints, rel_transforms


def lbs(betas, pose, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights):
    batch_size = max(betas.shape[0], pose.shape[0])
    v_shaped = v_template + blend_shapes(betas, shapedirs)
    J = vertices2joints(J_regressor, v_shaped)
    ident = torch.eye(3, dtype=betas.dtype)
    pose_feature = pose[:, 1:].view(batch_size, -1, 3, 3) - ident
    rot_mats = pose.view(batch_size, -1, 3, 3)
    pose_offsets = torch.matmul(pose_feature.view(batch_size, -1), posedirs).view(batch_size, -1, 3)
    v_posed = pose_offsets + v_shaped
    J_transformed, A = batch_rigid_transform(rot_mats, J, parents)
    W = lbs_weights.unsqueeze(dim=0).expand([batch_size, -1, -1])
    T = torch.matmul(W, A.view(batch_size, J_regressor.shape[0], 16)).view(batch_size, -1, 4, 4)
    v_posed_homo = torch.cat([v_posed, torch.ones([batch_size, v_posed.shape[1], 1], dtype=betas.dtype)], dim=2)
    v_homo = torch.matmul(T, torch.unsqueeze(v_posed_homo, dim=-1))
    return v_homo[:, :, :3, 0], J_transformed


class SMPLLayer(nn.Module):
    NUM_BODY_JOINTS = 23

    def __init__(self, model_path=None, num_betas=10, **kwargs):
        super().__init__()
        with open(model_path, "rb") as f:
            d = pickle.load(f, encoding="latin1")
        self.num_betas = num_betas
        f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)   # noqa: E731
        self.register_buffer("v_template", f32(d["v_template"]))
        self.register_buffer("shapedirs", f32(d["shapedirs"][:, :, :num_betas]))
        self.register_buffer("J_regressor", f32(d["J_regressor"]))
        self.register_buffer("posedirs", f32(np.reshape(d["posedirs"], [-1, d["posedirs"].shape[-1]]).T))
        parents = torch.tensor(np.asarray(d["kintree_table"][0]), dtype=torch.long)
        parents[0] = -1
        self.register_buffer("parents", parents)
        self.register_buffer("lbs_weights", f32(d["weights"]))

    def forward(self, betas=None, body_pose=None, global_orient=None, transl=None, **kwargs):
        full_pose = torch.cat([global_orient.reshape(-1, 1, 3, 3), body_pose.reshape(-1, self.NUM_BODY_JOINTS, 3, 3)], dim=1)
        vertices, joints = lbs(betas, full_pose, self.v_template, self.shapedirs, self.posedirs, self.J_regressor, self.parents,
                               self.lbs_weights)
        joints = torch.cat([joints, vertices[:, :21]], dim=1)     # stand-in for smplx's VertexJointSelector (see above)
        return types.SimpleNamespace(vertices=vertices, joints=joints)


def _install(tmp):
    sys.dont_write_bytecode = True
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    smplx = types.ModuleType("smplx")
    smplx.SMPLLayer = SMPLLayer
    smplx_lbs = types.ModuleType("smplx.lbs")
    smplx_lbs.vertices2joints = vertices2joints
    smplx.lbs = smplx_lbs
    sys.modules["smplx"], sys.modules["smplx.lbs"] = smplx, smplx_lbs
    sys.modules.setdefault("clip", types.ModuleType("clip"))
    import utils.config as cfg                                   # reference utils/config.py
    cfg.SMPL_DATA_PATH = tmp
    cfg.SMPL_MODEL_PATH = os.path.join(tmp, "SMPL_NEUTRAL.pkl")
    cfg.JOINT_REGRESSOR_TRAIN_EXTRA = os.path.join(tmp, "J_regressor_extra.npy")
    from model.rotation2xyz import Rotation2xyz                  # reference model/rotation2xyz.py -> model/smpl.py
    return Rotation2xyz


def make_x(B, T, seed, specials=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 25, 6, T, generator=g)
    if specials:   # valid frames of sample 0: a 6D half of norm 0 and one below F.normalize's 1e-12 clamp
        x[0, 3, 0:3, 5] = 0.0
        x[0, 7, 3:6, 9] = 0.0
        x[0, 0, 0:6, 2] = 0.0
        x[0, 11, 0:3, 7] = torch.tensor([3e-13, -2e-13, 1e-13])
        x[0, 2, 3:6, 8] = torch.tensor([-4e-14, 5e-13, 2e-13])
    return x


def ragged_mask(B, T, lengths, first_masked=()):
    m = torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]
    for b in first_masked:
        m[b, 0] = False
    return m


CASES = {   # name: (B, T, x seed, mask or None, specials)
    "smpl_joints_full_B2_T60": (2, 60, 1, "full", True),
    "smpl_joints_ragged_B3_T60": (3, 60, 2, ([60, 23, 1], [2]), True),
    "smpl_joints_ragged_B2_T196": (2, 196, 3, ([196, 90], [1]), False),
    "smpl_joints_nomask_B1_T60": (1, 60, 4, None, False),
}


def main(out_dir):
    model = synthetic_smpl(seed=0)
    report = {}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "SMPL_NEUTRAL.pkl"), "wb") as f:
            pickle.dump(model, f, protocol=2)
        np.save(os.path.join(tmp, "J_regressor_extra.npy"), np.random.default_rng(1).random((9, NUM_VERTS)))
        Rotation2xyz = _install(tmp)
        r2x = Rotation2xyz(device="cpu", dataset="humanact12")
        for name, (B, T, seed, mk, specials) in CASES.items():
            x = make_x(B, T, seed, specials)
            if mk == "full":
                mask = torch.ones(B, T, dtype=torch.bool)
            elif mk is None:
                mask = None
            else:
                mask = ragged_mask(B, T, *mk)
            with torch.no_grad():                                  # generate.py:167-171
                out = r2x(x=x, mask=mask, pose_rep="rot6d", glob=True, translation=True, jointstype="smpl", vertstrans=True,
                          betas=None, beta=0, glob_rot=None, get_rotations_back=False)
            assert out.shape == (B, 24, 3, T) and torch.isfinite(out).all()
            meta = dict(call="model/rotation2xyz.py Rotation2xyz.__call__ with sample/generate.py:167-171's arguments",
                        smplx="restated (smplx 0.1.28 SMPLLayer.forward / lbs / batch_rigid_transform), not a pinned run of smplx",
                        smpl_model="synthetic: SMPL's 24-joint tree, %d vertices, dense J_regressor" % NUM_VERTS)
            np.savez_compressed(os.path.join(out_dir, name + ".npz"), x=x.numpy(), out=out.numpy(),
                                mask=(mask.numpy() if mask is not None else np.zeros(0, bool)), has_mask=mask is not None,
                                v_template=model["v_template"], J_regressor=model["J_regressor"],
                                kintree_table=model["kintree_table"], meta=json.dumps(meta))
            report[name] = dict(B=B, T=T, absmax=float(out.abs().max()))
            print(name, report[name])
    return report


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden"))
