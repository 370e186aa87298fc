"""Shared scaffolding of the SMPL-joints tests (mdm_amd/rotation2xyz.py, csrc/smpl_joints.h): the reference-pinned fixtures
(tests/golden/smpl_joints_*.npz, tools/make_golden_smpl.py), a synthetic SMPL model file where the reference looks for it,
and an fp64 restatement of the transform."""
import glob
import os
import pickle

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMPL_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
# the arguments of every reference caller (sample/generate.py:167-171, sample/predict.py:134-138, eval/a2m/stgcn_eval.py:55,
# eval/a2m/gru_eval.py:39), apart from x and mask
CALLER_KW = dict(pose_rep="rot6d", glob=True, translation=True, jointstype="smpl", vertstrans=True, betas=None, beta=0,
                 glob_rot=None, get_rotations_back=False)


def fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "smpl_joints_*.npz")))


def load_fixture(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    mask = g["mask"] if bool(g["has_mask"]) else None
    return g, mask


def synthetic_model(seed=0, V=40):
    """SMPL's fields with SMPL's tree (the official kintree_table stores 2**32 - 1 for the root's parent)."""
    g = np.random.default_rng(seed)
    reg = g.random((24, V))
    reg /= reg.sum(1, keepdims=True)
    kin = np.array([[2 ** 32 - 1] + SMPL_PARENTS[1:], list(range(24))], dtype=np.int64)
    return dict(v_template=g.uniform(-0.9, 0.9, (V, 3)), J_regressor=reg, kintree_table=kin,
                shapedirs=g.normal(0, 0.01, (V, 3, 10)), weights=np.full((V, 24), 1 / 24))


def write_smpl_model(root, fields):
    """<root>/body_models/smpl/SMPL_NEUTRAL.pkl: the path the reference reads relative to its working directory."""
    d = os.path.join(str(root), "body_models", "smpl")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "SMPL_NEUTRAL.pkl")
    with open(path, "wb") as f:
        pickle.dump(fields, f, protocol=2)
    return path


def rest_tables(fields):
    """(rest joints [24, 3] float64, parents [24]) exactly as the loader defines them."""
    reg = fields["J_regressor"]
    reg = reg.toarray() if hasattr(reg, "toarray") else np.asarray(reg)
    parents = np.asarray(fields["kintree_table"][0]).astype(np.int64)
    parents[0] = -1
    return reg.astype(np.float64) @ np.asarray(fields["v_template"], np.float64), parents


def smpl_joints_fp64(x, mask, rest, parents):
    """fp64 restatement of model/rotation2xyz.py (rot6d, glob, translation, jointstype='smpl', vertstrans, beta=0):
    rotation_6d_to_matrix (utils/rotation_conversions.py:528-534) -> smplx batch_rigid_transform's chain -> posed joints minus
    the posed root (0 on masked frames) -> plus translation_t - translation_0.  x [B, J+1, 6, T], mask [B, T] bool or None."""
    x = np.asarray(x, np.float64)
    B, NJ, _, T = x.shape
    J = NJ - 1
    rest = np.asarray(rest, np.float64)
    rot = x[:, :J].transpose(0, 3, 1, 2)                                     # [B, T, J, 6]
    a1, a2 = rot[..., :3], rot[..., 3:]
    b1 = a1 / np.maximum(np.linalg.norm(a1, axis=-1, keepdims=True), 1e-12)
    b2 = a2 - (b1 * a2).sum(-1, keepdims=True) * b1
    b2 = b2 / np.maximum(np.linalg.norm(b2, axis=-1, keepdims=True), 1e-12)
    R = np.stack([b1, b2, np.cross(b1, b2)], axis=-2)                        # rows b1, b2, b3
    rel = rest.copy()
    rel[1:] -= rest[parents[1:]]
    GR, Gt = [R[:, :, 0]], [np.broadcast_to(rel[0], (B, T, 3))]
    for i in range(1, J):
        p = parents[i]
        GR.append(GR[p] @ R[:, :, i])
        Gt.append(np.einsum("btrk,k->btr", GR[p], rel[i]) + Gt[p])
    pos = np.stack(Gt, axis=2)                                               # [B, T, J, 3]
    pos = pos - pos[:, :, :1]
    if mask is not None:
        pos[~np.asarray(mask, bool)] = 0.0
    tr = x[:, J, :3, :]                                                      # [B, 3, T]
    return pos.transpose(0, 2, 3, 1) + (tr - tr[:, :, :1])[:, None]
