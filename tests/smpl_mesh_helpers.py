"""Shared scaffolding of the full-SMPL-pass tests (mdm_amd/smpl_mesh.py, csrc/smpl_mesh.h): the reference-pinned fixtures
(tests/golden/smpl_mesh_*.npz, tools/make_golden_smpl_mesh.py), an fp64 numpy restatement of the whole pass -- rotation front
ends, shape and pose blend, kinematic chain, linear blend skinning, selected and regressed joints, index maps, root, mask,
translation -- for shapes no fixture covers, and a seeded synthetic model at the real SMPL size."""
import glob
import json
import os

import numpy as np

from smpl_helpers import GOLDEN, SMPL_PARENTS, write_smpl_model

TOL = 1e-5                      # the project's SMPL bar: max-abs on O(1) coordinates
NUM_BETAS = 10
REP_FEATS = {"rot6d": 6, "rotvec": 3, "rotmat": 9, "rotquat": 4}
# model/smpl.py:11-84 restated as numbers (the fixtures carry the reference's own maps; test_host_smpl_mesh.py compares)
VIBE = [24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
        8, 5, 45, 46, 4, 7, 21, 19, 17, 16, 18, 20, 47, 48, 49, 50, 51, 52, 53, 24, 26, 25, 28, 27]
A2M_OF_VIBE = [8, 1, 2, 3, 4, 5, 6, 7, 0, 9, 10, 11, 12, 13, 14, 21, 24, 38]
ROOT = {"a2m": 0, "smpl": 0, "a2mpl": 0, "vibe": 8}


def maps():
    vibe = np.array(VIBE)
    a2m = vibe[A2M_OF_VIBE]
    return {"vibe": vibe, "a2m": a2m, "smpl": np.arange(24), "a2mpl": np.unique(np.r_[np.arange(24), a2m])}


def fixture_names():
    return sorted(os.path.basename(p)[10:-4] for p in glob.glob(os.path.join(GOLDEN, "smpl_mesh_*.npz"))
                  if not p.endswith("smpl_mesh_model.npz"))


def load_fixture(name):
    """(npz, call) -- call: the keyword arguments of Rotation2xyz.__call__ apart from x, mask and betas."""
    g = np.load(os.path.join(GOLDEN, "smpl_mesh_" + name + ".npz"))
    return g, json.loads(str(g["call"]))


def fixture_model():
    """(fields, J_regressor_extra, selector ids, the reference's own index maps) of the model every fixture was made on."""
    g = np.load(os.path.join(GOLDEN, "smpl_mesh_model.npz"))
    fields = {k: g[k].astype(np.float64) for k in ("v_template", "J_regressor", "shapedirs", "posedirs", "weights")}
    fields["kintree_table"] = g["kintree_table"]
    ref_maps = {k[4:]: g[k] for k in g.files if k.startswith("map_")}
    return fields, g["J_regressor_extra"].astype(np.float64), [int(i) for i in g["vertex_joint_ids"]], ref_maps


def fixture_inputs(g):
    """(x, mask or None, betas or None) of a fixture, as numpy arrays."""
    return g["x"], (g["mask"] if bool(g["has_mask"]) else None), (g["betas"] if bool(g["has_betas"]) else None)


def write_model_files(root, fields, extra):
    """SMPL_NEUTRAL.pkl and J_regressor_extra.npy under <root>/body_models/smpl/; returns both paths."""
    path = write_smpl_model(root, fields)
    epath = os.path.join(os.path.dirname(path), "J_regressor_extra.npy")
    np.save(epath, extra)
    return path, epath


def synthetic_full_model(seed=0, V=6890, dense=True):
    """SMPL's fields with SMPL's tree at a chosen vertex count: v_template in [-0.9, 0.9], J_regressor rows summing to 1,
    shapedirs and posedirs ~ N(0, 0.01), dense skinning weights summing to 1; plus a [9, V] extra regressor (rows summing to 1)
    and 21 distinct selector vertex ids."""
    g = np.random.default_rng(seed)
    reg = g.random((24, V)) * (g.random((24, V)) < 0.05 if V > 200 else 1.0)
    reg[np.arange(24), g.integers(0, V, 24)] += 1.0
    reg /= reg.sum(1, keepdims=True)
    kin = np.array([[2 ** 32 - 1] + SMPL_PARENTS[1:], list(range(24))], dtype=np.int64)
    w = g.random((V, 24)) if dense else g.random((V, 24)) * (g.random((V, 24)) < 0.2) + 1e-3
    extra = g.random((9, V)) * (g.random((9, V)) < 0.05 if V > 200 else 1.0)
    extra[np.arange(9), g.integers(0, V, 9)] += 1.0
    extra /= extra.sum(1, keepdims=True)
    fields = dict(v_template=g.uniform(-0.9, 0.9, (V, 3)), J_regressor=reg, kintree_table=kin,
                  shapedirs=g.normal(0, 0.01, (V, 3, NUM_BETAS)), posedirs=g.normal(0, 0.01, (V, 3, 207)),
                  weights=w / w.sum(1, keepdims=True))
    ids = [int(i) for i in g.choice(V, 21, replace=False)]
    return fields, extra, ids


def make_x(B, T, pose_rep, glob, translation, seed):
    """A random input of the right layout, float32 [B, rows, feats, T]: rotmat rows are rotation matrices (orthonormalised rot6d),
    the others are what a sampler would emit (unnormalised)."""
    g = np.random.default_rng(seed)
    NR = 24 if glob else 23
    F = REP_FEATS[pose_rep]
    if pose_rep == "rotmat":
        d6 = g.normal(size=(B, T, NR, 6))
        rot = rotations_fp64(d6, "rot6d").reshape(B, T, NR, 9).transpose(0, 2, 3, 1)
    elif pose_rep == "rotvec":
        rot = g.normal(0, 0.8, size=(B, NR, F, T))
    else:
        rot = g.normal(size=(B, NR, F, T))
    x = rot
    if translation:
        tr = np.zeros((B, 1, F, T))
        tr[:, 0, :3] = g.normal(0, 0.5, size=(B, 3, T))
        x = np.concatenate([rot, tr], axis=1)
    return np.ascontiguousarray(x, dtype=np.float32)


def with_small_angles(x):
    """Rotvec rows of sample 0 on both sides of axis_angle_to_quaternion's small-angle branch (|angle| < 1e-6): exact zeros (a body
    joint and row 0), angles of 1e-7 and 9e-7 below it, 1.1e-6 and 3e-6 just above.  In place; returns x."""
    x[0, 0, :3, 2] = 0.0
    x[0, 2, :3, 1] = 0.0
    x[0, 5, :3, 3] = [6e-8, -8e-8, 0.0]
    x[0, 7, :3, 4] = [0.0, 9e-7, 0.0]
    x[0, 9, :3, 5] = [1.1e-6, 0.0, 0.0]
    x[0, 11, :3, 6] = [2e-6, -2e-6, 1e-6]
    return x


# ---- fp64 restatement -----------------------------------------------------------------------------------------------------------
def quat_to_matrix(q):
    r, i, j, k = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two_s = 2.0 / (q * q).sum(-1)
    o = np.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                  two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                  two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], axis=-1)
    return o.reshape(q.shape[:-1] + (3, 3))


def axis_angle_to_matrix(aa):
    angle = np.linalg.norm(aa, axis=-1, keepdims=True)
    half = 0.5 * angle
    small = np.abs(angle) < 1e-6
    safe = np.where(small, 1.0, angle)
    s = np.where(small, 0.5 - angle * angle / 48, np.sin(half) / safe)
    return quat_to_matrix(np.concatenate([np.cos(half), aa * s], axis=-1))


def rotations_fp64(xr, pose_rep):
    """utils/rotation_conversions.py in float64; xr [..., feats] -> [..., 3, 3]."""
    xr = np.asarray(xr, np.float64)
    if pose_rep == "rot6d":
        a1, a2 = xr[..., :3], xr[..., 3:]
        b1 = a1 / np.maximum(np.linalg.norm(a1, axis=-1, keepdims=True), 1e-12)
        b2 = a2 - (b1 * a2).sum(-1, keepdims=True) * b1
        b2 = b2 / np.maximum(np.linalg.norm(b2, axis=-1, keepdims=True), 1e-12)
        return np.stack([b1, b2, np.cross(b1, b2)], axis=-2)
    if pose_rep == "rotmat":
        return xr.reshape(xr.shape[:-1] + (3, 3))
    if pose_rep == "rotquat":
        return quat_to_matrix(xr)
    if pose_rep == "rotvec":
        return axis_angle_to_matrix(xr)
    raise NotImplementedError(pose_rep)


def lbs_fp64(fields, betas, rot, chunk=128):
    """smplx lbs (pose2rot=False) in float64: betas [N, 10], rot [N, 24, 3, 3] -> (vertices [N, V, 3], posed joints [N, 24, 3])."""
    v_t = np.asarray(fields["v_template"], np.float64)
    V = v_t.shape[0]
    sd = np.asarray(fields["shapedirs"], np.float64)[:, :, :NUM_BETAS].reshape(V * 3, NUM_BETAS)
    pd = np.asarray(fields["posedirs"], np.float64).reshape(V * 3, -1)
    reg = fields["J_regressor"]
    reg = np.asarray(reg.toarray() if hasattr(reg, "toarray") else reg, np.float64)
    W = np.asarray(fields["weights"], np.float64)
    parents = np.asarray(fields["kintree_table"][0]).astype(np.int64)
    parents[0] = -1
    N, J = rot.shape[0], rot.shape[1]
    verts = np.empty((N, V, 3))
    joints = np.empty((N, J, 3))
    for s in range(0, N, chunk):
        R, be = rot[s:s + chunk], betas[s:s + chunk]
        n = R.shape[0]
        v_shaped = v_t[None] + (be @ sd.T).reshape(n, V, 3)
        Jr = np.einsum("jv,nvc->njc", reg, v_shaped)
        pf = (R[:, 1:] - np.eye(3)).reshape(n, -1)
        v_posed = v_shaped + (pf @ pd.T).reshape(n, V, 3)
        GR, Gt = [R[:, 0]], [Jr[:, 0]]
        for i in range(1, J):
            p = parents[i]
            GR.append(GR[p] @ R[:, i])
            Gt.append(np.einsum("nrk,nk->nr", GR[p], Jr[:, i] - Jr[:, p]) + Gt[p])
        GR, Gt = np.stack(GR, 1), np.stack(Gt, 1)                                  # [n, J, 3, 3], [n, J, 3]
        A = np.concatenate([GR, (Gt - np.einsum("njrk,njk->njr", GR, Jr))[..., None]], axis=-1)     # [n, J, 3, 4]
        Tm = (W @ A.reshape(n, J, 12)).reshape(n, V, 3, 4)
        verts[s:s + n] = np.einsum("nvrc,nvc->nvr", Tm[..., :3], v_posed) + Tm[..., 3]
        joints[s:s + n] = Gt
    return verts, joints


def smpl_full_fp64(x, mask, fields, ids, extra, pose_rep, translation, glob, jointstype, vertstrans, betas=None, beta=0,
                   glob_rot=None, get_rotations_back=False):
    """model/rotation2xyz.py:17-92 over model/smpl.py:86-97 in float64.  x [B, rows, feats, T]; returns [B, points, 3, T] (and the
    rotations and global orient of the valid frames when asked)."""
    x = np.asarray(x, np.float64)
    B, T = x.shape[0], x.shape[-1]
    mask = np.ones((B, T), bool) if mask is None else np.asarray(mask, bool)
    if translation:
        x_tr, xr = x[:, -1, :3], x[:, :-1]
    else:
        xr = x
    xr = xr.transpose(0, 3, 1, 2)[mask]                                            # [n, rows, feats]
    rot = rotations_fp64(xr, pose_rep)
    n = rot.shape[0]
    if not glob:
        go = np.broadcast_to(axis_angle_to_matrix(np.asarray(glob_rot, np.float64)), (n, 1, 3, 3))
        body = rot
    else:
        go, body = rot[:, :1], rot[:, 1:]
    if betas is None:
        be = np.zeros((n, NUM_BETAS))
        be[:, 1] = beta
    else:
        be = np.broadcast_to(np.asarray(betas, np.float64), (n, NUM_BETAS))
    verts, joints = lbs_fp64(fields, be, np.concatenate([go, body], axis=1))
    if jointstype == "vertices":
        pts = verts
    else:
        allj = np.concatenate([joints, verts[:, list(ids)], np.einsum("ev,nvc->nec", np.asarray(extra, np.float64), verts)], axis=1)
        pts = allj[:, maps()[jointstype]]
    out = np.zeros((B, T, pts.shape[1], 3))
    out[mask] = pts
    out = out.transpose(0, 2, 3, 1)
    if jointstype != "vertices":
        out = out - out[:, [ROOT[jointstype]]]
    if translation and vertstrans:
        out = out + (x_tr - x_tr[:, :, :1])[:, None]
    if get_rotations_back:
        return out, body, (go[:, 0] if glob else go)
    return out
