"""`Rotation2xyzFull` -- the reference's whole SMPL transform (model/rotation2xyz.py over model/smpl.py and smplx's lbs) on the
MI355X HIP path: every `pose_rep`, every `jointstype` ('vertices', 'smpl', 'a2m', 'a2mpl', 'vibe'), `glob=False` with `glob_rot`,
`translation=False`, `vertstrans=False`, `beta`, `betas` and `get_rotations_back`.

`mdm_amd.rotation2xyz.Rotation2xyz` (what `model.rot2xyz` is) keeps refusing all of that; the two reference programs that need it
construct their own object and are pointed here instead:
    visualize/vis_utils.py:15-40      Rotation2xyz(device) ... jointstype='vertices'      (meshes of a generated motion)
    eval/a2m/action2motion/models.py  Rotation2xyz(device="cuda") ... jointstype='a2m'    (the recognition model's input)

One C-ABI call (mdm_smpl_forward, csrc/smpl_mesh.h): a pose kernel, then the skinning kernel -- shape blend, pose blend shapes and
linear blend skinning of the 6,890 vertices on exact-fp32 MFMAs, the blended vertices and per-vertex transforms never leaving
registers -- and, for the joints families, a fixed-order regression of the extra joints from the mesh.  No CPU fallback.  The case
`Rotation2xyz` supports is delegated to it unchanged (bit-identical).
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from .rotation2xyz import DOWNLOAD_SCRIPT, SMPL_MODEL_PATH, Rotation2xyz, _dense, _SmplUnpickler

EXTRA_REGRESSOR_PATH = os.path.join("./body_models/smpl", "J_regressor_extra.npy")    # utils/config.py:8
JOINTSTYPES = ("a2m", "a2mpl", "smpl", "vibe", "vertices")                            # model/rotation2xyz.py:8
JOINTSTYPE_ROOT = {"a2m": 0, "smpl": 0, "a2mpl": 0, "vibe": 8}                        # model/smpl.py:17-20
NUM_BETAS = 10

# The 21 vertices smplx's VertexJointSelector appends after the 24 skeleton joints of an SMPL model (smplx vertex_ids['smplh']):
# nose, reye, leye, rear, lear; LBigToe, LSmallToe, LHeel, RBigToe, RSmallToe, RHeel; then the left-hand and the right-hand thumb,
# index, middle, ring and pinky tips.  RESTATED FROM MEMORY: smplx is not a dependency of this package and the table could not be
# compared with an installed smplx when this was written.  Check it against smplx/vertex_ids.py before trusting 'a2m', 'a2mpl' or
# 'vibe' positions of the face, feet and finger tips on the real model, or pass `vertex_joint_ids=`.
SMPLH_VERTEX_JOINT_IDS = (332, 6260, 2800, 4071, 583,
                          3216, 3226, 3387, 6617, 6624, 6787,
                          2746, 2319, 2445, 2556, 2673,
                          6191, 5782, 5905, 6016, 6133)

# model/smpl.py:22-84: the position in smplx's joint list (24 skeleton joints, 21 selected vertices, 9 regressed joints) of each of
# the 49 'vibe' joints, in JOINT_NAMES order; 'a2m' picks 18 of them, 'a2mpl' is the sorted union of 'smpl' and 'a2m'.
VIBE_INDEXES = (24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
                8, 5, 45, 46, 4, 7, 21, 19, 17, 16, 18, 20, 47, 48, 49, 50, 51, 52, 53, 24, 26, 25, 28, 27)
ACTION2MOTION_JOINTS = (8, 1, 2, 3, 4, 5, 6, 7, 0, 9, 10, 11, 12, 13, 14, 21, 24, 38)


def joint_maps():
    """{jointstype: int array of positions in the extended joint list}, as SMPL.__init__ builds them (model/smpl.py:76-84)."""
    vibe = np.array(VIBE_INDEXES)
    a2m = vibe[list(ACTION2MOTION_JOINTS)]
    smpl = np.arange(24)
    return {"vibe": vibe, "a2m": a2m, "smpl": smpl, "a2mpl": np.unique(np.r_[smpl, a2m])}


def load_smpl_model(path=SMPL_MODEL_PATH):
    """The fields of an SMPL model file the full pass reads, as float64 arrays: v_template [V, 3], J_regressor [J, V], shapedirs
    [V, 3, 10] (the first 10 components), posedirs [V, 3, (J - 1) * 9], weights [V, J], and parents int32 [J]."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"SMPL model file {path} not found (relative to {os.getcwd()}): rot2xyz with pose_rep != 'xyz' "
                                f"needs SMPL_NEUTRAL.pkl, which the reference's {DOWNLOAD_SCRIPT} puts there")
    with open(path, "rb") as f:
        data = _SmplUnpickler(f, encoding="latin1").load()
    if not isinstance(data, dict):
        raise ValueError(f"{path}: expected a dict of SMPL model fields, got {type(data).__name__}")
    for k in ("v_template", "J_regressor", "kintree_table", "shapedirs", "posedirs", "weights"):
        if k not in data:
            raise ValueError(f"{path}: no {k!r} field")
    v = _dense("v_template", data["v_template"], path)
    reg = _dense("J_regressor", data["J_regressor"], path)
    sd = _dense("shapedirs", data["shapedirs"], path)
    pd = _dense("posedirs", data["posedirs"], path)
    w = _dense("weights", data["weights"], path)
    kin = np.asarray(data["kintree_table"])
    if v.ndim != 2 or v.shape[1] != 3 or reg.ndim != 2 or reg.shape[1] != v.shape[0] or kin.ndim != 2 or kin.shape[1] != reg.shape[0]:
        raise ValueError(f"{path}: inconsistent shapes v_template {v.shape}, J_regressor {reg.shape}, kintree_table {kin.shape}")
    V, J = v.shape[0], reg.shape[0]
    if sd.ndim != 3 or sd.shape[:2] != (V, 3) or sd.shape[2] < NUM_BETAS:
        raise ValueError(f"{path}: shapedirs {sd.shape} is not [{V}, 3, >= {NUM_BETAS}]")
    if pd.shape != (V, 3, (J - 1) * 9):
        raise ValueError(f"{path}: posedirs {pd.shape} is not [{V}, 3, {(J - 1) * 9}]")
    if w.shape != (V, J):
        raise ValueError(f"{path}: weights {w.shape} is not [{V}, {J}]")
    parents = kin[0].astype(np.int64)
    parents[0] = -1
    faces = np.asarray(data["f"]).astype(np.int64) if "f" in data and not hasattr(data["f"], "state") else None
    return dict(faces=faces, v_template=v, J_regressor=reg, shapedirs=np.ascontiguousarray(sd[:, :, :NUM_BETAS]), posedirs=pd, weights=w,
                parents=np.ascontiguousarray(parents.astype(np.int32)))


def _blend_table(v_template, shapedirs, posedirs, Vpad):
    """B' = [posedirs; shapedirs; v_template] transposed to [3][KP][Vpad] (include/mdm_hip.h mdm_smpl_model_t.blend)."""
    V, _, P = posedirs.shape
    K = P + NUM_BETAS + 1
    KP = (K + 3) & ~3
    t = np.zeros((3, KP, Vpad), np.float32)
    t[:, :P, :V] = posedirs.transpose(1, 2, 0)
    t[:, P:P + NUM_BETAS, :V] = shapedirs.transpose(1, 2, 0)
    t[:, P + NUM_BETAS, :V] = v_template.T
    return t


def _weights_table(weights, Vpad):
    V, J = weights.shape
    t = np.zeros((24, Vpad), np.float32)
    t[:J, :V] = weights.T
    return t


def _axis_angle_to_matrix(glob_rot):
    """geometry.axis_angle_to_matrix(torch.tensor(glob_rot)) of rotation2xyz.py:54-55, in the reference's float32 arithmetic."""
    aa = torch.as_tensor(glob_rot, dtype=torch.float32, device="cpu").reshape(3)
    angle = torch.norm(aa, p=2)
    half = 0.5 * angle
    s = 0.5 - (angle * angle) / 48 if float(angle.abs()) < 1e-6 else torch.sin(half) / angle
    r, (i, j, k) = torch.cos(half), aa * s
    two_s = 2.0 / (r * r + i * i + j * j + k * k)
    m = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)))
    return np.ascontiguousarray(m.numpy(), dtype=np.float32)


class _SmplModelView(nn.Module):
    """What callers reach through `rot2xyz.smpl_model`: a module without parameters or buffers (train/train_mdm.py:47 calls
    .eval() on it) whose `faces` are the model file's triangles (visualize/vis_utils.py:16 reads them before the first call)."""

    def __init__(self, owner):
        super().__init__()
        self._owner = [owner]          # (a list: not registered as a submodule or attribute of the module tree)

    @property
    def faces(self):
        f = self._owner[0].model()["faces"]
        if f is None:
            raise ValueError(f"{self._owner[0].model_path}: no 'f' field (the triangles)")
        return f


class Rotation2xyzFull(Rotation2xyz):
    """model/rotation2xyz.py:10-92 with the reference's call signature and every argument honoured.  The SMPL file is read at the
    first call that needs it, J_regressor_extra.npy at the first 'a2m' / 'a2mpl' / 'vibe' call; the prepared tables are uploaded
    once per device and cached on the object (plain tensors: `smpl_model` stays a module without parameters or buffers).
    A call without `betas` does not synchronise with the device and can be captured into a graph after a warm-up call; per-frame
    `betas` are checked against the mask's valid-frame count on the host and scattered with a boolean index: that call synchronises
    and cannot be captured (the C ABI underneath takes betas as [B, 10, T] and can)."""

    def __init__(self, device=None, dataset="amass", model_path=SMPL_MODEL_PATH, extra_regressor_path=EXTRA_REGRESSOR_PATH,
                 vertex_joint_ids=None, _native_lib=None):
        super().__init__(device=device, dataset=dataset, model_path=model_path, _native_lib=_native_lib)
        self.extra_regressor_path = extra_regressor_path
        self.vertex_joint_ids = tuple(int(i) for i in (SMPLH_VERTEX_JOINT_IDS if vertex_joint_ids is None else vertex_joint_ids))
        self.maps = joint_maps()
        self.smpl_model = _SmplModelView(self)
        self._model = None
        self._extra = None
        self._host = {}
        self._dev = {}

    # ---- host tables ---------------------------------------------------------------------------------------------------------
    def model(self):
        if self._model is None:
            m = load_smpl_model(self.model_path)
            V = m["v_template"].shape[0]
            ids = self.vertex_joint_ids
            if len(ids) != 21:
                raise ValueError(f"vertex_joint_ids must hold the 21 vertices of smplx's VertexJointSelector, got {len(ids)}")
            if min(ids) < 0 or max(ids) >= V:
                raise ValueError(f"{self.model_path}: the model has {V} vertices, but vertex_joint_ids reaches vertex {max(ids)} "
                                 f"(the default table is the 6,890-vertex SMPL body's; pass vertex_joint_ids= for another mesh)")
            self._model = m
        return self._model

    def extra_regressor(self):
        if self._extra is None:
            path = self.extra_regressor_path
            if not os.path.isfile(path):
                raise FileNotFoundError(f"extra joint regressor {path} not found (relative to {os.getcwd()}): the 'a2m', 'a2mpl' "
                                        f"and 'vibe' joints need J_regressor_extra.npy, which the reference's {DOWNLOAD_SCRIPT} "
                                        f"puts there")
            e = np.asarray(np.load(path), np.float64)
            V = self.model()["v_template"].shape[0]
            if e.ndim != 2 or e.shape[1] != V or e.shape[0] != 9:
                raise ValueError(f"{path}: expected a [9, {V}] regressor, got {e.shape}")
            self._extra = e
        return self._extra

    def _host_tables(self, want_extra):
        if "base" not in self._host:
            m = self.model()
            V = m["v_template"].shape[0]
            ids = list(self.vertex_joint_ids)
            reg = m["J_regressor"]
            self._host["base"] = dict(
                j0=(reg @ m["v_template"]).astype(np.float32),                                   # folded in float64
                jdirs=np.einsum("jv,vcl->jcl", reg, m["shapedirs"]).astype(np.float32),
                blend=_blend_table(m["v_template"], m["shapedirs"], m["posedirs"], (V + 31) & ~31),
                weights_t=_weights_table(m["weights"], (V + 31) & ~31),
                sel_blend=_blend_table(m["v_template"][ids], m["shapedirs"][ids], m["posedirs"][ids], 32),
                sel_weights_t=_weights_table(m["weights"][ids], 32))
        if want_extra and "extra" not in self._host:
            self._host["extra"] = dict(extra_t=np.ascontiguousarray(self.extra_regressor().T, dtype=np.float32))
        return self._host

    def _device_tables(self, device, want_extra):
        host = self._host_tables(want_extra)
        dev = self._dev.setdefault(str(device), {})
        for group in ("base",) + (("extra",) if want_extra else ()):
            for k, a in host[group].items():
                if k not in dev:
                    dev[k] = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return dev

    # ---- the call ------------------------------------------------------------------------------------------------------------
    def __call__(self, x, mask, pose_rep, translation, glob, jointstype, vertstrans, betas=None, beta=0, glob_rot=None,
                 get_rotations_back=False, **kwargs):
        if pose_rep == "xyz":                                   # rotation2xyz.py:20-21
            return x
        if not glob and glob_rot is None:
            raise TypeError("You must specify global rotation if glob is False")
        if jointstype not in JOINTSTYPES:
            raise NotImplementedError("This jointstype is not implemented.")
        if pose_rep not in nat.SMPL_POSE_REPS:
            raise NotImplementedError("No geometry for this one.")
        if (pose_rep == "rot6d" and jointstype == "smpl" and glob and translation and vertstrans and betas is None and beta == 0
                and not get_rotations_back):                    # what Rotation2xyz runs: its kernel, its bits
            return super().__call__(x, mask=mask, pose_rep=pose_rep, translation=True, glob=True, jointstype="smpl",
                                    vertstrans=True, betas=None, beta=0, glob_rot=glob_rot, get_rotations_back=False)
        m = self.model()
        J, V = m["J_regressor"].shape
        F = nat.SMPL_REP_FEATS[pose_rep]
        NR = J if glob else J - 1
        rows = NR + (1 if translation else 0)
        if x.dim() != 4 or x.shape[1] != rows or x.shape[2] != F:
            raise ValueError(f"x must be [B, {rows}, {F}, T] for pose_rep={pose_rep!r}, glob={bool(glob)}, "
                             f"translation={bool(translation)} on a model of {J} joints, got {tuple(x.shape)}")
        lib = self._lib()
        stream = self._stream(lib, x, "tensors")
        B, T = x.shape[0], x.shape[-1]
        dev = x.device
        x = x.contiguous().float()
        mk = None
        if mask is not None:
            if tuple(mask.shape) != (B, T):
                raise ValueError(f"mask must be [B, T] = {(B, T)}, got {tuple(mask.shape)}")
            mk = mask.to(device=dev, dtype=torch.uint8).contiguous()
        bt = None
        if betas is not None:
            betas = torch.as_tensor(betas).to(device=dev, dtype=torch.float32)
            if betas.dim() != 2 or betas.shape[1] != NUM_BETAS:
                raise ValueError(f"betas must be [n_valid_frames, {NUM_BETAS}] or [1, {NUM_BETAS}], got {tuple(betas.shape)}")
            full = torch.zeros(B, T, NUM_BETAS, dtype=torch.float32, device=dev)
            if betas.shape[0] == 1:
                full[:] = betas[0]
            else:
                sel = mk.bool() if mk is not None else torch.ones(B, T, dtype=torch.bool, device=dev)
                n_valid = int(sel.sum())
                if betas.shape[0] != n_valid:
                    raise ValueError(f"betas has {betas.shape[0]} rows; the mask has {n_valid} valid frames")
                full[sel] = betas
            bt = full.permute(0, 2, 1).contiguous()             # [B, 10, T]
        joints = jointstype != "vertices"
        want_extra = joints and jointstype != "smpl"
        tab = self._device_tables(dev, want_extra)
        pmap = np.ascontiguousarray(self.maps[jointstype], dtype=np.int32) if joints else None
        n_points = len(pmap) if joints else 0
        grot = None if glob else _axis_angle_to_matrix(glob_rot)
        parents = m["parents"]
        i32p, f32p = nat.C.POINTER(nat.C.c_int32), nat.C.POINTER(nat.C.c_float)
        model = nat.MdmSmplModel(j0=tab["j0"].data_ptr(), jdirs=tab["jdirs"].data_ptr(), blend=tab["blend"].data_ptr(),
                                 weights_t=tab["weights_t"].data_ptr(), sel_blend=tab["sel_blend"].data_ptr(),
                                 sel_weights_t=tab["sel_weights_t"].data_ptr(),
                                 extra_t=tab["extra_t"].data_ptr() if want_extra else None,
                                 parents=parents.ctypes.data_as(i32p), J=J, V=V, n_sel=21, n_extra=9 if want_extra else 0)
        call = nat.MdmSmplCall(pose_rep=nat.SMPL_POSE_REPS[pose_rep], glob=1 if glob else 0, translation=1 if translation else 0,
                               vertstrans=1 if vertstrans else 0, n_points=n_points,
                               root_point=JOINTSTYPE_ROOT[jointstype] if joints else 0,
                               point_map=pmap.ctypes.data_as(i32p) if joints else None,
                               glob_rot_mat=grot.ctypes.data_as(f32p) if grot is not None else None, beta1=float(beta))
        ws, nbytes = self._workspace("mdm_smpl_workspace_bytes", model, call, B, T, dev=dev)
        out = torch.empty(B, n_points if joints else V, 3, T, dtype=torch.float32, device=dev)
        rot = torch.zeros(B, T, NR, 3, 3, dtype=torch.float32, device=dev) if get_rotations_back else None
        lib.check(lib.mdm_smpl_forward(nat.C.byref(model), nat.C.byref(call), x.data_ptr(), mk.data_ptr() if mk is not None else None,
                                       bt.data_ptr() if bt is not None else None, out.data_ptr(),
                                       rot.data_ptr() if rot is not None else None, B, T, rows, F, ws.data_ptr(), nbytes, stream),
                  "mdm_smpl_forward")
        if not get_rotations_back:
            return out
        rotations = rot[mk.bool()] if mk is not None else rot.reshape(B * T, NR, 3, 3)      # valid frames only, [n, rows, 3, 3]
        if glob:
            return out, rotations[:, 1:], rotations[:, 0]
        n = rotations.shape[0]
        return out, rotations, torch.from_numpy(grot.reshape(1, 1, 3, 3)).to(dev).repeat(n, 1, 1, 1)
