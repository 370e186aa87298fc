"""`Rotation2xyz` -- the reference's SMPL transform seam (model/rotation2xyz.py) on the MI355X HIP path.

Every reference script that consumes a rot6d (action-to-motion) sample calls
    model.rot2xyz(x=sample, mask=mask, pose_rep='rot6d', glob=True, translation=True, jointstype='smpl', vertstrans=True,
                  betas=None, beta=0, glob_rot=None, get_rotations_back=False)
(sample/generate.py:167-171, sample/predict.py:134-138, eval/a2m/stgcn_eval.py:55, eval/a2m/gru_eval.py:39).  With zero betas
the 'smpl' joints (model/smpl.py:86-96: smplx's posed skeleton joints 0..23) depend only on the 24 rotations, the rest-pose joints
J_regressor . v_template and the kinematic tree, so the reference's full 6,890-vertex SMPL pass reduces to rot6d -> rotation
matrices -> forward kinematics over 24 joints: one HIP kernel (csrc/smpl_joints.h behind mdm_rot6d_to_smpl_joints).  No CPU
fallback.

pose_rep='xyz' (the HumanML3D / KIT families) returns its input and never opens the SMPL file.  Everything that needs the full
vertex pass ('vertices', 'a2m', 'a2mpl', 'vibe'), shape parameters, another pose representation, glob=False, translation=False,
vertstrans=False or the rotations back raises NotImplementedError naming the argument.
"""
import os
import pickle

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from ._native_model import NativeModelMixin

SMPL_MODEL_PATH = os.path.join("./body_models/smpl", "SMPL_NEUTRAL.pkl")     # utils/config.py:3-6, relative to the working dir
DOWNLOAD_SCRIPT = "prepare/download_smpl_files.sh"


class ChumpyPlaceholder:
    """What a chumpy object of the SMPL pickle unpickles to when chumpy is not installed: its pickled state, nothing else."""

    def __init__(self, *args, **kwargs):
        self.state = None

    def __setstate__(self, state):
        self.state = state


class _SmplUnpickler(pickle.Unpickler):
    """Loads the official SMPL pickle (python 2, latin1) without chumpy: chumpy classes become ChumpyPlaceholder; only numpy,
    scipy and the builtins the pickle protocol itself needs are resolved."""
    _ALLOWED = ("numpy", "scipy", "builtins", "__builtin__", "copy_reg", "copyreg", "_codecs", "collections")

    def find_class(self, module, name):
        if module == "chumpy" or module.startswith("chumpy."):
            return ChumpyPlaceholder
        if module.split(".")[0] in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"SMPL model file: refusing to load {module}.{name}")


def _dense(field, value, path):
    if isinstance(value, ChumpyPlaceholder):
        raise ValueError(
            f"{path}: field {field!r} is a chumpy object, and chumpy is not a dependency of this package. Convert the model "
            f"file to plain numpy arrays with smplx's chumpy-free conversion (smplx tools/clean_ch.py, run where chumpy is "
            f"installed) and point at the converted file.")
    if hasattr(value, "toarray"):          # scipy.sparse (the official J_regressor is a csc_matrix)
        value = value.toarray()
    return np.asarray(value, dtype=np.float64)


def load_smpl_tables(path=SMPL_MODEL_PATH):
    """(rest_joints float32 [J, 3], parents int32 [J]) of an SMPL model file: J = J_regressor . v_template computed in float64
    (the shape blend term is zero: every caller passes beta=0), parents = kintree_table[0] with the root's entry set to -1
    (smplx body_models.py does the same).  Only v_template, J_regressor and kintree_table are read."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"SMPL model file {path} not found (relative to {os.getcwd()}): rot2xyz with pose_rep != 'xyz' "
                                f"needs SMPL_NEUTRAL.pkl, which the reference's {DOWNLOAD_SCRIPT} puts there")
    with open(path, "rb") as f:
        data = _SmplUnpickler(f, encoding="latin1").load()
    if not isinstance(data, dict):
        raise ValueError(f"{path}: expected a dict of SMPL model fields, got {type(data).__name__}")
    for k in ("v_template", "J_regressor", "kintree_table"):
        if k not in data:
            raise ValueError(f"{path}: no {k!r} field")
    v = _dense("v_template", data["v_template"], path)
    reg = _dense("J_regressor", data["J_regressor"], path)
    kin = np.asarray(data["kintree_table"])
    if v.ndim != 2 or v.shape[1] != 3 or reg.ndim != 2 or reg.shape[1] != v.shape[0] or kin.ndim != 2 or kin.shape[1] != reg.shape[0]:
        raise ValueError(f"{path}: inconsistent shapes v_template {v.shape}, J_regressor {reg.shape}, kintree_table {kin.shape}")
    rest = (reg @ v).astype(np.float32)
    parents = kin[0].astype(np.int64)
    parents[0] = -1
    return np.ascontiguousarray(rest), np.ascontiguousarray(parents.astype(np.int32))


class Rotation2xyz(NativeModelMixin):
    """model/rotation2xyz.py:10-90 with the reference's call signature.  `model_path` defaults to the reference's location; the
    file is read at the first non-'xyz' call and its tables are cached on the object."""

    def __init__(self, device=None, dataset="amass", model_path=SMPL_MODEL_PATH, _native_lib=None):
        self.device, self.dataset = device, dataset
        self.model_path = model_path
        self._native_lib = _native_lib
        # train/train_mdm.py:47 calls model.rot2xyz.smpl_model.eval(): a module without parameters or buffers
        self.smpl_model = nn.Module()
        self._tables = None

    def tables(self):
        if self._tables is None:
            self._tables = load_smpl_tables(self.model_path)
        return self._tables

    def __call__(self, x, mask=None, pose_rep="xyz", translation=True, glob=True, jointstype="smpl", vertstrans=True,
                 betas=None, beta=0, glob_rot=None, get_rotations_back=False, **kwargs):
        if pose_rep == "xyz":                                   # rotation2xyz.py:20-21
            return x
        for arg, value, ok in (("pose_rep", pose_rep, pose_rep == "rot6d"),
                               ("jointstype", jointstype, jointstype == "smpl"),
                               ("glob", glob, bool(glob)),
                               ("translation", translation, bool(translation)),
                               ("vertstrans", vertstrans, bool(vertstrans)),
                               ("betas", "a tensor" if betas is not None else None, betas is None),
                               ("beta", beta, beta == 0),
                               ("get_rotations_back", get_rotations_back, not get_rotations_back)):
            if not ok:
                raise NotImplementedError(
                    f"rot2xyz: {arg}={value!r} is not supported on the MI355X path (SMPL joints of rot6d samples only: "
                    f"pose_rep='rot6d', jointstype='smpl', glob=True, translation=True, vertstrans=True, beta=0, betas=None)")
        if x.dim() != 4 or x.shape[2] != 6:
            raise ValueError(f"x must be [B, joints + 1, 6, T] rot6d features, got {tuple(x.shape)}")
        rest, parents = self.tables()
        lib = self._lib()
        stream = self._stream(lib, x, "tensors")
        B, NJ, _, T = x.shape
        J = rest.shape[0]
        if NJ != J + 1:
            raise ValueError(f"x has {NJ} rows; the SMPL model has {J} joints plus the translation row = {J + 1}")
        x = x.contiguous().float()
        m = None
        if mask is not None:
            if tuple(mask.shape) != (B, T):
                raise ValueError(f"mask must be [B, T] = {(B, T)}, got {tuple(mask.shape)}")
            m = mask.to(device=x.device, dtype=torch.uint8).contiguous()
        out = torch.empty(B, J, 3, T, dtype=torch.float32, device=x.device)
        lib.check(lib.mdm_rot6d_to_smpl_joints(x.data_ptr(), m.data_ptr() if m is not None else None,
                                               rest.ctypes.data_as(nat.C.POINTER(nat.C.c_float)),
                                               parents.ctypes.data_as(nat.C.POINTER(nat.C.c_int32)),
                                               out.data_ptr(), B, T, NJ, J, stream), "mdm_rot6d_to_smpl_joints")
        return out
