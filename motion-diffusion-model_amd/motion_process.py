"""Device-side post-sampling transform: what sample/generate.py:160-166 does on the CPU after a
D2H copy -- `inv_transform` (data_loaders/humanml/data/dataset.py:132-133) followed by `recover_from_ric`
(data_loaders/humanml/scripts/motion_process.py:437-452) and the permute to [B, joints, 3, T] -- as one HIP kernel
on the sampler's output tensor (csrc/motion_recover.h behind mdm_recover_from_ric).  No CPU fallback.

And the way back (csrc/motion_features.h behind mdm_joints_to_features): joint positions -> normalised HumanML3D / KIT feature
vectors in the sampler's [B, 263 | 251, 1, T] layout -- `extract_features` and `process_file` of the same reference file
(motion_process.py:43-355) with the inverse / forward kinematics of common/skeleton.py -- so that a generated clip, a mocap take or an
earlier results.npy can be fed back as `init_image`, `y['inpainted_motion']` or DiP's `y['prefix']`."""
import ctypes as C

import numpy as np
import torch

from . import _native as nat
from ._native_model import native_stream


def recover_from_ric(sample, mean, std, joints_num=None, _native_lib=None):
    """sample: float32 [B, njoints_feat, 1, T] (the output of p_sample_loop, normalised features);
    mean/std: float32 [njoints_feat] (the dataset's Mean.npy / Std.npy);  returns float32 [B, joints_num, 3, T],
    i.e. generate.py's `recover_from_ric(inv_transform(sample.permute(0, 2, 3, 1)), n_joints)` reshaped as at :166."""
    lib = _native_lib if _native_lib is not None else nat.load_native()
    if sample.dim() != 4 or sample.shape[2] != 1:
        raise ValueError(f"sample must be [B, njoints_feat, 1, T], got {tuple(sample.shape)}")
    stream = native_stream(lib, sample, "tensors")
    B, JF, _, T = sample.shape
    if joints_num is None:
        joints_num = 22 if JF == 263 else 21            # generate.py:162
    x = sample.contiguous().float()
    mean = torch.as_tensor(mean, dtype=torch.float32, device=x.device).contiguous()
    std = torch.as_tensor(std, dtype=torch.float32, device=x.device).contiguous()
    if mean.numel() != JF or std.numel() != JF:
        raise ValueError("mean/std must have njoints_feat elements")
    out = torch.empty(B, joints_num, 3, T, dtype=torch.float32, device=x.device)
    lib.check(lib.mdm_recover_from_ric(x.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr(), B, T, JF,
                                       joints_num, stream), "mdm_recover_from_ric")
    return out


# The skeleton tables of the two datasets, as data: the kinematic chains and raw offsets of utils/paramUtil.py:4-55, the face joints
# (in the reference's list order r_hip, l_hip, sdr_r, sdr_l), the foot joints, the two leg bones of uniform_skeleton's scale ratio and
# the default foot threshold of motion_process.py:460-466 (HumanML3D) and :506-512 (KIT).
SKELETONS = {
    "humanml": dict(
        joints=22, feet_thre=0.002, face_joint_indx=[2, 1, 17, 16], fid_r=[8, 11], fid_l=[7, 10], l_idx1=5, l_idx2=8,
        kinematic_chain=[[0, 2, 5, 8, 11], [0, 1, 4, 7, 10], [0, 3, 6, 9, 12, 15], [9, 14, 17, 19, 21], [9, 13, 16, 18, 20]],
        raw_offsets=[[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, -1, 0], [0, 1, 0], [0, -1, 0], [0, -1, 0], [0, 1, 0],
                     [0, 0, 1], [0, 0, 1], [0, 1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, -1, 0], [0, -1, 0], [0, -1, 0],
                     [0, -1, 0], [0, -1, 0], [0, -1, 0]]),
    "kit": dict(
        joints=21, feet_thre=0.05, face_joint_indx=[11, 16, 5, 8], fid_r=[14, 15], fid_l=[19, 20], l_idx1=17, l_idx2=18,
        kinematic_chain=[[0, 11, 12, 13, 14, 15], [0, 16, 17, 18, 19, 20], [0, 1, 2, 3, 4], [3, 5, 6, 7], [3, 8, 9, 10]],
        raw_offsets=[[0, 0, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [1, 0, 0], [0, -1, 0], [0, -1, 0], [-1, 0, 0], [0, -1, 0],
                     [0, -1, 0], [1, 0, 0], [0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, -1, 0],
                     [0, 0, 1], [0, 0, 1]]),
}
CANONICAL_STEPS = ("floor", "origin_xz", "face_z")


def feature_dim(joints_num):
    """263 for 22 joints, 251 for 21: root 4, ric 3 (J - 1), rot6d 6 (J - 1), local velocity 3 J, foot contacts 4."""
    return 12 * joints_num - 1


def _skeleton_struct(raw_offsets, kinematic_chain, face_joint_indx, fid_r, fid_l, l_idx1=1, l_idx2=1):
    raw = np.asarray(raw_offsets.cpu() if torch.is_tensor(raw_offsets) else raw_offsets, dtype=np.float32)
    if raw.ndim != 2 or raw.shape[1] != 3 or not 2 <= raw.shape[0] <= nat.SKEL_MAX_JOINTS:
        raise ValueError(f"n_raw_offsets must be [J, 3] with 2 <= J <= {nat.SKEL_MAX_JOINTS}, got {raw.shape}")
    chains = [[int(j) for j in ch] for ch in kinematic_chain]
    if not 1 <= len(chains) <= nat.SKEL_MAX_CHAINS or any(not 2 <= len(ch) <= nat.SKEL_MAX_CHAIN_LEN for ch in chains):
        raise ValueError(f"kinematic_chain must hold 1 to {nat.SKEL_MAX_CHAINS} chains of 2 to {nat.SKEL_MAX_CHAIN_LEN} joints")
    if len(face_joint_indx) != 4 or len(fid_r) != 2 or len(fid_l) != 2:
        raise ValueError("face_joint_indx must name 4 joints, fid_r and fid_l 2 each")
    sk = nat.MdmSkeleton(joints=raw.shape[0], n_chains=len(chains), l_idx1=int(l_idx1), l_idx2=int(l_idx2))
    for c, ch in enumerate(chains):
        sk.chain_len[c] = len(ch)
        for i, j in enumerate(ch):
            sk.chains[c][i] = j
    for j in range(raw.shape[0]):
        for c in range(3):
            sk.raw_offsets[j][c] = float(raw[j, c])
    for k in range(4):
        sk.face_joints[k] = int(face_joint_indx[k])
    for k in range(2):
        sk.fid_r[k], sk.fid_l[k] = int(fid_r[k]), int(fid_l[k])
    return sk


def _dataset_tables(dataset):
    if dataset not in SKELETONS:
        raise ValueError(f"dataset must be one of {sorted(SKELETONS)}, got {dataset!r}")
    return SKELETONS[dataset]


def _run_features(lib, x, lengths, sk, feet_thre, steps, tgt_offsets, mean, std, layout, aux):
    """x: float32 tensor [B, J, 3, T] ('bj3t') or [B, T, J, 3] ('btj3') on the library's device -> [B, F, 1, T - 1] and, with `aux`,
    the positions the features were taken from and the rotation-invariant positions, both [B, J, 3, T]."""
    if layout not in nat.J2F_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(nat.J2F_LAYOUTS)}, got {layout!r}")
    J = sk.joints
    want = (J, 3) if layout == "bj3t" else None
    if x.dim() != 4 or (layout == "bj3t" and tuple(x.shape[1:3]) != want) or (layout == "btj3" and tuple(x.shape[2:]) != (J, 3)):
        raise ValueError(f"joints must be [B, {J}, 3, T] (layout 'bj3t') or [B, T, {J}, 3] ('btj3'), got {tuple(x.shape)} for layout {layout!r}")
    B, T = x.shape[0], (x.shape[3] if layout == "bj3t" else x.shape[1])
    if B < 1 or T < 2:
        raise ValueError(f"joints must hold at least one clip of at least 2 frames, got {tuple(x.shape)}")
    if T > nat.J2F_MAX_FRAMES:
        raise ValueError(f"joints: at most {nat.J2F_MAX_FRAMES} frames per clip, got {T}")
    len_arr = None
    if lengths is not None:
        host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).astype(np.int64).reshape(-1)
        if host.shape[0] != B or host.min() < 2 or host.max() > T:
            raise ValueError(f"lengths must hold {B} frame counts in [2, {T}], got {host.tolist()}")
        len_arr = (C.c_int32 * B)(*host.tolist())
    if not feet_thre > 0:
        raise ValueError(f"feet_thre must be positive, got {feet_thre}")
    F = feature_dim(J)
    x = x.contiguous().float()
    call = nat.MdmJointsToFeaturesCall(layout=nat.J2F_LAYOUTS[layout], feet_thre=float(feet_thre))
    for name in steps:
        if name not in CANONICAL_STEPS:
            raise ValueError(f"canonicalise names steps of {CANONICAL_STEPS}, got {name!r}")
        setattr(call, name, 1)
    keep = []
    if tgt_offsets is not None:
        tgt = np.ascontiguousarray(tgt_offsets.cpu() if torch.is_tensor(tgt_offsets) else tgt_offsets, dtype=np.float32)
        if tgt.shape != (J, 3):
            raise ValueError(f"tgt_offsets must be [{J}, 3], got {tgt.shape}")
        keep.append(tgt)
        call.tgt_offsets = tgt.ctypes.data_as(C.POINTER(C.c_float))
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    if mean is not None:
        mean = torch.as_tensor(mean, dtype=torch.float32, device=x.device).contiguous()
        std = torch.as_tensor(std, dtype=torch.float32, device=x.device).contiguous()
        if mean.numel() != F or std.numel() != F:
            raise ValueError(f"mean / std must have {F} elements")
        call.mean_dev, call.std_dev = mean.data_ptr(), std.data_ptr()
    stream = native_stream(lib, x, "joints")
    out = torch.empty(B, F, 1, T - 1, dtype=torch.float32, device=x.device)
    glob = ric = None
    if aux:
        glob = torch.empty(B, J, 3, T, dtype=torch.float32, device=x.device)
        ric = torch.empty_like(glob)
        call.global_dev, call.ric_dev = glob.data_ptr(), ric.data_ptr()
    ws, ws_bytes = None, 0
    if steps or tgt_offsets is not None:
        ws_bytes = lib.mdm_joints_to_features_workspace_bytes(B, T, J)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    lib.check(lib.mdm_joints_to_features(C.byref(sk), C.byref(call), x.data_ptr(), len_arr, out.data_ptr(), B, T, F,
                                         ws.data_ptr() if ws is not None else None, ws_bytes, stream), "mdm_joints_to_features")
    return out, glob, ric


def joints_to_features(joints, lengths=None, dataset="humanml", mean=None, std=None, feet_thre=None, canonicalise=True,
                       tgt_offsets=None, layout="bj3t", _native_lib=None):
    """Joint positions -> feature vectors, on the device: float32 [B, J, 3, T] (what `recover_from_ric` emits; layout='btj3' takes
    [B, T, J, 3]) -> float32 [B, F, 1, T - 1], F = 263 (22 joints, dataset='humanml') or 251 (21 joints, 'kit'); normalised
    `(x - mean) / std` when the dataset's Mean.npy / Std.npy are given.  The result goes straight into `init_image`,
    `y['inpainted_motion']` and `y['prefix']`.

    lengths          per-clip frame counts, 2 <= L <= T (None: T).  Frames >= L - 1 of a clip are exact zeros, and nothing beyond a
                     clip's length influences its valid frames.
    canonicalise     True: process_file's transform first (motion_process.py:181-217) -- the clip put on the floor, frame 0's root
                     xz at the origin, frame 0 facing +Z; False: extract_features on the positions as they are; or an iterable of
                     the steps to apply, from ('floor', 'origin_xz', 'face_z').
    tgt_offsets      [J, 3]: uniform_skeleton (motion_process.py:17-40) first, retargeting every clip onto these bone offsets (what
                     Skeleton.get_offsets_joints returns for the dataset's example clip, which this package does not ship: there is
                     no default, and without it the step is skipped).
    feet_thre        the squared foot displacement below which a foot counts as planted (default 0.002 / 0.05).

    The foot contacts are computed in fp32 exactly as numpy does on fp32 positions; everything else in fp64 on the device, rounded
    once.  One deliberate difference: the reference's qbetween calls torch.cross without `dim`, so for a clip of exactly 3 frames it
    crosses along the frame axis; this path always crosses over xyz."""
    lib = _native_lib if _native_lib is not None else nat.load_native()
    tab = _dataset_tables(dataset)
    if not torch.is_tensor(joints):
        raise ValueError("joints must be a tensor on the device")
    sk = _skeleton_struct(tab["raw_offsets"], tab["kinematic_chain"], tab["face_joint_indx"], tab["fid_r"], tab["fid_l"],
                          tab["l_idx1"], tab["l_idx2"])
    steps = CANONICAL_STEPS if canonicalise is True else (() if canonicalise is False or canonicalise is None else tuple(canonicalise))
    return _run_features(lib, joints, lengths, sk, tab["feet_thre"] if feet_thre is None else feet_thre, steps, tgt_offsets, mean, std,
                         layout, False)[0]


def _clip_tensor(lib, positions, joints_num=None):
    """[T, J, 3] numpy array or tensor -> (a float32 tensor [1, T, J, 3] on the library's device -- a copy, the argument stays as it
    is --, whether the caller gave numpy)."""
    is_np = not torch.is_tensor(positions)
    x = torch.as_tensor(np.asarray(positions, dtype=np.float32)) if is_np else positions.detach().float()
    if x.dim() != 3 or x.shape[2] != 3 or (joints_num is not None and x.shape[1] != joints_num):
        raise ValueError(f"positions must be [T, {joints_num or 'J'}, 3], got {tuple(x.shape)}")
    if is_np or x.device.type != "cuda":
        x = x.to("cuda" if lib.path.endswith(nat.LIB_NAME) else "cpu")
    return x.clone()[None], is_np


def extract_features(positions, feet_thre, n_raw_offsets, kinematic_chain, face_joint_indx, fid_r, fid_l, _native_lib=None):
    """The reference's extract_features (motion_process.py:43-170) with its signature: positions [T, J, 3] (numpy or tensor) ->
    [T - 1, F] of the same kind, float32.  Unlike the reference it does not modify `positions`."""
    lib = _native_lib if _native_lib is not None else nat.load_native()
    sk = _skeleton_struct(n_raw_offsets, kinematic_chain, face_joint_indx, fid_r, fid_l)
    x, is_np = _clip_tensor(lib, positions, sk.joints)
    data = _run_features(lib, x, None, sk, feet_thre, (), None, None, None, "btj3", False)[0][0, :, 0].t().contiguous()
    return data.cpu().numpy() if is_np else data


def process_file(positions, feet_thre, tgt_offsets=None, dataset="humanml", _native_lib=None):
    """The reference's process_file (motion_process.py:173-355): positions [T, J, 3] (numpy or tensor) -> the 4-tuple
    (data [T - 1, F], global_positions [T, J, 3], positions [T, J, 3] -- the rotation-invariant ones --, l_velocity [T - 1, 2]), float32
    and of the argument's kind.  The skeleton tables are `dataset`'s; `tgt_offsets` [J, 3] enables the uniform_skeleton step (the
    reference reads it from a module global).  `positions` is not modified."""
    lib = _native_lib if _native_lib is not None else nat.load_native()
    tab = _dataset_tables(dataset)
    sk = _skeleton_struct(tab["raw_offsets"], tab["kinematic_chain"], tab["face_joint_indx"], tab["fid_r"], tab["fid_l"],
                          tab["l_idx1"], tab["l_idx2"])
    x, is_np = _clip_tensor(lib, positions, sk.joints)
    out, glob, ric = _run_features(lib, x, None, sk, feet_thre, CANONICAL_STEPS, tgt_offsets, None, None, "btj3", True)
    data = out[0, :, 0].t().contiguous()
    res = (data, glob[0].permute(2, 0, 1).contiguous(), ric[0].permute(2, 0, 1).contiguous(), data[:, 1:3].contiguous())
    return tuple(r.cpu().numpy() for r in res) if is_np else res
