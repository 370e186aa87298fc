"""Inputs, the fp64 oracle and the bounds of the joints -> HumanML3D features tests (csrc/motion_features.h behind
mdm_joints_to_features; mdm_amd/motion_process.py joints_to_features / extract_features / process_file).

The ORACLE restates data_loaders/humanml/scripts/motion_process.py:43-355 with common/skeleton.py:55-104, :129-150 and the
quaternion helpers of common/quaternion.py in float64 numpy, written from the arithmetic (not shared with the device code), and
crosses over xyz always: the reference's qbetween calls torch.cross without `dim`, so for a clip of exactly 3 frames it crosses
along the frame axis (it warns, it does not raise) -- T = 3 is therefore compared with this oracle only.

The INPUTS are synthetic clips: a rest pose grown along the kinematic chains with random bone lengths, a smooth per-joint wobble,
a yaw that varies over time and a drifting root.  `make_clip` asserts the conditions under which the reference (fp32 torch
quaternions inside float64 numpy glue) is a meaningful yardstick:
  * every qbetween of the clip (root and bones, the retargeting pass included) has w >= W_MIN before normalisation: no bone and no
    facing direction within a few degrees of antiparallel to its target (the reference's error grows like 1 / w);
  * no bone has zero length;
  * every squared foot displacement is at least FOOT_MARGIN (relative) away from the threshold, so that the flags do not hang on
    the reference's fp32 rounding of the canonicalised positions.
The ADVERSARIAL foot case is the opposite on purpose: fp32 displacements whose squared length, summed in fp32 as (dx^2 + dy^2) +
dz^2, lands exactly on the fp32 number nearest the threshold, one ulp below it and one ulp above it; the expected flags are the
reference's.

BOUNDS.  Device against oracle: the device works in fp64 and rounds once at the store, so an element is off by at most one fp32
ulp of its own magnitude (half an ulp of rounding, and one more when a 1e-16 difference between two fp64 evaluations straddles a
rounding boundary): `oracle_tol(group) = 4 * 2^-24 * max|group|`.  Device against reference: `2 * d_ref` of the case and group
(tests/golden/PIN_REPORT_motion_features.json), d_ref = max|reference - oracle|: the device's own error adds to the reference's
at most once."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
PIN_REPORT = os.path.join(GOLDEN, "PIN_REPORT_motion_features.json")

W_MIN = 0.05
FOOT_MARGIN = 1e-3
RADIUS, SIGMA = 80, 20.0            # scipy gaussian_filter1d(sigma=20, truncate=4): int(4 * 20 + 0.5) taps each side

# utils/paramUtil.py:4-55 and motion_process.py:460-466, :506-512, restated as data (the test's own copy: the package's tables
# in mdm_amd/motion_process.py SKELETONS are compared with these in tests/test_host_motion_features.py)
SKELETONS = {
    "humanml": dict(
        joints=22, feet_thre=0.002, face=[2, 1, 17, 16], fid_r=[8, 11], fid_l=[7, 10], l_idx1=5, l_idx2=8,
        chains=[[0, 2, 5, 8, 11], [0, 1, 4, 7, 10], [0, 3, 6, 9, 12, 15], [9, 14, 17, 19, 21], [9, 13, 16, 18, 20]],
        raw=[[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, -1, 0], [0, 1, 0], [0, -1, 0], [0, -1, 0], [0, 1, 0],
             [0, 0, 1], [0, 0, 1], [0, 1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, -1, 0], [0, -1, 0], [0, -1, 0], [0, -1, 0],
             [0, -1, 0], [0, -1, 0]]),
    "kit": dict(
        joints=21, feet_thre=0.05, face=[11, 16, 5, 8], fid_r=[14, 15], fid_l=[19, 20], l_idx1=17, l_idx2=18,
        chains=[[0, 11, 12, 13, 14, 15], [0, 16, 17, 18, 19, 20], [0, 1, 2, 3, 4], [3, 5, 6, 7], [3, 8, 9, 10]],
        raw=[[0, 0, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [1, 0, 0], [0, -1, 0], [0, -1, 0], [-1, 0, 0], [0, -1, 0],
             [0, -1, 0], [1, 0, 0], [0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, -1, 0], [0, 0, 1],
             [0, 0, 1]]),
}
DATASET_OF_J = {22: "humanml", 21: "kit"}


def feat_dim(J):
    return 4 + 3 * (J - 1) + 6 * (J - 1) + 3 * J + 4


def groups(J):
    """Feature groups of the [.., F] vector (motion_process.py:147-168)."""
    a = 4 + 3 * (J - 1)
    b = a + 6 * (J - 1)
    c = b + 3 * J
    return {"root": slice(0, 4), "ric": slice(4, a), "rot6d": slice(a, b), "local_velocity": slice(b, c), "feet": slice(c, c + 4)}


def parents_of(sk):
    par = [0] * sk["joints"]
    par[0] = -1
    for ch in sk["chains"]:
        for i in range(1, len(ch)):
            par[ch[i]] = ch[i - 1]
    return par


# ------------------------------------------------------------------------------------------------------------------ oracle (fp64)
def _qmul(q, r):
    w = q[..., 0] * r[..., 0] - q[..., 1] * r[..., 1] - q[..., 2] * r[..., 2] - q[..., 3] * r[..., 3]
    x = q[..., 0] * r[..., 1] + q[..., 1] * r[..., 0] + q[..., 2] * r[..., 3] - q[..., 3] * r[..., 2]
    y = q[..., 0] * r[..., 2] - q[..., 1] * r[..., 3] + q[..., 2] * r[..., 0] + q[..., 3] * r[..., 1]
    z = q[..., 0] * r[..., 3] + q[..., 1] * r[..., 2] - q[..., 2] * r[..., 1] + q[..., 3] * r[..., 0]
    return np.stack([w, x, y, z], axis=-1)


def _qinv(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def _qrot(q, v):
    qv = q[..., 1:]
    uv = np.cross(qv, v, axis=-1)
    uuv = np.cross(qv, uv, axis=-1)
    return v + 2.0 * (q[..., :1] * uv + uuv)


def _qbetween(v0, v1, ws=None):
    """quaternion.py:389-399 with the cross over xyz; qnormalize (:28-31) adds 1e-4 to the LAST component before it normalises."""
    v = np.cross(v0, v1, axis=-1)
    w = np.sqrt((v0 ** 2).sum(-1, keepdims=True) * (v1 ** 2).sum(-1, keepdims=True)) + (v0 * v1).sum(-1, keepdims=True)
    if ws is not None:
        ws.append(float(w.min()))
    q = np.concatenate([w, v], axis=-1)
    q[..., 3] += 1e-4
    return q / np.sqrt((q ** 2).sum(-1, keepdims=True))


def _unit(v):
    return v / np.sqrt((v ** 2).sum(-1, keepdims=True))


def gaussian_weights():
    x = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    w = np.exp(-0.5 / (SIGMA * SIGMA) * x ** 2)
    return w / w.sum()


def _smooth_nearest(f):
    L = len(f)
    w = gaussian_weights()
    idx = np.clip(np.arange(L)[:, None] + np.arange(-RADIUS, RADIUS + 1)[None, :], 0, L - 1)
    return (f[idx] * w[None, :, None]).sum(axis=1)


def _cross_y(a):
    """cross((0, 1, 0), a)."""
    return np.stack([a[..., 2], np.zeros_like(a[..., 0]), -a[..., 0]], axis=-1)


def ik(sk, P, smooth, ws=None, bone_min=None):
    """Skeleton.inverse_kinematics_np (skeleton.py:55-104): quat_params [L, J, 4]."""
    f = sk["face"]
    across = (P[:, f[1]] - P[:, f[0]]) + (P[:, f[2]] - P[:, f[3]])           # :61-64: the list is read as l_hip, r_hip, sdr_r, sdr_l
    forward = _cross_y(_unit(across))
    if smooth:
        forward = _smooth_nearest(forward)
    forward = _unit(forward)
    root = _qbetween(forward, np.broadcast_to(np.array([0.0, 0.0, 1.0]), forward.shape), ws)
    raw = np.asarray(sk["raw"], dtype=np.float64)
    quat = np.zeros(P.shape[:-1] + (4,))
    quat[:, 0] = root
    for ch in sk["chains"]:
        R = root
        for j in range(len(ch) - 1):
            v = P[:, ch[j + 1]] - P[:, ch[j]]
            if bone_min is not None:
                bone_min.append(float(np.sqrt((v ** 2).sum(-1)).min()))
            rot = _qbetween(np.broadcast_to(raw[ch[j + 1]], v.shape), _unit(v), ws)
            loc = _qmul(_qinv(R), rot)
            quat[:, ch[j + 1]] = loc
            R = _qmul(R, loc)
    return quat


def uniform_skeleton(sk, P, tgt, ws=None, bone_min=None):
    """motion_process.py:17-40."""
    par = parents_of(sk)
    raw = np.asarray(sk["raw"], dtype=np.float64)
    tgt = np.asarray(tgt, dtype=np.float64)

    def leg(off):
        return np.abs(off[sk["l_idx1"]]).max() + np.abs(off[sk["l_idx2"]]).max()
    src = np.zeros_like(raw)
    for i in range(1, sk["joints"]):
        src[i] = np.sqrt(((P[0, i] - P[0, par[i]]) ** 2).sum()) * raw[i]
    scale = leg(tgt) / leg(src)
    quat = ik(sk, P, False, ws, bone_min)
    out = np.zeros_like(P)
    out[:, 0] = P[:, 0] * scale
    for ch in sk["chains"]:
        R = quat[:, 0]
        for i in range(1, len(ch)):
            R = _qmul(R, quat[:, ch[i]])
            out[:, ch[i]] = _qrot(R, np.broadcast_to(tgt[ch[i]], R.shape[:-1] + (3,))) + out[:, ch[i - 1]]
    return out


def canonicalise(sk, P, tgt=None, floor=True, origin_xz=True, face_z=True, ws=None, bone_min=None):
    """process_file's transform of the clip (motion_process.py:178-222) -> the reference's `global_positions`."""
    P = np.array(P, dtype=np.float64)
    if tgt is not None:
        P = uniform_skeleton(sk, P, tgt, ws, bone_min)
    if floor:
        P[:, :, 1] -= P[:, :, 1].min()
    init = P[0].copy()
    if origin_xz:
        P = P - init[0] * np.array([1.0, 0.0, 1.0])
    if face_z:
        f = sk["face"]
        across = (init[f[0]] - init[f[1]]) + (init[f[2]] - init[f[3]])       # :198-201: r_hip, l_hip, sdr_r, sdr_l
        forward = _unit(_cross_y(_unit(across)))
        q = _qbetween(forward[None], np.array([[0.0, 0.0, 1.0]]), ws)
        P = _qrot(np.broadcast_to(q, P.shape[:-1] + (4,)), P)
    return P


def foot_flags(sk, P32, thre):
    """motion_process.py:47-63 on fp32 positions: fp32 squares, (x + y) + z in fp32, compared with the threshold as a double.
    Returns (flags [L-1, 4] in the order feet_l, feet_r; the fp32 sums)."""
    P32 = np.asarray(P32, dtype=np.float32)
    idx = list(sk["fid_l"]) + list(sk["fid_r"])
    d = P32[1:, idx] - P32[:-1, idx]
    s = (d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2
    assert s.dtype == np.float32
    return (s.astype(np.float64) < float(thre)).astype(np.float64), s


def extract(sk, P, thre, ws=None, bone_min=None, foot_sums=None):
    """extract_features (motion_process.py:43-170) on float64 positions [L, J, 3] -> (data [L-1, F], ric positions [L, J, 3])."""
    P = np.array(P, dtype=np.float64)
    feet, s = foot_flags(sk, P.astype(np.float32), thre)
    if foot_sums is not None:
        foot_sums.append(s)
    quat = ik(sk, P, True, ws, bone_min)
    r_rot = quat[:, 0]
    q = quat / np.sqrt((quat ** 2).sum(-1, keepdims=True))        # quaternion_to_matrix divides by |q|^2 (quaternion.py:285-302)
    r, i, j, k = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    cont6d = np.stack([1 - 2 * (j * j + k * k), 2 * (i * j + k * r), 2 * (i * k - j * r),
                       2 * (i * j - k * r), 1 - 2 * (i * i + k * k), 2 * (j * k + i * r)], axis=-1)
    velocity = _qrot(r_rot[1:], P[1:, 0] - P[:-1, 0])
    r_vel = _qmul(r_rot[1:], _qinv(r_rot[:-1]))
    local = P.copy()
    local[..., 0] -= P[:, 0:1, 0]
    local[..., 2] -= P[:, 0:1, 2]
    ric = _qrot(np.broadcast_to(r_rot[:, None], local.shape[:-1] + (4,)), local)
    local_vel = _qrot(np.broadcast_to(r_rot[:-1, None], (len(P) - 1, P.shape[1], 4)), P[1:] - P[:-1])
    L = len(P)
    data = np.concatenate([np.arcsin(r_vel[:, 2:3]), velocity[:, [0, 2]], ric[:-1, 0, 1:2], ric[:-1, 1:].reshape(L - 1, -1),
                           cont6d[:-1, 1:].reshape(L - 1, -1), local_vel.reshape(L - 1, -1), feet], axis=-1)
    return data, ric


def process(sk, P, thre, tgt=None, ws=None, bone_min=None, foot_sums=None):
    """process_file (motion_process.py:173-355): (data, global_positions, ric positions, l_velocity)."""
    G = canonicalise(sk, P, tgt, ws=ws, bone_min=bone_min)
    data, ric = extract(sk, G, thre, ws, bone_min, foot_sums)
    return data, G, ric, data[:, 1:3].copy()


def recover_from_ric(data, J):
    """recover_from_ric (motion_process.py:437-452, :366-385) on [L, F] float64."""
    ang = np.concatenate([[0.0], np.cumsum(data[:-1, 0])])
    q = np.zeros((len(data), 4))
    q[:, 0], q[:, 2] = np.cos(ang), np.sin(ang)
    v = np.zeros((len(data), 3))
    v[1:, 0], v[1:, 2] = data[:-1, 1], data[:-1, 2]
    r_pos = np.cumsum(_qrot(_qinv(q), v), axis=0)
    r_pos[:, 1] = data[:, 3]
    ric = data[:, 4:4 + 3 * (J - 1)].reshape(len(data), J - 1, 3)
    pos = _qrot(np.broadcast_to(_qinv(q)[:, None], ric.shape[:-1] + (4,)), ric)
    pos[..., 0] += r_pos[:, None, 0]
    pos[..., 2] += r_pos[:, None, 2]
    return np.concatenate([r_pos[:, None], pos], axis=1)


# ------------------------------------------------------------------------------------------------------------------ inputs
# Rest directions the synthetic pose is grown along.  HumanML3D: the raw offsets themselves.  KIT: the raw offsets put the hips and
# the shoulders on the side that process_file's face order calls the other one, so a pose grown along them faces -Z for
# process_file and is turned by 180 degrees, which leaves every x bone antiparallel to its raw offset; the four x bones therefore
# lean to the other side (at most 127 degrees from their raw offset), as a recorded KIT pose does.
REST_DIRS = {"humanml": {}, "kit": {11: (-0.5, -0.85, 0.0), 16: (0.5, -0.85, 0.0), 5: (-0.6, 0.8, 0.0), 8: (0.6, 0.8, 0.0)}}
BASE_LEN = {"humanml": {1: 0.10, 2: 0.10, 13: 0.19, 14: 0.19}, "kit": {11: 0.10, 16: 0.10, 5: 0.24, 8: 0.24}}


def _roty(a, v):
    c, s = np.cos(a)[..., None], np.sin(a)[..., None]
    return np.concatenate([c * v[..., 0:1] + s * v[..., 2:3], v[..., 1:2], -s * v[..., 0:1] + c * v[..., 2:3]], axis=-1)


def bone_lengths(dataset, rng):
    sk = SKELETONS[dataset]
    base = np.full(sk["joints"], 0.16)
    for j, v in BASE_LEN[dataset].items():
        base[j] = v
    return base * rng.uniform(0.9, 1.1, sk["joints"])


def target_offsets(dataset, seed=77):
    """A target skeleton for the retargeting pass: what Skeleton.get_offsets_joints returns, bone length times raw offset."""
    sk = SKELETONS[dataset]
    rng = np.random.default_rng(seed)
    return (bone_lengths(dataset, rng)[:, None] * 1.15 * np.asarray(sk["raw"], dtype=np.float64)).astype(np.float32)


def raw_clip(dataset, T, seed):
    sk = SKELETONS[dataset]
    J = sk["joints"]
    rng = np.random.default_rng(seed)
    lens = bone_lengths(dataset, rng)
    dirs = np.asarray(sk["raw"], dtype=np.float64)
    for j, d in REST_DIRS[dataset].items():
        dirs[j] = np.asarray(d) / np.linalg.norm(d)
    t = np.arange(T, dtype=np.float64)
    yaw = 0.7 * np.sin(2 * np.pi * t / 150.0 + rng.uniform(0, 6.28)) + 0.25 * np.sin(2 * np.pi * t / 37.0 + rng.uniform(0, 6.28))
    amp, freq, ph = rng.uniform(0.1, 0.3, (J, 3)), rng.uniform(0.01, 0.06, (J, 3)), rng.uniform(0, 6.28, (J, 3))
    P = np.zeros((T, J, 3))
    P[:, 0] = np.stack([0.02 * t * np.cos(0.3 + 0.01 * t) + 0.3, 0.95 + 0.03 * np.sin(0.21 * t), 0.015 * t + 0.1 * np.sin(0.05 * t) - 0.2], -1)
    for ch in sk["chains"]:
        for i in range(1, len(ch)):
            c = ch[i]
            d = _unit(dirs[c][None] + amp[c] * np.sin(2 * np.pi * freq[c] * t[:, None] + ph[c]))
            P[:, c] = P[:, ch[i - 1]] + lens[c] * _roty(yaw, d)
    return P.astype(np.float32)


def check_conditions(dataset, P32, thre, tgt=None, canon=False, foot=True):
    """The conditions of the module docstring for one clip; returns what was measured."""
    sk = SKELETONS[dataset]
    ws, bone_min, sums = [], [], []
    P = np.asarray(P32, dtype=np.float64)
    if canon or tgt is not None:
        process(sk, P, thre, tgt, ws, bone_min, sums)
    else:
        extract(sk, P, thre, ws, bone_min, sums)
    rel = np.abs(sums[0].astype(np.float64) - thre) / thre
    got = {"w_min": min(ws), "bone_min": min(bone_min), "foot_margin": float(rel.min())}
    assert got["w_min"] >= W_MIN, got
    assert got["bone_min"] > 1e-3, got
    if foot:
        assert got["foot_margin"] >= FOOT_MARGIN, got
    return got


def make_clip(dataset, T, seed, tgt=None, canon=False):
    """An ordinary clip: the first of up to 20 seeds from `seed` whose clip meets the conditions."""
    thre = SKELETONS[dataset]["feet_thre"]
    last = None
    for k in range(20):
        P = raw_clip(dataset, T, seed + 1000 * k)
        try:
            check_conditions(dataset, P, thre, tgt, canon)
            return P
        except AssertionError as e:
            last = e
    raise AssertionError(f"no clip of {dataset} T={T} seed={seed} meets the yardstick conditions: {last}")


def adversarial_foot_clip(dataset, T=26, seed=5):
    """fp32 displacements of the four foot joints whose (dx^2 + dy^2) + dz^2, in fp32, is the fp32 number nearest the threshold,
    its lower and its upper neighbour.  A foot joint sits at c_j on even frames and at c_j + e on odd ones, c_j and e on a 2^-24
    grid inside (-1, 1), so that both the positions and their differences are exact in fp32."""
    sk = SKELETONS[dataset]
    thre = sk["feet_thre"]
    rng = np.random.default_rng(seed)
    P = raw_clip(dataset, T, seed + 31).astype(np.float64)
    P[:, :, 0] -= P[:, 0:1, 0]                       # root above the origin, so that the legs reach the planted feet
    P[:, :, 2] -= P[:, 0:1, 2]
    P = P.astype(np.float32)
    centre = np.float32(thre)
    targets = [centre, np.nextafter(centre, np.float32(0)), np.nextafter(centre, np.float32(1))]
    ankle_toe = {"humanml": ((8, 11), (7, 10)), "kit": ((14, 15), (19, 20))}[dataset]      # the -x leg, the +x leg of raw_clip's pose
    grid = 2.0 ** -24
    k = 0
    for (a, b), side in zip(ankle_toe, (-1.0, 1.0)):
        for joint, c in ((a, (0.0625 * side, 0.0625, 0.0)), (b, (0.0625 * side, 0.03125, 0.15625))):
            c = np.asarray(c, dtype=np.float32)
            for t in range(T):
                P[t, joint] = c
            for t in range(1, T, 2):
                target = targets[k % 3]
                k += 1
                r = np.sqrt(float(target))
                for _ in range(200):
                    u = rng.normal(size=(20000, 3))
                    e = (np.round(u / np.linalg.norm(u, axis=1, keepdims=True) * r / grid + rng.uniform(-8, 8, (20000, 3))) * grid).astype(np.float32)
                    ss = (e[:, 0] ** 2 + e[:, 1] ** 2) + e[:, 2] ** 2
                    hit = np.nonzero((ss == target) & (np.abs(e).max(axis=1) < 0.7 * r))[0]
                    if len(hit):
                        P[t, joint] = c + e[hit[0]]
                        assert np.array_equal((P[t, joint] - c), e[hit[0]])
                        break
                else:
                    raise AssertionError("no displacement found for the adversarial foot case")
    check_conditions(dataset, P, thre, foot=False)
    _, sums = foot_flags(sk, P, thre)
    for target in targets:
        assert (sums == target).sum() >= 4, "every target is hit on several joints"
    return P


# ------------------------------------------------------------------------------------------------------------------ cases
T_LIST = (2, 3, 4, 41, 81, 82, 162, 197, 257, 258)
EMU_T = (2, 4, 82, 258)
RAGGED_T, RAGGED_LENGTHS = 197, (197, 2, 60)
STORE_ORACLE_MAX_T = 82             # fixtures of longer clips hold the joints and the reference's output only


def case_names():
    """name -> dict(kind, dataset, T): every fixture of tests/golden/motion_features_<name>.npz."""
    cases = {}
    for ds in ("humanml", "kit"):
        for T in T_LIST:
            cases[f"{ds}_T{T}"] = dict(kind="extract", dataset=ds, T=T)
        cases[f"{ds}_process"] = dict(kind="process", dataset=ds, T=64 if ds == "humanml" else 47, tgt=False)
        cases[f"{ds}_retarget"] = dict(kind="process", dataset=ds, T=64 if ds == "humanml" else 47, tgt=True)
        cases[f"{ds}_foot"] = dict(kind="foot", dataset=ds, T=26)
    cases["humanml_ragged"] = dict(kind="ragged", dataset="humanml", T=RAGGED_T)
    return cases


def case_input(name):
    """The fp32 joints [T, J, 3] ([B, T, J, 3] with NaN beyond each length for the ragged batch) and the target offsets or None."""
    c = case_names()[name]
    ds, T = c["dataset"], c["T"]
    seed = 100 + 7 * T + (0 if ds == "humanml" else 3)
    if c["kind"] == "extract":
        return make_clip(ds, T, seed), None
    if c["kind"] == "process":
        tgt = target_offsets(ds) if c["tgt"] else None
        return make_clip(ds, T, seed + 1, tgt, canon=True), tgt
    if c["kind"] == "foot":
        return adversarial_foot_clip(ds, T), None
    clips = np.full((len(RAGGED_LENGTHS), T, SKELETONS[ds]["joints"], 3), np.nan, dtype=np.float32)
    for b, L in enumerate(RAGGED_LENGTHS):
        clips[b, :L] = make_clip(ds, L, seed + 11 * b)
    return clips, None


def oracle_case(name, joints, tgt):
    """The oracle's outputs of a case: dict of arrays (data [T-1, F]; for process cases also global / ric positions)."""
    c = case_names()[name]
    sk = SKELETONS[c["dataset"]]
    thre = sk["feet_thre"]
    if c["kind"] == "process":
        data, G, ric, lv = process(sk, joints, thre, tgt)
        return {"fp64_data": data, "fp64_global": G, "fp64_ric": ric, "fp64_l_velocity": lv}
    if c["kind"] == "ragged":
        out = np.zeros((joints.shape[0], joints.shape[1] - 1, feat_dim(sk["joints"])))
        for b, L in enumerate(RAGGED_LENGTHS):
            out[b, :L - 1] = extract(sk, joints[b, :L], thre)[0]
        return {"fp64_data": out}
    return {"fp64_data": extract(sk, joints, thre)[0]}


def load_case(name):
    """The fixture of a case; the oracle's outputs (`fp64_*`) are recomputed where the file does not hold them."""
    with np.load(os.path.join(GOLDEN, f"motion_features_{name}.npz")) as z:
        d = {k: z[k] for k in z.files}
    if "fp64_data" not in d:
        d.update(oracle_case(name, d["joints"], d.get("tgt_offsets")))
    return d


def pin_report():
    with open(PIN_REPORT) as fh:
        return json.load(fh)


def oracle_tol(group_values):
    """Device against oracle, one feature group: see BOUNDS in the module docstring."""
    return 4.0 * 2.0 ** -24 * max(float(np.abs(group_values).max()), 1e-30)


def group_errors(got, want, J):
    """max|got - want| per feature group over [.., F] arrays."""
    return {g: float(np.abs(np.asarray(got, dtype=np.float64)[..., s] - np.asarray(want, dtype=np.float64)[..., s]).max())
            for g, s in groups(J).items()}


def to_bj3t(P):
    """[T, J, 3] or [B, T, J, 3] -> [B, J, 3, T] float32, the layout recover_from_ric emits."""
    P = np.asarray(P, dtype=np.float32)
    if P.ndim == 3:
        P = P[None]
    return np.ascontiguousarray(P.transpose(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------------------------------ shared checks
def run_case(name, d, device, lib=None):
    """A fixture through mdm_amd.motion_process on `device` (`lib`: the emulated library): {'data': [.., T-1, F] float32 numpy, and for
    the process cases 'global', 'ric' [T, J, 3] and 'l_velocity'}."""
    import torch
    from mdm_amd import motion_process as mp
    c = case_names()[name]
    sk = SKELETONS[c["dataset"]]
    if c["kind"] == "process":
        got = mp.process_file(torch.from_numpy(d["joints"]).to(device), sk["feet_thre"], d.get("tgt_offsets"), c["dataset"], _native_lib=lib)
        return dict(zip(("data", "global", "ric", "l_velocity"), (g.cpu().numpy() for g in got)))
    x = torch.from_numpy(to_bj3t(d["joints"])).to(device)
    out = mp.joints_to_features(x, lengths=d.get("lengths"), dataset=c["dataset"], canonicalise=False, _native_lib=lib)
    out = out[:, :, 0].permute(0, 2, 1).cpu().numpy()
    return {"data": out if c["kind"] == "ragged" else out[0]}


def check_case(name, d, got, report):
    """The bounds of the module docstring for one case; prints every figure before it asserts."""
    c = case_names()[name]
    J = SKELETONS[c["dataset"]]["joints"]
    g = groups(J)
    data = got["data"]
    assert data.shape == d["fp64_data"].shape and np.isfinite(data).all(), (name, data.shape)
    e_orc = group_errors(data, d["fp64_data"], J)
    tol = {k: oracle_tol(d["fp64_data"][..., s]) for k, s in g.items() if k != "feet"}
    line = f"[motion_features] {name}: vs oracle " + " ".join(f"{k}={e_orc[k]:.2e}/{tol[k]:.2e}" for k in tol)
    e_ref, d_ref = None, report["cases"][name].get("d_ref")
    if d_ref is not None:
        e_ref = group_errors(data, d["ref_data"], J)
        line += "  vs reference " + " ".join(f"{k}={e_ref[k]:.2e}/{2 * d_ref[k]:.2e}" for k in d_ref)
    feet_bad = int((data[..., g["feet"]] != d["fp64_data"][..., g["feet"]]).sum())
    print(line + f"  foot mismatches {feet_bad}", flush=True)
    assert feet_bad == 0, (name, feet_bad)
    if "ref_data" in d:
        assert np.array_equal(data[..., g["feet"]], d["ref_data"][..., g["feet"]]), name
    for k in tol:
        assert e_orc[k] <= tol[k], (name, k, e_orc[k], tol[k])
        if d_ref is not None:
            assert e_ref[k] <= 2.0 * d_ref[k], (name, k, e_ref[k], d_ref[k])
    if c["kind"] == "process":
        for key, want in (("global", d["fp64_global"]), ("ric", d["fp64_ric"])):
            err, bound = float(np.abs(got[key] - want).max()), oracle_tol(want)
            print(f"[motion_features] {name}: {key} positions vs oracle {err:.2e}/{bound:.2e}", flush=True)
            assert err <= bound, (name, key, err, bound)
        assert np.array_equal(got["l_velocity"], data[:, 1:3])
    if c["kind"] == "ragged":
        for b, L in enumerate(d["lengths"]):
            assert not data[b, L - 1:].any(), (name, b)       # exact zeros from frame L - 1 on
