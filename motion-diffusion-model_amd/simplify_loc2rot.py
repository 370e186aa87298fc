"""`joints2smpl` -- the reference's SMPLify step (visualize/simplify_loc2rot.py over visualize/joints2smpl/src/{smplify,customloss,
prior,config}.py) on the MI355X HIP path: generated xyz joints [T, 22, 3] -> SMPL rotations, the `thetas` [1, 25, 6, T] that
`mdm_amd.smpl_mesh.Rotation2xyzFull(..., jointstype='vertices')` turns into a mesh (visualize/vis_utils.py:24-39).

One C-ABI call (mdm_smplify_fit, csrc/smplify.h): the two fitting losses and their analytic gradients in one launch per closure
evaluation over all frames, the vector updates of torch.optim.LBFGS on the device and its strong-Wolfe control flow on the host.  The
losses read the 24 skeleton joints only: no vertex is computed, and `smplx` is not a dependency.  No CPU fallback.

What is restated from the reference, quirks included: `use_lbfgs=True`, `use_collision=False`, `joints_category="AMASS"`, betas per
frame (`seq_ind = 0`), the camera loss's depth term counted four times, `'pose'` of the returned dictionary = the 24 fitted model
JOINTS of frame 0, flattened (simplify_loc2rot.py:114), not a pose.
"""
import os
import pickle

import numpy as np
import torch

from . import _native as nat
from ._native_model import NativeModelMixin
from .rotation2xyz import SMPL_MODEL_PATH
from .smpl_mesh import load_smpl_model

GMM_MODEL_DIR = "./visualize/joints2smpl/smpl_models/"                                     # joints2smpl/src/config.py:37-38
GMM_PATH = os.path.join(GMM_MODEL_DIR, "gmm_08.pkl")
SMPL_MEAN_FILE = os.path.join(GMM_MODEL_DIR, "neutral_smpl_mean_params.h5")
NUM_JOINTS = 22                                                                            # HumanML3D
NUM_GAUSSIANS, POSE_DIM = 8, 69
FOOT_JOINTS = (7, 8, 10, 11)

_PREPARED = {}      # (files and their stamps, device) -> the prepared tables on that device


def prepare_gmm(gmm):
    """MaxMixturePrior.__init__ (prior.py:126-159) on the dictionary of gmm_08.pkl: means and precisions in float32 -- the covariances
    are cast to float32 and inverted in float32 -- and nll_weights computed in float64 from the unrounded covariances, then cast.
    Returns float32 arrays means [8, 69], precisions [8, 69, 69], nll_weights [1, 8] and -log(nll_weights) [8] (torch's float32 log,
    as merged_log_likelihood takes it)."""
    for k in ("means", "covars", "weights"):
        if k not in gmm:
            raise ValueError(f"mixture prior: no {k!r} entry")
    means64, covs64, w64 = (np.asarray(gmm[k]) for k in ("means", "covars", "weights"))
    if means64.shape != (NUM_GAUSSIANS, POSE_DIM) or covs64.shape != (NUM_GAUSSIANS, POSE_DIM, POSE_DIM) or w64.shape != (NUM_GAUSSIANS,):
        raise ValueError(f"mixture prior: expected means [{NUM_GAUSSIANS}, {POSE_DIM}], covars [{NUM_GAUSSIANS}, {POSE_DIM}, {POSE_DIM}] "
                         f"and weights [{NUM_GAUSSIANS}], got {means64.shape}, {covs64.shape}, {w64.shape}")
    means = means64.astype(np.float32)
    covs = covs64.astype(np.float32)
    precisions = np.stack([np.linalg.inv(cov) for cov in covs]).astype(np.float32)
    sqrdets = np.array([np.sqrt(np.linalg.det(c)) for c in covs64])
    const = (2 * np.pi) ** (69 / 2.)
    nll_weights = torch.tensor(np.asarray(w64 / (const * (sqrdets / sqrdets.min()))), dtype=torch.float32).unsqueeze(dim=0)
    neg_log = (-torch.log(nll_weights))[0].numpy()
    return dict(means=means, precisions=precisions, nll_weights=nll_weights.numpy(), neg_log_nll_weights=np.ascontiguousarray(neg_log))


def load_gmm(path=GMM_PATH):
    if not os.path.isfile(path):
        raise FileNotFoundError(f"mixture prior file {path} not found (relative to {os.getcwd()}): joints2smpl needs gmm_08.pkl, which "
                                f"the reference's prepare/download_smpl_files.sh puts under {GMM_MODEL_DIR}")
    with open(path, "rb") as f:
        gmm = pickle.load(f, encoding="latin1")
    if not isinstance(gmm, dict):
        raise ValueError(f"{path}: expected a dict with 'means', 'covars' and 'weights', got {type(gmm).__name__}")
    try:
        return prepare_gmm(gmm)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None


def load_mean_params(path=SMPL_MEAN_FILE):
    """(pose [72], shape [10]) of neutral_smpl_mean_params.h5 (simplify_loc2rot.py:29-33), through h5py."""
    hint = "pass mean_params=(pose[72], shape[10]) instead"
    try:
        import h5py
    except ImportError:
        raise ImportError(f"reading {path} needs h5py, which is not installed: {hint}") from None
    if not os.path.isfile(path):
        raise FileNotFoundError(f"mean-parameter file {path} not found (relative to {os.getcwd()}): {hint}")
    with h5py.File(path, "r") as f:
        return np.asarray(f["pose"][:]), np.asarray(f["shape"][:])


def _stamp(path):
    st = os.stat(path)
    return (os.path.abspath(path), st.st_mtime_ns, st.st_size)


class joints2smpl(NativeModelMixin):
    """visualize/simplify_loc2rot.py:13-114 with the reference's constructor and methods.  Keyword-only extras: where the SMPL model and
    the mixture prior are read from, `mean_params=(pose[72], shape[10])` in place of neutral_smpl_mean_params.h5,
    `num_smplify_iters` (150) and `fix_foot` (False: confidence 1.5 on the ankles and feet).  The prepared tables are cached per
    (files, device).  `last_stats` holds the last fit's function evaluations, iterations and final loss per step."""

    def __init__(self, num_frames, device_id, cuda=True, *, smpl_model_path=SMPL_MODEL_PATH, gmm_path=GMM_PATH, mean_params=None,
                 mean_params_path=SMPL_MEAN_FILE, num_smplify_iters=150, fix_foot=False, _native_lib=None, _call_overrides=None):
        self.device = torch.device("cuda:" + str(device_id) if cuda else "cpu")
        self.batch_size = int(num_frames)
        self.num_joints = NUM_JOINTS
        self.joint_category = "AMASS"
        self.num_smplify_iters = int(num_smplify_iters)
        self.fix_foot = fix_foot
        self.smpl_model_path, self.gmm_path = smpl_model_path, gmm_path
        self._native_lib = _native_lib
        self._call_overrides = dict(_call_overrides or {})
        self._ws = {}
        if self.batch_size < 1:
            raise ValueError(f"num_frames must be at least 1, got {num_frames}")
        pose, shape = load_mean_params(mean_params_path) if mean_params is None else mean_params
        pose, shape = np.asarray(pose, np.float32).reshape(-1), np.asarray(shape, np.float32).reshape(-1)
        if pose.shape != (72,) or shape.shape != (10,):
            raise ValueError(f"mean_params must be (pose[72], shape[10]), got {pose.shape} and {shape.shape}")
        self.init_mean_pose = torch.from_numpy(pose).unsqueeze(0).repeat(self.batch_size, 1).to(self.device)
        self.init_mean_shape = torch.from_numpy(shape).unsqueeze(0).repeat(self.batch_size, 1).to(self.device)
        self.cam_trans_zero = torch.zeros(1, 3, device=self.device)
        self.last_stats = None
        self._native_version()          # both files are looked at now, as the reference's constructor does

    # ---- the prepared model ----------------------------------------------------------------------------------------------------
    def _native_version(self):
        if not os.path.isfile(self.gmm_path):
            load_gmm(self.gmm_path)     # raises, naming the file
        if not os.path.isfile(self.smpl_model_path):
            load_smpl_model(self.smpl_model_path)
        return (_stamp(self.smpl_model_path), _stamp(self.gmm_path), str(self.device))

    def _build_native(self, keep):
        key = self._native_version()
        if key not in _PREPARED:
            m = load_smpl_model(self.smpl_model_path)
            if m["J_regressor"].shape[0] != 24:
                raise ValueError(f"{self.smpl_model_path}: the fit needs SMPL's 24 joints, the model has {m['J_regressor'].shape[0]}")
            g = load_gmm(self.gmm_path)
            host = dict(j0=(m["J_regressor"] @ m["v_template"]).astype(np.float32),                       # folded in float64
                        jdirs=np.einsum("jv,vcl->jcl", m["J_regressor"], m["shapedirs"]).astype(np.float32),
                        means=g["means"], precisions=g["precisions"], neg_log_nll_weights=g["neg_log_nll_weights"])
            if len(_PREPARED) >= 8:
                _PREPARED.clear()
            _PREPARED[key] = ({k: torch.from_numpy(np.ascontiguousarray(v)).to(self.device) for k, v in host.items()},
                              np.ascontiguousarray(m["parents"], dtype=np.int32))
        dev, parents = _PREPARED[key]
        keep.extend([dev, parents])
        return nat.MdmSmplifyModel(parents=parents.ctypes.data_as(nat.C.POINTER(nat.C.c_int32)), **{k: v.data_ptr() for k, v in dev.items()})

    def _call(self):
        return nat.MdmSmplifyCall(**dict(dict(num_iters=self.num_smplify_iters), **self._call_overrides))

    # ---- the reference's methods -----------------------------------------------------------------------------------------------
    def npy2smpl(self, npy_path):
        out_path = npy_path.replace(".npy", "_rot.npy")
        motions = np.load(npy_path, allow_pickle=True)[None][0]
        n_samples = motions["motion"].shape[0]
        all_thetas = []
        for sample_i in range(n_samples):
            thetas, _ = self.joint2smpl(motions["motion"][sample_i].transpose(2, 0, 1))      # [nframes, njoints, 3]
            all_thetas.append(thetas.cpu().numpy())
        motions["motion"] = np.concatenate(all_thetas, axis=0)
        print("motions", motions["motion"].shape)
        print(f"Saving [{out_path}]")
        np.save(out_path, motions)
        exit()

    def joint2smpl(self, input_joints, init_params=None):
        T = self.batch_size
        keypoints_3d = torch.as_tensor(np.asarray(input_joints) if not torch.is_tensor(input_joints) else input_joints)
        keypoints_3d = keypoints_3d.to(device=self.device, dtype=torch.float32).contiguous()
        if keypoints_3d.dim() != 3 or tuple(keypoints_3d.shape) != (T, self.num_joints, 3):
            raise ValueError(f"input_joints must be [num_frames, {self.num_joints}, 3] = {(T, self.num_joints, 3)}, got "
                             f"{tuple(keypoints_3d.shape)}")
        if init_params is None:
            pred_betas, pred_pose = self.init_mean_shape, self.init_mean_pose
        else:       # (init_params['cam'] is read by the reference and then replaced by guess_init_3d)
            pred_betas = torch.as_tensor(init_params["betas"]).to(device=self.device, dtype=torch.float32).reshape(-1, 10)
            pred_pose = torch.as_tensor(init_params["pose"]).to(device=self.device, dtype=torch.float32).reshape(-1, 72)
            pred_betas, pred_pose = pred_betas.expand(T, 10), pred_pose.expand(T, 72)
        pred_betas, pred_pose = pred_betas.contiguous(), pred_pose.contiguous()
        confidence_input = torch.ones(self.num_joints)
        if self.fix_foot:
            confidence_input[list(FOOT_JOINTS)] = 1.5
        conf = confidence_input.to(self.device)

        lib = self._lib()
        stream = self._stream(lib, keypoints_3d, "the joints")
        model, call = self._model(), self._call()
        ws, nbytes = self._workspace("mdm_smplify_workspace_bytes", model, call, T, dev=self.device)
        dev = self.device
        pose = torch.empty(T, 72, dtype=torch.float32, device=dev)
        betas = torch.empty(T, 10, dtype=torch.float32, device=dev)
        cam = torch.empty(T, 1, 3, dtype=torch.float32, device=dev)
        joints = torch.empty(T, 24, 3, dtype=torch.float32, device=dev)
        thetas = torch.empty(1, 25, 6, T, dtype=torch.float32, device=dev)
        stats = (nat.C.c_double * 6)()
        lib.check(lib.mdm_smplify_fit(nat.C.byref(model), nat.C.byref(call), pred_pose.data_ptr(), pred_betas.data_ptr(),
                                      keypoints_3d.data_ptr(), conf.data_ptr(), T, pose.data_ptr(), betas.data_ptr(), cam.data_ptr(),
                                      joints.data_ptr(), thetas.data_ptr(), stats, ws.data_ptr(), nbytes, stream), "mdm_smplify_fit")
        self.last_stats = dict(stage1=dict(func_evals=int(stats[0]), n_iter=int(stats[1]), loss=stats[2]),
                               stage2=dict(func_evals=int(stats[3]), n_iter=int(stats[4]), loss=stats[5]))
        self.last_fit = dict(pose=pose, joints=joints)
        return thetas, {"pose": joints[0, :24].flatten().clone(), "betas": betas, "cam": cam}
