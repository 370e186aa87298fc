"""ctypes binding of libmdm_hip.so (C ABI: include/mdm_hip.h).

The product path REQUIRES the HIP library: `load_native()` raises if it is missing -- there is no CPU
or eager-PyTorch fallback.  (tests/emu builds a CPU emulation of the same sources purely as test
infrastructure and points `MdmLib` at it explicitly.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libmdm_hip.so"
LIB_PATH = os.path.join(_HERE, "csrc", LIB_NAME)
PROBE_LIB_PATH = os.path.join(_HERE, "csrc", "libmdm_hip_probe.so")   # -DMDM_PROBES build: tools/ and probe-only tests

MDM_OK = 0
BRANCH_COND, BRANCH_UNCOND, BRANCH_BOTH = 0, 1, 2
ACT_NONE, ACT_GELU, ACT_SILU = 0, 1, 2
PRECISIONS = {"f32": 0, "f16x3": 1}
PROF_CLASSES = ("linear", "attention", "layernorm", "embed", "outproj", "elementwise")

EXPORTED_SYMBOLS = [
    "mdm_abi_version", "mdm_build_info", "mdm_last_error", "mdm_create", "mdm_destroy", "mdm_set_weight", "mdm_const_bytes",
    "mdm_prepare", "mdm_workspace_bytes", "mdm_forward", "mdm_sampler_step", "mdm_randn", "mdm_sample_loop",
    "mdm_linear", "mdm_layernorm", "mdm_attention", "mdm_profile_enable", "mdm_profile_read", "mdm_profile_reset",
    "mdm_set_precision", "mdm_linear_x3", "mdm_linear_x3_scratch_bytes", "mdm_attention_x3", "mdm_attention_x3_scratch_bytes",
    "mdm_recover_from_ric", "mdm_workspace_bytes_dec", "mdm_forward_dec", "mdm_workspace_bytes_dec_loop",
    "mdm_sample_loop_dec", "mdm_weights_in_range", "mdm_set_option", "mdm_get_option", "mdm_set_time_add",
    "mdm_rot6d_to_smpl_joints", "mdm_smpl_workspace_bytes", "mdm_smpl_forward",
    "mdm_eval_workspace_bytes", "mdm_eval_motion_embeddings", "mdm_eval_text_embeddings",
    "mdm_text_workspace_bytes", "mdm_text_encode",
    "mdm_stgcn_workspace_bytes", "mdm_stgcn_forward",
    "mdm_gru_cls_workspace_bytes", "mdm_gru_cls_forward",
    "mdm_clip_text_workspace_bytes", "mdm_clip_text_encode",
    "mdm_metrics_workspace_bytes", "mdm_knn_radius", "mdm_manifold_members", "mdm_gather_dist", "mdm_poly_mmd", "mdm_feature_stats",
    "mdm_retrieval_ranks", "mdm_dist_matrix", "mdm_confusion",
    "mdm_frechet_workspace_bytes", "mdm_frechet_distance",
    "mdm_smplify_workspace_bytes", "mdm_smplify_value_grad", "mdm_smplify_fit", "mdm_smplify_strong_wolfe",
    "mdm_joints_to_features_workspace_bytes", "mdm_joints_to_features",
]
# include/mdm_hip_probe.h: exported by the probe build only
PROBE_SYMBOLS = ["mdm_debug_set", "mdm_debug_get", "mdm_linear_f16f6", "mdm_linear_f16f6_scratch_bytes", "mdm_probe_in_proj",
                 "mdm_probe_attention_x3"]
ABI_VERSION = 10
# include/mdm_hip.h MDM_OPT_*: per-handle run-time options (the library reads no environment variable)
OPTIONS = {"small_gemm_max_seqs": 1, "small_gemm_row_tiles": 2, "dec_fused_xattn": 3, "dec_fused_selfattn": 4, "attn_direct_out": 5,
           "dec_time_token": 6, "enc_shared_layer0": 7, "attn_wide": 8}
ARCH = {"trans_enc": 0, "trans_dec": 1}


class MdmConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("njoints", "nfeats", "latent_dim", "ff_size", "num_layers", "num_heads",
                                         "clip_dim", "max_len", "mask_frames", "arch", "context_len")]


class MdmSmplModel(C.Structure):
    """include/mdm_hip.h mdm_smpl_model_t: device pointers of the prepared SMPL tables (parents: host)."""
    _fields_ = [(n, C.c_void_p) for n in ("j0", "jdirs", "blend", "weights_t", "sel_blend", "sel_weights_t", "extra_t")] + \
               [("parents", C.POINTER(C.c_int32))] + [(n, C.c_int32) for n in ("J", "V", "n_sel", "n_extra")]


class MdmSmplCall(C.Structure):
    """include/mdm_hip.h mdm_smpl_call_t."""
    _fields_ = [(n, C.c_int32) for n in ("pose_rep", "glob", "translation", "vertstrans", "n_points", "root_point")] + \
               [("point_map", C.POINTER(C.c_int32)), ("glob_rot_mat", C.POINTER(C.c_float)), ("beta1", C.c_float)]


class MdmEvalGru(C.Structure):
    """include/mdm_hip.h mdm_eval_gru_t: one BiGRU encoder (input_emb, gru, output_net) of the evaluator."""
    _fields_ = [(n, C.c_void_p) for n in ("in_w", "in_b", "w_ih", "b_ih", "w_hh", "b_hh", "h0", "o1_w", "o1_b", "ln_g", "ln_b",
                                          "o2_w", "o2_b")] + [(n, C.c_int32) for n in ("in_dim", "hidden", "out")]


class MdmEvalModel(C.Structure):
    """include/mdm_hip.h mdm_eval_model_t."""
    _fields_ = [(n, C.c_void_p) for n in ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "out_w", "out_b", "pos_w", "pos_b")] + \
               [("motion", MdmEvalGru), ("text", MdmEvalGru)] + \
               [(n, C.c_int32) for n in ("dim_pose", "conv_hidden", "latent", "word", "pos", "unit_length")]


class MdmTextLayer(C.Structure):
    """include/mdm_hip.h mdm_text_layer_t: one DistilBERT layer (q | k | v stacked, the q rows pre-scaled by 1/8)."""
    _fields_ = [(n, C.c_void_p) for n in ("qkv_w", "qkv_b", "out_w", "out_b", "sa_ln_g", "sa_ln_b", "lin1_w", "lin1_b", "lin2_w",
                                          "lin2_b", "out_ln_g", "out_ln_b")]


class MdmTextModel(C.Structure):
    """include/mdm_hip.h mdm_text_model_t."""
    _fields_ = [(n, C.c_void_p) for n in ("word_emb", "pos_emb", "emb_ln_g", "emb_ln_b")] + [("layers", C.POINTER(MdmTextLayer))] + \
               [(n, C.c_int32) for n in ("n_layers", "dim", "n_heads", "hidden", "vocab", "max_pos")] + [("ln_eps", C.c_float)]


class MdmStgcnBlock(C.Structure):
    """include/mdm_hip.h mdm_stgcn_block_t: one st_gcn block (graph convolution with its neighbour lists, temporal convolution, residual)."""
    _fields_ = [(n, C.c_void_p) for n in ("gcn_w", "gcn_scale", "gcn_shift", "nbr_idx", "nbr_w", "nbr_cnt", "tcn_w", "tcn_scale",
                                          "tcn_shift", "res_w", "res_scale", "res_shift")] + \
               [(n, C.c_int32) for n in ("c_in", "c_out", "stride", "residual")]


class MdmStgcnModel(C.Structure):
    """include/mdm_hip.h mdm_stgcn_model_t."""
    _fields_ = [("blocks", C.POINTER(MdmStgcnBlock))] + [(n, C.c_void_p) for n in ("in_scale", "in_shift", "fcn_w", "fcn_b")] + \
               [(n, C.c_int32) for n in ("n_blocks", "V", "K", "num_class")]


class MdmGruClsLayer(C.Structure):
    """include/mdm_hip.h mdm_gru_cls_layer_t: one nn.GRU layer in PyTorch's layouts (gates r | z | n)."""
    _fields_ = [(n, C.c_void_p) for n in ("w_ih", "w_hh", "b_ih", "b_hh")]


GRU_CLS_MAX_LAYERS = 4      # MDM_GRU_CLS_MAX_LAYERS


class MdmGruClsModel(C.Structure):
    """include/mdm_hip.h mdm_gru_cls_model_t."""
    _fields_ = [("layers", MdmGruClsLayer * GRU_CLS_MAX_LAYERS)] + [(n, C.c_void_p) for n in ("lin1_w", "lin1_b", "lin2_w", "lin2_b")] + \
               [(n, C.c_int32) for n in ("input_size", "hidden_size", "num_layers", "mid", "num_class")]


class MdmClipTextLayer(C.Structure):
    """include/mdm_hip.h mdm_clip_text_layer_t: one residual block of CLIP's text tower (in_proj stacked q | k | v, the q rows pre-scaled by 1/8)."""
    _fields_ = [(n, C.c_void_p) for n in ("ln1_g", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_g", "ln2_b", "fc_w", "fc_b", "proj_w",
                                          "proj_b")]


class MdmClipTextModel(C.Structure):
    """include/mdm_hip.h mdm_clip_text_model_t."""
    _fields_ = [(n, C.c_void_p) for n in ("tok_emb", "pos_emb", "lnf_g", "lnf_b", "text_proj")] + [("layers", C.POINTER(MdmClipTextLayer))] + \
               [(n, C.c_int32) for n in ("n_layers", "dim", "n_heads", "mlp", "vocab", "max_pos", "embed")]


class MdmSmplifyModel(C.Structure):
    """include/mdm_hip.h mdm_smplify_model_t: device pointers of the rest-joint tables and the mixture prior (parents: host)."""
    _fields_ = [(n, C.c_void_p) for n in ("j0", "jdirs", "means", "precisions", "neg_log_nll_weights")] + [("parents", C.POINTER(C.c_int32))]


class MdmSmplifyCall(C.Structure):
    """include/mdm_hip.h mdm_smplify_call_t; the defaults are SMPLify3D's as simplify_loc2rot.py constructs it."""
    _fields_ = [(n, C.c_int32) for n in ("num_iters", "history", "stage1_calls", "stage2_calls")] + \
               [(n, C.c_double) for n in ("step_size", "tolerance_grad", "tolerance_change", "joint_weight", "sigma", "pose_prior_weight",
                                          "angle_prior_weight", "shape_prior_weight", "pose_preserve_weight", "depth_weight")]

    def __init__(self, num_iters=150, history=100, stage1_calls=10, stage2_calls=None, **over):
        kw = dict(step_size=1e-2, tolerance_grad=1e-7, tolerance_change=1e-9, joint_weight=600.0, sigma=100.0,
                  pose_prior_weight=4.78 * 1.5, angle_prior_weight=15.2, shape_prior_weight=5.0, pose_preserve_weight=5.0,
                  depth_weight=100.0)
        kw.update(over)
        super().__init__(num_iters=num_iters, history=history, stage1_calls=stage1_calls,
                         stage2_calls=num_iters if stage2_calls is None else stage2_calls, **kw)


SKEL_MAX_JOINTS, SKEL_MAX_CHAINS, SKEL_MAX_CHAIN_LEN = 22, 8, 8      # MDM_SKEL_MAX_*
J2F_LAYOUTS = {"bj3t": 0, "btj3": 1}      # MDM_J2F_LAYOUT_*
J2F_MAX_FRAMES = 1024       # csrc/motion_features.h kMfMaxT


class MdmSkeleton(C.Structure):
    """include/mdm_hip.h mdm_skeleton_t: the skeleton tables of mdm_joints_to_features (host data)."""
    _fields_ = [("joints", C.c_int32), ("n_chains", C.c_int32), ("chain_len", C.c_int32 * SKEL_MAX_CHAINS),
                ("chains", (C.c_int32 * SKEL_MAX_CHAIN_LEN) * SKEL_MAX_CHAINS), ("raw_offsets", (C.c_float * 3) * SKEL_MAX_JOINTS),
                ("face_joints", C.c_int32 * 4), ("fid_r", C.c_int32 * 2), ("fid_l", C.c_int32 * 2), ("l_idx1", C.c_int32),
                ("l_idx2", C.c_int32)]


class MdmJointsToFeaturesCall(C.Structure):
    """include/mdm_hip.h mdm_joints_to_features_call_t."""
    _fields_ = [(n, C.c_int32) for n in ("layout", "floor", "origin_xz", "face_z")] + [("feet_thre", C.c_double),
               ("tgt_offsets", C.POINTER(C.c_float))] + [(n, C.c_void_p) for n in ("mean_dev", "std_dev", "global_dev", "ric_dev")]


SMPLIFY_FRAMES = 32         # csrc/smplify.h SMF_FRAMES: frames per workgroup
SMPLIFY_TERMS = 6           # SMF_TERMS
METRICS_KINDS = {"knn_radius": 0, "manifold_members": 1, "gather_dist": 2, "poly_mmd": 3, "feature_stats": 4,
                 "retrieval_ranks": 5, "dist_matrix": 6, "confusion": 7}      # MDM_METRICS_*
RETRIEVAL_TOPK_MAX = 16     # csrc/humanml_metrics.h RET_TOPK_MAX
METRICS_TILE = 64           # csrc/metrics.h MET_TILE
FRECHET_MAX_D, FRECHET_SMALL_MAX, FRECHET_MAX_SWEEPS = 1024, 64, 30      # csrc/frechet.h FR_MAX_D, FR_SMALL_MAX, FR_MAX_SWEEPS
STGCN_RES = {"none": 0, "identity": 1, "conv": 2}      # MDM_STGCN_RES_*
STGCN_MAX_BLOCKS, STGCN_MAX_NEIGHBOURS = 16, 8

SMPL_POSE_REPS = {"rot6d": 0, "rotvec": 1, "rotmat": 2, "rotquat": 3}      # MDM_SMPL_*: feature counts 6, 3, 9, 4
SMPL_REP_FEATS = {"rot6d": 6, "rotvec": 3, "rotmat": 9, "rotquat": 4}


class MdmStep(C.Structure):
    _fields_ = [("a_x0", C.c_float), ("a_xt", C.c_float), ("sigma", C.c_float), ("clip_denoised", C.c_int32),
                ("seed", C.c_uint64), ("sample_base", C.c_uint32), ("draw", C.c_uint32), ("const_noise", C.c_int32)]


class MdmSampleParams(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("T", C.c_int32), ("num_timesteps", C.c_int32), ("start_index", C.c_int32),
        ("a_x0", C.c_void_p), ("a_xt", C.c_void_p), ("sigma", C.c_void_p), ("timestep_map", C.c_void_p),
        ("text_embed_dev", C.c_void_p), ("scale_dev", C.c_void_p), ("lengths_dev", C.c_void_p),
        ("inpaint_mask_dev", C.c_void_p), ("inpaint_motion_dev", C.c_void_p), ("noise_dev", C.c_void_p),
        ("seed", C.c_uint64), ("sample_base", C.c_uint32), ("clip_denoised", C.c_int32),
        ("force_uncond", C.c_int32), ("x0_dev", C.c_void_p), ("dump_steps", C.c_void_p), ("num_dump", C.c_int32),
        ("dump_dev", C.c_void_p), ("const_noise", C.c_int32),
    ]


class MdmSampleDecParams(C.Structure):
    """mdm_sample_dec_params_t: the loop block (T = pred_len, text_embed_dev = token-major text tokens) + the DiP inputs."""
    _fields_ = [("loop", MdmSampleParams), ("ntok", C.c_int32), ("prefix_dev", C.c_void_p),
                ("text_lengths_dev", C.c_void_p)]


class MdmError(RuntimeError):
    pass


class MdmLib:
    """Thin typed view of the shared library.  Pointers are passed as integers (tensor.data_ptr())."""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise MdmError(
                f"{path} not found: the MI355X HIP extension is not built. Run `python __graft_entry__.py build` "
                f"(hipcc --offload-arch=gfx950). There is no CPU fallback for this path.")
        self.path = path
        lib = self.lib = C.CDLL(path)
        vp, i32, i64, u32, u64, f32, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_size_t
        P = C.POINTER
        sig = {
            "mdm_abi_version": (C.c_int, []),
            "mdm_last_error": (C.c_char_p, []),
            "mdm_build_info": (C.c_char_p, []),
            "mdm_create": (C.c_int, [P(MdmConfig), P(vp)]),
            "mdm_destroy": (None, [vp]),
            "mdm_set_weight": (C.c_int, [vp, C.c_char_p, vp, i64]),
            "mdm_const_bytes": (sz, [vp]),
            "mdm_prepare": (C.c_int, [vp, vp, sz, vp]),
            "mdm_workspace_bytes": (sz, [vp, i32, i32]),
            "mdm_forward": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]),
            "mdm_sampler_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, P(MdmStep), vp]),
            "mdm_randn": (C.c_int, [vp, vp, vp, f32, f32, i32, i32, u64, u32, u32, vp]),
            "mdm_sample_loop": (C.c_int, [vp, P(MdmSampleParams), vp, vp, sz, vp]),
            "mdm_linear": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
            "mdm_layernorm": (C.c_int, [vp, vp, vp, i32, i32, vp]),
            "mdm_attention": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, vp]),
            "mdm_set_precision": (C.c_int, [vp, i32]),
            "mdm_weights_in_range": (C.c_int, [vp, P(i32), vp]),
            "mdm_linear_x3_scratch_bytes": (sz, [i32, i32, i32]),
            "mdm_linear_x3": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
            "mdm_attention_x3_scratch_bytes": (sz, [i32, i32, i32]),
            "mdm_attention_x3": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
            "mdm_recover_from_ric": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
            "mdm_workspace_bytes_dec": (sz, [vp, i32, i32, i32]),
            "mdm_forward_dec": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, sz, vp]),
            "mdm_workspace_bytes_dec_loop": (sz, [vp, i32, i32, i32, i32]),
            "mdm_sample_loop_dec": (C.c_int, [vp, P(MdmSampleDecParams), vp, vp, sz, vp]),
            "mdm_profile_enable": (C.c_int, [vp, C.c_int]),
            "mdm_profile_read": (C.c_int, [vp, i32, P(C.c_double), P(i64), P(C.c_double)]),
            "mdm_profile_reset": (C.c_int, [vp]),
            "mdm_set_option": (C.c_int, [vp, i32, i32]),
            "mdm_get_option": (C.c_int, [vp, i32, P(i32)]),
            "mdm_set_time_add": (C.c_int, [vp, vp, i32]),
            "mdm_rot6d_to_smpl_joints": (C.c_int, [vp, vp, P(f32), P(i32), vp, i32, i32, i32, i32, vp]),
            "mdm_smpl_workspace_bytes": (sz, [P(MdmSmplModel), P(MdmSmplCall), i32, i32]),
            "mdm_smpl_forward": (C.c_int, [P(MdmSmplModel), P(MdmSmplCall), vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
            "mdm_eval_workspace_bytes": (sz, [P(MdmEvalModel), i32, i32, i32]),
            "mdm_eval_motion_embeddings": (C.c_int, [P(MdmEvalModel), vp, vp, vp, i32, i32, i32, vp, sz, vp]),
            "mdm_eval_text_embeddings": (C.c_int, [P(MdmEvalModel), vp, vp, vp, vp, i32, i32, i32, vp, sz, vp]),
            "mdm_text_workspace_bytes": (sz, [P(MdmTextModel), i32, i32]),
            "mdm_text_encode": (C.c_int, [P(MdmTextModel), vp, vp, vp, i32, i32, i32, vp, sz, vp]),
            "mdm_clip_text_workspace_bytes": (sz, [P(MdmClipTextModel), i32, i32]),
            "mdm_clip_text_encode": (C.c_int, [P(MdmClipTextModel), vp, vp, vp, i32, i32, vp, sz, vp]),
            "mdm_stgcn_workspace_bytes": (sz, [P(MdmStgcnModel), i32, i32]),
            "mdm_stgcn_forward": (C.c_int, [P(MdmStgcnModel), vp, vp, vp, i32, i32, vp, sz, vp]),
            "mdm_gru_cls_workspace_bytes": (sz, [P(MdmGruClsModel), i32, i32]),
            "mdm_gru_cls_forward": (C.c_int, [P(MdmGruClsModel), vp, vp, vp, vp, vp, i32, i32, vp, sz, vp]),
            "mdm_metrics_workspace_bytes": (sz, [i32, i32, i32]),
            "mdm_knn_radius": (C.c_int, [vp, i32, i32, i32, vp, vp, sz, vp]),
            "mdm_manifold_members": (C.c_int, [vp, vp, i32, vp, i32, i32, vp, vp, vp, sz, vp]),
            "mdm_gather_dist": (C.c_int, [vp, i32, i32, vp, vp, i32, vp, vp, vp, sz, vp]),
            "mdm_poly_mmd": (C.c_int, [vp, i32, vp, i32, i32, vp, vp, i32, i32, C.c_double, C.c_double, i32, i32, vp, vp, vp, sz, vp]),
            "mdm_feature_stats": (C.c_int, [vp, i32, i32, vp, vp, vp, sz, vp]),
            "mdm_retrieval_ranks": (C.c_int, [vp, vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
            "mdm_dist_matrix": (C.c_int, [vp, i32, vp, i32, i32, vp, vp, sz, vp]),
            "mdm_confusion": (C.c_int, [vp, vp, i32, i32, vp, vp, vp, vp, sz, vp]),
            "mdm_frechet_workspace_bytes": (sz, [i32]),
            "mdm_frechet_distance": (C.c_int, [vp, vp, vp, vp, i32, vp, vp, vp, sz, vp]),
            "mdm_smplify_workspace_bytes": (sz, [P(MdmSmplifyModel), P(MdmSmplifyCall), i32]),
            "mdm_smplify_value_grad": (C.c_int, [P(MdmSmplifyModel), P(MdmSmplifyCall), i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp,
                                                 P(f32), vp, sz, vp]),
            "mdm_smplify_fit": (C.c_int, [P(MdmSmplifyModel), P(MdmSmplifyCall), vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, P(C.c_double),
                                          vp, sz, vp]),
            "mdm_smplify_strong_wolfe": (C.c_int, [P(C.c_double), P(C.c_double), i32, C.c_double, C.c_double, C.c_double, C.c_double,
                                                   C.c_double, i32, i32, P(C.c_double), P(i32), P(C.c_double), P(C.c_double)]),
            "mdm_joints_to_features_workspace_bytes": (sz, [i32, i32, i32]),
            "mdm_joints_to_features": (C.c_int, [P(MdmSkeleton), P(MdmJointsToFeaturesCall), vp, P(i32), vp, i32, i32, i32, vp, sz, vp]),
        }
        probe_sig = {
            "mdm_debug_set": (C.c_int, [C.c_int, C.c_int]),
            "mdm_debug_get": (C.c_int, [C.c_int, P(C.c_double)]),
            "mdm_linear_f16f6_scratch_bytes": (sz, [i32, i32, i32]),
            "mdm_linear_f16f6": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
            "mdm_probe_in_proj": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
            "mdm_probe_attention_x3": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
        }
        self.has_probes = hasattr(lib, "mdm_debug_set")   # libmdm_hip_probe.so / the emulator build
        if self.has_probes:
            sig.update(probe_sig)
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        if lib.mdm_abi_version() != ABI_VERSION:
            raise MdmError(f"{path}: ABI version {lib.mdm_abi_version()} != {ABI_VERSION}")
        self.build_info = dict(kv.split("=", 1) for kv in lib.mdm_build_info().decode().split(";"))
        # A GPU library built WITH packed fp32 VALU math (hipcc's SLP vectorizer) returns rare wrong DiP samples whenever another
        # LDS-using kernel shares a CU with its small GEMM (include/mdm_hip.h CONCURRENCY; profiles/r03g_dip_groups.md): refuse
        # it at load time instead of trusting whoever built it.  (The CPU emulator of tests/emu has no such hazard.)
        if self.build_info.get("emu") != "1" and self.build_info.get("slp") != "off" \
                and os.environ.get("MDM_ALLOW_SLP_BUILD") != "1":
            raise MdmError(f"{path} was built without -fno-slp-vectorize -DMDM_NO_SLP=1 (mdm_build_info: "
                           f"{lib.mdm_build_info().decode()}): rebuild with `python __graft_entry__.py`, or set "
                           f"MDM_ALLOW_SLP_BUILD=1 for an A/B experiment on an otherwise idle device")

    def check(self, rc, what):
        if rc != MDM_OK:
            msg = self.lib.mdm_last_error()
            raise MdmError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")

    def __getattr__(self, name):
        return getattr(self.lib, name)


_LIB = None


def load_native():
    """The one and only way the product path reaches its kernels; raises MdmError if the .so is absent."""
    global _LIB
    if _LIB is None:
        _LIB = MdmLib(os.environ.get("MDM_HIP_LIB", LIB_PATH))
    return _LIB


_PROBE_LIB = None


def load_probe():
    """libmdm_hip_probe.so (include/mdm_hip_probe.h): experiments and probe-only tests; never used by the seams."""
    global _PROBE_LIB
    if _PROBE_LIB is None:
        _PROBE_LIB = MdmLib(os.environ.get("MDM_HIP_PROBE_LIB", PROBE_LIB_PATH))
        if not _PROBE_LIB.has_probes:
            raise MdmError(f"{_PROBE_LIB.path} was not built with -DMDM_PROBES")
    return _PROBE_LIB
