// smpl_api.h -- part of the ONE translation unit csrc/mdm_api.hip: mdm_recover_from_ric, mdm_rot6d_to_smpl_joints and
// mdm_smpl_workspace_bytes / mdm_smpl_forward (include/mdm_hip.h) over the kernels of motion_recover.h, smpl_joints.h and smpl_mesh.h.
#pragma once
// (included by mdm_api.hip behind its own entry points; relies on its includes, api_runtime.h and `using namespace mdm`)

extern "C" {

int mdm_recover_from_ric(const float* x, const float* mean, const float* stdv, float* out, int32_t B, int32_t T,
                         int32_t njoints_feat, int32_t joints, void* stream) {
  ChainGuard chain_guard(stream);
  if (!x || !mean || !stdv || !out || B <= 0 || T <= 0 || joints < 1) return fail(MDM_EINVAL, "mdm_recover_from_ric: bad argument");
  if (njoints_feat < 4 + 3 * (joints - 1)) return fail(MDM_EINVAL, "mdm_recover_from_ric: feature width too small for the joint count");
  if (T > 1024) return fail(MDM_EUNSUPPORTED, "mdm_recover_from_ric: at most 1024 frames");
  auto k = &recover_from_ric_kernel;
  MDM_LAUNCH(k, dim3(B), dim3(256), (size_t)3 * T * sizeof(float), static_cast<hipStream_t>(stream), x, mean, stdv, out, T,
             njoints_feat, joints);
  return rt_launch_status();
}

int mdm_rot6d_to_smpl_joints(const float* x, const uint8_t* mask, const float* rest_joints, const int32_t* parents, float* out,
                             int32_t B, int32_t T, int32_t njoints_in, int32_t J, void* stream) {
  if (!x || !rest_joints || !parents || !out) return fail(MDM_EINVAL, "mdm_rot6d_to_smpl_joints: null pointer");
  if (B <= 0 || T <= 0 || J < 1) return fail(MDM_EINVAL, "mdm_rot6d_to_smpl_joints: need B >= 1, T >= 1 and J >= 1");
  if (njoints_in != J + 1)
    return fail(MDM_EINVAL, "mdm_rot6d_to_smpl_joints: njoints_in must be J + 1 (the joint rotations, then the translation row)");
  if (J > kSmplMaxJoints) return fail(MDM_EUNSUPPORTED, "mdm_rot6d_to_smpl_joints: at most 24 joints");
  if (T > 4096 || (int64_t)B * T > (1 << 24)) return fail(MDM_EUNSUPPORTED, "mdm_rot6d_to_smpl_joints: at most 4096 frames and 2^24 frames in all");
  if (parents[0] != -1) return fail(MDM_EINVAL, "mdm_rot6d_to_smpl_joints: parents[0] must be -1 (the root)");
  for (int i = 1; i < J; ++i)
    if (parents[i] < 0 || parents[i] >= i)
      return fail(MDM_EINVAL, "mdm_rot6d_to_smpl_joints: parents[" + std::to_string(i) + "] must lie in [0, " + std::to_string(i) + ")");
  SmplFkTables tab;
  if (smpl_fk_tables(rest_joints, parents, J, tab) < 0) return fail(MDM_EUNSUPPORTED, "mdm_rot6d_to_smpl_joints: tree needs too many live transforms");
  ChainGuard chain_guard(stream);
  auto k = &smpl_joints_kernel;
  MDM_LAUNCH(k, dim3((unsigned)(((int64_t)B * T + kSmplLanes - 1) / kSmplLanes)), dim3(kSmplLanes), 0, static_cast<hipStream_t>(stream),
             x, mask, out, B, T, J, tab);
  return rt_launch_status();
}

}  // extern "C"

namespace {

struct SmplPlan {
  int J, V, Vpad, KP, NA;          // NA: rows of the extended joint list
  bool joints, need_sel, need_mesh;
  size_t feat, aws, delta, allj, mesh;   // workspace extents, floats
};

// Validation shared by mdm_smpl_workspace_bytes and mdm_smpl_forward; 0 or a negative code with the message set.
int smpl_plan(const char* fn, const mdm_smpl_model_t* m, const mdm_smpl_call_t* c, int B, int T, SmplPlan& p) {
  const std::string f = std::string(fn) + ": ";
  if (m == nullptr || c == nullptr) return fail(MDM_EINVAL, f + "null model or call");
  if (B <= 0 || T <= 0) return fail(MDM_EINVAL, f + "need B >= 1 and T >= 1");
  if (T > 4096 || (int64_t)B * T > (1 << 24)) return fail(MDM_EUNSUPPORTED, f + "at most 4096 frames and 2^24 frames in all");
  if (m->J < 1) return fail(MDM_EINVAL, f + "need J >= 1");
  if (m->J > kSmplMaxJoints) return fail(MDM_EUNSUPPORTED, f + "at most 24 joints");
  if (m->V < 1 || m->V > (1 << 20)) return fail(MDM_EINVAL, f + "the vertex count V must lie in [1, 2^20]");
  if (m->n_sel < 0 || m->n_sel > 32) return fail(MDM_EINVAL, f + "n_sel must lie in [0, 32]");
  if (m->n_extra < 0 || m->n_extra > kSmplMaxExtra) return fail(MDM_EINVAL, f + "n_extra must lie in [0, 16]");
  if (m->parents == nullptr) return fail(MDM_EINVAL, f + "null parents");
  if (m->parents[0] != -1) return fail(MDM_EINVAL, f + "parents[0] must be -1 (the root)");
  for (int i = 1; i < m->J; ++i)
    if (m->parents[i] < 0 || m->parents[i] >= i)
      return fail(MDM_EINVAL, f + "parents[" + std::to_string(i) + "] must lie in [0, " + std::to_string(i) + ")");
  if (c->pose_rep < MDM_SMPL_ROT6D || c->pose_rep > MDM_SMPL_ROTQUAT) return fail(MDM_EINVAL, f + "pose_rep must be one of MDM_SMPL_ROT6D .. MDM_SMPL_ROTQUAT");
  if (!c->glob && c->glob_rot_mat == nullptr) return fail(MDM_EINVAL, f + "glob = 0 needs glob_rot_mat");
  if (c->n_points < 0 || c->n_points > kSmplMaxPoints) return fail(MDM_EINVAL, f + "n_points must lie in [0, 64]");
  p.J = m->J;
  p.V = m->V;
  p.Vpad = (m->V + 31) & ~31;
  p.KP = smpl_feat_kp(m->J);
  p.NA = m->J + m->n_sel + m->n_extra;
  p.joints = c->n_points > 0;
  p.need_sel = p.need_mesh = false;
  if (p.joints) {
    if (c->point_map == nullptr) return fail(MDM_EINVAL, f + "n_points > 0 needs point_map");
    if (c->root_point < 0 || c->root_point >= c->n_points) return fail(MDM_EINVAL, f + "root_point must lie in [0, n_points)");
    for (int i = 0; i < c->n_points; ++i) {
      const int s = c->point_map[i];
      if (s < 0 || s >= p.NA)
        return fail(MDM_EINVAL, f + "point_map[" + std::to_string(i) + "] = " + std::to_string(s) + " is outside the joint list of " +
                                    std::to_string(p.NA) + " (J + n_sel + n_extra)");
      if (s >= m->J + m->n_sel) p.need_mesh = true;
      else if (s >= m->J) p.need_sel = true;
    }
  }
  p.feat = (size_t)B * p.KP * T;
  p.aws = (size_t)B * 12 * kSmplMaxJoints * T;
  p.delta = (size_t)B * 3 * T;
  p.allj = (size_t)B * p.NA * 3 * T;
  p.mesh = p.need_mesh ? (size_t)kSkinChunkTiles * kSkinFrames * 3 * p.V : 0;
  return 0;
}

size_t smpl_plan_bytes(const SmplPlan& p) { return ws_bytes_of(p.feat + p.aws + p.delta + p.allj + p.mesh); }

template <int REP> void launch_smpl_pose(const SmplPoseArgs& a, hipStream_t s) {
  auto k = &smpl_pose_kernel<REP>;
  MDM_LAUNCH(k, dim3((unsigned)(((int64_t)a.B * a.T + kSmplLanes - 1) / kSmplLanes)), dim3(kSmplLanes), 0, s, a);
}

}  // namespace

extern "C" {

size_t mdm_smpl_workspace_bytes(const mdm_smpl_model_t* model, const mdm_smpl_call_t* call, int32_t B, int32_t T) {
  SmplPlan p;
  if (smpl_plan("mdm_smpl_workspace_bytes", model, call, B, T, p) != 0) return 0;
  return smpl_plan_bytes(p);
}

int mdm_smpl_forward(const mdm_smpl_model_t* m, const mdm_smpl_call_t* c, const float* x, const uint8_t* mask, const float* betas,
                     float* out, float* rot_out, int32_t B, int32_t T, int32_t rows_x, int32_t feats_x, void* ws, size_t ws_bytes,
                     void* stream) {
  const char* fn = "mdm_smpl_forward";
  SmplPlan p;
  if (int rc = smpl_plan(fn, m, c, B, T, p)) return rc;
  if (!x || !out || !ws) return fail(MDM_EINVAL, "mdm_smpl_forward: null x, out or workspace");
  if (!m->j0 || !m->jdirs) return fail(MDM_EINVAL, "mdm_smpl_forward: null j0 or jdirs table");
  const bool skin = !p.joints || p.need_mesh;
  if (skin && (!m->blend || !m->weights_t)) return fail(MDM_EINVAL, "mdm_smpl_forward: null blend or weights_t table");
  if (p.need_sel && (!m->sel_blend || !m->sel_weights_t)) return fail(MDM_EINVAL, "mdm_smpl_forward: the map names a selected vertex: null sel_blend or sel_weights_t table");
  if (p.need_mesh && !m->extra_t) return fail(MDM_EINVAL, "mdm_smpl_forward: the map names a regressed joint: null extra_t table");
  const int NR = c->glob ? p.J : p.J - 1;
  const int has_trans = c->translation ? 1 : 0;
  if (rows_x != NR + has_trans)
    return fail(MDM_EINVAL, "mdm_smpl_forward: x has " + std::to_string(rows_x) + " rows; need " + std::to_string(NR) +
                                " rotation rows" + (has_trans ? " and the translation row" : ""));
  if (feats_x != smpl_rep_feats(c->pose_rep))
    return fail(MDM_EINVAL, "mdm_smpl_forward: x has " + std::to_string(feats_x) + " features per row; this pose_rep has " +
                                std::to_string(smpl_rep_feats(c->pose_rep)));
  if (NR < 1) return fail(MDM_EINVAL, "mdm_smpl_forward: no rotation row");
  if (ws_bytes < smpl_plan_bytes(p)) return fail(MDM_ENOSPC, "mdm_smpl_forward: workspace too small (mdm_smpl_workspace_bytes)");
  SmplFkTables tab;
  {
    float zero[kSmplMaxJoints * 3] = {};
    if (smpl_fk_tables(zero, m->parents, p.J, tab) < 0) return fail(MDM_EUNSUPPORTED, "mdm_smpl_forward: tree needs too many live transforms");
  }
  float* feat = ws_floats(ws);
  float* aws = feat + p.feat;
  float* delta = aws + p.aws;
  float* allj = delta + p.delta;
  float* mesh = allj + p.allj;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);

  SmplPoseArgs pa;
  pa.x = x; pa.mask = mask; pa.betas = betas; pa.j0 = m->j0; pa.jdirs = m->jdirs;
  pa.feat = feat; pa.aws = aws; pa.joints = allj; pa.delta = delta; pa.rot_out = rot_out;
  pa.B = B; pa.T = T; pa.J = p.J; pa.NR = NR; pa.F = feats_x; pa.KP = p.KP; pa.joints_rows = p.NA;
  pa.glob = c->glob ? 1 : 0; pa.has_trans = has_trans; pa.add_trans = has_trans && c->vertstrans ? 1 : 0;
  pa.beta1 = c->beta1;
  for (int i = 0; i < 9; ++i) pa.grot[i] = c->glob ? 0.f : c->glob_rot_mat[i];
  for (int i = 0; i < kSmplMaxJoints; ++i) {
    pa.parent[i] = i < p.J && i > 0 ? m->parents[i] : 0;
    pa.pslot[i] = tab.pslot[i];
    pa.oslot[i] = tab.oslot[i];
  }
  switch (c->pose_rep) {
    case MDM_SMPL_ROT6D: launch_smpl_pose<kRepRot6d>(pa, s); break;
    case MDM_SMPL_ROTVEC: launch_smpl_pose<kRepRotvec>(pa, s); break;
    case MDM_SMPL_ROTMAT: launch_smpl_pose<kRepRotmat>(pa, s); break;
    default: launch_smpl_pose<kRepRotquat>(pa, s); break;
  }
  if (int rc = rt_launch_status()) return rc;

  const int tps = (T + kSkinFrames - 1) / kSkinFrames, ntiles = B * tps;
  SmplSkinArgs sa;
  sa.feat = feat; sa.aws = aws; sa.delta = delta; sa.mask = mask;
  sa.T = T; sa.KP = p.KP; sa.tiles_per_sample = tps;
  auto skin_k = &smpl_skin_kernel;
  if (!p.joints) {                       // 'vertices': the mesh is the output
    sa.blend = m->blend; sa.wt = m->weights_t; sa.out = out; sa.V = p.V; sa.Vpad = p.Vpad;
    sa.tile0 = 0; sa.mode = 0; sa.out_rows = p.V; sa.row_off = 0; sa.finish = 1;
    MDM_LAUNCH(skin_k, dim3(ntiles, (p.Vpad / 32 + kSkinTiles - 1) / kSkinTiles), dim3(kSkinWaves * 64), 0, s, sa);
    return rt_launch_status();
  }
  if (p.need_sel) {                      // the selected vertices, skinned from their gathered tables into the joint list
    sa.blend = m->sel_blend; sa.wt = m->sel_weights_t; sa.out = allj; sa.V = m->n_sel; sa.Vpad = (m->n_sel + 31) & ~31;
    sa.tile0 = 0; sa.mode = 0; sa.out_rows = p.NA; sa.row_off = p.J; sa.finish = 0;
    MDM_LAUNCH(skin_k, dim3(ntiles, 1), dim3(kSkinWaves * 64), 0, s, sa);
    if (int rc = rt_launch_status()) return rc;
  }
  if (p.need_mesh) {                     // the regressed joints: the mesh of 16 frame tiles at a time, then a fixed-order reduction
    sa.blend = m->blend; sa.wt = m->weights_t; sa.out = mesh; sa.V = p.V; sa.Vpad = p.Vpad;
    sa.mode = 1; sa.out_rows = 0; sa.row_off = 0; sa.finish = 0;
    auto extra_k = &smpl_extra_kernel;
    for (int t0 = 0; t0 < ntiles; t0 += kSkinChunkTiles) {
      const int n = std::min(kSkinChunkTiles, ntiles - t0);
      sa.tile0 = t0;
      MDM_LAUNCH(skin_k, dim3(n, (p.Vpad / 32 + kSkinTiles - 1) / kSkinTiles), dim3(kSkinWaves * 64), 0, s, sa);
      MDM_LAUNCH(extra_k, dim3(n, 3, m->n_extra), dim3(256), 0, s, (const float*)mesh, m->extra_t, allj, (int)T, p.V, (int)m->n_extra, tps, t0, p.NA,
                 p.J + m->n_sel);
      if (int rc = rt_launch_status()) return rc;
    }
  }
  SmplPointMap map;
  for (int i = 0; i < kSmplMaxPoints; ++i) map.src[i] = i < c->n_points ? c->point_map[i] : 0;
  auto points_k = &smpl_points_kernel;
  const size_t n = (size_t)B * c->n_points * 3 * T;
  MDM_LAUNCH(points_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)allj, (const float*)delta, mask, out, (int)B, (int)T,
             (int)c->n_points, p.NA, (int)c->root_point, map);
  return rt_launch_status();
}

}  // extern "C"
