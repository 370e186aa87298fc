// motion_features_api.h -- part of the ONE translation unit csrc/mdm_api.hip: mdm_joints_to_features_workspace_bytes and
// mdm_joints_to_features (include/mdm_hip.h) over the kernels of motion_features.h.
#pragma once
// (included by mdm_api.hip behind its own entry points; relies on its includes, api_runtime.h and `using namespace mdm`)

namespace {

// mdm_skeleton_t -> the kernels' bone list; 0 or a failure that names the field
int mf_tables(const mdm_skeleton_t* s, MfSkeleton& sk) {
  const std::string f = "mdm_joints_to_features: ";
  const int J = s->joints;
  if (J < 2 || J > kMfMaxJoints) return fail(MDM_EINVAL, f + "skeleton.joints must lie in [2, " + std::to_string(kMfMaxJoints) + "]");
  if (s->n_chains < 1 || s->n_chains > MDM_SKEL_MAX_CHAINS) return fail(MDM_EINVAL, f + "skeleton.n_chains out of range");
  sk = MfSkeleton{};
  sk.J = J;
  int parent[kMfMaxJoints];
  bool placed[kMfMaxJoints] = {};
  placed[0] = true;
  parent[0] = -1;
  for (int c = 0; c < s->n_chains; ++c) {
    const int n = s->chain_len[c];
    if (n < 2 || n > MDM_SKEL_MAX_CHAIN_LEN) return fail(MDM_EINVAL, f + "skeleton.chain_len[" + std::to_string(c) + "] out of range");
    for (int i = 0; i < n; ++i)
      if (s->chains[c][i] < 0 || s->chains[c][i] >= J) return fail(MDM_EINVAL, f + "skeleton.chains[" + std::to_string(c) + "] names a joint out of range");
    if (!placed[s->chains[c][0]])
      return fail(MDM_EINVAL, f + "skeleton.chains[" + std::to_string(c) + "] starts at a joint no earlier chain reaches (the root, joint 0, comes first)");
    for (int i = 1; i < n; ++i) {
      const int ch = s->chains[c][i];
      if (placed[ch]) return fail(MDM_EINVAL, f + "skeleton.chains: joint " + std::to_string(ch) + " is reached twice");
      placed[ch] = true;
      parent[ch] = s->chains[c][i - 1];
      sk.parent[sk.nbones] = (unsigned char)parent[ch];
      sk.child[sk.nbones] = (unsigned char)ch;
      sk.first[sk.nbones] = i == 1;
      ++sk.nbones;
    }
  }
  for (int j = 0; j < J; ++j)
    if (!placed[j]) return fail(MDM_EINVAL, f + "skeleton.chains: joint " + std::to_string(j) + " is on no chain");
  for (int j = 0; j < J; ++j)
    for (int c = 0; c < 3; ++c) sk.raw[j][c] = s->raw_offsets[j][c];
  auto in_range = [&](int v) { return v >= 0 && v < J; };
  for (int k = 0; k < 4; ++k) {
    if (!in_range(s->face_joints[k])) return fail(MDM_EINVAL, f + "skeleton.face_joints out of range");
    sk.face[k] = s->face_joints[k];
  }
  for (int k = 0; k < 2; ++k) {
    if (!in_range(s->fid_l[k]) || !in_range(s->fid_r[k])) return fail(MDM_EINVAL, f + "skeleton.fid_l / fid_r out of range");
    sk.foot[k] = s->fid_l[k];
    sk.foot[2 + k] = s->fid_r[k];
  }
  if (s->l_idx1 < 1 || s->l_idx1 >= J || s->l_idx2 < 1 || s->l_idx2 >= J) return fail(MDM_EINVAL, f + "skeleton.l_idx1 / l_idx2 must name non-root joints");
  sk.l_idx1 = s->l_idx1; sk.l_par1 = parent[s->l_idx1];
  sk.l_idx2 = s->l_idx2; sk.l_par2 = parent[s->l_idx2];
  return 0;
}

inline size_t mf_lds_bytes(int T) { return ((size_t)kMfTapsPad + 4 * (size_t)T) * sizeof(double); }

}  // namespace

extern "C" {

size_t mdm_joints_to_features_workspace_bytes(int32_t B, int32_t T, int32_t joints) {
  if (B <= 0 || T <= 0 || joints <= 0) return 0;
  return (size_t)B * joints * 3 * T * sizeof(double) + 64;
}

int mdm_joints_to_features(const mdm_skeleton_t* skel, const mdm_joints_to_features_call_t* call, const float* joints,
                           const int32_t* lengths, float* out, int32_t B, int32_t T, int32_t F, void* ws_dev, size_t ws_bytes,
                           void* stream) {
  if (!skel || !call || !joints || !out) return fail(MDM_EINVAL, "mdm_joints_to_features: null pointer");
  if (B <= 0 || T < 2) return fail(MDM_EINVAL, "mdm_joints_to_features: need B >= 1 and T >= 2");
  MfSkeleton sk;
  if (int rc = mf_tables(skel, sk)) return rc;
  const int J = sk.J;
  if (F != 4 + 3 * (J - 1) + 6 * (J - 1) + 3 * J + 4)
    return fail(MDM_EINVAL, "mdm_joints_to_features: F must be 12 J - 1 (263 for 22 joints, 251 for 21), got F = " + std::to_string(F) +
                                " for J = " + std::to_string(J));
  if ((call->mean_dev == nullptr) != (call->std_dev == nullptr)) return fail(MDM_EINVAL, "mdm_joints_to_features: mean_dev and std_dev go together");
  if (call->layout != MDM_J2F_LAYOUT_BJ3T && call->layout != MDM_J2F_LAYOUT_BTJ3) return fail(MDM_EINVAL, "mdm_joints_to_features: bad layout");
  if (!(call->feet_thre > 0.0)) return fail(MDM_EINVAL, "mdm_joints_to_features: feet_thre must be positive");
  if (lengths != nullptr)
    for (int b = 0; b < B; ++b)
      if (lengths[b] < 2 || lengths[b] > T)
        return fail(MDM_EINVAL, "mdm_joints_to_features: lengths[" + std::to_string(b) + "] = " + std::to_string(lengths[b]) +
                                    " must lie in [2, T = " + std::to_string(T) + "]");
  if (T > kMfMaxT) return fail(MDM_EUNSUPPORTED, "mdm_joints_to_features: at most " + std::to_string(kMfMaxT) + " frames (the forward vectors of a clip are staged in LDS)");
  const bool canon = call->tgt_offsets != nullptr || call->floor || call->origin_xz || call->face_z;
  double* ws = nullptr;
  if (canon) {
    if (ws_dev == nullptr) return fail(MDM_EINVAL, "mdm_joints_to_features: the canonicalising options need a workspace");
    if (ws_bytes < mdm_joints_to_features_workspace_bytes(B, T, J)) return fail(MDM_ENOSPC, "mdm_joints_to_features: workspace too small");
    ws = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(ws_dev) + 15) & ~(uintptr_t)15);
  }
  MfCanon cn{};
  cn.retarget = call->tgt_offsets != nullptr;
  cn.floor = call->floor != 0; cn.origin_xz = call->origin_xz != 0; cn.face_z = call->face_z != 0;
  if (cn.retarget) {
    double leg[2] = {0.0, 0.0};
    for (int j = 0; j < J; ++j)
      for (int c = 0; c < 3; ++c) {
        cn.tgt[j][c] = call->tgt_offsets[j * 3 + c];
        if (j == sk.l_idx1) leg[0] = std::max(leg[0], std::fabs((double)cn.tgt[j][c]));
        if (j == sk.l_idx2) leg[1] = std::max(leg[1], std::fabs((double)cn.tgt[j][c]));
      }
    cn.tgt_leg = leg[0] + leg[1];
    if (!(cn.tgt_leg > 0.0)) return fail(MDM_EINVAL, "mdm_joints_to_features: tgt_offsets has no leg length at l_idx1 / l_idx2");
  }
  const bool btj3 = call->layout == MDM_J2F_LAYOUT_BTJ3;
  const long long sb = (long long)J * 3 * T, sj = btj3 ? 3 : 3LL * T, sc = btj3 ? 1 : T, st = btj3 ? 3LL * J : 1;
  MfOutput o{out, call->mean_dev, call->std_dev, call->global_dev, call->ric_dev};
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  for (int b0 = 0; b0 < B; b0 += kMfClipsPerLaunch) {       // the frame counts travel as kernel arguments: no upload, capture-safe
    const int nb = std::min(kMfClipsPerLaunch, B - b0);
    MfLengths len{};
    for (int i = 0; i < nb; ++i) len.v[i] = lengths != nullptr ? lengths[b0 + i] : T;
    const float* in_b = joints + (size_t)b0 * sb;
    double* ws_b = canon ? ws + (size_t)b0 * sb : nullptr;
    if (canon) {
      auto kc = &motion_canon_kernel;
      MDM_LAUNCH(kc, dim3(nb), dim3(kMfLanes), 0, s, in_b, ws_b, sk, cn, len, sb, sj, sc, st, T);
      if (int rc = rt_launch_status()) return rc;
    }
    MfOutput ob = o;
    ob.out = out + (size_t)b0 * F * (T - 1);
    if (ob.global_out != nullptr) ob.global_out += (size_t)b0 * sb;
    if (ob.ric_out != nullptr) ob.ric_out += (size_t)b0 * sb;
    auto kf = &motion_features_kernel;
    MDM_LAUNCH(kf, dim3(nb), dim3(kMfLanes), mf_lds_bytes(T), s, in_b, (const double*)ws_b, ob, sk, len, sb, sj, sc, st, T, F, call->feet_thre);
    if (int rc = rt_launch_status()) return rc;
  }
  return MDM_OK;
}

}  // extern "C"
