// SMPL joint positions of rot6d samples (the action-to-motion families' post-sampling transform), fused on the device:
//     model.rot2xyz(x=sample, mask, pose_rep='rot6d', glob=True, translation=True, jointstype='smpl', vertstrans=True, beta=0)
//                                                              sample/generate.py:167-171, eval/a2m/stgcn_eval.py:55
// i.e. model/rotation2xyz.py:17-90 over utils/rotation_conversions.py:528-534 (rotation_6d_to_matrix) and the joints path of
// smplx's lbs (batch_rigid_transform).  With zero betas the posed SMPL joints depend only on the 24 rotations, the rest-pose
// joints J = J_regressor . v_template and the kinematic tree: no vertex, blend shape or skinning weight enters.
//   * one lane per (sample, frame); frames are the contiguous axis of x [B, J+1, 6, T] and out [B, J, 3, T]: every load and
//     store is coalesced;
//   * the chain G_i = G_parent(i) . [R_i | rel_i] runs in joint order; a transform that a later joint reads waits in LDS, in a
//     slot the host assigned (smpl_fk_slots): a joint's slot is free again after its last child, so at most J / 2 transforms
//     are ever live (each live joint has a distinct unprocessed child) -- 12 slots of 12 floats per lane for SMPL's 24 joints;
//   * the tables (rest-pose offsets, slots) travel as kernel arguments: no device allocation, nothing to set up per device.
#pragma once
#include "common.h"

namespace mdm {

constexpr int kSmplMaxJoints = 24;
constexpr int kSmplSlots = kSmplMaxJoints / 2;
constexpr int kSmplLanes = 64;

struct SmplFkTables {
  float rel[kSmplMaxJoints][3];      // rel_0 = J_0, rel_i = J_i - J_parent(i)            (batch_rigid_transform)
  int32_t pslot[kSmplMaxJoints];     // LDS slot holding the parent's transform (unused for joint 0)
  int32_t oslot[kSmplMaxJoints];     // LDS slot receiving this joint's transform, -1: no later joint reads it
};

// F.normalize(v, dim=-1): v / max(|v|, 1e-12) -- the clamp keeps zero and tiny 6D halves finite, as in the reference
__device__ __forceinline__ void smpl_normalize3(float& x, float& y, float& z) {
  const float n = fmaxf(sqrtf(x * x + y * y + z * z), 1e-12f);
  x = x / n;
  y = y / n;
  z = z / n;
}

// x [B][J+1][6][T], mask [B][T] (nullptr: every frame valid), out [B][J][3][T]; blockDim = kSmplLanes.
__global__ __launch_bounds__(kSmplLanes) void smpl_joints_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                                 float* __restrict__ out, int B, int T, int J, SmplFkTables tab) {
  __shared__ float s_g[kSmplSlots * 12 * kSmplLanes];   // [slot][12][lane]: lane-contiguous, conflict-free
  const int lane = threadIdx.x;
  const int gid = blockIdx.x * kSmplLanes + lane;
  if (gid >= B * T) return;          // (no barrier below: every lane works on its own LDS column)
  const int b = gid / T, t = gid - b * T;
  const float* xb = x + (size_t)b * (J + 1) * 6 * T;
  float* ob = out + (size_t)b * J * 3 * T;
  // x_translations - x_translations[:, :, [0]]: every frame, masked ones included (rotation2xyz.py:72-87)
  const float* tr = xb + (size_t)J * 6 * T;
  const float dx = tr[t] - tr[0], dy = tr[(size_t)T + t] - tr[T], dz = tr[(size_t)2 * T + t] - tr[2 * T];
  const bool valid = mask == nullptr || mask[(size_t)b * T + t] != 0;
  if (!valid) {                      // x_xyz[~mask] = 0, minus root (0), plus translation
    for (int i = 0; i < J; ++i) {
      ob[((size_t)i * 3 + 0) * T + t] = 0.f + dx;
      ob[((size_t)i * 3 + 1) * T + t] = 0.f + dy;
      ob[((size_t)i * 3 + 2) * T + t] = 0.f + dz;
    }
    return;
  }
  const float r0x = tab.rel[0][0], r0y = tab.rel[0][1], r0z = tab.rel[0][2];   // joint 0's posed position is J_0
  for (int i = 0; i < J; ++i) {
    // rotation_6d_to_matrix: rows b1, b2, b3 (torch.stack(..., dim=-2))
    const float* xi = xb + (size_t)i * 6 * T + t;
    float a1x = xi[0], a1y = xi[T], a1z = xi[2 * T];
    float a2x = xi[3 * T], a2y = xi[4 * T], a2z = xi[5 * T];
    smpl_normalize3(a1x, a1y, a1z);
    const float d = a1x * a2x + a1y * a2y + a1z * a2z;
    a2x = a2x - d * a1x;
    a2y = a2y - d * a1y;
    a2z = a2z - d * a1z;
    smpl_normalize3(a2x, a2y, a2z);
    const float R[3][3] = {{a1x, a1y, a1z},
                           {a2x, a2y, a2z},
                           {a1y * a2z - a1z * a2y, a1z * a2x - a1x * a2z, a1x * a2y - a1y * a2x}};
    const float rx = tab.rel[i][0], ry = tab.rel[i][1], rz = tab.rel[i][2];
    float G[12];                     // G[3r + c] rotation, G[9 + r] translation
    if (i == 0) {                    // glob=True: joint 0's rotation is the global orient
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) G[3 * r + c] = R[r][c];
      }
      G[9] = rx;
      G[10] = ry;
      G[11] = rz;
    } else {
      const float* p = s_g + (size_t)tab.pslot[i] * 12 * kSmplLanes + lane;
      float P[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) P[k] = p[k * kSmplLanes];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) G[3 * r + c] = P[3 * r] * R[0][c] + P[3 * r + 1] * R[1][c] + P[3 * r + 2] * R[2][c];
        G[9 + r] = P[3 * r] * rx + P[3 * r + 1] * ry + P[3 * r + 2] * rz + P[9 + r];
      }
    }
    if (tab.oslot[i] >= 0) {
      float* q = s_g + (size_t)tab.oslot[i] * 12 * kSmplLanes + lane;
#pragma unroll
      for (int k = 0; k < 12; ++k) q[k * kSmplLanes] = G[k];
    }
    // x_xyz - x_xyz[:, [root]] + translation
    ob[((size_t)i * 3 + 0) * T + t] = (G[9] - r0x) + dx;
    ob[((size_t)i * 3 + 1) * T + t] = (G[10] - r0y) + dy;
    ob[((size_t)i * 3 + 2) * T + t] = (G[11] - r0z) + dz;
  }
}

// Host: the kernel's tables from the rest-pose joints [J][3] and parents [J] (validated by the caller: parents[0] = -1,
// 0 <= parents[i] < i).  Returns the number of LDS slots used, or -1 if the tree needs more than kSmplSlots.
inline int smpl_fk_tables(const float* rest, const int32_t* parents, int J, SmplFkTables& tab) {
  int last_child[kSmplMaxJoints];
  for (int i = 0; i < J; ++i) last_child[i] = -1;
  for (int i = 1; i < J; ++i) last_child[parents[i]] = i;
  int slot_of[kSmplMaxJoints];
  bool busy[kSmplSlots] = {};
  int used = 0;
  for (int i = 0; i < J; ++i) {
    for (int c = 0; c < 3; ++c) tab.rel[i][c] = i == 0 ? rest[c] : rest[3 * i + c] - rest[3 * parents[i] + c];
    tab.pslot[i] = i == 0 ? 0 : slot_of[parents[i]];
    if (i > 0 && last_child[parents[i]] == i) busy[slot_of[parents[i]]] = false;   // read before this joint writes
    slot_of[i] = -1;
    if (last_child[i] >= 0) {
      int s = 0;
      while (s < kSmplSlots && busy[s]) ++s;
      if (s == kSmplSlots) return -1;
      busy[s] = true;
      slot_of[i] = s;
      used = s + 1 > used ? s + 1 : used;
    }
    tab.oslot[i] = slot_of[i];
  }
  for (int i = J; i < kSmplMaxJoints; ++i) {
    tab.rel[i][0] = tab.rel[i][1] = tab.rel[i][2] = 0.f;
    tab.pslot[i] = 0;
    tab.oslot[i] = -1;
  }
  return used;
}

}  // namespace mdm
