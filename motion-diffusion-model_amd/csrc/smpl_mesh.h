// The full SMPL body pass of model/rotation2xyz.py (every pose_rep, jointstype, betas, glob_rot; model/smpl.py:64-97 over smplx's
// lbs), fused on the device.  Four kernels, no floating-point atomics, no device allocation:
//   smpl_pose_kernel     one lane per (sample, frame), as smpl_joints_kernel (whose LDS slot scheme it reuses): rotation front end
//                        (rot6d / rotvec / rotmat / rotquat, utils/rotation_conversions.py), rest joints J0 + Jdirs . beta, the
//                        kinematic chain; writes, frames contiguous, the pose feature rows [R_1 - I ... R_23 - I | beta | 1], the 24
//                        relative transforms A_j = [G_R | G_t - G_R . J_j], the posed joints and the translation offsets.
//   smpl_skin_kernel     the hot path.  A workgroup owns 32 frames of ONE sample by up to 8 tiles of 32 vertices.  Frames are the
//                        MFMA column = lane dimension, vertices the rows: D[reg] of v_mfma_f32_32x32x2_f32 holds one vertex row
//                        over 32 consecutive frames, so every store to out [B, V, 3, T] is a 128-byte run along T.
//                          v_posed_c = B'_c . P'      B' = [posedirs; shapedirs; v_template] (K = 207 + 10 + 1, padded to 220),
//                                                     the A operand, straight from global memory ([3][KP][Vpad], vertices
//                                                     contiguous: one 128-byte run per lane half and k), one block of k ahead;
//                                                     P' the pose features of the 32 frames, staged once per workgroup in LDS;
//                          T_comp    = W . A_comp     K = 24, twelve components, four at a time (one output row);
//                          v_r = T_r0 v_posed_0 + T_r1 v_posed_1 + T_r2 v_posed_2 + T_r3 in the accumulator layout; the epilogue
//                        zeroes masked frames and adds the translation.  v_posed and the per-vertex transforms never leave registers.
//                        Exact fp32 (the MFMA is a k-ordered fmaf chain).
//   smpl_extra_kernel    J_regressor_extra . vertices over a chunk of the mesh in the workspace: eight vertex slices per output, each
//                        summed in a register, then the slices through LDS in slice order -- a fixed order, bit-identical run to run.
//   smpl_points_kernel   index map, root subtraction, mask and translation of the joints families.
#pragma once
#include "common.h"
#include "smpl_joints.h"

namespace mdm {

constexpr int kSmplBetas = 10;
constexpr int kSmplMaxExtra = 16;                 // rows of J_regressor_extra (9 in the reference)
constexpr int kSmplMaxPoints = 64;                // output points of a joints family (vibe: 49)
constexpr int kSkinFrames = 32;                   // frames per workgroup = MFMA columns
constexpr int kSkinWaves = 4;
constexpr int kSkinTiles = 8;                     // vertex tiles of 32 per workgroup (two per wave)
constexpr int kSkinKPMax = 220;                   // (24 - 1) * 9 + 10 + 1 = 218, rounded up to the k block of 4
constexpr int kSkinChunkTiles = 16;               // frame tiles of the mesh a joints family keeps in the workspace at a time

constexpr int smpl_feat_k(int J) { return (J - 1) * 9 + kSmplBetas + 1; }
constexpr int smpl_feat_kp(int J) { return (smpl_feat_k(J) + 3) & ~3; }

enum SmplRep { kRepRot6d = 0, kRepRotvec = 1, kRepRotmat = 2, kRepRotquat = 3 };
constexpr int smpl_rep_feats(int rep) { return rep == kRepRot6d ? 6 : rep == kRepRotvec ? 3 : rep == kRepRotmat ? 9 : 4; }

struct SmplPoseArgs {
  const float* x;          // [B][NX][F][T]
  const uint8_t* mask;     // [B][T] or nullptr
  const float* betas;      // [B][10][T] or nullptr: beta = (0, beta1, 0, ...)
  const float* j0;         // [J][3]
  const float* jdirs;      // [J][3][10]
  float* feat;             // [B][KP][T]
  float* aws;              // [B][12][24][T]
  float* joints;           // [B][joints_rows][3][T], rows 0 .. J-1
  float* delta;            // [B][3][T]
  float* rot_out;          // [B][T][NR][9] or nullptr
  int B, T, J, NR, F, KP, joints_rows;
  int glob, has_trans, add_trans;
  float beta1;
  float grot[9];           // glob = 0: the global orient of every frame
  int32_t parent[kSmplMaxJoints], pslot[kSmplMaxJoints], oslot[kSmplMaxJoints];
};

// quaternion_to_matrix (utils/rotation_conversions.py:49-66), real part first
__device__ __forceinline__ void smpl_quat_to_matrix(float r, float i, float j, float k, float R[3][3]) {
  const float two_s = 2.0f / (r * r + i * i + j * j + k * k);
  R[0][0] = 1.f - two_s * (j * j + k * k);
  R[0][1] = two_s * (i * j - k * r);
  R[0][2] = two_s * (i * k + j * r);
  R[1][0] = two_s * (i * j + k * r);
  R[1][1] = 1.f - two_s * (i * i + k * k);
  R[1][2] = two_s * (j * k - i * r);
  R[2][0] = two_s * (i * k - j * r);
  R[2][1] = two_s * (j * k + i * r);
  R[2][2] = 1.f - two_s * (i * i + j * j);
}

// one joint's rotation matrix from its features xi[f * T]
template <int REP> __device__ __forceinline__ void smpl_load_rotation(const float* xi, int T, float R[3][3]) {
  if constexpr (REP == kRepRot6d) {            // rotation_6d_to_matrix: rows b1, b2, b3
    float a1x = xi[0], a1y = xi[T], a1z = xi[2 * T];
    float a2x = xi[3 * T], a2y = xi[4 * T], a2z = xi[5 * T];
    smpl_normalize3(a1x, a1y, a1z);
    const float d = a1x * a2x + a1y * a2y + a1z * a2z;
    a2x = a2x - d * a1x;
    a2y = a2y - d * a1y;
    a2z = a2z - d * a1z;
    smpl_normalize3(a2x, a2y, a2z);
    R[0][0] = a1x; R[0][1] = a1y; R[0][2] = a1z;
    R[1][0] = a2x; R[1][1] = a2y; R[1][2] = a2z;
    R[2][0] = a1y * a2z - a1z * a2y;
    R[2][1] = a1z * a2x - a1x * a2z;
    R[2][2] = a1x * a2y - a1y * a2x;
  } else if constexpr (REP == kRepRotmat) {    // x_rotations[mask].view(-1, njoints, 3, 3)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) R[r][c] = xi[(3 * r + c) * T];
    }
  } else if constexpr (REP == kRepRotquat) {
    smpl_quat_to_matrix(xi[0], xi[T], xi[2 * T], xi[3 * T], R);
  } else {                                     // axis_angle_to_matrix: through the quaternion, with its small-angle branch
    const float ax = xi[0], ay = xi[T], az = xi[2 * T];
    const float angle = sqrtf(ax * ax + ay * ay + az * az);
    const float half = 0.5f * angle;
    const float s = fabsf(angle) < 1e-6f ? 0.5f - (angle * angle) / 48.f : sinf(half) / angle;
    smpl_quat_to_matrix(cosf(half), ax * s, ay * s, az * s, R);
  }
}

template <int REP> __global__ __launch_bounds__(kSmplLanes) void smpl_pose_kernel(SmplPoseArgs a) {
  __shared__ float s_g[kSmplSlots * 12 * kSmplLanes];   // [slot][12][lane], as smpl_joints_kernel
  const int lane = threadIdx.x;
  const int gid = blockIdx.x * kSmplLanes + lane;
  const int B = a.B, T = a.T, J = a.J;
  if (gid >= B * T) return;          // (no barrier below)
  const int b = gid / T, t = gid - b * T;
  const int NX = a.NR + a.has_trans;
  const float* xb = a.x + (size_t)b * NX * a.F * T;
  float* feat = a.feat + (size_t)b * a.KP * T + t;
  float* aws = a.aws + (size_t)b * 12 * kSmplMaxJoints * T + t;
  float* jo = a.joints + (size_t)b * a.joints_rows * 3 * T + t;
  float* dl = a.delta + (size_t)b * 3 * T + t;
  if (a.add_trans) {                 // x_translations - x_translations[:, :, [0]]: every frame, masked ones included
    const float* tr = xb + (size_t)a.NR * a.F * T;
    dl[0] = tr[t] - tr[0];
    dl[T] = tr[(size_t)T + t] - tr[T];
    dl[2 * T] = tr[(size_t)2 * T + t] - tr[2 * T];
  } else {
    dl[0] = 0.f;
    dl[T] = 0.f;
    dl[2 * T] = 0.f;
  }
  const bool valid = a.mask == nullptr || a.mask[(size_t)b * T + t] != 0;
  const int NP = (J - 1) * 9;
  if (!valid) {                      // a masked frame contributes nothing: every product of the skinning pass is 0
    for (int k = 0; k < a.KP; ++k) feat[(size_t)k * T] = 0.f;
    for (int k = 0; k < 12 * kSmplMaxJoints; ++k) aws[(size_t)k * T] = 0.f;
    for (int k = 0; k < 3 * J; ++k) jo[(size_t)k * T] = 0.f;
    return;
  }
  float be[kSmplBetas];
#pragma unroll
  for (int l = 0; l < kSmplBetas; ++l)
    be[l] = a.betas != nullptr ? a.betas[((size_t)b * kSmplBetas + l) * T + t] : (l == 1 ? a.beta1 : 0.f);
#pragma unroll
  for (int l = 0; l < kSmplBetas; ++l) feat[(size_t)(NP + l) * T] = be[l];
  feat[(size_t)(NP + kSmplBetas) * T] = 1.f;
  for (int k = NP + kSmplBetas + 1; k < a.KP; ++k) feat[(size_t)k * T] = 0.f;
  for (int i = J; i < kSmplMaxJoints; ++i) {
#pragma unroll
    for (int c = 0; c < 12; ++c) aws[((size_t)c * kSmplMaxJoints + i) * T] = 0.f;
  }
  for (int i = 0; i < J; ++i) {
    float R[3][3];
    if (a.glob) {
      smpl_load_rotation<REP>(xb + (size_t)i * a.F * T + t, T, R);
    } else if (i == 0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = a.grot[3 * r + c];
      }
    } else {
      smpl_load_rotation<REP>(xb + (size_t)(i - 1) * a.F * T + t, T, R);
    }
    if (a.rot_out != nullptr && (a.glob || i > 0)) {
      float* ro = a.rot_out + (((size_t)b * T + t) * a.NR + (a.glob ? i : i - 1)) * 9;
#pragma unroll
      for (int k = 0; k < 9; ++k) ro[k] = R[k / 3][k % 3];
    }
    // rest joints of this shape: J0 + Jdirs . beta (this joint's and its parent's)
    const int p = a.parent[i];
    float ji[3], rel[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = a.j0[3 * i + c];
#pragma unroll
      for (int l = 0; l < kSmplBetas; ++l) v = fmaf(a.jdirs[(3 * i + c) * kSmplBetas + l], be[l], v);
      ji[c] = v;
      rel[c] = v;
    }
    if (i > 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = a.j0[3 * p + c];
#pragma unroll
        for (int l = 0; l < kSmplBetas; ++l) v = fmaf(a.jdirs[(3 * p + c) * kSmplBetas + l], be[l], v);
        rel[c] = ji[c] - v;
      }
    }
    float G[12];                     // G[3r + c] rotation, G[9 + r] translation
    if (i == 0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) G[3 * r + c] = R[r][c];
        G[9 + r] = rel[r];
      }
    } else {
      const float* ps = s_g + (size_t)a.pslot[i] * 12 * kSmplLanes + lane;
      float P[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) P[k] = ps[k * kSmplLanes];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) G[3 * r + c] = P[3 * r] * R[0][c] + P[3 * r + 1] * R[1][c] + P[3 * r + 2] * R[2][c];
        G[9 + r] = P[3 * r] * rel[0] + P[3 * r + 1] * rel[1] + P[3 * r + 2] * rel[2] + P[9 + r];
      }
    }
    if (a.oslot[i] >= 0) {
      float* q = s_g + (size_t)a.oslot[i] * 12 * kSmplLanes + lane;
#pragma unroll
      for (int k = 0; k < 12; ++k) q[k * kSmplLanes] = G[k];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      jo[((size_t)i * 3 + r) * T] = G[9 + r];
      // rel_transforms = transforms - pad(transforms . joints_homogen)
      aws[((size_t)(9 + r) * kSmplMaxJoints + i) * T] = G[9 + r] - (G[3 * r] * ji[0] + G[3 * r + 1] * ji[1] + G[3 * r + 2] * ji[2]);
#pragma unroll
      for (int c = 0; c < 3; ++c) aws[((size_t)(3 * r + c) * kSmplMaxJoints + i) * T] = G[3 * r + c];
    }
    if (i > 0) {                     // pose_feature = rot_mats[:, 1:] - I
#pragma unroll
      for (int k = 0; k < 9; ++k) feat[(size_t)((i - 1) * 9 + k) * T] = R[k / 3][k % 3] - ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f);
    }
  }
}

struct SmplSkinArgs {
  const float* blend;      // [3][KP][Vpad]: B'_c transposed, vertices contiguous, zero beyond K and V
  const float* wt;         // [24][Vpad]: lbs weights transposed, zero beyond J and V
  const float* feat;       // [B][KP][T]
  const float* aws;        // [B][12][24][T]
  const float* delta;      // [B][3][T]
  const uint8_t* mask;     // [B][T] or nullptr
  float* out;
  int T, V, Vpad, KP;
  int tiles_per_sample;    // ceil(T / 32)
  int tile0;               // first frame tile of this launch (blockIdx.x counts from it)
  int mode;                // 0: out [B][out_rows][3][T] at row row_off + v; 1: chunk [tile - tile0][V][3][32], raw
  int out_rows, row_off;
  int finish;              // mode 0: zero masked frames and add delta
};

__global__ __launch_bounds__(kSkinWaves * 64) void smpl_skin_kernel(SmplSkinArgs a) {
  __shared__ float s_p[(kSkinKPMax + 12 * kSmplMaxJoints) * kSkinFrames];   // 65,024 B: [k][frame] features, then [comp][joint][frame]
  float* s_feat = s_p;
  float* s_aws = s_p + a.KP * kSkinFrames;
  const int tid = threadIdx.x;
  const int tile = a.tile0 + blockIdx.x;
  const int b = tile / a.tiles_per_sample;
  const int t0 = (tile - b * a.tiles_per_sample) * kSkinFrames;
  const int T = a.T;
  {
    const int c = tid & 31, t = t0 + c;
    const float* f = a.feat + (size_t)b * a.KP * T;
    for (int k = tid >> 5; k < a.KP; k += kSkinWaves * 2) s_feat[k * kSkinFrames + c] = t < T ? f[(size_t)k * T + t] : 0.f;
    const float* g = a.aws + (size_t)b * 12 * kSmplMaxJoints * T;
    for (int k = tid >> 5; k < 12 * kSmplMaxJoints; k += kSkinWaves * 2) s_aws[k * kSkinFrames + c] = t < T ? g[(size_t)k * T + t] : 0.f;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int t = t0 + r;
  const int nvt = a.Vpad / 32;
  const int vt_end = min((int)(blockIdx.y + 1) * kSkinTiles, nvt);
  const int nkb = a.KP / 4;                         // k blocks of two MFMA steps
  float d[3] = {0.f, 0.f, 0.f};
  bool valid = true;
  if (a.mode == 0 && a.finish && t < T) {
    valid = a.mask == nullptr || a.mask[(size_t)b * T + t] != 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = a.delta[((size_t)b * 3 + c) * T + t];
  }
  for (int vt = blockIdx.y * kSkinTiles + wave; vt < vt_end; vt += kSkinWaves) {
    const int v0 = vt * 32;
    // ---- v_posed = B' . P': lane supplies A[i = r][k = 2 s + h] = blend[c][k][v0 + r], B[k][j = r] = s_feat[k][r]
    const float* bl = a.blend + (size_t)h * a.Vpad + v0 + r;
    const size_t cs = (size_t)a.KP * a.Vpad;       // stride between coordinates
    f32x16 vp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int e = 0; e < 16; ++e) vp[c][e] = 0.f;
    }
    float cur[2][3], nxt[2][3];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int c = 0; c < 3; ++c) cur[u][c] = bl[c * cs + (size_t)(2 * u) * a.Vpad];
    }
    for (int kb = 0; kb < nkb; ++kb) {
      const int kn = min(kb + 1, nkb - 1);          // the next block's operands (the last block re-reads itself)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int c = 0; c < 3; ++c) nxt[u][c] = bl[c * cs + (size_t)(4 * kn + 2 * u) * a.Vpad];
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float pv = s_feat[(4 * kb + 2 * u + h) * kSkinFrames + r];
#pragma unroll
        for (int c = 0; c < 3; ++c) vp[c] = mfma_f32(cur[u][c], pv, vp[c]);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int c = 0; c < 3; ++c) cur[u][c] = nxt[u][c];
      }
    }
    // ---- per-vertex transform, one output row at a time: T_comp = W . A_comp, K = 24
    float w[kSmplMaxJoints / 2];
#pragma unroll
    for (int s = 0; s < kSmplMaxJoints / 2; ++s) w[s] = a.wt[(size_t)(2 * s + h) * a.Vpad + v0 + r];
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      f32x16 acc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
      }
#pragma unroll
      for (int s = 0; s < kSmplMaxJoints / 2; ++s) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int comp = q < 3 ? 3 * rr + q : 9 + rr;
          acc[q] = mfma_f32(w[s], s_aws[(comp * kSmplMaxJoints + 2 * s + h) * kSkinFrames + r], acc[q]);
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int v = v0 + mfma_row(e, h);
        float o = acc[0][e] * vp[0][e] + acc[1][e] * vp[1][e] + acc[2][e] * vp[2][e] + acc[3][e];
        if (v < a.V) {
          if (a.mode == 0) {
            if (a.finish) o = (valid ? o : 0.f) + d[rr];
            if (t < T) a.out[(((size_t)b * a.out_rows + a.row_off + v) * 3 + rr) * T + t] = o;
          } else {
            a.out[(((size_t)(tile - a.tile0) * a.V + v) * 3 + rr) * kSkinFrames + r] = o;
          }
        }
      }
    }
  }
}

// mesh chunk [tiles][V][3][32] -> joints rows row_off .. row_off + ne - 1 of [B][joints_rows][3][T]; grid (tiles, 3, ne), 256 threads:
// 32 frames x 8 vertex slices, each slice summed in vertex order in a register, the slices then summed in slice order
__global__ __launch_bounds__(256) void smpl_extra_kernel(const float* __restrict__ mesh, const float* __restrict__ extra_t,
                                                         float* __restrict__ joints, int T, int V, int ne, int tiles_per_sample, int tile0,
                                                         int joints_rows, int row_off) {
  __shared__ float s_red[8 * 32];
  const int tl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int c = blockIdx.y, e = blockIdx.z;
  const float* m = mesh + ((size_t)blockIdx.x * V * 3 + c) * 32 + tl;
  const float* w = extra_t + e;
  float acc = 0.f;
#pragma unroll 8
  for (int v = sl; v < V; v += 8) acc = fmaf(w[(size_t)v * ne], m[(size_t)v * 96], acc);
  s_red[sl * 32 + tl] = acc;
  __syncthreads();
  if (sl != 0) return;
  const int tile = tile0 + blockIdx.x;
  const int b = tile / tiles_per_sample;
  const int t = (tile - b * tiles_per_sample) * 32 + tl;
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) s += s_red[q * 32 + tl];     // slice order: fixed
  if (t < T) joints[(((size_t)b * joints_rows + row_off + e) * 3 + c) * T + t] = s;
}

struct SmplPointMap {
  int32_t src[kSmplMaxPoints];
};

// out [B][NP][3][T] = joints[map[p]] - joints[map[root]] (0 on masked frames) + delta
__global__ __launch_bounds__(256) void smpl_points_kernel(const float* __restrict__ joints, const float* __restrict__ delta,
                                                          const uint8_t* __restrict__ mask, float* __restrict__ out, int B, int T, int NP,
                                                          int joints_rows, int root, SmplPointMap map) {
  const size_t n = (size_t)B * NP * 3 * T;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int t = (int)(idx % T);
  const int c = (int)((idx / T) % 3);
  const int p = (int)((idx / ((size_t)3 * T)) % NP);
  const int b = (int)(idx / ((size_t)3 * T * NP));
  const float* jb = joints + (size_t)b * joints_rows * 3 * T;
  const bool valid = mask == nullptr || mask[(size_t)b * T + t] != 0;
  float v = 0.f;
  if (valid) v = jb[((size_t)map.src[p] * 3 + c) * T + t] - jb[((size_t)map.src[root] * 3 + c) * T + t];
  out[idx] = v + delta[((size_t)b * 3 + c) * T + t];
}

}  // namespace mdm
