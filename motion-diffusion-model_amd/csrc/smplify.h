// SMPLify fitting of 3-D joints (visualize/simplify_loc2rot.py over visualize/joints2smpl/src/{smplify,customloss,prior}.py) on gfx950:
// the value and the analytic gradient of the two fitting losses in one launch per closure evaluation, the vector updates of
// torch.optim.LBFGS on the flat parameter vector, and the tail that turns the fitted pose into `thetas`.
//
// smplify_eval_kernel<STAGE>: one workgroup of 256 threads per SMF_FRAMES = 32 frames, thread (f = tid & 31, g = tid >> 5).
//   The point is x + t d of the optimiser's flat vector (d may be null), element by element fmaf(t, d, x) -- the statement
//   smplify_step_kernel repeats, so the accepted point of a line search is the evaluated point bit for bit.
//   STAGE 2 first runs the mixture prior (prior.py merged_log_likelihood): for each of the 8 components the frames' d = pose - mean
//   are the 32 rows of A, and Y1 = A P^T, Y2 = A P (the two halves of the gradient of d^T P d; P is an fp32 inverse and not
//   symmetric) are three 32 x 32 tiles each on v_mfma_f32_32x32x2_f32 (common.h mfma_f32: exact fp32, k ascending, rows and k behind
//   69 zero-filled).  One thread per frame adds d . Y1 in ascending order, keeps the minimum (the lowest index on a tie, as
//   torch.min backpropagates) and the frame's threads copy that component's weighted gradient into LDS.
//   Then, all stages: R_j by smplx's batch_rodrigues (angle = |theta + 1e-8|, dir = theta / angle), rest joints J0 + Jdirs beta,
//   batch_rigid_transform's chain one tree level at a time (world rotations overwrite the local ones), the residuals' derivative
//   r_j = dL/dp_j, and per joint k, in ascending order of its descendants d:
//       S_k = sum r_d (d in the subtree of k),    M_k = sum r_d (p_d - p_k)^T (d below k),
//       dL/dR_k = W_parent^T M_k W_k,  dL/drel_k = W_parent^T S_k,  dL/dcam = S_0,
//   through the derivative of batch_rodrigues to theta_k and through Jdirs to beta.  No autograd, no atomics: one thread per frame
//   adds the frame's terms and its share of max|g| and g . d in a fixed order, thread 0 adds the workgroup's frames in order and
//   writes four floats (loss, max|g|, g . d, a non-finite flag) per workgroup; the host adds the workgroups' records in order.
//   A frame's arithmetic does not depend on its position or on T.
//   STAGE 0 is the start of a fit: the inputs' finiteness, the kinematic chain at the initial pose and guess_init_3d.
// smplify_direction_kernel: one workgroup; the y / s / ys / H_diag update of the history (a ring in the workspace), the two-loop
//   recursion over up to `history` pairs, prev_flat_grad, and g . d, max|d|, |g|_1 of the new direction -- every dot product per
//   thread over its strided elements, then a tree over the threads: one fixed order for a given n.
// smplify_step_kernel: x += t d.  smplify_tail_kernel: axis-angle -> matrix through the quaternion
//   (utils/rotation_conversions.axis_angle_to_matrix), its first two rows as rot6d, row 24 = (j3d[:, 0], 0, 0, 0).
// No kernel waits for another workgroup.
#pragma once
#include "common.h"
#include "smpl_mesh.h"

namespace mdm {

constexpr int SMF_FRAMES = 32;      // frames per workgroup: the rows of an MFMA tile
constexpr int SMF_THREADS = 256;
constexpr int SMF_GROUPS = SMF_THREADS / SMF_FRAMES;
constexpr int SMF_J = 24;           // model joints
constexpr int SMF_FIT = 22;         // joints the stage-2 loss reads (config.amass_smpl_idx)
constexpr int SMF_BODY = 69;        // body_pose
constexpr int SMF_BETAS = 10;
constexpr int SMF_GMM = 8;
constexpr int SMF_ROW = 72;         // floats per frame of a [frames][69 or 24 x 3] LDS array
constexpr int SMF_TERMS = 6;        // stage 2: joints, prior, angle, shape, preserve, total; stage 1: joints, depth, 0, 0, 0, total
constexpr int SMF_REC = 4;          // floats per workgroup record: loss, max|g|, g . d, non-finite
constexpr int SMF_YLD = 192;        // floats per frame of the prior's products: Y1 at 0, Y2 at 96

struct SmplifyEvalArgs {
  // model
  const float* j0;        // [24][3]
  const float* jdirs;     // [24][3][10]
  const float* means;     // [8][69]
  const float* prec;      // [8][69][69]
  const float* nlw;       // [8]: -log(nll_weights)
  int32_t parent[SMF_J];
  uint32_t anc[SMF_J];    // bit a of anc[d]: a is d or an ancestor of d
  uint8_t lvl_joint[SMF_J];   // the joints sorted by depth in the tree ...
  uint8_t lvl_start[SMF_J + 2];  // ... and where each depth starts
  int32_t nlvl;
  // the point: x + t d of the flat vector; a group with offset < 0 is not a variable and comes from fix_*
  const float* x;
  const float* d;         // or nullptr
  float t;
  int32_t off_body, off_betas, off_go, off_cam;   // [T][69], [T][10], [T][3], [T][3] blocks of the flat vector
  const float* fix_body;  // [T][69]
  const float* fix_betas; // [T][10]
  // data
  const float* j3d;       // [T][22][3]
  const float* conf;      // [22]
  const float* cam_est;   // [T][3]   (stage 1)
  const float* preserve;  // [T][69]  (stage 2)
  float w_joint, sigma2, w_prior, w_angle, w_shape, w_preserve, w_depth;   // the squared weights
  // outputs
  float* grad;            // flat layout, or nullptr
  float* terms;           // [T][SMF_TERMS], or nullptr
  float* joints;          // [T][24][3] model joints, or nullptr
  float* cam_out;         // STAGE 0: guess_init_3d [T][3] ...
  float* cam_out2;        // ... and a second copy (the camera block of the stage-1 vector), or nullptr
  float* partial;         // [workgroups][SMF_REC]
  int32_t T;
};

__device__ __forceinline__ float smf_point(const SmplifyEvalArgs& a, int i) {
  return a.d != nullptr ? fmaf(a.t, a.d[i], a.x[i]) : a.x[i];
}
__device__ __forceinline__ float smf_body(const SmplifyEvalArgs& a, int fr, int i) {
  return a.off_body >= 0 ? smf_point(a, a.off_body + fr * SMF_BODY + i) : a.fix_body[(size_t)fr * SMF_BODY + i];
}
__device__ __forceinline__ float smf_beta(const SmplifyEvalArgs& a, int fr, int l) {
  return a.off_betas >= 0 ? smf_point(a, a.off_betas + fr * SMF_BETAS + l) : a.fix_betas[(size_t)fr * SMF_BETAS + l];
}
// component c of joint k's axis-angle: the global orient, then the body pose
__device__ __forceinline__ float smf_theta(const SmplifyEvalArgs& a, int fr, int k, int c) {
  return k == 0 ? smf_point(a, a.off_go + fr * 3 + c) : smf_body(a, fr, (k - 1) * 3 + c);
}
__device__ __forceinline__ bool smf_finite(float v) { return fabsf(v) <= 3.4028234664e38f; }   // false for NaN and +-inf

// smplx batch_rodrigues of one vector
struct SmfRod { float rx, ry, rz, angle, s, c; };
__device__ __forceinline__ SmfRod smf_rodrigues(float tx, float ty, float tz, float R[9]) {
  const float ax = tx + 1e-8f, ay = ty + 1e-8f, az = tz + 1e-8f;
  SmfRod q;
  q.angle = sqrtf(ax * ax + ay * ay + az * az);
  q.rx = tx / q.angle; q.ry = ty / q.angle; q.rz = tz / q.angle;
  q.s = sinf(q.angle);
  q.c = cosf(q.angle);
  const float oc = 1.f - q.c, rx = q.rx, ry = q.ry, rz = q.rz;
  R[0] = 1.f + oc * (-rz * rz - ry * ry);
  R[1] = q.s * -rz + oc * (ry * rx);
  R[2] = q.s * ry + oc * (rz * rx);
  R[3] = q.s * rz + oc * (rx * ry);
  R[4] = 1.f + oc * (-rz * rz - rx * rx);
  R[5] = q.s * -rx + oc * (rz * ry);
  R[6] = q.s * -ry + oc * (rx * rz);
  R[7] = q.s * rx + oc * (ry * rz);
  R[8] = 1.f + oc * (-ry * ry - rx * rx);
  return q;
}

// dL/dtheta from G = dL/dR through R = I + sin K + (1 - cos) K^2, dir = theta / angle, angle = |theta + 1e-8|
__device__ __forceinline__ void smf_rodrigues_grad(float tx, float ty, float tz, const float G[9], float out[3]) {
  float R[9];
  const SmfRod q = smf_rodrigues(tx, ty, tz, R);
  const float rx = q.rx, ry = q.ry, rz = q.rz, oc = 1.f - q.c;
  const float K[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
  const float KK[9] = {-rz * rz - ry * ry, ry * rx, rz * rx, rx * ry, -rz * rz - rx * rx, rz * ry, rx * rz, ry * rz, -ry * ry - rx * rx};
  float gs = 0.f, goc = 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    gs = fmaf(G[i], K[i], gs);
    goc = fmaf(G[i], KK[i], goc);
  }
  // dL/dK = sin G + (1 - cos) (G K^T + K^T G)
  float GK[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = 0.f;
#pragma unroll
      for (int m = 0; m < 3; ++m) v = fmaf(G[3 * r + m], K[3 * c + m], v);     // G K^T
#pragma unroll
      for (int m = 0; m < 3; ++m) v = fmaf(K[3 * m + r], G[3 * m + c], v);     // K^T G
      GK[3 * r + c] = fmaf(q.s, G[3 * r + c], oc * v);
    }
  const float gx = GK[7] - GK[5], gy = GK[2] - GK[6], gz = GK[3] - GK[1];
  const float gang = fmaf(q.c, gs, q.s * goc) - (gx * rx + gy * ry + gz * rz) / q.angle;
  out[0] = fmaf(gang, (tx + 1e-8f) / q.angle, gx / q.angle);
  out[1] = fmaf(gang, (ty + 1e-8f) / q.angle, gy / q.angle);
  out[2] = fmaf(gang, (tz + 1e-8f) / q.angle, gz / q.angle);
}

// out = A B, out = A^T B (3 x 3, row-major)
__device__ __forceinline__ void smf_mm(const float* A, const float* B, float* out) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * r + c] = fmaf(A[3 * r + 2], B[6 + c], fmaf(A[3 * r + 1], B[3 + c], A[3 * r] * B[c]));
}
__device__ __forceinline__ void smf_mtm(const float* A, const float* B, float* out) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * r + c] = fmaf(A[6 + r], B[6 + c], fmaf(A[3 + r], B[3 + c], A[r] * B[c]));
}

template <int STAGE> __global__ __launch_bounds__(SMF_THREADS) void smplify_eval_kernel(SmplifyEvalArgs a) {
  // [frames][24][9] rotations | [frames][72] relative rest joints | [frames][72] positions | [frames][72] dL/dp | [frames][72] prior
  // gradient.  The prior phase lays its products, its operand and the pose over the first three; behind the joints' pass the
  // frame's gradient lies over the rotations, dL/drel over dL/dp and the joints' loss terms over the relative joints.
  constexpr int kRW = 0, kREL = SMF_FRAMES * 216, kPOS = kREL + SMF_FRAMES * SMF_ROW, kRJ = kPOS + SMF_FRAMES * SMF_ROW,
                kGP = kRJ + SMF_FRAMES * SMF_ROW, kTotal = kGP + SMF_FRAMES * SMF_ROW;
  static_assert(SMF_FRAMES * SMF_YLD <= kREL, "the prior's products fit over the rotations");
  __shared__ __attribute__((aligned(16))) float smem[kTotal];
  __shared__ float red[SMF_FRAMES][SMF_REC];
  __shared__ int take[SMF_FRAMES];
  float* RW = smem + kRW;
  float* REL = smem + kREL;
  float* POS = smem + kPOS;
  float* RJ = smem + kRJ;
  float* GP = smem + kGP;

  const int tid = threadIdx.x, f = tid & (SMF_FRAMES - 1), g = tid >> 5;
  const int fr = (int)blockIdx.x * SMF_FRAMES + f;
  const bool valid = fr < a.T;
  const int frc = valid ? fr : a.T - 1;      // a frame behind T computes on the last frame's values and stores nothing
  float prior_val = 0.f;

  if constexpr (STAGE == 2) {
    float* Y = smem + kRW;       // [frames][SMF_YLD]
    float* A = smem + kREL;      // [frames][72]: pose - mean, zeros behind 69
    float* POSE = smem + kPOS;   // [frames][72]
    const int lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    for (int i = g; i < SMF_ROW; i += SMF_GROUPS) POSE[f * SMF_ROW + i] = (i < SMF_BODY && valid) ? smf_body(a, frc, i) : 0.f;
    float best = 0.f;
    for (int m = 0; m < SMF_GMM; ++m) {
      __syncthreads();           // POSE is written; the previous component's A and Y are no longer read
      for (int i = g; i < SMF_ROW; i += SMF_GROUPS)
        A[f * SMF_ROW + i] = (i < SMF_BODY && valid) ? POSE[f * SMF_ROW + i] - a.means[m * SMF_BODY + i] : 0.f;
      __syncthreads();
      const float* P = a.prec + (size_t)m * SMF_BODY * SMF_BODY;
      for (int tile = wave; tile < 6; tile += SMF_THREADS / 64) {
        const int which = tile / 3, col = (tile % 3) * 32 + li;
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        for (int k0 = 0; k0 < SMF_BODY + 1; k0 += 2) {
          const int k = k0 + lh;
          float b = 0.f;
          if (col < SMF_BODY && k < SMF_BODY) b = which == 0 ? P[col * SMF_BODY + k] : P[k * SMF_BODY + col];
          acc = mfma_f32(A[li * SMF_ROW + k], b, acc);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) Y[mfma_row(e, lh) * SMF_YLD + which * 96 + col] = acc[e];
      }
      __syncthreads();
      if (g == 0) {
        float q = 0.f;
        for (int i = 0; i < SMF_BODY; ++i) q = fmaf(Y[f * SMF_YLD + i], A[f * SMF_ROW + i], q);
        const float ll = 0.5f * q + a.nlw[m];
        const int better = (m == 0 || ll < best) ? 1 : 0;
        if (better) best = ll;
        take[f] = better;
      }
      __syncthreads();
      if (take[f])
        for (int i = g; i < SMF_BODY; i += SMF_GROUPS) GP[f * SMF_ROW + i] = a.w_prior * (0.5f * (Y[f * SMF_YLD + i] + Y[f * SMF_YLD + 96 + i]));
    }
    prior_val = a.w_prior * best;
    __syncthreads();             // the products and the operand make room for the joints' pass
  }

  // ---- rotations and rest joints
  bool finite = true;
  for (int k = g; k < SMF_J; k += SMF_GROUPS) {
    const float tx = smf_theta(a, frc, k, 0), ty = smf_theta(a, frc, k, 1), tz = smf_theta(a, frc, k, 2);
    float R[9];
    smf_rodrigues(tx, ty, tz, R);
#pragma unroll
    for (int i = 0; i < 9; ++i) RW[(f * SMF_J + k) * 9 + i] = R[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = a.j0[k * 3 + c];
      for (int l = 0; l < SMF_BETAS; ++l) v = fmaf(a.jdirs[(k * 3 + c) * SMF_BETAS + l], smf_beta(a, frc, l), v);
      POS[f * SMF_ROW + k * 3 + c] = v;
    }
    if constexpr (STAGE == 0) {
      finite = finite && smf_finite(tx) && smf_finite(ty) && smf_finite(tz);
      if (k < SMF_FIT)
#pragma unroll
        for (int c = 0; c < 3; ++c) finite = finite && smf_finite(a.j3d[((size_t)frc * SMF_FIT + k) * 3 + c]);
      if (k < SMF_BETAS) finite = finite && smf_finite(smf_beta(a, frc, k));
      if (k < SMF_FIT) finite = finite && smf_finite(a.conf[k]);
    }
  }
  __syncthreads();
  for (int k = g; k < SMF_J; k += SMF_GROUPS) {
    const int p = a.parent[k];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      REL[f * SMF_ROW + k * 3 + c] = k == 0 ? POS[f * SMF_ROW + c] : POS[f * SMF_ROW + k * 3 + c] - POS[f * SMF_ROW + p * 3 + c];
  }
  __syncthreads();
  // ---- the chain, one depth of the tree at a time: W_k = W_p R_k in place, p_k = p_p + W_p rel_k
  if (g == 0)
#pragma unroll
    for (int c = 0; c < 3; ++c) POS[f * SMF_ROW + c] = REL[f * SMF_ROW + c];
  for (int lv = 1; lv < a.nlvl; ++lv) {
    __syncthreads();
    for (int idx = a.lvl_start[lv] + g; idx < a.lvl_start[lv + 1]; idx += SMF_GROUPS) {
      const int k = a.lvl_joint[idx], p = a.parent[k];
      float Wp[9], Rk[9], Wk[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        Wp[i] = RW[(f * SMF_J + p) * 9 + i];
        Rk[i] = RW[(f * SMF_J + k) * 9 + i];
      }
      smf_mm(Wp, Rk, Wk);
#pragma unroll
      for (int i = 0; i < 9; ++i) RW[(f * SMF_J + k) * 9 + i] = Wk[i];
      const float* rel = REL + f * SMF_ROW + k * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        POS[f * SMF_ROW + k * 3 + c] =
            fmaf(Wp[3 * c + 2], rel[2], fmaf(Wp[3 * c + 1], rel[1], fmaf(Wp[3 * c], rel[0], POS[f * SMF_ROW + p * 3 + c])));
    }
  }
  __syncthreads();
  if (a.joints != nullptr && valid)
    for (int i = g; i < SMF_ROW; i += SMF_GROUPS) a.joints[(size_t)fr * SMF_ROW + i] = POS[f * SMF_ROW + i];

  if constexpr (STAGE == 0) {
    // guess_init_3d: the mean offset of the hips and shoulders (joints 2, 1, 17, 16), and the inputs' finiteness
    red[f][3] = 0.f;
    __syncthreads();
    if (!finite && valid) red[f][3] = 1.f;     // (any of the frame's threads; they store the same value)
    if (g == 0 && valid) {
      const int sel[4] = {2, 1, 17, 16};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) s += a.j3d[((size_t)fr * SMF_FIT + sel[i]) * 3 + c] - POS[f * SMF_ROW + sel[i] * 3 + c];
        a.cam_out[(size_t)fr * 3 + c] = s / 4.0f;
        if (a.cam_out2 != nullptr) a.cam_out2[(size_t)fr * 3 + c] = s / 4.0f;
      }
    }
    __syncthreads();
    if (tid == 0) {
      float bad = 0.f;
      const int nf = min(SMF_FRAMES, a.T - (int)blockIdx.x * SMF_FRAMES);
      for (int i = 0; i < nf; ++i) bad = fmaxf(bad, red[i][3]);
      float* out = a.partial + (size_t)blockIdx.x * SMF_REC;
      out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; out[3] = bad;
    }
    return;
  } else {
    // ---- r_k = dL/dp_k and the joints' loss terms (over the relative joints, which the chain no longer needs)
    float* LK = REL;
    const float cam[3] = {smf_point(a, a.off_cam + frc * 3), smf_point(a, a.off_cam + frc * 3 + 1), smf_point(a, a.off_cam + frc * 3 + 2)};
    for (int k = g; k < SMF_J; k += SMF_GROUPS) {
      float r[3] = {0.f, 0.f, 0.f}, lk = 0.f;
      if (STAGE == 2 ? k < SMF_FIT : (k == 1 || k == 2 || k == 16 || k == 17)) {
        const float cf = STAGE == 2 ? a.conf[k] : 1.f;
        float e = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float target = a.j3d[((size_t)frc * SMF_FIT + k) * 3 + c], model = POS[f * SMF_ROW + k * 3 + c] + cam[c];
          if constexpr (STAGE == 2) {
            const float x = model - target, x2 = x * x, den = a.sigma2 + x2;     // gmof
            e += (a.sigma2 * x2) / den;
            r[c] = a.w_joint * ((cf * cf) * ((2.f * a.sigma2 * a.sigma2) * x / (den * den)));
          } else {
            const float x = target - model;
            e += x * x;
            r[c] = -2.f * x;
          }
        }
        lk = STAGE == 2 ? a.w_joint * ((cf * cf) * e) : e;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) RJ[f * SMF_ROW + k * 3 + c] = r[c];
      LK[f * SMF_ROW + k] = lk;
    }
    __syncthreads();
    // ---- per joint: the subtree sums and the gradient of its rotation
    float gth[3][3], ek[3][3];
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {
      const int k = g + SMF_GROUPS * jj;
      float S[3] = {0.f, 0.f, 0.f}, M[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const float pk[3] = {POS[f * SMF_ROW + k * 3], POS[f * SMF_ROW + k * 3 + 1], POS[f * SMF_ROW + k * 3 + 2]};
      for (int dsc = k; dsc < SMF_J; ++dsc) {
        if (((a.anc[dsc] >> k) & 1u) == 0) continue;
        const float* r = RJ + f * SMF_ROW + dsc * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) S[c] += r[c];
        if (dsc != k) {
          const float dp[3] = {POS[f * SMF_ROW + dsc * 3] - pk[0], POS[f * SMF_ROW + dsc * 3 + 1] - pk[1], POS[f * SMF_ROW + dsc * 3 + 2] - pk[2]};
#pragma unroll
          for (int r0 = 0; r0 < 3; ++r0)
#pragma unroll
            for (int c = 0; c < 3; ++c) M[3 * r0 + c] = fmaf(r[r0], dp[c], M[3 * r0 + c]);
        }
      }
      const float* Wk = RW + (f * SMF_J + k) * 9;
      float G[9];
      if (k == 0) {
        smf_mm(M, Wk, G);
#pragma unroll
        for (int c = 0; c < 3; ++c) ek[jj][c] = S[c];
      } else {
        const float* Wp = RW + (f * SMF_J + a.parent[k]) * 9;
        float MW[9];
        smf_mm(M, Wk, MW);
        smf_mtm(Wp, MW, G);
#pragma unroll
        for (int c = 0; c < 3; ++c) ek[jj][c] = fmaf(Wp[6 + c], S[2], fmaf(Wp[3 + c], S[1], Wp[c] * S[0]));
      }
      gth[jj][0] = gth[jj][1] = gth[jj][2] = 0.f;
      if (STAGE == 2 || k == 0)
        smf_rodrigues_grad(smf_theta(a, frc, k, 0), smf_theta(a, frc, k, 1), smf_theta(a, frc, k, 2), G, gth[jj]);
    }
    __syncthreads();             // the rotations, positions and dL/dp are no longer read
    float* GO = RW + f * 216;    // the frame's gradient in the order body, betas, global orient, camera (stage 1: orient, camera)
    float* E = RJ;               // dL/drel
    constexpr int kGoAt = STAGE == 2 ? SMF_BODY + SMF_BETAS : 0;
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {
      const int k = g + SMF_GROUPS * jj;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        E[f * SMF_ROW + k * 3 + c] = ek[jj][c];
        if (k == 0) {
          GO[kGoAt + c] = gth[jj][c];
          GO[kGoAt + 3 + c] = STAGE == 2 ? ek[jj][c] : fmaf(4.f * a.w_depth, 2.f * (cam[c] - a.cam_est[(size_t)frc * 3 + c]), ek[jj][c]);
        } else if (STAGE == 2) {
          const int i = (k - 1) * 3 + c;
          const float pose = smf_body(a, frc, i);
          float v = gth[jj][c] + GP[f * SMF_ROW + i];
          if (i == 52 || i == 55 || i == 9 || i == 12) {          // angle_prior: exp(s pose)^2, s = (1, -1, -1, -1)
            const float sg = i == 52 ? 1.f : -1.f, ex = expf(pose * sg);
            v += a.w_angle * (2.f * (ex * ex) * sg);
          }
          v += a.w_preserve * (2.f * (pose - a.preserve[(size_t)frc * SMF_BODY + i]));
          GO[i] = v;
        }
      }
    }
    __syncthreads();
    if constexpr (STAGE == 2) {
      for (int l = g; l < SMF_BETAS; l += SMF_GROUPS) {
        float v = 0.f;
        for (int k = 0; k < SMF_J; ++k)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float dir = a.jdirs[(k * 3 + c) * SMF_BETAS + l] - (k == 0 ? 0.f : a.jdirs[(a.parent[k] * 3 + c) * SMF_BETAS + l]);
            v = fmaf(E[f * SMF_ROW + k * 3 + c], dir, v);
          }
        GO[SMF_BODY + l] = fmaf(a.w_shape, 2.f * smf_beta(a, frc, l), v);
      }
      __syncthreads();
    }
    // ---- the frame's gradient to the flat vector; its terms and its share of the three scalars in one fixed order
    constexpr int kVars = STAGE == 2 ? SMF_BODY + SMF_BETAS + 6 : 6;
    if (valid && a.grad != nullptr)
      for (int i = g; i < kVars; i += SMF_GROUPS) {
        int at;
        if (STAGE == 2 && i < SMF_BODY) at = a.off_body + fr * SMF_BODY + i;
        else if (STAGE == 2 && i < SMF_BODY + SMF_BETAS) at = a.off_betas + fr * SMF_BETAS + (i - SMF_BODY);
        else if (i < kGoAt + 3) at = a.off_go + fr * 3 + (i - kGoAt);
        else at = a.off_cam + fr * 3 + (i - kGoAt - 3);
        a.grad[at] = GO[i];
      }
    if (g == 0) {
      float t_joint = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f, t4 = 0.f, total;
      for (int k = 0; k < SMF_J; ++k) t_joint += LK[f * SMF_ROW + k];
      if constexpr (STAGE == 2) {
        t1 = prior_val;
        const int ai[4] = {52, 55, 9, 12};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float ex = expf(smf_body(a, frc, ai[i]) * (i == 0 ? 1.f : -1.f));
          t2 += ex * ex;
        }
        t2 = a.w_angle * t2;
        for (int l = 0; l < SMF_BETAS; ++l) {
          const float b = smf_beta(a, frc, l);
          t3 = fmaf(b, b, t3);
        }
        t3 = a.w_shape * t3;
        for (int i = 0; i < SMF_BODY; ++i) {
          const float dv = smf_body(a, frc, i) - a.preserve[(size_t)frc * SMF_BODY + i];
          t4 = fmaf(dv, dv, t4);
        }
        t4 = a.w_preserve * t4;
        total = (((t_joint + t1) + t2) + t3) + t4;
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float dv = cam[c] - a.cam_est[(size_t)frc * 3 + c];
          t1 = fmaf(dv, dv, t1);
        }
        t1 = a.w_depth * t1;
        total = fmaf(4.f, t1, t_joint);       // the reference adds its [T, 1, 3] depth term to the [T, 4, 3] joint errors: four times
      }
      float gmax = 0.f, gd = 0.f;
      bool fin = smf_finite(total);
      for (int i = 0; i < kVars; ++i) {
        const float v = GO[i];
        gmax = fmaxf(gmax, fabsf(v));
        fin = fin && smf_finite(v);
        if (a.d != nullptr) {
          int at;
          if (STAGE == 2 && i < SMF_BODY) at = a.off_body + frc * SMF_BODY + i;
          else if (STAGE == 2 && i < SMF_BODY + SMF_BETAS) at = a.off_betas + frc * SMF_BETAS + (i - SMF_BODY);
          else if (i < kGoAt + 3) at = a.off_go + frc * 3 + (i - kGoAt);
          else at = a.off_cam + frc * 3 + (i - kGoAt - 3);
          gd = fmaf(v, a.d[at], gd);
        }
      }
      fin = fin && smf_finite(gd);
      red[f][0] = total; red[f][1] = gmax; red[f][2] = gd; red[f][3] = fin ? 0.f : 1.f;
      if (valid && a.terms != nullptr) {
        float* o = a.terms + (size_t)fr * SMF_TERMS;
        o[0] = t_joint; o[1] = t1; o[2] = t2; o[3] = t3; o[4] = t4; o[5] = total;
      }
    }
    __syncthreads();
    if (tid == 0) {
      float loss = 0.f, gmax = 0.f, gd = 0.f, bad = 0.f;
      const int nf = min(SMF_FRAMES, a.T - (int)blockIdx.x * SMF_FRAMES);
      for (int i = 0; i < nf; ++i) {
        loss += red[i][0];
        gmax = fmaxf(gmax, red[i][1]);
        gd += red[i][2];
        bad = fmaxf(bad, red[i][3]);
      }
      float* out = a.partial + (size_t)blockIdx.x * SMF_REC;
      out[0] = loss; out[1] = gmax; out[2] = gd; out[3] = bad;
    }
  }
}

// ---- the L-BFGS vector updates ------------------------------------------------------------------------------------------------
constexpr int SMF_DIR_REC = 8;        // floats: g . d, max|d|, |g|_1, ys, pairs in the history
constexpr int SMF_HIST_MAX = 128;

struct SmplifyDirArgs {
  const float* g;        // flat_grad
  float* prev_g;         // prev_flat_grad
  float* d;              // the direction: the previous one on entry, the new one on return
  float* hist_y;         // [history][n] old_dirs, a ring
  float* hist_s;         // [history][n] old_stps
  float* ro;             // [history]
  float* hdiag;          // [1]
  int32_t* ring;         // [2]: first slot, pairs
  float* rec;            // [SMF_DIR_REC]
  float t;               // the previous iteration's step length
  int32_t n, history, first;
};

template <int NT> __device__ __forceinline__ float smf_block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}
template <int NT> __device__ __forceinline__ float smf_block_max(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  return red[0];
}

template <int NT> __global__ __launch_bounds__(NT) void smplify_direction_kernel(SmplifyDirArgs a) {
  __shared__ float red[NT];
  __shared__ float al[SMF_HIST_MAX];
  const int tid = threadIdx.x, n = a.n;
  int head = 0, cnt = 0;
  float hd = 1.f, ys = 0.f;
  if (a.first) {
    for (int i = tid; i < n; i += NT) {
      const float gv = a.g[i];
      a.d[i] = -gv;
      a.prev_g[i] = gv;
    }
  } else {
    head = a.ring[0];
    cnt = a.ring[1];
    hd = a.hdiag[0];
    float pys = 0.f, pyy = 0.f;
    for (int i = tid; i < n; i += NT) {
      const float y = a.g[i] - a.prev_g[i], s = a.d[i] * a.t;
      pys = fmaf(y, s, pys);
      pyy = fmaf(y, y, pyy);
    }
    ys = smf_block_sum<NT>(pys, red);
    const float yy = smf_block_sum<NT>(pyy, red);
    __syncthreads();
    if (ys > 1e-10f) {
      int slot;
      if (cnt == a.history) { slot = head; head = (head + 1) % a.history; }
      else { slot = (head + cnt) % a.history; ++cnt; }
      for (int i = tid; i < n; i += NT) {
        a.hist_y[(size_t)slot * n + i] = a.g[i] - a.prev_g[i];
        a.hist_s[(size_t)slot * n + i] = a.d[i] * a.t;
      }
      hd = ys / yy;
      if (tid == 0) a.ro[slot] = 1.0f / ys;
    }
    __syncthreads();              // ro[slot] is visible to the workgroup
    for (int i = tid; i < n; i += NT) {
      const float gv = a.g[i];
      a.prev_g[i] = gv;
      a.d[i] = -gv;                // q
    }
    for (int j = cnt - 1; j >= 0; --j) {
      const int slot = (head + j) % a.history;
      const float* S = a.hist_s + (size_t)slot * n;
      const float* Yv = a.hist_y + (size_t)slot * n;
      float p = 0.f;
      for (int i = tid; i < n; i += NT) p = fmaf(S[i], a.d[i], p);
      const float alj = smf_block_sum<NT>(p, red) * a.ro[slot];
      if (tid == 0) al[j] = alj;
      for (int i = tid; i < n; i += NT) a.d[i] = fmaf(-alj, Yv[i], a.d[i]);
    }
    // (not vectorised: two elements at a time become a packed fp32 multiply, which this library keeps out of its binary)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int i = tid; i < n; i += NT) a.d[i] = a.d[i] * hd;
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const int slot = (head + j) % a.history;
      const float* S = a.hist_s + (size_t)slot * n;
      const float* Yv = a.hist_y + (size_t)slot * n;
      float p = 0.f;
      for (int i = tid; i < n; i += NT) p = fmaf(Yv[i], a.d[i], p);
      const float be = smf_block_sum<NT>(p, red) * a.ro[slot];
      const float co = al[j] - be;
      for (int i = tid; i < n; i += NT) a.d[i] = fmaf(co, S[i], a.d[i]);
    }
  }
  float pgd = 0.f, pmax = 0.f, pl1 = 0.f;
  for (int i = tid; i < n; i += NT) {
    const float gv = a.g[i], dv = a.d[i];
    pgd = fmaf(gv, dv, pgd);
    pmax = fmaxf(pmax, fabsf(dv));
    pl1 += fabsf(gv);
  }
  const float gd = smf_block_sum<NT>(pgd, red);
  const float dmax = smf_block_max<NT>(pmax, red);
  const float l1 = smf_block_sum<NT>(pl1, red);
  if (tid == 0) {
    a.ring[0] = head;
    a.ring[1] = cnt;
    a.hdiag[0] = hd;
    a.rec[0] = gd; a.rec[1] = dmax; a.rec[2] = l1; a.rec[3] = ys; a.rec[4] = (float)cnt;
  }
}

// x += t d, the statement smf_point evaluates
__global__ __launch_bounds__(256) void smplify_step_kernel(float* x, const float* d, float t, int n) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i < n) x[i] = fmaf(t, d[i], x[i]);
}

// The start of a stage: the flat vector from its parts.  Stage 1: [orient | camera] from init_pose [T][72] and the camera guess;
// stage 2: [body | betas | orient | camera] from the stage-1 vector and the fixed parts.
struct SmplifyPackArgs {
  const float* init_pose;   // [T][72]
  const float* init_betas;  // [T][10]
  const float* cam;         // [T][3] the stage-1 camera block, or nullptr: left to smplify_eval_kernel<0>
  const float* x1;          // the stage-1 vector
  float* body;              // [T][69]: body pose of the initial pose (fixed in stage 1, preserve_pose in stage 2)
  float* betas;             // [T][10]
  float* x;                 // the vector to fill
  int32_t T, stage;
};

__global__ __launch_bounds__(256) void smplify_pack_kernel(SmplifyPackArgs a) {
  const int fr = (int)blockIdx.x, T = a.T;
  for (int i = threadIdx.x; i < 85; i += 256) {
    if (a.stage == 1) {
      if (i < SMF_BODY) a.body[(size_t)fr * SMF_BODY + i] = a.init_pose[(size_t)fr * 72 + 3 + i];
      else if (i < SMF_BODY + SMF_BETAS) a.betas[(size_t)fr * SMF_BETAS + i - SMF_BODY] = a.init_betas[(size_t)fr * SMF_BETAS + i - SMF_BODY];
      else if (i < 82) a.x[fr * 3 + i - 79] = a.init_pose[(size_t)fr * 72 + i - 79];
      else if (a.cam != nullptr) a.x[T * 3 + fr * 3 + i - 82] = a.cam[(size_t)fr * 3 + i - 82];
    } else {
      if (i < SMF_BODY) a.x[fr * SMF_BODY + i] = a.body[(size_t)fr * SMF_BODY + i];
      else if (i < 79) a.x[T * SMF_BODY + fr * SMF_BETAS + i - SMF_BODY] = a.betas[(size_t)fr * SMF_BETAS + i - SMF_BODY];
      else if (i < 82) a.x[T * 79 + fr * 3 + i - 79] = a.x1[fr * 3 + i - 79];
      else a.x[T * 82 + fr * 3 + i - 82] = a.x1[T * 3 + fr * 3 + i - 82];
    }
  }
}

struct SmplifyTailArgs {
  const float* x;          // the stage-2 vector
  const float* j3d;        // [T][22][3]
  float* pose;             // [T][72]: orient | body
  float* betas;            // [T][10]
  float* cam;              // [T][3]
  float* thetas;           // [25][6][T]
  int32_t T;
};

__global__ __launch_bounds__(256) void smplify_tail_kernel(SmplifyTailArgs a) {
  const int fr = (int)blockIdx.x, T = a.T;
  const float* body = a.x + (size_t)fr * SMF_BODY;
  const float* go = a.x + (size_t)T * 79 + fr * 3;
  for (int i = threadIdx.x; i < 85; i += 256) {
    if (i < SMF_BODY) a.pose[(size_t)fr * 72 + 3 + i] = body[i];
    else if (i < 79) a.betas[(size_t)fr * SMF_BETAS + i - SMF_BODY] = a.x[(size_t)T * SMF_BODY + fr * SMF_BETAS + i - SMF_BODY];
    else if (i < 82) a.pose[(size_t)fr * 72 + i - 79] = go[i - 79];
    else a.cam[(size_t)fr * 3 + i - 82] = a.x[(size_t)T * 82 + fr * 3 + i - 82];
  }
  const int k = threadIdx.x;
  if (k < SMF_J) {            // axis_angle_to_matrix through the quaternion; matrix_to_rotation_6d: the first two rows
    const float* th = k == 0 ? go : body + (k - 1) * 3;
    const float ax = th[0], ay = th[1], az = th[2];
    const float angle = sqrtf(ax * ax + ay * ay + az * az);
    const float half = 0.5f * angle;
    const float s = fabsf(angle) < 1e-6f ? 0.5f - (angle * angle) / 48.f : sinf(half) / angle;
    float R[3][3];
    smpl_quat_to_matrix(cosf(half), ax * s, ay * s, az * s, R);
#pragma unroll
    for (int c = 0; c < 6; ++c) a.thetas[((size_t)k * 6 + c) * T + fr] = R[c / 3][c % 3];
  } else if (k == SMF_J) {
#pragma unroll
    for (int c = 0; c < 6; ++c) a.thetas[((size_t)SMF_J * 6 + c) * T + fr] = c < 3 ? a.j3d[(size_t)fr * SMF_FIT * 3 + c] : 0.f;
  }
}

}  // namespace mdm
