// The inverse of motion_recover.h: joint positions -> HumanML3D / KIT feature vectors, on the device.  Restates
//     extract_features   data_loaders/humanml/scripts/motion_process.py:43-170
//     process_file       motion_process.py:173-355 (uniform_skeleton :17-40, floor, xz origin, initial facing onto +Z)
//     Skeleton.inverse_kinematics_np / forward_kinematics_np   data_loaders/humanml/common/skeleton.py:55-104, :129-150
//     qbetween, qnormalize, qmul, qinv, qrot, quaternion_to_matrix, quaternion_to_cont6d   common/quaternion.py
// The reference does this per clip on the host, in float64 numpy glue around fp32 torch quaternions; here one workgroup owns one
// clip, one lane one frame (strided), frames are the contiguous axis of the input [B, J, 3, T] and of the output [B, F, 1, T-1], so
// every load and store is coalesced.  Two launches:
//   motion_canon_kernel     (only when process_file's transform is asked for) retargeting IK + FK, the floor reduction over the
//                           clip, frame 0's root xz and facing -> canonicalised positions, fp64, in the caller's workspace;
//   motion_features_kernel  facing direction per frame -> LDS, the 161-tap temporal filter of gaussian_filter1d(sigma=20,
//                           mode='nearest') over the clip's own valid frames, root rotation, chain IK -> cont6d, root / ric /
//                           local-velocity features, foot contacts.
// Arithmetic: the foot test in fp32 exactly as numpy does it on fp32 positions -- (dx^2 + dy^2) + dz^2 without contraction, compared
// with the threshold as a double -- so its flags are bit-exact; everything else in fp64, rounded once at the store (a few hundred
// flops per joint and frame: the fp64 VALU rate does not matter, and the kernel is the more accurate side of any comparison with
// the reference).  No per-lane array is indexed at run time: the chain walk keeps one running rotation and reloads positions.
// Two places where the reference's names mislead, kept as the arithmetic has them:
//   * the face-joint list is read as idx[1] - idx[0] inside inverse_kinematics_np (skeleton.py:61-62) and as idx[0] - idx[1] in
//     process_file's initial facing (motion_process.py:198-199);
//   * every chain starts from the ROOT rotation, also the chains that start at another joint (skeleton.py:87-88).
// One place where this kernel does NOT follow it: qbetween calls torch.cross without `dim`, so for a clip of exactly 3 frames the
// reference crosses along the frame axis; this kernel crosses over xyz always.
#pragma once
#include "common.h"

namespace mdm {

constexpr int kMfMaxJoints = 22;
constexpr int kMfMaxBones = kMfMaxJoints - 1;
constexpr int kMfRadius = 80;                       // int(truncate * sigma + 0.5), truncate = 4, sigma = 20
constexpr int kMfTaps = 2 * kMfRadius + 1;
constexpr int kMfTapsPad = 168;
constexpr int kMfMaxT = 1024;                       // LDS: (kMfTapsPad + 4 T) doubles = 34 KB
constexpr int kMfLanes = 256;
constexpr int kMfClipsPerLaunch = 64;               // frame counts travel as kernel arguments, 64 clips a launch

// The skeleton tables (utils/paramUtil.py:4-55; motion_process.py:460-466, :506-512) in the order the kernels walk them: the bones of
// every chain, chain after chain.  `first` marks a chain's first bone (the running rotation restarts from the root's).
struct MfSkeleton {
  int J, nbones;
  unsigned char parent[kMfMaxBones], child[kMfMaxBones], first[kMfMaxBones];
  float raw[kMfMaxJoints][3];                       // raw offsets (unit axes)
  int face[4];
  int foot[4];                                      // fid_l[0], fid_l[1], fid_r[0], fid_r[1]: the order of the last four features
  int l_idx1, l_par1, l_idx2, l_par2;               // the two leg bones of uniform_skeleton's scale ratio
};

struct MfLengths { int v[kMfClipsPerLaunch]; };

// Where a kernel reads joint positions: the caller's fp32 tensor with its strides, or the canonicalised fp64 block [J][3][T].
struct MfSource {
  const float* in;
  const double* ws;
  long long sj, sc, st;                             // strides of `in` within a clip, in elements
  int T;
  __device__ __forceinline__ double at(int j, int c, int t) const {
    return ws != nullptr ? ws[((size_t)j * 3 + c) * T + t] : (double)in[j * sj + c * sc + t * st];
  }
  __device__ __forceinline__ float at32(int j, int c, int t) const {
    return ws != nullptr ? (float)ws[((size_t)j * 3 + c) * T + t] : in[j * sj + c * sc + t * st];
  }
};

struct MfQuat { double w, x, y, z; };

__device__ __forceinline__ MfQuat mf_qmul(const MfQuat& q, const MfQuat& r) {          // quaternion.py:34-53
  return MfQuat{q.w * r.w - q.x * r.x - q.y * r.y - q.z * r.z, q.w * r.x + q.x * r.w + q.y * r.z - q.z * r.y,
                q.w * r.y - q.x * r.z + q.y * r.w + q.z * r.x, q.w * r.z + q.x * r.y - q.y * r.x + q.z * r.w};
}
__device__ __forceinline__ MfQuat mf_qinv(const MfQuat& q) { return MfQuat{q.w, -q.x, -q.y, -q.z}; }
__device__ __forceinline__ void mf_qrot(const MfQuat& q, double vx, double vy, double vz, double& ox, double& oy, double& oz) {   // :56-75
  const double uvx = q.y * vz - q.z * vy, uvy = q.z * vx - q.x * vz, uvz = q.x * vy - q.y * vx;
  const double uuvx = q.y * uvz - q.z * uvy, uuvy = q.z * uvx - q.x * uvz, uuvz = q.x * uvy - q.y * uvx;
  ox = vx + 2.0 * (q.w * uvx + uuvx);
  oy = vy + 2.0 * (q.w * uvy + uuvy);
  oz = vz + 2.0 * (q.w * uvz + uuvz);
}
// qbetween (:389-399) with qnormalize's 1e-4 on the last component (:28-31)
__device__ __forceinline__ MfQuat mf_qbetween(double ax, double ay, double az, double bx, double by, double bz) {
  MfQuat q;
  q.x = ay * bz - az * by;
  q.y = az * bx - ax * bz;
  q.z = ax * by - ay * bx + 1e-4;
  q.w = sqrt((ax * ax + ay * ay + az * az) * (bx * bx + by * by + bz * bz)) + (ax * bx + ay * by + az * bz);
  const double inv = 1.0 / sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  q.w *= inv; q.x *= inv; q.y *= inv; q.z *= inv;
  return q;
}
// the root rotation of a frame from its unit forward vector (fx, 0, fz): qbetween(forward, +Z)
__device__ __forceinline__ MfQuat mf_root_quat(double fx, double fz) { return mf_qbetween(fx, 0.0, fz, 0.0, 0.0, 1.0); }

// cross(+Y, normalised across) of frame t, `sign` +1: across = (f1 - f0) + (f2 - f3) (skeleton.py:61-69); -1: (f0 - f1) + (f2 - f3)
// (motion_process.py:198-205)
__device__ __forceinline__ void mf_forward(const MfSkeleton& sk, const MfSource& src, int t, double sign, double& fx, double& fz) {
  const double ax = sign * (src.at(sk.face[1], 0, t) - src.at(sk.face[0], 0, t)) + (src.at(sk.face[2], 0, t) - src.at(sk.face[3], 0, t));
  const double ay = sign * (src.at(sk.face[1], 1, t) - src.at(sk.face[0], 1, t)) + (src.at(sk.face[2], 1, t) - src.at(sk.face[3], 1, t));
  const double az = sign * (src.at(sk.face[1], 2, t) - src.at(sk.face[0], 2, t)) + (src.at(sk.face[2], 2, t) - src.at(sk.face[3], 2, t));
  const double inv = 1.0 / sqrt(ax * ax + ay * ay + az * az);
  fx = az * inv;
  fz = -(ax * inv);
}

// one bone of the chain walk (skeleton.py:89-102): the local rotation of `child` and the updated chain rotation R
__device__ __forceinline__ MfQuat mf_bone(const MfSkeleton& sk, const MfSource& src, int i, int t, MfQuat& R) {
  const int p = sk.parent[i], c = sk.child[i];
  double vx = src.at(c, 0, t) - src.at(p, 0, t), vy = src.at(c, 1, t) - src.at(p, 1, t), vz = src.at(c, 2, t) - src.at(p, 2, t);
  const double inv = 1.0 / sqrt(vx * vx + vy * vy + vz * vz);
  vx *= inv; vy *= inv; vz *= inv;
  const MfQuat rot = mf_qbetween((double)sk.raw[c][0], (double)sk.raw[c][1], (double)sk.raw[c][2], vx, vy, vz);
  const MfQuat loc = mf_qmul(mf_qinv(R), rot);
  R = mf_qmul(R, loc);
  return loc;
}

__device__ __forceinline__ double mf_bone_len0(const MfSource& src, int c, int p) {
  const double x = src.at(c, 0, 0) - src.at(p, 0, 0), y = src.at(c, 1, 0) - src.at(p, 1, 0), z = src.at(c, 2, 0) - src.at(p, 2, 0);
  return sqrt(x * x + y * y + z * z);
}

struct MfCanon {
  int retarget, floor, origin_xz, face_z;
  float tgt[kMfMaxJoints][3];
  double tgt_leg;                                   // max|tgt[l_idx1]| + max|tgt[l_idx2]|
};

// process_file's transform of clip blockIdx.x (motion_process.py:178-222): ws [B][J][3][T] fp64.  Static LDS only.
__global__ __launch_bounds__(kMfLanes) void motion_canon_kernel(const float* __restrict__ in, double* __restrict__ ws, MfSkeleton sk,
                                                                MfCanon cn, MfLengths len, long long sb, long long sj, long long sc,
                                                                long long st, int T) {
  __shared__ double s_min[kMfLanes];
  __shared__ double s_init[16];
  const int b = blockIdx.x, L = len.v[b], J = sk.J;
  double* W = ws + (size_t)b * J * 3 * T;
  const MfSource src{in + b * sb, nullptr, sj, sc, st, T};
  auto w_at = [&](int j, int c, int t) -> double& { return W[((size_t)j * 3 + c) * T + t]; };

  double scale = 1.0;
  if (cn.retarget) {   // the leg-length ratio of frame 0 (:25-28); raw offsets are unit axes times the bone length
    const double r1 = fmax(fmax(fabs((double)sk.raw[sk.l_idx1][0]), fabs((double)sk.raw[sk.l_idx1][1])), fabs((double)sk.raw[sk.l_idx1][2]));
    const double r2 = fmax(fmax(fabs((double)sk.raw[sk.l_idx2][0]), fabs((double)sk.raw[sk.l_idx2][1])), fabs((double)sk.raw[sk.l_idx2][2]));
    scale = cn.tgt_leg / (mf_bone_len0(src, sk.l_idx1, sk.l_par1) * r1 + mf_bone_len0(src, sk.l_idx2, sk.l_par2) * r2);
  }
  double ymin = INFINITY;
  for (int t = threadIdx.x; t < L; t += blockDim.x) {
    if (cn.retarget) {   // IK with the unsmoothed forward (:34), then FK along the target offsets (:38-39): the chain rotations are the same
      double fx, fz;
      mf_forward(sk, src, t, 1.0, fx, fz);
      const double inv = 1.0 / sqrt(fx * fx + fz * fz);
      const MfQuat root = mf_root_quat(fx * inv, fz * inv);
      double px = src.at(0, 0, t) * scale, py = src.at(0, 1, t) * scale, pz = src.at(0, 2, t) * scale;
      w_at(0, 0, t) = px; w_at(0, 1, t) = py; w_at(0, 2, t) = pz;
      ymin = fmin(ymin, py);
      MfQuat R = root;
      for (int i = 0; i < sk.nbones; ++i) {
        const int p = sk.parent[i], c = sk.child[i];
        if (sk.first[i]) {
          R = root;
          px = w_at(p, 0, t); py = w_at(p, 1, t); pz = w_at(p, 2, t);      // this lane's own store
        }
        mf_bone(sk, src, i, t, R);
        double ox, oy, oz;
        mf_qrot(R, (double)cn.tgt[c][0], (double)cn.tgt[c][1], (double)cn.tgt[c][2], ox, oy, oz);
        px += ox; py += oy; pz += oz;
        w_at(c, 0, t) = px; w_at(c, 1, t) = py; w_at(c, 2, t) = pz;
        ymin = fmin(ymin, py);
      }
    } else {
      for (int j = 0; j < J; ++j) {
        const double y = src.at(j, 1, t);
        w_at(j, 0, t) = src.at(j, 0, t); w_at(j, 1, t) = y; w_at(j, 2, t) = src.at(j, 2, t);
        ymin = fmin(ymin, y);
      }
    }
    if (t == 0) {        // frame 0: root xz and the four face joints (:189-201)
      s_init[0] = w_at(0, 0, 0);
      s_init[1] = w_at(0, 2, 0);
      for (int k = 0; k < 4; ++k)
        for (int c = 0; c < 3; ++c) s_init[2 + 3 * k + c] = w_at(sk.face[k], c, 0);
    }
  }
  s_min[threadIdx.x] = ymin;
  __syncthreads();
  for (int half = kMfLanes / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) s_min[threadIdx.x] = fmin(s_min[threadIdx.x], s_min[threadIdx.x + half]);
    __syncthreads();
  }
  const double floor_y = cn.floor ? s_min[0] : 0.0;
  const double ox0 = cn.origin_xz ? s_init[0] : 0.0, oz0 = cn.origin_xz ? s_init[1] : 0.0;
  MfQuat q0{1.0, 0.0, 0.0, 0.0};
  if (cn.face_z) {
    double a[3];
    for (int c = 0; c < 3; ++c) a[c] = (s_init[2 + c] - s_init[5 + c]) + (s_init[8 + c] - s_init[11 + c]);
    const double inv = 1.0 / sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    double fx = a[2] * inv, fz = -(a[0] * inv);
    const double invf = 1.0 / sqrt(fx * fx + fz * fz);
    q0 = mf_root_quat(fx * invf, fz * invf);
  }
  for (int t = threadIdx.x; t < L; t += blockDim.x)      // every lane revisits the frames it wrote itself
    for (int j = 0; j < J; ++j) {
      double x = w_at(j, 0, t) - ox0, y = w_at(j, 1, t) - floor_y, z = w_at(j, 2, t) - oz0;
      if (cn.face_z) mf_qrot(q0, x, y, z, x, y, z);
      w_at(j, 0, t) = x; w_at(j, 1, t) = y; w_at(j, 2, t) = z;
    }
}

// (dx^2 + dy^2) + dz^2 in fp32, every operation rounded on its own (motion_process.py:50-55 on fp32 positions)
__device__ __forceinline__ float mf_foot_sq(const MfSource& src, int j, int t) {
#pragma clang fp contract(off)
  const float dx = src.at32(j, 0, t + 1) - src.at32(j, 0, t);
  const float dy = src.at32(j, 1, t + 1) - src.at32(j, 1, t);
  const float dz = src.at32(j, 2, t + 1) - src.at32(j, 2, t);
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float xy = xx + yy;
  return xy + zz;
}

struct MfOutput {
  float* out;                                       // [B][F][T-1]
  const float* mean;                                // [F] or null
  const float* stdv;
  float* global_out;                                // optional [B][J][3][T]: the positions the features were taken from
  float* ric_out;                                   // optional [B][J][3][T]: the rotation-invariant positions of every frame
};

// Dynamic LDS: (kMfTapsPad + 4 T) doubles.
__global__ __launch_bounds__(kMfLanes) void motion_features_kernel(const float* __restrict__ in, const double* __restrict__ ws,
                                                                   MfOutput o, MfSkeleton sk, MfLengths len, long long sb, long long sj,
                                                                   long long sc, long long st, int T, int F, double feet_thre) {
  MDM_DYN_SMEM(double, sm);
  double* s_w = sm;                                 // the filter's normalised weights
  double* s_fx = sm + kMfTapsPad;                   // cross(+Y, across) per frame: (x, 0, z)
  double* s_fz = s_fx + T;
  double* s_gx = s_fz + T;                          // filtered and renormalised
  double* s_gz = s_gx + T;
  const int b = blockIdx.x, L = len.v[b], J = sk.J, T1 = T - 1;
  const MfSource src{ws != nullptr ? nullptr : in + b * sb, ws != nullptr ? ws + (size_t)b * J * 3 * T : nullptr, sj, sc, st, T};
  float* ob = o.out + (size_t)b * F * T1;
  auto put = [&](int f, int t, double v) {
    if (o.mean != nullptr) v = (v - (double)o.mean[f]) / (double)o.stdv[f];
    ob[(size_t)f * T1 + t] = (float)v;
  };

  for (int t = threadIdx.x; t < L; t += blockDim.x) mf_forward(sk, src, t, 1.0, s_fx[t], s_fz[t]);
  for (int k = threadIdx.x; k < kMfTaps; k += blockDim.x) {
    const double x = (double)(k - kMfRadius);
    s_w[k] = exp(-0.5 / (20.0 * 20.0) * x * x);
  }
  __syncthreads();
  double wsum = 0.0;
  for (int k = 0; k < kMfTaps; ++k) wsum += s_w[k];
  __syncthreads();
  for (int k = threadIdx.x; k < kMfTaps; k += blockDim.x) s_w[k] = s_w[k] / wsum;
  __syncthreads();
  for (int t = threadIdx.x; t < L; t += blockDim.x) {   // gaussian_filter1d(forward, 20, axis=0, mode='nearest') (skeleton.py:71-73)
    double ax = 0.0, az = 0.0;
    for (int k = 0; k < kMfTaps; ++k) {
      const int u = min(max(t + k - kMfRadius, 0), L - 1);
      ax += s_w[k] * s_fx[u];
      az += s_w[k] * s_fz[u];
    }
    const double inv = 1.0 / sqrt(ax * ax + az * az);
    s_gx[t] = ax * inv;
    s_gz[t] = az * inv;
  }
  __syncthreads();

  const int f_ric = 4, f_rot = 4 + 3 * (J - 1), f_vel = f_rot + 6 * (J - 1), f_foot = f_vel + 3 * J;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    const bool has_pose = t < L, has_feat = t < L - 1;
    if (!has_feat && t < T1)
      for (int f = 0; f < F; ++f) ob[(size_t)f * T1 + t] = 0.f;
    if (!has_pose) {
      for (int r = 0; r < J * 3; ++r) {
        if (o.global_out != nullptr) o.global_out[((size_t)b * J * 3 + r) * T + t] = 0.f;
        if (o.ric_out != nullptr) o.ric_out[((size_t)b * J * 3 + r) * T + t] = 0.f;
      }
      continue;
    }
    const MfQuat r0 = mf_root_quat(s_gx[t], s_gz[t]);
    const double rx = src.at(0, 0, t), rz = src.at(0, 2, t);
    for (int j = 0; j < J; ++j) {                      // get_rifke (:72-78): subtract the root's xz, rotate by r_rot
      const double px = src.at(j, 0, t), py = src.at(j, 1, t), pz = src.at(j, 2, t);
      double lx, ly, lz;
      mf_qrot(r0, px - rx, py, pz - rz, lx, ly, lz);
      if (o.global_out != nullptr) {
        float* g = o.global_out + ((size_t)b * J + j) * 3 * T + t;
        g[0] = (float)px; g[(size_t)T] = (float)py; g[(size_t)2 * T] = (float)pz;
      }
      if (o.ric_out != nullptr) {
        float* g = o.ric_out + ((size_t)b * J + j) * 3 * T + t;
        g[0] = (float)lx; g[(size_t)T] = (float)ly; g[(size_t)2 * T] = (float)lz;
      }
      if (!has_feat) continue;
      if (j == 0) {
        put(3, t, ly);                                 // root height (:139)
      } else {
        put(f_ric + 3 * (j - 1) + 0, t, lx);
        put(f_ric + 3 * (j - 1) + 1, t, ly);
        put(f_ric + 3 * (j - 1) + 2, t, lz);
      }
      double vx, vy, vz;                               // local velocity (:159-160): rotated by r_rot[:-1]
      mf_qrot(r0, src.at(j, 0, t + 1) - px, src.at(j, 1, t + 1) - py, src.at(j, 2, t + 1) - pz, vx, vy, vz);
      put(f_vel + 3 * j + 0, t, vx);
      put(f_vel + 3 * j + 1, t, vy);
      put(f_vel + 3 * j + 2, t, vz);
    }
    if (!has_feat) continue;
    {   // root linear velocity rotated by r_rot[1:] (:114-116), angular velocity asin((r_rot[1:] . r_rot[:-1]^-1).y) (:119, :144)
      const MfQuat r1 = mf_root_quat(s_gx[t + 1], s_gz[t + 1]);
      double vx, vy, vz;
      mf_qrot(r1, src.at(0, 0, t + 1) - rx, src.at(0, 1, t + 1) - src.at(0, 1, t), src.at(0, 2, t + 1) - rz, vx, vy, vz);
      const MfQuat rv = mf_qmul(r1, mf_qinv(r0));
      put(0, t, asin(rv.y));
      put(1, t, vx);
      put(2, t, vz);
    }
    MfQuat R = r0;
    for (int i = 0; i < sk.nbones; ++i) {              // chain IK -> matrix -> its first two columns (quaternion.py:276-313)
      if (sk.first[i]) R = r0;
      const MfQuat q = mf_bone(sk, src, i, t, R);
      const double s2 = 2.0 / (q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
      const int f = f_rot + 6 * (sk.child[i] - 1);
      put(f + 0, t, 1.0 - s2 * (q.y * q.y + q.z * q.z));
      put(f + 1, t, s2 * (q.x * q.y + q.z * q.w));
      put(f + 2, t, s2 * (q.x * q.z - q.y * q.w));
      put(f + 3, t, s2 * (q.x * q.y - q.z * q.w));
      put(f + 4, t, 1.0 - s2 * (q.x * q.x + q.z * q.z));
      put(f + 5, t, s2 * (q.y * q.z + q.x * q.w));
    }
    for (int k = 0; k < 4; ++k) put(f_foot + k, t, (double)mf_foot_sq(src, sk.foot[k], t) < feet_thre ? 1.0 : 0.0);
  }
}

}  // namespace mdm
