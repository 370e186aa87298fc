// The Frechet distance of two Gaussians (eval/a2m/action2motion/fid.py, data_loaders/humanml/utils/metrics.py
// calculate_frechet_distance) on gfx950, in fp64, without a matrix square root:
//
//   Tr sqrtm(S1 S2) = sum_i sqrt(lambda_i(M)),   M = S^T S2 S,   S = V diag(sqrt(max(w, 0))),   S1 = V diag(w) V^T
//
// for symmetric positive semi-definite S1, S2: two symmetric eigen-solves (the first with vectors) and two D x D x D products in
// between.  Nothing is complex, nothing divides by a small eigenvalue, a singular product is finite.
//
// Eigen-solver: two-sided cyclic Jacobi on the round-robin schedule -- n = D rounded up to even, n - 1 rounds of n / 2 disjoint pairs
// per sweep; the partner of index i in round r is (2 r - i) mod (n - 1), index n - 1 meets r.  A pair (p, q) is rotated when
//   |a_pq| > 2^-52 sqrt|a_pp a_qq|   and   |a_pq| > floor = 2^-52 |A|_F / D
// (the floor ends the sweeps on the null space of a rank-deficient matrix, where the relative test alone never does; what it leaves
// moves an eigenvalue by at most 2^-52 |A|_F).  An odd D has a zero pad row / column: its a_pq is 0, so it is never rotated.  All
// rotations of a round commute, so A' = J^T A J is formed at once: every element of A' is a combination of four elements of A,
//   a'_ij = (al_i al_j) a_ij + (be_i be_j) a_i'j' + ((al_i be_j) a_ij' + (be_i al_j) a_i'j),      i', j' the partners,
// added in this order without fused multiply-adds: the two middle terms trade places under (i, j) -> (j, i), so a bit-symmetric A
// stays bit-symmetric.  The rotated element itself is set to 0, the pair's diagonal becomes a_pp - t a_pq, a_qq + t a_pq.
//   small form, n <= 64: one workgroup, A and V in LDS, all rounds of all sweeps behind workgroup barriers, one launch.
//   round form: one launch per round, out of place between two buffers (ping-pong); every workgroup recomputes the rotations of the
//     rows and columns it touches from the input buffer's diagonal; V' = V J in the same launch (grid z = 1).  Workgroup (0, 0, 0)
//     adds the round's rotations to the sweep's counter (integer atomics).  A launch of sweep s returns at once when sweep s - 1
//     performed no rotation -- its counter, or that of an earlier sweep that ended the solve, is 0 -- so the host enqueues the
//     fixed maximum of FR_MAX_SWEEPS sweeps without reading anything back.  fr_extract_kernel finds the first sweep without a
//     rotation, hence the buffer the solve ended in, and copies the diagonal; without such a sweep the eigenvalues are NaN.
//
// Products: fr_gemm_kernel, C = X^T Y on v_mfma_f64_16x16x4_f64 (common.h mfma16_f64), a 64 x 64 tile per workgroup (a 32 x 32
// block per wave), 16 k at a time through LDS, edges masked.  T = S2 S (S2 symmetric) and M = S^T T; fr_sym_kernel stores
// (m_ij + m_ji) / 2, as it does for both inputs (feature_cov_kernel does not promise bit-symmetry).
//
// Every sum is fp64 in one fixed order; the only atomics count rotations: repeated calls return the same bits.
#pragma once
#include "common.h"

namespace mdm {

constexpr int FR_MAX_D = 1024;
constexpr int FR_SMALL_MAX = 64;          // n up to which the one-launch form runs
constexpr int FR_MAX_SWEEPS = 30;         // twice the worst count seen
constexpr int FR_CNT = 32;                // ints per solve's counter row
constexpr double FR_EPS = 2.220446049250313e-16;   // 2^-52

// The head of the workspace (1 KB): what the kernels of one call tell each other
struct FrHeader {
  int cnt[2][FR_CNT];       // rotations performed per sweep, per solve (round form)
  int sweeps[2];            // sweeps that rotated; FR_MAX_SWEEPS: not converged
  int vbuf;                 // which V buffer holds the first solve's vectors
  int pad0[61];
  double floor[2];          // the absolute rotation threshold per solve
  double pad1[62];
};
static_assert(sizeof(FrHeader) == 1024, "the workspace layout counts on it");

__device__ __forceinline__ int fr_partner(int i, int r, int n) {
  const int m = n - 1;
  if (i == m) return r;
  int p = 2 * r - i;
  if (p < 0) p += m;
  else if (p >= m) p -= m;
  return p == i ? m : p;
}

// What a round does to index i: new_i = alpha old_i + beta old_partner; `diag` is a'_ii.  beta != 0 exactly when the pair is rotated.
struct FrCoef {
  double alpha, beta, diag;
  int partner, pad;
};

__device__ __forceinline__ FrCoef fr_coef(const double* A, int ld, int i, int r, int n, double thr) {
  FrCoef o;
  o.partner = fr_partner(i, r, n);
  o.pad = 0;
  const int lo = min(i, o.partner), hi = max(i, o.partner);
  const double app = A[(size_t)lo * ld + lo], aqq = A[(size_t)hi * ld + hi], apq = A[(size_t)lo * ld + hi];
  const double g = fabs(apq);
  o.alpha = 1.0;
  o.beta = 0.0;
  o.diag = i == lo ? app : aqq;
  if (g > thr && g > FR_EPS * sqrt(fabs(app * aqq))) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    o.alpha = c;
    o.beta = i == lo ? -s : s;
    o.diag = i == lo ? app - t * apq : aqq + t * apq;
  }
  return o;
}

// a'_ij of the header's formula
__device__ __forceinline__ double fr_elem(const double* A, int ld, int i, int j, const FrCoef& ci, const FrCoef& cj) {
#pragma clang fp contract(off)
  if (i == j) return ci.diag;
  const double a = A[(size_t)i * ld + j];
  if (j == ci.partner) return ci.beta != 0.0 ? 0.0 : a;
  const double b = A[(size_t)i * ld + cj.partner], c = A[(size_t)ci.partner * ld + j], d = A[(size_t)ci.partner * ld + cj.partner];
  const double t1 = (ci.alpha * cj.alpha) * a, t4 = (ci.beta * cj.beta) * d;
  const double t2 = (ci.alpha * cj.beta) * b, t3 = (ci.beta * cj.alpha) * c;
  return (t1 + t4) + (t2 + t3);
}

// dst [n][n] = the symmetric part of src [D][D], zero in the pad row / column; `eye`: identity [n][n] beside it (the vectors' start)
__global__ __launch_bounds__(256) void fr_sym_kernel(const double* src, int D, int ld_src, double* dst, int n, double* eye) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= n * n) return;
  const int i = e / n, j = e - i * n;
  dst[e] = (i < D && j < D) ? 0.5 * (src[(size_t)i * ld_src + j] + src[(size_t)j * ld_src + i]) : 0.0;
  if (eye != nullptr) eye[e] = i == j ? 1.0 : 0.0;
}

// floor[solve] = 2^-52 |A|_F / D and the solve's counters zeroed: one workgroup, thread t adds elements t, t + 256, ... in order, thread 0
// the threads' sums in order
__global__ __launch_bounds__(256) void fr_norm_kernel(const double* A, int n, int D, FrHeader* h, int solve) {
  __shared__ double part[256];
  double s = 0.0;
  for (int e = threadIdx.x; e < n * n; e += 256) s = fma(A[e], A[e], s);
  part[threadIdx.x] = s;
  if (threadIdx.x < FR_CNT) h->cnt[solve][threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += part[i];
    h->floor[solve] = FR_EPS * sqrt(t) / (double)D;
    h->sweeps[solve] = FR_MAX_SWEEPS;
  }
}

struct FrSmallArgs {
  const double* a;      // [n][n] symmetric, pad zero
  double* w;            // [n]: the eigenvalues (unordered), 0 in the pad; NaN when the sweeps ran out
  double* v;            // [n][n]: the vectors in columns, or null
  FrHeader* h;
  int n, D, solve;
};

constexpr int FR_SMALL_LDS = 2 * FR_SMALL_MAX * FR_SMALL_MAX * 8 + FR_SMALL_MAX * (int)sizeof(FrCoef) + FR_SMALL_MAX * 4;

__global__ __launch_bounds__(256) void fr_eig_small_kernel(FrSmallArgs p) {
  MDM_DYN_SMEM(double, sm);
  double* As = sm;
  double* Vs = sm + FR_SMALL_MAX * FR_SMALL_MAX;
  FrCoef* co = reinterpret_cast<FrCoef*>(sm + 2 * FR_SMALL_MAX * FR_SMALL_MAX);
  int* rc = reinterpret_cast<int*>(co + FR_SMALL_MAX);
  const int tid = threadIdx.x, n = p.n, j = tid & 63, g = tid >> 6;
  const bool vectors = p.v != nullptr;
  const double thr = p.h->floor[p.solve];
  for (int e = tid; e < n * n; e += 256) {
    As[e] = p.a[e];
    Vs[e] = (e / n == e % n) ? 1.0 : 0.0;
  }
  __syncthreads();
  int used = FR_MAX_SWEEPS;
  for (int sweep = 0; sweep < FR_MAX_SWEEPS; ++sweep) {
    int mine = 0;
    for (int r = 0; r < n - 1; ++r) {
      if (tid < n) {
        const FrCoef c = fr_coef(As, n, tid, r, n, thr);
        co[tid] = c;
        mine += (tid < c.partner && c.beta != 0.0) ? 1 : 0;
      }
      __syncthreads();
      double an[16], vn[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int i = g + 4 * k;
        an[k] = vn[k] = 0.0;
        if (i < n && j < n) {
          const FrCoef cj = co[j];
          an[k] = fr_elem(As, n, i, j, co[i], cj);
          if (vectors) vn[k] = cj.alpha * Vs[i * n + j] + cj.beta * Vs[i * n + cj.partner];
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int i = g + 4 * k;
        if (i < n && j < n) {
          As[i * n + j] = an[k];
          if (vectors) Vs[i * n + j] = vn[k];
        }
      }
      __syncthreads();
    }
    if (tid < n) rc[tid] = mine;
    __syncthreads();
    int total = 0;
    for (int i = 0; i < n; ++i) total += rc[i];
    __syncthreads();
    if (total == 0) {
      used = sweep;
      break;
    }
  }
  if (tid < n) p.w[tid] = tid >= p.D ? 0.0 : (used < FR_MAX_SWEEPS ? As[tid * n + tid] : __builtin_nan(""));
  if (vectors)
    for (int e = tid; e < n * n; e += 256) p.v[e] = Vs[e];
  if (tid == 0) {
    p.h->sweeps[p.solve] = used;
    if (vectors) p.h->vbuf = 0;
  }
}

inline int launch_fr_eig_small(const FrSmallArgs& a, hipStream_t stream) {
  static bool configured[kMaxDevices] = {};
  if (const int rc = rt_dyn_lds_once(fr_eig_small_kernel, FR_SMALL_LDS, configured, stream)) return rc;
  MDM_LAUNCH(fr_eig_small_kernel, dim3(1), dim3(256), FR_SMALL_LDS, stream, a);
  return 0;
}

struct FrRoundArgs {
  const double* a_in;
  double* a_out;
  const double* v_in;    // null: values only
  double* v_out;
  FrHeader* h;
  int n, solve, sweep, round;
};

constexpr int FR_ROUND_ROWS = 16;

// grid (ceil(n / 64), ceil(n / 16), vectors ? 2 : 1): z = 0 forms 16 rows x 64 columns of A', z = 1 of V'
__global__ __launch_bounds__(256) void fr_round_kernel(FrRoundArgs p) {
  __shared__ FrCoef rowc[FR_ROUND_ROWS];
  int* cnt = p.h->cnt[p.solve];
  if (p.sweep > 0 && cnt[p.sweep - 1] == 0) return;          // the solve has ended: an earlier sweep rotated nothing
  const int tid = threadIdx.x, n = p.n;
  const int j = (int)blockIdx.x * 64 + (tid & 63), i0 = (int)blockIdx.y * FR_ROUND_ROWS;
  const bool values = blockIdx.z == 0;
  const double thr = p.h->floor[p.solve];
  if (values && tid < FR_ROUND_ROWS && i0 + tid < n) rowc[tid] = fr_coef(p.a_in, n, i0 + tid, p.round, n, thr);
  FrCoef cj;
  cj.alpha = 1.0;
  cj.beta = cj.diag = 0.0;
  cj.partner = cj.pad = 0;
  if (j < n) cj = fr_coef(p.a_in, n, j, p.round, n, thr);
  if (values && blockIdx.x == 0 && blockIdx.y == 0) {
    int mine = 0;
    for (int i = tid; i < n; i += 256) {
      const FrCoef c = fr_coef(p.a_in, n, i, p.round, n, thr);
      mine += (i < c.partner && c.beta != 0.0) ? 1 : 0;
    }
    if (mine != 0) atomic_add_i32(&cnt[p.sweep], mine);
  }
  __syncthreads();
  if (j >= n) return;
#pragma unroll
  for (int k = 0; k < FR_ROUND_ROWS / 4; ++k) {
    const int il = (tid >> 6) + 4 * k, i = i0 + il;
    if (i >= n) continue;
    if (values) p.a_out[(size_t)i * n + j] = fr_elem(p.a_in, n, i, j, rowc[il], cj);
    else p.v_out[(size_t)i * n + j] = cj.alpha * p.v_in[(size_t)i * n + j] + cj.beta * p.v_in[(size_t)i * n + cj.partner];
  }
}

// The end of a round-form solve: the first sweep without a rotation, the buffer it left the matrix in, the diagonal
__global__ __launch_bounds__(256) void fr_extract_kernel(const double* a0, const double* a1, int n, int D, FrHeader* h, int solve,
                                                         int vectors, double* w) {
  int used = FR_MAX_SWEEPS;
  for (int s = FR_MAX_SWEEPS - 1; s >= 0; --s)
    if (h->cnt[solve][s] == 0) used = s;
  // sweeps 0 .. used ran, (used + 1) (n - 1) launches swapped the buffers
  const int buf = (int)(((long long)(used + 1) * (n - 1)) & 1);
  const double* a = buf ? a1 : a0;
  for (int i = threadIdx.x; i < n; i += 256)
    w[i] = i >= D ? 0.0 : (used < FR_MAX_SWEEPS ? a[(size_t)i * n + i] : __builtin_nan(""));
  __syncthreads();          // (every thread has read the header)
  if (threadIdx.x == 0) {
    h->sweeps[solve] = used;
    if (vectors) h->vbuf = buf;
  }
}

// s [n][n] = V diag(sqrt(max(w, 0))): the columns of the first solve's vectors, scaled
__global__ __launch_bounds__(256) void fr_scale_kernel(const double* v0, const double* v1, const FrHeader* h, const double* w, double* s, int n) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= n * n) return;
  const double* v = h->vbuf ? v1 : v0;
  const int j = e % n;
  s[e] = v[e] * sqrt(fmax(w[j], 0.0));       // (fmax drops a NaN: keep it)
  if (w[j] != w[j]) s[e] = w[j];
}

// C [n][n] = X^T Y for X, Y [n][n]: C_ij = sum_k X_ki Y_kj, k ascending in steps of 4
constexpr int FR_KC = 16, FR_LD = 64 + 16;      // (rows 0, 1 / 2, 3 of a k step on disjoint LDS banks)

__global__ __launch_bounds__(256) void fr_gemm_kernel(const double* X, const double* Y, double* C, int n) {
  __shared__ double xs[FR_KC][FR_LD], ys[FR_KC][FR_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, li = lane & 15, lk = lane >> 4;
  const int i0 = (int)blockIdx.y * 64, j0 = (int)blockIdx.x * 64;
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int sk = tid >> 4, sc = (tid & 15) * 4;
  for (int k0 = 0; k0 < n; k0 += FR_KC) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = k0 + sk, ci = i0 + sc + e, cj = j0 + sc + e;
      xs[sk][sc + e] = (k < n && ci < n) ? X[(size_t)k * n + ci] : 0.0;
      ys[sk][sc + e] = (k < n && cj < n) ? Y[(size_t)k * n + cj] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < FR_KC / 4; ++ks) {
      const int k = 4 * ks + lk;
      const double a0 = xs[k][32 * wr + li], a1 = xs[k][32 * wr + 16 + li];
      const double b0 = ys[k][32 * wc + li], b1 = ys[k][32 * wc + 16 + li];
      acc[0][0] = mfma16_f64(a0, b0, acc[0][0]);
      acc[0][1] = mfma16_f64(a0, b1, acc[0][1]);
      acc[1][0] = mfma16_f64(a1, b0, acc[1][0]);
      acc[1][1] = mfma16_f64(a1, b1, acc[1][1]);
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i0 + 32 * wr + 16 * a + lk + 4 * reg, col = j0 + 32 * wc + 16 * b + li;
        if (row < n && col < n) C[(size_t)row * n + col] = acc[a][b][reg];
      }
}

struct FrFinishArgs {
  const double *mu1, *sigma1, *mu2, *sigma2;    // the caller's inputs [D], [D][D]
  const double *w1, *w2;                        // eigenvalues of sigma1's symmetric part and of M
  const FrHeader* h;
  double* result;      // [4]
  int* sweeps;         // [2]
  int D;
};

// One thread, every sum in index order.  min / max of an all-zero spectrum is 0; with no positive eigenvalue and a negative one, -inf.
__device__ __forceinline__ double fr_ratio(double lo, double hi) {
  if (hi > 0.0) return lo / hi;
  return lo < 0.0 ? -__builtin_huge_val() : (lo == 0.0 ? 0.0 : lo);       // (a NaN spectrum stays NaN)
}

__global__ __launch_bounds__(64) void fr_finish_kernel(FrFinishArgs p) {
  if (threadIdx.x != 0) return;
  const int D = p.D;
  double d2 = 0.0, tr1 = 0.0, tr2 = 0.0, root = 0.0;
  double lo1 = p.w1[0], hi1 = p.w1[0], lo2 = p.w2[0], hi2 = p.w2[0];
  bool nan1 = false, nan2 = false;
  for (int i = 0; i < D; ++i) {
    const double d = p.mu1[i] - p.mu2[i];
    d2 = fma(d, d, d2);
    tr1 += p.sigma1[(size_t)i * D + i];
    tr2 += p.sigma2[(size_t)i * D + i];
    const double w = p.w1[i], l = p.w2[i];
    nan1 |= w != w;
    nan2 |= l != l;
    lo1 = fmin(lo1, w);
    hi1 = fmax(hi1, w);
    lo2 = fmin(lo2, l);
    hi2 = fmax(hi2, l);
    root += l != l ? l : sqrt(fmax(l, 0.0));
  }
  const double nan = __builtin_nan("");
  p.result[0] = d2 + tr1 + tr2 - 2.0 * root;
  p.result[1] = root;
  p.result[2] = nan1 ? nan : fr_ratio(lo1, hi1);
  p.result[3] = nan2 ? nan : fr_ratio(lo2, hi2);
  p.sweeps[0] = p.h->sweeps[0];
  p.sweeps[1] = p.h->sweeps[1];
}

}  // namespace mdm
