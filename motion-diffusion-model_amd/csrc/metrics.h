// The metrics of the unconstrained HumanAct12 evaluation (eval/unconstrained/evaluate.py) on gfx950: what the reference computes on
// the host from the ST-GCN's features [N, D] -- improved precision / recall (metrics/precision_recall.py), KID (metrics/kid.py),
// the FID statistics (calculate_activation_statistics) and diversity (eval/a2m/action2motion/diversity.py) -- on the device.
//
// Distances.  dist2_add4 is the ONE statement of d2(a, b) = sum_j (a_j - b_j)^2: direct differences, fp32, one fused multiply-add per
// feature in ascending j.  No Gram form anywhere: |a|^2 + |b|^2 - 2 a.b cancels relative to the norms, not to the distance, and
// does not return 0 for duplicated rows.  The order over j does not depend on the tile, the row's position or N (a thread keeps a
// pair's accumulator across the feature chunks; features behind D are staged as zeros and add an exact 0), and (a - b)^2 == (b - a)^2,
// so d2 of a pair of rows is the same bits wherever the two rows stand.
//   dist_tile: a 64 x 64 tile of pairs per 256-thread workgroup, thread (ty, tx) owns rows 4 ty .. + 3 and columns tx + 16 c; both
//     operand tiles go through LDS in chunks of 64 features (16-byte global loads when D % 4 == 0, 16-byte LDS reads always).
//   knn_radius_kernel: one workgroup per row tile of A streams all column tiles of A; after each, one thread per row merges the
//     tile's 64 values into its k + 1 smallest (registers).  radius2[i] = the (k+1)-th smallest d2 of row i, self included
//     (np.partition(d, k)[k]); the value is a property of the multiset, so it does not depend on the order of the rows.
//   manifold_members_kernel: one workgroup per row tile of B streams the column tiles of A with their radius2: member[b] =
//     exists a': d2(b, a') <= radius2[a'], compared in the squared domain on the same function's values.  count_members_kernel sums
//     the bytes (one workgroup, fixed order; integers).
//   gather_dist_kernel: sqrt(d2(x[i_p], x[j_p])) of P index pairs, one thread per pair; mean_f64_kernel: their mean in fp64.
// No atomics, no cross-workgroup communication inside a kernel.
//
// Polynomial MMD (kid.py polynomial_mmd / _mmd2_and_variance, the `unbiased` estimator) for all subsets in one call.  Workgroup
// (row tile, side, subset): side 0 takes 64 gathered rows of X = g[idx_g[s]] and streams the column tiles of X (K_XX), then of
// Y = r[idx_r[s]] (K_XY); side 1 takes rows of Y against Y (K_YY) and X (K_YX = K_XY^T: its row sums are K_XY's column sums, so no
// column partials exist).  A 64 x 64 tile of G = rows . cols^T is four 32 x 32 blocks, one per wave, on v_mfma_f32_32x32x2_f32
// (common.h mfma_f32: exact fp32, k ascending; the k tail behind D is zero-filled).  Epilogue in fp64: K = (gamma G + coef0)^degree by
// repeated multiplication; per accumulator row the lane adds K (off the diagonal of K_XX / K_YY) and K^2 over the column tiles in
// ascending order; the lane that holds a diagonal element stores it.  Per phase the lanes' partials cross through LDS and one thread
// per row adds them in column order.  Thread 0 then adds the tile's rows in order into nine fp64 sums -- the row sums, their
// squares, the squares of K, the diagonal and its squares, and the dot product of the two phases' row sums -- and writes them to the
// workspace [S][2][row tiles][MMD_PARTIALS].  No m x m matrix exists in memory.  poly_mmd_finish_kernel: one thread per subset adds
// the row tiles' sums in order and evaluates mmd2, zeta1_est, zeta2_est and var_est in fp64.  A subset's workgroups read nothing of
// another subset, and every partial is written before the finishing kernel reads it (no zero-initialised workspace).
//
// Feature statistics: feature_mean_kernel (one thread per column, rows in order, fp64) and feature_cov_kernel (16 x 16 tile of sigma
// per workgroup, 64 centred rows at a time through LDS in fp64, one fused multiply-add per row in order, divisor N - 1):
// np.mean(axis=0) and np.cov(rowvar=False) of the promoted features.
#pragma once
#include "common.h"

namespace mdm {

constexpr int MET_TILE = 64;             // rows and columns of a pair tile, at every N
constexpr int MET_KC = 64;               // features per LDS chunk
constexpr int MET_LD = MET_KC + 4;       // floats per LDS row: 16-byte aligned rows, the 16 rows of a wave's reads on distinct banks
constexpr int MET_KNN_MAX = 8;           // k + 1 <= 8
constexpr int MMD_PARTIALS = 16;         // doubles per (subset, side, row tile) in the workspace; the first nine are used

// d2 += (a - b)^2 over four features, ascending: the one distance statement of this file
__device__ __forceinline__ float dist2_add4(float acc, float4 a, float4 b) {
  float d = a.x - b.x;
  acc = fmaf(d, d, acc);
  d = a.y - b.y;
  acc = fmaf(d, d, acc);
  d = a.z - b.z;
  acc = fmaf(d, d, acc);
  d = a.w - b.w;
  return fmaf(d, d, acc);
}

// features k .. k + 3 of a row of D features; zero behind D.  16-byte load when every row is 16-byte aligned (`vec`).
__device__ __forceinline__ float4 met_load4(const float* row, int k, int D, bool vec) {
  if (vec && k + 4 <= D) return ld4(row + k);
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = (k + i < D) ? row[k + i] : 0.f;
  return make_float4(v[0], v[1], v[2], v[3]);
}

// d2 of two rows in global memory (gather_dist): the same chain, four features at a time
__device__ __forceinline__ float pair_dist2(const float* a, const float* b, int D, bool vec) {
  float acc = 0.f;
  for (int k = 0; k < D; k += 4) acc = dist2_add4(acc, met_load4(a, k, D, vec), met_load4(b, k, D, vec));
  return acc;
}

// Stage features [k0, k0 + MET_KC) of the 64 rows first .. first + 63 of x (through `idx` when given) into tile[64][MET_LD]; rows
// behind n and features behind D are zeros.  256 threads: 16 float4 per row, 4 rows per thread.
__device__ __forceinline__ void met_stage(float (*tile)[MET_LD], const float* x, const int* idx, int first, int n, int D, int k0, bool vec) {
  const int tid = threadIdx.x;
  const int c4 = (tid & 15) * 4;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = (tid >> 4) + 16 * p;
    float4 v = zero4();
    if (first + r < n) {
      const size_t src = idx ? (size_t)idx[first + r] : (size_t)(first + r);
      v = met_load4(x + src * (size_t)D, k0 + c4, D, vec);
    }
    st4(&tile[r][c4], v);
  }
}

// acc[i][c] = d2(row first_a + 4 ty + i of a, row first_b + tx + 16 c of b), through the two LDS tiles; ends behind a barrier-free read
// phase, so the caller synchronises before it restages
__device__ __forceinline__ void dist_tile(float (*as)[MET_LD], float (*bs)[MET_LD], const float* a, int first_a, int na, const float* b,
                                          int first_b, int nb, int D, bool vec, float (&acc)[4][4]) {
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;
  for (int k0 = 0; k0 < D; k0 += MET_KC) {
    __syncthreads();                       // the previous chunk's (or the caller's) reads of the tiles are over
    met_stage(as, a, nullptr, first_a, na, D, k0, vec);
    met_stage(bs, b, nullptr, first_b, nb, D, k0, vec);
    __syncthreads();
    const int kn = min(MET_KC, (D - k0 + 3) & ~3);
    for (int k = 0; k < kn; k += 4) {
      float4 av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = ld4(&as[4 * ty + i][k]);
#pragma unroll
      for (int c = 0; c < 4; ++c) bv[c] = ld4(&bs[tx + 16 * c][k]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = dist2_add4(acc[i][c], av[i], bv[c]);
    }
  }
}

struct KnnArgs {
  const float* a;       // [N][D]
  float* radius2;       // [N]
  int N, D, k, vec;      // vec: D % 4 == 0 and a 16-byte aligned base, so every row takes 16-byte loads
};

__global__ __launch_bounds__(256) void knn_radius_kernel(KnnArgs p) {
  __shared__ __attribute__((aligned(16))) float as[MET_TILE][MET_LD];
  __shared__ __attribute__((aligned(16))) float bs[MET_TILE][MET_LD];
  __shared__ float ds[MET_TILE][MET_TILE + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int row0 = (int)blockIdx.x * MET_TILE;
  const bool vec = p.vec != 0;
  const float inf = __builtin_huge_valf();
  float best[MET_KNN_MAX];                 // ascending; thread r < 64 keeps row row0 + r's
#pragma unroll
  for (int i = 0; i < MET_KNN_MAX; ++i) best[i] = inf;
  for (int col0 = 0; col0 < p.N; col0 += MET_TILE) {
    float acc[4][4];
    dist_tile(as, bs, p.a, row0, p.N, p.a, col0, p.N, p.D, vec, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) ds[4 * ty + i][tx + 16 * c] = acc[i][c];
    __syncthreads();
    if (tid < MET_TILE) {
      const int nc = min(MET_TILE, p.N - col0);
      for (int c = 0; c < nc; ++c) {
        float v = ds[tid][c];
        if (v < best[MET_KNN_MAX - 1]) {
#pragma unroll
          for (int i = 0; i < MET_KNN_MAX; ++i) {      // insert: v sinks to its place, the largest falls out
            const float lo = fminf(best[i], v);
            v = fmaxf(best[i], v);
            best[i] = lo;
          }
        }
      }
    }
    // (ds is rewritten behind dist_tile's barriers of the next column tile)
  }
  if (tid < MET_TILE && row0 + tid < p.N) {
    float r = best[0];
#pragma unroll
    for (int i = 1; i < MET_KNN_MAX; ++i) r = (i == p.k) ? best[i] : r;
    p.radius2[row0 + tid] = r;
  }
}

struct MemberArgs {
  const float* a;        // [NA][D]
  const float* radius2;  // [NA]
  const float* b;        // [NB][D]
  uint8_t* member;       // [NB]
  int NA, NB, D, vec;
};

__global__ __launch_bounds__(256) void manifold_members_kernel(MemberArgs p) {
  __shared__ __attribute__((aligned(16))) float as[MET_TILE][MET_LD];
  __shared__ __attribute__((aligned(16))) float bs[MET_TILE][MET_LD];
  __shared__ int hit[MET_TILE][16];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int row0 = (int)blockIdx.x * MET_TILE;
  const bool vec = p.vec != 0;
  int in[4] = {0, 0, 0, 0};
  for (int col0 = 0; col0 < p.NA; col0 += MET_TILE) {
    float acc[4][4];
    dist_tile(as, bs, p.b, row0, p.NB, p.a, col0, p.NA, p.D, vec, acc);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = col0 + tx + 16 * c;
      if (col < p.NA) {
        const float r2 = p.radius2[col];
#pragma unroll
        for (int i = 0; i < 4; ++i) in[i] |= (acc[i][c] <= r2) ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) hit[4 * ty + i][tx] = in[i];
  __syncthreads();
  if (tid < MET_TILE && row0 + tid < p.NB) {
    int any = 0;
    for (int c = 0; c < 16; ++c) any |= hit[tid][c];
    p.member[row0 + tid] = (uint8_t)any;
  }
}

// count = sum of member[0 .. n): one workgroup, thread t adds elements t, t + 256, ..., then the threads' sums in order
__global__ __launch_bounds__(256) void count_members_kernel(const uint8_t* member, int n, int* count) {
  __shared__ int part[256];
  int s = 0;
  for (int i = threadIdx.x; i < n; i += 256) s += member[i] != 0;
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int i = 0; i < 256; ++i) t += part[i];
    *count = t;
  }
}

struct GatherDistArgs {
  const float* x;       // [N][D]
  const int* first;     // [P]
  const int* second;    // [P]
  float* dist;          // [P]
  int P, D, vec;
};

__global__ __launch_bounds__(256) void gather_dist_kernel(GatherDistArgs p) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= p.P) return;
  const bool vec = p.vec != 0;
  p.dist[i] = sqrtf(pair_dist2(p.x + (size_t)p.first[i] * p.D, p.x + (size_t)p.second[i] * p.D, p.D, vec));
}

// mean of v[0 .. n) in fp64: one workgroup, thread t adds elements t, t + 256, ... in order, then thread 0 the threads' sums in order
__global__ __launch_bounds__(256) void mean_f64_kernel(const float* v, int n, double* mean) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)v[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += part[i];
    *mean = t / (double)n;
  }
}

// ---- polynomial MMD ---------------------------------------------------------------------------------------------------------------------
struct PolyMmdArgs {
  const float* g;       // [Ng][D]
  const float* r;       // [Nr][D]
  const int* idx_g;     // [S][m]
  const int* idx_r;     // [S][m]
  double* partial;      // [S][2][tiles][MMD_PARTIALS]
  double gamma, coef0;
  int m, D, degree, tiles, vec;
};

__device__ __forceinline__ double poly_kernel_value(float g, double gamma, double coef0, int degree) {
  const double base = gamma * (double)g + coef0;
  double k = base;
  for (int d = 1; d < degree; ++d) k *= base;
  return k;
}

__global__ __launch_bounds__(256) void poly_mmd_kernel(PolyMmdArgs p) {
  // the operand tiles and, between the phases, the lanes' fp64 partials [64 rows][64 column slots] share one block of LDS
  constexpr int kTileFloats = MET_TILE * MET_LD;
  static_assert(2 * kTileFloats * sizeof(float) >= MET_TILE * MET_TILE * sizeof(double), "the partials fit into the tiles");
  __shared__ __attribute__((aligned(16))) float smem[2 * kTileFloats];
  __shared__ double row_sum[2][MET_TILE], row_sq[2][MET_TILE], diag[MET_TILE];
  float (*as)[MET_LD] = reinterpret_cast<float (*)[MET_LD]>(smem);
  float (*bs)[MET_LD] = reinterpret_cast<float (*)[MET_LD]>(smem + kTileFloats);
  double (*red)[MET_TILE] = reinterpret_cast<double (*)[MET_TILE]>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;          // the wave's 32 x 32 block of the tile
  const int li = lane & 31, lh = lane >> 5;
  const int rt = (int)blockIdx.x, side = (int)blockIdx.y, s = (int)blockIdx.z;
  const int m = p.m, D = p.D;
  const bool vec = p.vec != 0;
  const float* x_rows = side == 0 ? p.g : p.r;
  const int* i_rows = (side == 0 ? p.idx_g : p.idx_r) + (size_t)s * m;
  const float* x_other = side == 0 ? p.r : p.g;
  const int* i_other = (side == 0 ? p.idx_r : p.idx_g) + (size_t)s * m;
  const int row0 = rt * MET_TILE;

  if (tid < MET_TILE) diag[tid] = 0.0;
  for (int phase = 0; phase < 2; ++phase) {         // 0: against the rows' own set (diagonal left out of the row sums); 1: the other set
    const float* x_cols = phase == 0 ? x_rows : x_other;
    const int* i_cols = phase == 0 ? i_rows : i_other;
    double sum[16], sq[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) sum[e] = sq[e] = 0.0;
    for (int col0 = 0; col0 < m; col0 += MET_TILE) {
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
      for (int k0 = 0; k0 < D; k0 += MET_KC) {
        __syncthreads();
        met_stage(as, x_rows, i_rows, row0, m, D, k0, vec);
        met_stage(bs, x_cols, i_cols, col0, m, D, k0, vec);
        __syncthreads();
        const int kn = min(MET_KC, (D - k0 + 1) & ~1);
        const float* ap = &as[32 * wr + li][lh];
        const float* bp = &bs[32 * wc + li][lh];
        for (int k = 0; k < kn; k += 2) acc = mfma_f32(ap[k], bp[k], acc);
      }
      const int col = col0 + 32 * wc + li;
      if (col < m) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int rl = 32 * wr + mfma_row(e, lh);
          const int row = row0 + rl;
          if (row < m) {
            const double kv = poly_kernel_value(acc[e], p.gamma, p.coef0, p.degree);
            sq[e] = fma(kv, kv, sq[e]);
            if (phase == 0 && row == col) diag[rl] = kv;
            else sum[e] += kv;
          }
        }
      }
    }
    // the lanes' partials of a row, in column-slot order: first the sums, then the squares
    for (int what = 0; what < 2; ++what) {
      __syncthreads();                               // the tiles (or the previous partials) are no longer read
#pragma unroll
      for (int e = 0; e < 16; ++e) red[32 * wr + mfma_row(e, lh)][32 * wc + li] = what == 0 ? sum[e] : sq[e];
      __syncthreads();
      if (tid < MET_TILE) {
        double t = 0.0;
        for (int c = 0; c < MET_TILE; ++c) t += red[tid][c];
        (what == 0 ? row_sum : row_sq)[phase][tid] = t;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    double o[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int nr = min(MET_TILE, m - row0);
    for (int r = 0; r < nr; ++r) {
      const double a = row_sum[0][r], b = row_sum[1][r], d = diag[r];
      o[0] += a;                      // Kt_sum of the own set
      o[1] = fma(a, a, o[1]);         // _sqn(Kt_sums)
      o[2] += row_sq[0][r];           // _sqn(K) of the own set, diagonal included
      o[3] += d;                      // sum_diag
      o[4] = fma(d, d, o[4]);         // sum_diag2
      o[5] += b;                      // K_XY_sum
      o[6] = fma(b, b, o[6]);         // _sqn(K_XY_sums_1) (side 0) / _sqn(K_XY_sums_0) (side 1)
      o[7] += row_sq[1][r];           // K_XY_2_sum
      o[8] = fma(a, b, o[8]);         // dot_XX_XY (side 0) / dot_YY_YX (side 1)
    }
    double* out = p.partial + (((size_t)s * 2 + side) * p.tiles + rt) * MMD_PARTIALS;
    for (int i = 0; i < 9; ++i) out[i] = o[i];
  }
}

struct PolyMmdFinishArgs {
  const double* partial;
  double* mmd2;         // [S]
  double* var;          // [S]
  int S, m, tiles, var_at_m;
};

// kid.py _mmd2_and_variance, mmd_est = 'unbiased', from the sums of both sides
__global__ __launch_bounds__(64) void poly_mmd_finish_kernel(PolyMmdFinishArgs p) {
  const int s = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (s >= p.S) return;
  double t[2][9];
  for (int side = 0; side < 2; ++side) {
    for (int i = 0; i < 9; ++i) t[side][i] = 0.0;
    for (int rt = 0; rt < p.tiles; ++rt) {
      const double* in = p.partial + (((size_t)s * 2 + side) * p.tiles + rt) * MMD_PARTIALS;
      for (int i = 0; i < 9; ++i) t[side][i] += in[i];
    }
  }
  const double m = (double)p.m, m1 = m - 1.0, m2 = m - 2.0;
  const double Kt_XX_sum = t[0][0], Kt_YY_sum = t[1][0], K_XY_sum = t[0][5];
  const double Kt_XX_2_sum = t[0][2] - t[0][4], Kt_YY_2_sum = t[1][2] - t[1][4], K_XY_2_sum = t[0][7];
  const double sqn_Kt_XX_sums = t[0][1], sqn_Kt_YY_sums = t[1][1], sqn_K_XY_sums_1 = t[0][6], sqn_K_XY_sums_0 = t[1][6];
  const double dot_XX_XY = t[0][8], dot_YY_YX = t[1][8];
  const double mmd2 = (Kt_XX_sum + Kt_YY_sum) / (m * m1) - 2.0 * K_XY_sum / (m * m);
  const double mm1sq = (m * m1) * (m * m1), m4 = m * m * m * m, m3 = m * m * m;
  const double zeta1 = 1.0 / (m * m1 * m2) * (sqn_Kt_XX_sums - Kt_XX_2_sum + sqn_Kt_YY_sums - Kt_YY_2_sum)
                       - 1.0 / mm1sq * (Kt_XX_sum * Kt_XX_sum + Kt_YY_sum * Kt_YY_sum)
                       + 1.0 / (m * m * m1) * (sqn_K_XY_sums_1 + sqn_K_XY_sums_0 - 2.0 * K_XY_2_sum)
                       - 2.0 / m4 * K_XY_sum * K_XY_sum
                       - 2.0 / (m * m * m1) * (dot_XX_XY + dot_YY_YX)
                       + 2.0 / (m3 * m1) * (Kt_XX_sum + Kt_YY_sum) * K_XY_sum;
  const double zeta2 = 1.0 / (m * m1) * (Kt_XX_2_sum + Kt_YY_2_sum)
                       - 1.0 / mm1sq * (Kt_XX_sum * Kt_XX_sum + Kt_YY_sum * Kt_YY_sum)
                       + 2.0 / (m * m) * K_XY_2_sum
                       - 2.0 / m4 * K_XY_sum * K_XY_sum
                       - 4.0 / (m * m * m1) * (dot_XX_XY + dot_YY_YX)
                       + 4.0 / (m3 * m1) * (Kt_XX_sum + Kt_YY_sum) * K_XY_sum;
  const double v = (double)p.var_at_m;
  p.mmd2[s] = mmd2;
  p.var[s] = 4.0 * (v - 2.0) / (v * (v - 1.0)) * zeta1 + 2.0 / (v * (v - 1.0)) * zeta2;
}

// ---- feature statistics -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void feature_mean_kernel(const float* x, int N, int D, double* mu) {
  const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (j >= D) return;
  double s = 0.0;
  for (int n = 0; n < N; ++n) s += (double)x[(size_t)n * D + j];
  mu[j] = s / (double)N;
}

constexpr int COV_TILE = 16, COV_ROWS = 64;

__global__ __launch_bounds__(256) void feature_cov_kernel(const float* x, const double* mu, int N, int D, double* sigma) {
  __shared__ double xi[COV_ROWS][COV_TILE], xj[COV_ROWS][COV_TILE + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = (int)blockIdx.y * COV_TILE, j0 = (int)blockIdx.x * COV_TILE;
  const double mi = i0 + tx < D ? mu[i0 + tx] : 0.0, mj = j0 + tx < D ? mu[j0 + tx] : 0.0;
  double acc = 0.0;
  for (int n0 = 0; n0 < N; n0 += COV_ROWS) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < COV_ROWS / 16; ++q) {       // thread (ty, tx) stages rows ty + 16 q, column tx of both blocks, centred
      const int r = ty + 16 * q, n = n0 + r;
      xi[r][tx] = (n < N && i0 + tx < D) ? (double)x[(size_t)n * D + i0 + tx] - mi : 0.0;
      xj[r][tx] = (n < N && j0 + tx < D) ? (double)x[(size_t)n * D + j0 + tx] - mj : 0.0;
    }
    __syncthreads();
    const int nn = min(COV_ROWS, N - n0);
    for (int r = 0; r < nn; ++r) acc = fma(xi[r][ty], xj[r][tx], acc);
  }
  if (i0 + ty < D && j0 + tx < D) sigma[(size_t)(i0 + ty) * D + j0 + tx] = acc / (double)(N - 1);
}

}  // namespace mdm
