// The metrics of the HumanML3D / KIT evaluation (data_loaders/humanml/utils/metrics.py behind eval/eval_humanml.py) and of the a2m
// family (eval/a2m/*/accuracy.py) on gfx950, on features that are already on the device: R-precision and matching score over the
// reference's batches, the Euclidean distance matrix, and argmax + confusion matrix of a recogniser's scores.
//
// Distances are metrics.h's: dist2_add4 is the one statement of d2, met_stage / dist_tile the one 64 x 64 pair tile.  d2 of two rows
// is the same bits wherever the rows stand (metrics.h), so a row's rank and distance do not depend on its group's place in the call.
//   retrieval_ranks_kernel: workgroup (group g, 64-row tile rt of the group).  The group is rows [b, e) of q (texts) and c (motions),
//     from group_offsets; every offset is clamped into [0, N], e to >= b and e - b to max_group_rows, so a corrupt table gives wrong
//     ranks, never an access outside q, c, rank or diag.  A workgroup whose row tile starts behind e exits (before any barrier).
//     Column tile rt comes first: it holds the diagonal d2(q_i, c_i), which the owning thread passes through LDS to the 16 threads of
//     row i; then the other column tiles of the group.  Per tile a thread compares its 4 x 4 values in the squared domain:
//       rank[i] = #{j in [b, e): d2(q_i, c_j) < d2(q_i, c_i)} + #{j in [b, i): d2(q_i, c_j) == d2(q_i, c_i)}
//     -- the position of i in a stable ascending sort of row i.  The 16 partial counts of a row are added in thread order (integers).
//     diag[i] = sqrt(d2(q_i, c_i)).
//   retrieval_finish_kernel: one workgroup.  topk_count[k] = #{i: rank[i] <= k}, k < top_k (int64; thread t counts rows t, t + 256,
//     ..., thread 0 adds the threads' histograms in order and accumulates over k); diag_sum = sum_i diag[i] in fp64 in row order (256
//     values at a time through LDS, added by thread 0).
//   dist_matrix_kernel: out[i][j] = sqrt(d2(a_i, b_j)), one dist_tile per workgroup: exactly 0 for equal rows, never NaN for finite rows.
//   confusion_kernel: one thread per sample: pred[n] = argmax_c yhat[n][c], the lowest index among equal maxima, a NaN counts as the
//     maximum and the first NaN wins (torch.max(dim=1) on the CPU); confusion[label[n]][pred[n]] += 1 (int64, integer atomics: the result
//     does not depend on their order; the caller zeroes the matrix and may accumulate several calls); a label outside [0, C) is not
//     counted but adds 1 to `bad` (int32).
#pragma once
#include "metrics.h"

namespace mdm {

constexpr int RET_TOPK_MAX = 16;

struct RetrievalArgs {
  const float* q;            // [N][D] queries (text embeddings)
  const float* c;            // [N][D] candidates (motion embeddings)
  const int* group_offsets;  // [n_groups + 1]
  int* rank;                 // [N]
  float* diag;               // [N]
  int N, D, n_groups, max_group_rows, row_tiles, vec;
};

__global__ __launch_bounds__(256) void retrieval_ranks_kernel(RetrievalArgs p) {
  __shared__ __attribute__((aligned(16))) float as[MET_TILE][MET_LD];
  __shared__ __attribute__((aligned(16))) float bs[MET_TILE][MET_LD];
  __shared__ float dsh[MET_TILE];
  __shared__ int hit[MET_TILE][16];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int g = (int)blockIdx.x / p.row_tiles, rt = (int)blockIdx.x % p.row_tiles;
  const bool vec = p.vec != 0;
  const int b = min(max(p.group_offsets[g], 0), p.N);
  int e = min(max(p.group_offsets[g + 1], b), p.N);
  e = b + min(e - b, p.max_group_rows);
  const int row0 = b + rt * MET_TILE;
  if (row0 >= e) return;                    // (the whole workgroup: b, e and rt are uniform)
  const int tiles = (e - b + MET_TILE - 1) / MET_TILE;
  float dg[4] = {0.f, 0.f, 0.f, 0.f};
  int cnt[4] = {0, 0, 0, 0};
  for (int t = 0; t < tiles; ++t) {
    const int ct = t == 0 ? rt : (t <= rt ? t - 1 : t);      // the diagonal's tile first, then the others in ascending order
    const int col0 = b + ct * MET_TILE;
    float acc[4][4];
    dist_tile(as, bs, p.q, row0, e, p.c, col0, e, p.D, vec, acc);
    if (t == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (4 * ty + i == tx + 16 * c) dsh[4 * ty + i] = acc[i][c];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) dg[i] = dsh[4 * ty + i];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = col0 + tx + 16 * c;
      if (col < e) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = row0 + 4 * ty + i;
          cnt[i] += (acc[i][c] < dg[i] || (acc[i][c] == dg[i] && col < row)) ? 1 : 0;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) hit[4 * ty + i][tx] = cnt[i];
  __syncthreads();
  if (tid < MET_TILE && row0 + tid < e) {
    int r = 0;
    for (int c = 0; c < 16; ++c) r += hit[tid][c];
    p.rank[row0 + tid] = r;
    p.diag[row0 + tid] = sqrtf(dsh[tid]);
  }
}

__global__ __launch_bounds__(256) void retrieval_finish_kernel(const int* rank, const float* diag, int n, int top_k, long long* topk_count,
                                                               double* diag_sum) {
  __shared__ int hist[256][RET_TOPK_MAX];
  __shared__ float dv[256];
  const int tid = threadIdx.x;
  int h[RET_TOPK_MAX];
#pragma unroll
  for (int k = 0; k < RET_TOPK_MAX; ++k) h[k] = 0;
  for (int i = tid; i < n; i += 256) {
    const int r = rank[i];
#pragma unroll
    for (int k = 0; k < RET_TOPK_MAX; ++k) h[k] += (r == k) ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < RET_TOPK_MAX; ++k) hist[tid][k] = h[k];
  double s = 0.0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    __syncthreads();                               // thread 0 has read the previous 256 values (and, the first time, hist is written)
    dv[tid] = i0 + tid < n ? diag[i0 + tid] : 0.f;
    __syncthreads();
    if (tid == 0) {
      const int nn = min(256, n - i0);
      for (int i = 0; i < nn; ++i) s += (double)dv[i];
    }
  }
  if (tid == 0) {
    *diag_sum = s;
    long long run = 0;
    for (int k = 0; k < top_k; ++k) {
      long long t = 0;
      for (int i = 0; i < 256; ++i) t += hist[i][k];
      run += t;
      topk_count[k] = run;
    }
  }
}

struct DistMatrixArgs {
  const float* a;       // [NA][D]
  const float* b;       // [NB][D]
  float* out;           // [NA][NB]
  int NA, NB, D, vec;
};

__global__ __launch_bounds__(256) void dist_matrix_kernel(DistMatrixArgs p) {
  __shared__ __attribute__((aligned(16))) float as[MET_TILE][MET_LD];
  __shared__ __attribute__((aligned(16))) float bs[MET_TILE][MET_LD];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int row0 = (int)blockIdx.y * MET_TILE, col0 = (int)blockIdx.x * MET_TILE;
  float acc[4][4];
  dist_tile(as, bs, p.a, row0, p.NA, p.b, col0, p.NB, p.D, p.vec != 0, acc);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + 4 * ty + i;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = col0 + tx + 16 * c;
      if (row < p.NA && col < p.NB) p.out[(size_t)row * p.NB + col] = sqrtf(acc[i][c]);
    }
  }
}

struct ConfusionArgs {
  const float* yhat;      // [N][C]
  const int* labels;      // [N]
  int* pred;              // [N]
  long long* confusion;   // [C][C], accumulated
  int* bad;               // accumulated
  int N, C;
};

__global__ __launch_bounds__(256) void confusion_kernel(ConfusionArgs p) {
  const int n = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (n >= p.N) return;
  const float* y = p.yhat + (size_t)n * p.C;
  float best = y[0];
  int bi = 0;
  for (int c = 1; c < p.C; ++c) {
    const float v = y[c];
    if (best == best && (v != v || v > best)) {      // a NaN, once taken, stays; a NaN beats every number; ties keep the lower index
      best = v;
      bi = c;
    }
  }
  p.pred[n] = bi;
  const int label = p.labels[n];
  if (label >= 0 && label < p.C) atomic_add_i64(p.confusion + (size_t)label * p.C + bi, 1);
  else atomic_add_i32(p.bad, 1);
}

}  // namespace mdm
