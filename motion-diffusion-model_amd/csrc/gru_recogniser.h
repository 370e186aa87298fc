// The HumanAct12 GRU action recogniser behind A2MEvaluation (eval/a2m/action2motion/models.py:6-61 MotionDiscriminator /
// MotionDiscriminatorForFID; eval/a2m/gru_eval.py), eval mode, on gfx950 in exact fp32:
//   x [B, njoints, nfeats, T] = [B, I, T]  ->  nn.GRU(I, H, L) over the frames from h0 [L, B, H]  ->  the last layer's output at frame
//   lengths[b] - 1  ->  features = tanh(linear1(h)) [B, mid]  ->  yhat = linear2(features) [B, num_class].
// Per layer:
//   * the input projections of ALL frames, gi[(b T + t)][3H] = x_t W_ih^T + b_ih, are ONE GEMM on gemm_f32.h's v_mfma_f32_32x32x2_f32
//     kernel (always the 64-row tile).  Layer 0 reads x[b][k][t] in place through GruFrameLoader (T innermost, no permuted copy; k >= I
//     reads as zero, so I need be no multiple of anything) against W_ih through evaluator.h's ScalarRowLoader (I = 54: rows of W_ih are
//     not 16-byte aligned); layers >= 1 read the previous layer's [B][T][H] output through RowMajorLoader;
//   * gru_seq_kernel<H> runs the WHOLE recurrence of the layer in one launch.  PyTorch's gate equations (evaluator.h:108-109), gate
//     order r, z, n, b_hn inside the r (...) term:
//       r = s(gi_r + W_hr h + b_hr)   z = s(gi_z + W_hz h + b_hz)   n = tanh(gi_n + r (W_hn h + b_hn))   h' = (1 - z) n + z h
//     One workgroup owns GRU_SEQ_ROWS = 16 sequences and all H hidden units, H / 16 waves; wave w owns hidden units [16 w, 16 w + 16)
//     and their r, z and n columns together, so the gate math is the wave's own epilogue.  Its 3 x 16 x H slice of W_hh sits in
//     registers in v_mfma_f32_16x16x4_f32 B-operand layout for all steps (H = 128: 96 VGPRs); h_{t-1} [16][H] is the A operand, read
//     from LDS; gi of frame t + 1 is fetched under the MFMAs of frame t; the wave writes its 16 columns of h_t into the OTHER LDS
//     buffer (and to [B][T][H] when a further layer follows); ONE workgroup barrier ends the step.  Nothing crosses workgroups.
//   * lengths: len_b is read from device memory and clamped to [1, T]; a row with t >= len_b keeps its h bit for bit (it neither
//     loads gi nor stores); the workgroup runs max(len_b) <= T steps over its own rows; pad rows of the last tile have length 0 and
//     touch no memory.  After the last step h[b] IS gru_o[lengths[b] - 1, b] of this layer and is written as [B][H].
// gru_tail_kernel: one 64-thread workgroup per row, both linear layers, sums in one fixed order.
// Row invariance: one tile shape, one k order per sum, and no value of a row ever meets another row's -- a sample's features and
// logits are the same bits alone, at any row of any batch and beside any lengths.
#pragma once
#include "common.h"
#include "gemm_f32.h"
#include "evaluator.h"      // ScalarRowLoader, LeakyEpilogue (out = acc + bias), sigmoid_f32

namespace mdm {

constexpr int GRU_SEQ_ROWS = 16;        // sequences per workgroup of gru_seq_kernel, at every batch size
constexpr int GRU_TAIL_MAX = 64;        // linear1's width (30) and num_class are run-time values up to this

// A operand of layer 0's input projection over x [B][I][T] (T contiguous): logical row m = b T + t, logical k = feature ->
// x[b][k][t], zero for k >= I.  Consecutive threads take consecutive rows (frames): 4-byte loads, coalesced along t.
struct GruFrameLoader {
  static constexpr bool kColumnStaging = true;
  static constexpr bool kGather = true;
  static constexpr bool kFragments = false;
  const float* x;
  int T, I, rows;
  __device__ __forceinline__ float4 load4(int row, int k) const {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < rows) {
      const int b = row / T, t = row - b * T;
      const float* base = x + (size_t)b * I * T + t;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (k + i < I) v[i] = base[(size_t)(k + i) * T];
    }
    return make_float4(v[0], v[1], v[2], v[3]);
  }
};

__device__ __forceinline__ int gru_seq_len(const int* lens, int m, int T) {
  const int l = lens[m];
  return l < 1 ? 1 : (l > T ? T : l);
}

struct GruSeqArgs {
  const float* gi;      // [B T][3H]: W_ih x_t + b_ih of every frame, row b T + t
  const float* w_hh;    // [3H][H]
  const float* b_hh;    // [3H]
  const float* h0;      // [B][H]: this layer's initial state
  const int* lens;      // [B]
  float* seq;           // [B][T][H]: h_t of the frames t < len_b, for the next layer's projection; null for the last layer
  float* h_last;        // [B][H]: h after the row's last step; may be null
  int B, T;
};

template <int H>
__global__ __launch_bounds__(H * 4) void gru_seq_kernel(GruSeqArgs a) {
  static_assert(H % 16 == 0 && H >= 16 && H <= 256, "one wave per 16 hidden units, at most 16 waves");
  constexpr int KB = H / 16;            // 16-deep k blocks: lane (i, q) holds k = 16 kb + 4 q .. + 3 of row i as one float4
  constexpr int LD = H + 4;             // floats per LDS row: the 16-byte fragment reads of a 16-lane group fall on distinct banks
  __shared__ __attribute__((aligned(16))) float hs[2][GRU_SEQ_ROWS][LD];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int jl = lane & 15, q = lane >> 4;
  const int j = 16 * wid + jl;          // the lane's hidden unit: B-operand column and accumulator column
  const int m0 = (int)blockIdx.x * GRU_SEQ_ROWS;
  const int B = a.B, T = a.T;

  // the tile's step count, and the lengths of the lane's four accumulator rows 4 q + r (0: a pad row)
  int steps = 0;
  for (int i = 0; i < GRU_SEQ_ROWS; ++i)
    if (m0 + i < B) {
      const int l = gru_seq_len(a.lens, m0 + i, T);
      steps = l > steps ? l : steps;
    }
  int len[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + 4 * q + r;
    len[r] = m < B ? gru_seq_len(a.lens, m, T) : 0;
  }

  // W_hh: B[k][j] = W_hh[g H + j][k]; MFMA number 4 kb + e of a step pairs the k = 16 kb + 4 q + e of both operands
  float4 w[3][KB];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) w[g][kb] = ld4(a.w_hh + ((size_t)g * H + j) * H + 16 * kb + 4 * q);
  const float br = a.b_hh[j], bz = a.b_hh[H + j], bn = a.b_hh[2 * H + j];

  float hv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    hv[r] = len[r] > 0 ? a.h0[(size_t)(m0 + 4 * q + r) * H + j] : 0.f;
    hs[0][4 * q + r][j] = hv[r];
  }

  // gi of the lane's four rows at frame t, one vector per gate; a row that has ended (or a pad row) loads nothing
  struct Gates { f32x4 r, z, n; };
  auto fetch = [&](int t) __attribute__((always_inline)) {
    Gates g{f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (t < len[r]) {
        const float* p = a.gi + ((size_t)(m0 + 4 * q + r) * T + t) * (3 * (size_t)H) + j;
        g.r[r] = p[0];
        g.z[r] = p[H];
        g.n[r] = p[2 * H];
      }
    return g;
  };
  Gates gc = fetch(0);
  wg_barrier();

  for (int t = 0; t < steps; ++t) {
    const int cur = t & 1;
    const Gates gn = fetch(t + 1);       // in flight under this step's MFMAs
    f32x4 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the lane's whole A row first: the fragment reads retire in order under the MFMAs in front of them
    float4 fa[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) fa[kb] = ld4(&hs[cur][jl][16 * kb + 4 * q]);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int g = 0; g < 3; ++g) acc[g] = mfma16_f32(fa[kb].x, w[g][kb].x, acc[g]);
#pragma unroll
      for (int g = 0; g < 3; ++g) acc[g] = mfma16_f32(fa[kb].y, w[g][kb].y, acc[g]);
#pragma unroll
      for (int g = 0; g < 3; ++g) acc[g] = mfma16_f32(fa[kb].z, w[g][kb].z, acc[g]);
#pragma unroll
      for (int g = 0; g < 3; ++g) acc[g] = mfma16_f32(fa[kb].w, w[g][kb].w, acc[g]);
    }
    // gate math: the lane holds hidden unit j of rows 4 q + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (t < len[r]) {
        const float rg = sigmoid_f32(gc.r[r] + (acc[0][r] + br));
        const float zg = sigmoid_f32(gc.z[r] + (acc[1][r] + bz));
        const float ng = tanhf(gc.n[r] + rg * (acc[2][r] + bn));
        hv[r] = (1.0f - zg) * ng + zg * hv[r];
        if (a.seq != nullptr) a.seq[((size_t)(m0 + 4 * q + r) * T + t) * H + j] = hv[r];
      }
      hs[cur ^ 1][4 * q + r][j] = hv[r];
    }
    gc = gn;
    wg_barrier();       // h_t complete in hs[cur ^ 1]; every read of hs[cur] is behind its wave (the next step overwrites it)
  }

  if (a.h_last != nullptr) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (len[r] > 0) a.h_last[(size_t)(m0 + 4 * q + r) * H + j] = hv[r];
  }
}

// features[b][i] = tanh(W1[i] . h[b] + b1[i]), i < mid;  yhat[b][c] = W2[c] . features[b] + b2[c], c < num_class.  One 64-thread
// workgroup per row.  Orders, the same for every row whatever B is: k into the partial sum k % 4, then (s0 + s1) + (s2 + s3), + bias
// for linear1 (H % 4 == 0); k ascending in one chain for linear2.
struct GruTailArgs {
  const float* h;       // [B][H]
  const float* w1;      // [mid][H]
  const float* b1;
  const float* w2;      // [num_class][mid]
  const float* b2;
  float* features;      // [B][mid]
  float* yhat;          // [B][num_class]
  int H, mid, num_class;
};

__global__ __launch_bounds__(64) void gru_tail_kernel(GruTailArgs a) {
  __shared__ float feat[GRU_TAIL_MAX];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  if (tid < a.mid) {
    const float* hp = a.h + b * a.H;
    const float* wp = a.w1 + (size_t)tid * a.H;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
    for (int k = 0; k < a.H; k += 4) {
      const float4 wv = ld4(wp + k), xv = ld4(hp + k);
      d0 = fmaf(wv.x, xv.x, d0);
      d1 = fmaf(wv.y, xv.y, d1);
      d2 = fmaf(wv.z, xv.z, d2);
      d3 = fmaf(wv.w, xv.w, d3);
    }
    const float f = tanhf(((d0 + d1) + (d2 + d3)) + a.b1[tid]);
    feat[tid] = f;
    a.features[b * a.mid + tid] = f;
  }
  __syncthreads();
  if (tid < a.num_class) {
    const float* wp = a.w2 + (size_t)tid * a.mid;
    float d = 0.f;
    for (int k = 0; k < a.mid; ++k) d = fmaf(wp[k], feat[k], d);
    a.yhat[b * a.num_class + tid] = d + a.b2[tid];
  }
}

}  // namespace mdm
