// The HumanML3D / KIT evaluator's three networks (data_loaders/humanml/networks/modules.py:79-98 MovementConvEncoder, :311-350
// TextEncoderBiGRUCo, :353-386 MotionEncoderBiGRUCo) behind EvaluatorMDMWrapper.get_co_embeddings / get_motion_embeddings
// (evaluator_wrapper.py:121-187), on gfx950.  Everything is exact fp32:
//   * every linear layer, the input projections of ALL time steps of both GRU directions ([B T', H] x [H, 6H]) and the two
//     Conv1d(., ., 4, 2, 1) layers run on gemm_f32.h's v_mfma_f32_32x32x2_f32 skeleton through the loaders / epilogue below (the
//     convolutions as a gather of their 4-tap, stride-2, zero-padded windows: no im2col buffer, no copy of `motions[..., :-4]`);
//   * gru_step_kernel is one recurrent step of both directions: h . W_hh^T on the same MFMA, the gate math in its epilogue.
// Row invariance: the k order of every sum of a row is fixed by the kernels, never by the batch -- gemm_f32.h accumulates in one k
// order under either tile shape, and the step kernel's split-K tree is the same for every row -- so a sequence's embedding does not
// depend on how many other sequences, or which lengths, share the call.
#pragma once
#include "common.h"
#include "gemm_f32.h"

namespace mdm {

__device__ __forceinline__ float leaky02(float v) { return v > 0.f ? v : 0.2f * v; }     // nn.LeakyReLU(0.2)
__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

// A operand of Conv1d(C, ., kernel 4, stride 2, padding 1) over x [B, Tin, ldx] (channels last; the first C of the ldx features
// of a frame are read -- `motions[..., :-4]` for the first layer): logical row m = b * Tout + t, logical k = tap * C + c  ->
// x[b][2 t - 1 + tap][c], zero outside [0, Tin).  The weights come re-laid as [Cout][4][C] (evaluator.py does it once).
struct Conv4GatherLoader {
  static constexpr bool kColumnStaging = false;
  static constexpr bool kGather = true;
  static constexpr bool kFragments = false;
  const float* x;
  int Tin, Tout, ldx, C, rows;
  __device__ __forceinline__ float4 load4(int row, int k) const {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < rows && k < 4 * C) {
      const int b = row / Tout, t = row - b * Tout;
      int tap = k / C, c = k - tap * C;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int tin = 2 * t - 1 + tap;
        if (tap < 4 && tin >= 0 && tin < Tin) v[i] = x[((size_t)b * Tin + tin) * ldx + c];
        if (++c == C) { c = 0; ++tap; }
      }
    }
    return make_float4(v[0], v[1], v[2], v[3]);
  }
};

// A row-major operand whose row stride or K is no multiple of 4 (pos_ohot [B L, 15] and pos_emb.weight [300, 15])
struct ScalarRowLoader {
  static constexpr bool kColumnStaging = false;
  static constexpr bool kGather = true;
  static constexpr bool kFragments = false;
  const float* p;
  int ld, rows, K;
  __device__ __forceinline__ float4 load4(int row, int k) const {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < rows) {
      const float* q = p + (size_t)row * ld;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (k + i < K) v[i] = q[k + i];
    }
    return make_float4(v[0], v[1], v[2], v[3]);
  }
};

// RowMajorLoader with LeakyReLU(0.2) applied on the way in: output_net's activation sits between its LayerNorm and its last Linear
struct LeakyRowLoader {
  static constexpr bool kColumnStaging = false;
  static constexpr bool kGather = false;
  static constexpr bool kFragments = false;
  const float* p;
  int ld, rows, K;
  __device__ __forceinline__ float4 load4(int row, int k) const {
    if (row < rows && k < K) {
      const float4 v = ld4(p + (size_t)row * ld + k);
      return make_float4(leaky02(v.x), leaky02(v.y), leaky02(v.z), leaky02(v.w));
    }
    return zero4();
  }
};

// out[m][n] = acc + bias[n], through LeakyReLU(0.2) when `leaky` (the convolutions)
struct LeakyEpilogue {
  static constexpr bool kVec4 = true;
  static constexpr bool kLn = false;
  float* out;
  const float* bias;
  int ld;
  int leaky;
  struct Row { size_t base; };
  struct Col { int n; float bias; };
  __device__ __forceinline__ Row row(int m) const { return Row{(size_t)m * ld}; }
  __device__ __forceinline__ Col col(int n) const { return Col{n, bias[n]}; }
  __device__ __forceinline__ float pre(const Row&, const Col&) const { return 0.f; }
  __device__ __forceinline__ void store(const Row& r, const Col& c, float acc, float) const {
    const float v = acc + c.bias;
    out[r.base + c.n] = leaky ? leaky02(v) : v;
  }
  __device__ __forceinline__ bool vec4_ok() const { return (ld & 3) == 0; }
  __device__ __forceinline__ float4 pre4(int, int) const { return zero4(); }
  __device__ __forceinline__ void store4(int m, int n, float4 a, float4) const {
    const float4 b4 = ld4(bias + n);
    float4 v = make_float4(a.x + b4.x, a.y + b4.y, a.z + b4.z, a.w + b4.w);
    if (leaky) v = make_float4(leaky02(v.x), leaky02(v.y), leaky02(v.z), leaky02(v.w));
    st4(out + (size_t)m * ld + n, v);
  }
};

// ------------------------------------------------------------------------------------------------
// One step of a bidirectional GRU over packed (variable-length) sequences, PyTorch's equations:
//   r = s(gi_r + W_hr h + b_hr)   z = s(gi_z + W_hz h + b_hz)   n = tanh(gi_n + r (W_hn h + b_hn))   h' = (1 - z) n + z h
// gi [B T'][6H] = W_ih x_t + b_ih of every time step, forward direction's 3H columns first (one GEMM in front of the recurrence).
// Row b has len_b = min(lens[b] / len_div, T') steps; at step s the forward direction reads time s, the backward direction time
// len_b - 1 - s (pack_padded_sequence: it starts at the sequence's own last element); a row with s >= len_b keeps its h bit for bit.
// h lives as [B][2][H] -- after the last step it IS cat(gru_last[0], gru_last[1]) -- and is double-buffered: every workgroup reads all
// H columns of h_in and writes its own 32 of h_out.
//
// Grid (H / 32, ceil(B / 32), 2 directions), 8 waves: a workgroup owns 32 rows x 32 hidden units, i.e. three 32x32 accumulators
// (the r, z and n columns of the SAME units, so the gate math needs nothing from another workgroup); wave w sums k in
// [w H / 8, (w + 1) H / 8) on v_mfma_f32_32x32x2_f32 with both operands straight from global memory (lane (r, hh) holds k = 16 hh ..
// + 15 of a 32-deep tile of its row, as in gemm_f32.h), the next tile's loads in flight under the current tile's 48 MFMAs; the eight
// partial tiles meet in LDS in a fixed tree ((w0 + w4) + (w1 + w5)) + ..., identical for every row.  What bounds it: at H = 1024 a
// step streams both directions' W_hh (25 MB, L2 / MALL resident across steps) into 64 workgroups per 32 rows, and a wave's 192 MFMAs
// are 12k matrix-pipe cycles: a few microseconds either way, next to the 2.6 us of the dependent launch itself.
// ------------------------------------------------------------------------------------------------
constexpr int GRU_WAVES = 8;
constexpr int GRU_THREADS = GRU_WAVES * 64;

__device__ __forceinline__ int gru_len(const int* lens, int m, int len_div, int Tp) {
  int l = lens[m] / len_div;
  l = l < 0 ? 0 : l;
  return l < Tp ? l : Tp;
}

__global__ __launch_bounds__(GRU_THREADS) void gru_step_kernel(const float* __restrict__ gi, const float* __restrict__ w_hh,
                                                               const float* __restrict__ b_hh, const float* __restrict__ h_in,
                                                               float* __restrict__ h_out, const int* __restrict__ lens,
                                                               int len_div, int B, int Tp, int H, int s) {
  __shared__ float part[4 * 48 * 64];      // 48 KB: the partial tiles of waves 4-7, then of waves 1-3
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int j0 = blockIdx.x * 32, m0 = blockIdx.y * 32, d = blockIdx.z;

  // a tile whose rows have all ended only carries h over (the rows of a call are sorted by length: whole tiles end early)
  bool live = false;
  for (int i = 0; i < 32; ++i)
    if (m0 + i < B && s < gru_len(lens, m0 + i, len_div, Tp)) live = true;
  if (!live) {
    for (int e = tid; e < 32 * 32; e += GRU_THREADS) {
      const int m = m0 + (e >> 5);
      const size_t o = ((size_t)m * 2 + d) * H + j0 + (e & 31);
      if (m < B) h_out[o] = h_in[o];
    }
    return;
  }

  // rows beyond B read row B - 1 (in bounds); their accumulator rows are never stored
  const int ma = m0 + r < B ? m0 + r : B - 1;
  const float* ap = h_in + ((size_t)ma * 2 + d) * H + 16 * hh;
  const float* wp = w_hh + ((size_t)d * 3 * H + j0 + r) * H + 16 * hh;
  const size_t gate = (size_t)H * H;
  const int kw = H / GRU_WAVES, k0 = wid * kw, nt = kw / 32;

  f32x16 acc[3];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[g][e] = 0.f;

  float4 fa[2][4], fw[2][3][4];
  auto fetch = [&](auto set_tag, int t) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_tag)::value;
    const int kb = k0 + 32 * t;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      fa[SET][c] = ld4(ap + kb + 4 * c);
#pragma unroll
      for (int g = 0; g < 3; ++g) fw[SET][g][c] = ld4(wp + g * gate + kb + 4 * c);
    }
  };
  auto mac = [&](auto set_tag) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_tag)::value;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        acc[g] = mfma_f32(fa[SET][c].x, fw[SET][g][c].x, acc[g]);
        acc[g] = mfma_f32(fa[SET][c].y, fw[SET][g][c].y, acc[g]);
        acc[g] = mfma_f32(fa[SET][c].z, fw[SET][g][c].z, acc[g]);
        acc[g] = mfma_f32(fa[SET][c].w, fw[SET][g][c].w, acc[g]);
      }
  };
  fetch(std::integral_constant<int, 0>{}, 0);
  for (int t = 0; t < nt; t += 2) {
    if (t + 1 < nt) fetch(std::integral_constant<int, 1>{}, t + 1);
    mac(std::integral_constant<int, 0>{});
    if (t + 2 < nt) fetch(std::integral_constant<int, 0>{}, t + 2);
    if (t + 1 < nt) mac(std::integral_constant<int, 1>{});
  }

  // split-K tree, lane-major [wave][reg][lane] (conflict-free on both sides): waves 4-7 -> waves 0-3, then waves 1-3 -> wave 0
  if (wid >= 4) {
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int e = 0; e < 16; ++e) part[((wid - 4) * 48 + g * 16 + e) * 64 + lane] = acc[g][e];
  }
  __syncthreads();
  if (wid < 4) {
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[g][e] += part[(wid * 48 + g * 16 + e) * 64 + lane];
  }
  __syncthreads();
  if (wid >= 1 && wid < 4) {
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int e = 0; e < 16; ++e) part[((wid - 1) * 48 + g * 16 + e) * 64 + lane] = acc[g][e];
  }
  __syncthreads();
  if (wid != 0) return;
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float p01 = acc[g][e] + part[(0 * 48 + g * 16 + e) * 64 + lane];
      const float p23 = part[(1 * 48 + g * 16 + e) * 64 + lane] + part[(2 * 48 + g * 16 + e) * 64 + lane];
      acc[g][e] = p01 + p23;
    }

  // gate math: lane (r, hh) holds hidden unit j0 + r of rows mfma_row(e, hh); lanes 0-31 run along j (128-byte runs)
  const int j = j0 + r;
  const float* bh = b_hh + (size_t)d * 3 * H + j;
  const float br = bh[0], bz = bh[H], bn = bh[2 * H];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int m = m0 + mfma_row(e, hh);
    if (m < B) {
      const int len = gru_len(lens, m, len_div, Tp);
      const size_t o = ((size_t)m * 2 + d) * H + j;
      const float hp = h_in[o];
      float hv = hp;
      if (s < len) {
        const int t = d == 0 ? s : len - 1 - s;
        const float* g = gi + ((size_t)m * Tp + t) * (6 * (size_t)H) + (size_t)d * 3 * H + j;
        const float rg = sigmoid_f32(g[0] + (acc[0][e] + br));
        const float zg = sigmoid_f32(g[H] + (acc[1][e] + bz));
        const float ng = tanhf(g[2 * H] + rg * (acc[2][e] + bn));
        hv = (1.0f - zg) * ng + zg * hp;
      }
      h_out[o] = hv;
    }
  }
}

// h[b][d][:] = hidden[d][:]   (`self.hidden.repeat(1, num_samples, 1)`, modules.py:341, :377)
__global__ __launch_bounds__(256) void gru_init_kernel(float* __restrict__ h, const float* __restrict__ h0, int B, int H) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)B * 2 * H) h[i] = h0[i % ((size_t)2 * H)];
}

}  // namespace mdm
