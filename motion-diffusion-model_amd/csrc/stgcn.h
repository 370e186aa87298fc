// The ST-GCN action recogniser behind the UESTC and the unconstrained evaluations (eval/a2m/recognition/models/stgcn.py with
// stgcnutils/tgcn.py, and the six-block copy under eval/unconstrained/models/), eval mode, one person per sample, on gfx950 in
// exact fp32.  Activations live channels-last, [N, T, V, C] with row m = (n T + t) V + v, so every convolution of the net is a
// product gemm_f32.h's v_mfma_f32_32x32x2_f32 kernel computes under the loaders and the epilogue below:
//   * graph convolution, ONE GEMM per block.  The 1x1 convolution and the einsum with A_b = A * edge_importance[b] are both linear,
//     so the mix over the nodes goes in FRONT of the convolution:
//       out[(n,t,w), c] = sum_{k,ci} W[k C_out + c, ci] (sum_v x[(n,t,v), ci] A_b[k,v,w])  +  sum_k b[k C_out + c] sum_v A_b[k,v,w]
//     GraphMixLoader forms the inner sum on the fly from the neighbour lists of (k, w) -- A_b keeps the zeros of the skeleton tree,
//     a handful of v per list -- the contraction is K C_in deep, the second term is a [V][C_out] table, and BatchNorm2d + ReLU are
//     the epilogue's per-column scale and per-(node, column) shift;
//   * temporal convolution (9 x 1, stride s, zero padding 4), ONE GEMM: Tap9GatherLoader reads logical k = tap C + c from row
//     (n, t_out s + tap - 4, v), zero outside [0, T); bias and the second BatchNorm2d are the epilogue's scale / shift, then the
//     residual (the block's input, or what the residual GEMM wrote into the output buffer just before) and the ReLU;
//   * convolutional residual (1 x 1, stride s, BatchNorm2d): a GEMM over StrideRowLoader, written to the block's output first.
// stgcn_input_kernel permutes [N, V, C, T] to rows and applies data_bn; stgcn_tail_kernel pools a sample's rows and applies fcn.
// Row invariance: always the 64-row tile, k in the kernel's one order, neighbour lists and pooling in a fixed order -- nothing
// depends on N, so a sample's features and logits are the same bits alone and at any row of any batch.
#pragma once
#include "common.h"
#include "gemm_f32.h"

namespace mdm {

constexpr int STGCN_MAX_NB = 8;          // entries per neighbour list (include/mdm_hip.h MDM_STGCN_MAX_NEIGHBOURS)
constexpr int STGCN_TAPS = 9;
constexpr int STGCN_MAX_POOL_C = 1024;   // channels of the last block (the tail kernel's LDS row)

// A operand of the graph convolution over x [rows / V][V][C] (C % 4 == 0): logical row m = (nt, w), logical k = kk C + ci ->
//   sum_j wgt[kk][w][j] x[nt][idx[kk][w][j]][ci],  j < cnt[kk][w], in list order
struct GraphMixLoader {
  static constexpr bool kColumnStaging = false;
  static constexpr bool kGather = true;
  static constexpr bool kFragments = false;
  const float* x;
  const int* idx;      // [K][V][STGCN_MAX_NB]
  const float* wgt;    // [K][V][STGCN_MAX_NB]
  const int* cnt;      // [K][V]
  int V, C, KC, rows;  // KC = K * C
  __device__ __forceinline__ float4 load4(int row, int k) const {
    if (row >= rows || k >= KC) return zero4();
    const int kk = k / C, ci = k - kk * C;
    const int nt = row / V, w = row - nt * V;
    const int e = kk * V + w;
    // (the lists are the caller's; a malformed one must still not leave them or the sample's V rows)
    const int n = cnt[e] < STGCN_MAX_NB ? cnt[e] : STGCN_MAX_NB;
    const float* xb = x + (size_t)nt * V * C + ci;
    float4 a = zero4();
    for (int j = 0; j < n; ++j) {
      const float g = wgt[e * STGCN_MAX_NB + j];
      int src = idx[e * STGCN_MAX_NB + j];
      src = src < 0 ? 0 : (src >= V ? V - 1 : src);
      const float4 v = ld4(xb + (size_t)src * C);
      a.x = fmaf(g, v.x, a.x); a.y = fmaf(g, v.y, a.y); a.z = fmaf(g, v.z, a.z); a.w = fmaf(g, v.w, a.w);
    }
    return a;
  }
};

// A operand of Conv2d(C, ., (9, 1), (s, 1), (4, 0)) over x [N][Tin][V][C]: logical row m = (n, t_out, v), logical k = tap C + c ->
// x[n][t_out s + tap - 4][v][c], zero outside [0, Tin).  The weights come re-laid as [C_out][9][C].
struct Tap9GatherLoader {
  static constexpr bool kColumnStaging = false;
  static constexpr bool kGather = true;
  static constexpr bool kFragments = false;
  const float* x;
  int Tin, Tout, V, C, stride, rows;
  __device__ __forceinline__ float4 load4(int row, int k) const {
    if (row >= rows || k >= STGCN_TAPS * C) return zero4();
    const int tap = k / C, c = k - tap * C;
    const int nt = row / V, v = row - nt * V;
    const int n = nt / Tout, t = nt - n * Tout;
    const int tin = t * stride + tap - STGCN_TAPS / 2;
    if (tin < 0 || tin >= Tin) return zero4();
    return ld4(x + (((size_t)n * Tin + tin) * V + v) * C + c);
  }
};

// A operand of the residual's Conv2d(C, ., 1, stride = (s, 1)): logical row m = (n, t_out, v) reads row (n, t_out s, v)
struct StrideRowLoader {
  static constexpr bool kColumnStaging = false;
  static constexpr bool kGather = true;
  static constexpr bool kFragments = false;
  const float* x;
  int Tin, Tout, V, C, stride, rows;
  __device__ __forceinline__ float4 load4(int row, int k) const {
    if (row >= rows || k >= C) return zero4();
    const int nt = row / V, v = row - nt * V;
    const int n = nt / Tout, t = nt - n * Tout;
    return ld4(x + (((size_t)n * Tin + (size_t)t * stride) * V + v) * C + k);
  }
};

// out[m][n] = act(acc * scale[n] + shift[m % period][n] + (res ? res[m][n] : 0)),  act = ReLU when `relu`.
// BatchNorm2d in eval mode and whatever bias sits in front of it, as one multiply-add: scale = gamma / sqrt(var + eps) and
// shift = (bias - mean) scale + beta, formed in fp64 and rounded once (mdm_amd/stgcn.py).  period = V for the graph convolution
// (its bias depends on the node: the table of the header comment), 1 otherwise.  res may alias out: each element is read, then
// written, by the same lane (the kernel fetches pre4 of all its rows before the first store).
struct StgcnEpilogue {
  static constexpr bool kVec4 = true;
  static constexpr bool kLn = false;
  float* out;
  const float* scale;   // [N]
  const float* shift;   // [period][ld]
  const float* res;
  int ld, period, relu;
  struct Row { size_t base; const float* sh; };
  struct Col { int n; float sc; };
  __device__ __forceinline__ Row row(int m) const { return Row{(size_t)m * ld, shift + (size_t)(m % period) * ld}; }
  __device__ __forceinline__ Col col(int n) const { return Col{n, scale[n]}; }
  __device__ __forceinline__ float pre(const Row& r, const Col& c) const { return res != nullptr ? res[r.base + c.n] : 0.f; }
  __device__ __forceinline__ float act(float v) const { return relu ? fmaxf(v, 0.f) : v; }
  __device__ __forceinline__ void store(const Row& r, const Col& c, float acc, float rv) const {
    out[r.base + c.n] = act(fmaf(acc, c.sc, r.sh[c.n]) + rv);
  }
  __device__ __forceinline__ bool vec4_ok() const { return (ld & 3) == 0; }
  __device__ __forceinline__ float4 pre4(int m, int n) const { return res != nullptr ? ld4(res + (size_t)m * ld + n) : zero4(); }
  __device__ __forceinline__ void store4(int m, int n, float4 a, float4 rv) const {
    const float4 sc = ld4(scale + n), sh = ld4(shift + (size_t)(m % period) * ld + n);
    st4(out + (size_t)m * ld + n, make_float4(act(fmaf(a.x, sc.x, sh.x) + rv.x), act(fmaf(a.y, sc.y, sh.y) + rv.y),
                                              act(fmaf(a.z, sc.z, sh.z) + rv.z), act(fmaf(a.w, sc.w, sh.w) + rv.w)));
  }
};

// x [N, V, C, T] (the reference's batch["output"]) -> out [N, T, V, Cp] with data_bn applied: out = x scale[v C + c] + shift[v C + c]
// for c < C, zero for the pad channels C .. Cp - 1 (the first block's weights carry zero columns there).
struct StgcnInputArgs {
  const float* x;
  const float* scale;   // [V C]
  const float* shift;
  float* out;
  int N, V, C, Cp, T;
};

__global__ __launch_bounds__(256) void stgcn_input_kernel(StgcnInputArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)a.N * a.T * a.V * a.Cp;
  if (i >= total) return;
  const int c = (int)(i % a.Cp);
  const size_t r = i / a.Cp;
  const int v = (int)(r % a.V);
  const size_t nt = r / a.V;
  const int t = (int)(nt % a.T);
  const size_t n = nt / a.T;
  float o = 0.f;
  if (c < a.C) o = fmaf(a.x[((n * a.V + v) * a.C + c) * a.T + t], a.scale[v * a.C + c], a.shift[v * a.C + c]);
  a.out[i] = o;
}

// One workgroup per sample: features[n][c] = mean over the sample's `rows` = T' V rows of x [N][rows][C], then
// yhat[n][j] = fcn_w[j] . features[n] + fcn_b[j].  Orders (the same for every sample, whatever N is): rows r = 0, 1, ... into the
// partial sum r % 4, then (s0 + s1) + (s2 + s3), divided by rows; the dot product likewise over c % 4.
struct StgcnTailArgs {
  const float* x;
  const float* fcn_w;   // [num_class][C]
  const float* fcn_b;
  float* features;      // [N][C]
  float* yhat;          // [N][num_class]
  int rows, C, num_class;
};

__global__ __launch_bounds__(256) void stgcn_tail_kernel(StgcnTailArgs a) {
  __shared__ float feat[STGCN_MAX_POOL_C];
  const int tid = threadIdx.x;
  const size_t n = blockIdx.x;
  const int C = a.C;
  const float inv_den = (float)a.rows;
  for (int c = 4 * tid; c < C; c += 4 * 256) {
    const float* p = a.x + n * a.rows * C + c;
    float4 s0 = zero4(), s1 = zero4(), s2 = zero4(), s3 = zero4();
    int r = 0;
    for (; r + 4 <= a.rows; r += 4) {
      s0 = add4(s0, ld4(p + (size_t)(r + 0) * C));
      s1 = add4(s1, ld4(p + (size_t)(r + 1) * C));
      s2 = add4(s2, ld4(p + (size_t)(r + 2) * C));
      s3 = add4(s3, ld4(p + (size_t)(r + 3) * C));
    }
    if (r < a.rows) s0 = add4(s0, ld4(p + (size_t)(r + 0) * C));
    if (r + 1 < a.rows) s1 = add4(s1, ld4(p + (size_t)(r + 1) * C));
    if (r + 2 < a.rows) s2 = add4(s2, ld4(p + (size_t)(r + 2) * C));
    const float4 s = add4(add4(s0, s1), add4(s2, s3));
    const float4 f = make_float4(s.x / inv_den, s.y / inv_den, s.z / inv_den, s.w / inv_den);
    st4(&feat[c], f);
    st4(a.features + n * C + c, f);
  }
  __syncthreads();
  for (int j = tid; j < a.num_class; j += 256) {
    const float* w = a.fcn_w + (size_t)j * C;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
    for (int c = 0; c < C; c += 4) {
      const float4 wv = ld4(w + c);
      d0 = fmaf(wv.x, feat[c + 0], d0);
      d1 = fmaf(wv.y, feat[c + 1], d1);
      d2 = fmaf(wv.z, feat[c + 2], d2);
      d3 = fmaf(wv.w, feat[c + 3], d3);
    }
    a.yhat[n * a.num_class + j] = ((d0 + d1) + (d2 + d3)) + a.fcn_b[j];
  }
}

}  // namespace mdm
