// The DistilBERT text encoder of the `text_encoder_type='bert'` checkpoints (model/BERT/BERT_encoder.py: HF DistilBertModel in eval
// mode, fp32): token ids -> last_hidden_state, on gfx950, in exact fp32.
//   x0 = LN(word_emb[id] + pos_emb[t]);   per layer:  q, k, v = x W^T + b (one GEMM, 1/8 folded into the q rows), heads of 64,
//   p = softmax(q k^T over keys t' < len_b),  x = LN(ctx Wo^T + bo + x),  x = LN(gelu_erf(x W1^T + b1) W2^T + b2 + x)
// The dense layers run on gemm_f32.h's exact-fp32 kernel (LinearEpilogue: bias, GELU(erf), in-place residual); this file holds what
// that kernel set lacked: attention over heads of 64 and a LayerNorm with a run-time eps (DistilBERT's 1e-12) that also gathers
// the embeddings in front of the first layer and lays the last layer's rows out token-major.
// Prompts are right-padded: row (b, t) is valid iff t < lens[b].  Every kernel here writes ZEROS to the rows behind a length and
// never reads them as keys or values, so neither what the caller left behind a prompt's end nor the padded length L reaches a valid
// row: the key tiles of a sequence are ceil(len_b / 32), whatever L is, and every sum of a row runs in an order the kernel fixes.
#pragma once
#include "common.h"

namespace mdm {

constexpr int TXT_HD = 64;               // DistilBERT's head width
constexpr int TXT_KLD = TXT_HD + 4;      // K / O staging row stride (floats): lanes r, r + 1 of a b128 read land 4 banks apart
constexpr int TXT_MAX_L = 128;           // word pieces per prompt: 4 key tiles of 32 kept in registers
constexpr int TXT_MAX_DIM = 1024;        // LayerNorm rows: at most 4 float4 per lane

inline size_t text_attn_lds_bytes(int L) { return (size_t)((L + 31) / 32) * 32 * TXT_KLD * sizeof(float); }

// One workgroup (one wave) per (sequence, head, 32-query tile); qkv [B L][3 D] with the q columns pre-scaled, ctx [B L][D].
// Computed transposed, as attention_f32.h does: St[key][query] = K . Q^T with the K rows from LDS and this wave's Q rows in
// registers, so lane (query = l & 31, half = l >> 5) holds 16 keys of every 32-key tile, the softmax is lane-local plus one
// cross-half exchange, and the probabilities feed Ot[d][query] = V^T . P^T from the registers they are in.  K, then V, then the
// output tile share the LDS buffer.  Key tiles: nkt = ceil(len / 32) of this sequence; keys len .. 32 nkt - 1 are zero-filled in
// LDS and get p = 0 exactly; the sums over keys run tile by tile, register by register, in that one order.
// CAUSAL (clip_text.h): query t sees the keys t' <= t only, so query tile qt runs the key tiles 0 .. qt and masks the diagonal one
// per element; a row's sums still run over its own key tiles in the one order, whatever the tiles behind them hold.
template <bool CAUSAL>
__global__ __launch_bounds__(64) void text_attn_kernel(const float* __restrict__ qkv, const int* __restrict__ lens,
                                                       float* __restrict__ ctx, int L, int D, int H) {
  MDM_DYN_SMEM(float, smem);             // ceil(L / 32) * 32 rows x TXT_KLD floats
  const int lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const int nqt = (L + 31) / 32;
  const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt;
  const int b = bh / H, head = bh - b * H;
  int len = lens[b];
  len = len < 0 ? 0 : (len > L ? L : len);
  const int q0 = 32 * qt;
  const int nq = min(32, L - q0);        // rows of this tile inside the padded length
  const size_t ld = 3 * (size_t)D;
  const float* base = qkv + (size_t)b * L * ld + head * TXT_HD;
  float* obase = ctx + ((size_t)b * L + q0) * D + head * TXT_HD;

  if (q0 >= len) {                       // a tile of padding only
    for (int idx = lane; idx < nq * 16; idx += 64) st4(obase + (size_t)(idx >> 4) * D + 4 * (idx & 15), zero4());
    return;
  }
  const int nkt = CAUSAL ? qt + 1 : (len + 31) / 32;      // (q0 < len here, so tile qt holds keys)

  // ---- Q fragment: query row q0 + r, this lane-half's 32 d's
  float qf[32];
  {
    const float* qp = base + (size_t)(q0 + r) * ld + 32 * h;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float4 v = (q0 + r < len) ? ld4(qp + 4 * j) : zero4();
      qf[4 * j + 0] = v.x; qf[4 * j + 1] = v.y; qf[4 * j + 2] = v.z; qf[4 * j + 3] = v.w;
    }
  }
  // ---- stage K (rows >= len zero-filled)
  for (int idx = lane; idx < nkt * 32 * 16; idx += 64) {
    const int key = idx >> 4, c4 = idx & 15;
    const float4 v = (key < len) ? ld4(base + D + (size_t)key * ld + 4 * c4) : zero4();
    st4(&smem[key * TXT_KLD + 4 * c4], v);
  }
  __syncthreads();

  // ---- phase 1: St tiles
  f32x16 p[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) p[kt][e] = 0.f;
    if (kt < nkt) {
      const float* kp = &smem[(kt * 32 + r) * TXT_KLD + 32 * h];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float4 kf = ld4(kp + 4 * c);
        p[kt] = mfma_f32(kf.x, qf[4 * c + 0], p[kt]);
        p[kt] = mfma_f32(kf.y, qf[4 * c + 1], p[kt]);
        p[kt] = mfma_f32(kf.z, qf[4 * c + 2], p[kt]);
        p[kt] = mfma_f32(kf.w, qf[4 * c + 3], p[kt]);
      }
    }
  }

  // ---- softmax over the keys below len (key 0 is always one of them)
  float mx = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = kt * 32 + mfma_row(e, h);
      const float s = (key < len && (!CAUSAL || key <= q0 + r)) ? p[kt][e] : -INFINITY;
      p[kt][e] = s;
      mx = fmaxf(mx, s);
    }
  mx = fmaxf(mx, shfl_xor_f32(mx, 32));
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
    if (kt < nkt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float pe = expf(p[kt][e] - mx);   // exp(-inf) = 0 for the keys behind len
        p[kt][e] = pe;
        sum += pe;
      }
    }
  sum += shfl_xor_f32(sum, 32);
  const float inv = 1.0f / sum;

  __syncthreads();                       // K has been read
  // ---- stage V into the same buffer, row stride TXT_HD
  for (int idx = lane; idx < nkt * 32 * 16; idx += 64) {
    const int key = idx >> 4, c4 = idx & 15;
    const float4 v = (key < len) ? ld4(base + 2 * D + (size_t)key * ld + 4 * c4) : zero4();
    st4(&smem[key * TXT_HD + 4 * c4], v);
  }
  __syncthreads();

  // ---- phase 2: Ot[d][query]
  f32x16 o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
    if (kt < nkt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float* vp = &smem[(kt * 32 + mfma_row(e, h)) * TXT_HD + r];
        const float pv = p[kt][e] * inv;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) o[dt] = mfma_f32(vp[32 * dt], pv, o[dt]);
      }
    }
  __syncthreads();                       // V has been read

  // ---- stage O[q][d] and store 16 bytes per lane; rows behind len are written as zeros
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)          // registers 4g .. 4g + 3 of half h are 4 consecutive d's
      st4(&smem[r * TXT_KLD + dt * 32 + 8 * g + 4 * h], make_float4(o[dt][4 * g + 0], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]));
  __syncthreads();
  for (int idx = lane; idx < nq * 16; idx += 64) {
    const int qq = idx >> 4, c4 = idx & 15;
    const float4 v = (q0 + qq < len) ? ld4(&smem[qq * TXT_KLD + 4 * c4]) : zero4();
    st4(obase + (size_t)qq * D + 4 * c4, v);
  }
}

// LayerNorm with a run-time eps over rows of D floats (D % 4 == 0, D <= TXT_MAX_DIM), one wave per row, two-pass statistics in
// registers with a fixed reduction order.  Row (b, t) of [B L]:
//   ids != null: the row is word_emb[ids[b, t]] + pos_emb[t] (the embedding layer), else row (b, t) of `in` (which may be `out`);
//   t >= lens[b]: zeros are written and nothing is read;
//   token_major: the row goes to out[t][b] instead of out[b][t].
struct TextLnArgs {
  const float* in;
  const int* ids;
  const float* word_emb;
  const float* pos_emb;
  const float* gamma;
  const float* beta;
  const int* lens;
  float* out;
  int B, L, D, vocab;
  float eps;
  int token_major;
};

__global__ __launch_bounds__(256) void text_ln_kernel(TextLnArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.B * a.L) return;          // (row is wave-uniform)
  const int b = row / a.L, t = row - b * a.L;
  const int D = a.D;
  float* o = a.out + (size_t)(a.token_major ? t * a.B + b : row) * D;
  if (t >= a.lens[b]) {
    for (int c = 4 * lane; c < D; c += 256) st4(o + c, zero4());
    return;
  }
  int id = 0;
  if (a.ids != nullptr) {                // (ids < vocab is the caller's duty; an id outside the table must still not leave it)
    id = a.ids[row];
    id = id < 0 ? 0 : (id >= a.vocab ? a.vocab - 1 : id);
  }
  const float* x0 = a.ids != nullptr ? a.word_emb + (size_t)id * D : a.in + (size_t)row * D;
  const float* x1 = a.ids != nullptr ? a.pos_emb + (size_t)t * D : nullptr;
  float4 v[4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 256 * i + 4 * lane;
    v[i] = zero4();
    if (c < D) {
      v[i] = ld4(x0 + c);
      if (x1 != nullptr) v[i] = add4(v[i], ld4(x1 + c));
    }
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += shfl_xor_f32(s, m);
  const float mean = s / (float)D;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (256 * i + 4 * lane < D) {
      v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
      ss += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) ss += shfl_xor_f32(ss, m);
  const float rstd = 1.0f / sqrtf(ss / (float)D + a.eps);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 256 * i + 4 * lane;
    if (c < D) {
      const float4 g = ld4(a.gamma + c), be = ld4(a.beta + c);
      st4(o + c, make_float4(v[i].x * rstd * g.x + be.x, v[i].y * rstd * g.y + be.y, v[i].z * rstd * g.z + be.z,
                             v[i].w * rstd * g.w + be.w));
    }
  }
}

}  // namespace mdm
