// The text tower of OpenAI CLIP (clip/model.py CLIP.encode_text; ViT-B/32 for the `text_encoder_type='clip'` checkpoints): token ids
// -> text_embed, on gfx950, in exact fp32.
//   x = token_embedding[id] + positional_embedding[t];   per layer (pre-LN, eps 1e-5):
//   x += out_proj(attn(ln_1(x)))  causal, heads of 64, 1/8 folded into the q rows;   x += c_proj(quick_gelu(c_fc(ln_2(x))))
//   e[b] = ln_final(x[b, len_b - 1]) @ text_projection,   len_b - 1 = argmax(ids[b]) = the prompt's EOT
// The dense layers run on gemm_f32.h's exact-fp32 kernel (LinearEpilogue with ACT_QGELU), the attention on text_encoder.h's
// text_attn_kernel<CAUSAL = true>, ln_1 / ln_2 on its text_ln_kernel (in != out: x stays the residual).  This file holds the two
// ends: the embedding without a LayerNorm behind it, and the gather of the EOT rows with ln_final.
// Causality makes everything behind a prompt's EOT dead: a row t >= len_b cannot reach row len_b - 1.  The embedding, attention and
// LayerNorm kernels write zeros there and read none of it, the residual rows there collect the biases of the dense layers and
// nothing reads them, and the padded length L reaches no valid row.
#pragma once
#include "text_encoder.h"

namespace mdm {

constexpr float CLIP_LN_EPS = 1e-5f;     // nn.LayerNorm's default, which clip/model.py keeps

// x[b, t] = tok_emb[ids[b, t]] + pos_emb[t], rows of D floats (D % 4 == 0), 16 bytes per lane; zeros for t >= lens[b], where the id
// is not read.  (ids < vocab is the caller's duty; an id outside the table must still not leave it.)
__global__ __launch_bounds__(256) void clip_embed_kernel(const int* __restrict__ ids, const int* __restrict__ lens,
                                                         const float* __restrict__ tok_emb, const float* __restrict__ pos_emb,
                                                         float* __restrict__ x, int B, int L, int D, int vocab) {
  const int c4 = D >> 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * L * c4) return;
  const int row = idx / c4, c = 4 * (idx - row * c4);
  const int b = row / L, t = row - b * L;
  float4 v = zero4();
  if (t < lens[b]) {
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    v = add4(ld4(tok_emb + (size_t)id * D + c), ld4(pos_emb + (size_t)t * D + c));
  }
  st4(x + (size_t)row * D + c, v);
}

// One wave per prompt: out[b] = LN(x[b, len_b - 1]), [B][D]  (ln_final over the EOT rows only; len_b clamped into [1, L]).  The
// row's arithmetic is text_ln_kernel's: two-pass statistics in registers, D <= TXT_MAX_DIM, fixed reduction order.
__global__ __launch_bounds__(256) void clip_eot_ln_kernel(const float* __restrict__ x, const int* __restrict__ lens,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ out, int B, int L, int D) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;                    // (b is wave-uniform)
  int len = lens[b];
  len = len < 1 ? 1 : (len > L ? L : len);
  const float* xr = x + ((size_t)b * L + len - 1) * D;
  float* o = out + (size_t)b * D;
  float4 v[4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 256 * i + 4 * lane;
    v[i] = c < D ? ld4(xr + c) : zero4();
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
  const float rstd = 1.0f / sqrtf(ss / (float)D + CLIP_LN_EPS);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 256 * i + 4 * lane;
    if (c < D) {
      const float4 g = ld4(gamma + c), be = ld4(beta + c);
      st4(o + c, make_float4(v[i].x * rstd * g.x + be.x, v[i].y * rstd * g.y + be.y, v[i].z * rstd * g.z + be.z,
                             v[i].w * rstd * g.w + be.w));
    }
  }
}

}  // namespace mdm
