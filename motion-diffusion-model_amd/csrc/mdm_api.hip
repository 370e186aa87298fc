// libmdm_hip.so -- host orchestration + C ABI (include/mdm_hip.h) for the MDM sampling hot path.
// Native counterpart of: MDM.forward (model/mdm.py:189-283), ClassifierFreeSampleModel.forward
// (utils/sampler_util.py:27-34), GaussianDiffusion.p_sample_loop / ddim_sample_loop
// (diffusion/gaussian_diffusion.py:591-727, :876-990).  No torch, no allocation: caller-owned pointers.
#include "../../include/mdm_hip.h"
#ifdef MDM_PROBES
#include "../../include/mdm_hip_probe.h"
#endif

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "attention_x3.h"
#include "attention_long.h"
#include "attention_f32.h"
#include "common.h"
#include "elementwise.h"
#include "gemm_f32.h"
#include "gemm_x3.h"
#include "gemm_x3s.h"
#include "xattn_block.h"
#include "selfattn_block.h"
#ifdef MDM_PROBES   // the rejected fp16 + MX-FP6 GEMM arithmetic of round 1: an experiment of the probe library, kept under lab/
#include "../../lab/csrc_probe/gemm_f16f6.h"
#endif
#include "motion_recover.h"
#include "smpl_joints.h"
#include "smpl_mesh.h"
#include "evaluator.h"
#include "text_encoder.h"
#include "clip_text.h"
#include "stgcn.h"
#include "gru_recogniser.h"

using namespace mdm;

#include "api_runtime.h"
#include "api_launch.h"
#include "encoder.h"

extern "C" {

int mdm_abi_version(void) { return MDM_ABI_VERSION; }

// How this binary was built (include/mdm_hip.h): the loaders refuse a product library whose string lacks "slp=off".
const char* mdm_build_info(void) {
  return "slp="
#ifdef MDM_NO_SLP
         "off"
#else
         "on"
#endif
         ";probes="
#ifdef MDM_PROBES
         "1"
#else
         "0"
#endif
         ";emu="
#ifdef MDM_EMU
         "1"
#else
         "0"
#endif
         ";planes=f16";
}
const char* mdm_last_error(void) { return g_err.c_str(); }

int mdm_create(const mdm_config_t* cfg, mdm_model_t** out) {
  if (cfg == nullptr || out == nullptr) return fail(MDM_EINVAL, "mdm_create: null argument");
  const int D = cfg->latent_dim, H = cfg->num_heads;
  if (D <= 0 || D % 256 != 0 || D > 1024) return fail(MDM_EUNSUPPORTED, "latent_dim must be 256, 512, 768 or 1024");
  if (H <= 0 || D != H * ATT_HD) return fail(MDM_EUNSUPPORTED, "latent_dim / num_heads must be 128");
  if (cfg->ff_size <= 0 || cfg->ff_size % 32) return fail(MDM_EUNSUPPORTED, "ff_size must be a positive multiple of 32");
  if (cfg->clip_dim <= 0 || cfg->clip_dim % 4) return fail(MDM_EUNSUPPORTED, "clip_dim must be a positive multiple of 4");
  if (cfg->njoints <= 0 || cfg->nfeats <= 0 || cfg->num_layers <= 0 || cfg->max_len < 2)
    return fail(MDM_EINVAL, "mdm_create: non-positive dimension");
  if (cfg->arch != MDM_ARCH_TRANS_ENC && cfg->arch != MDM_ARCH_TRANS_DEC) return fail(MDM_EUNSUPPORTED, "arch must be trans_enc or trans_dec");
  if (cfg->context_len < 0 || (cfg->arch == MDM_ARCH_TRANS_ENC && cfg->context_len != 0))
    return fail(MDM_EUNSUPPORTED, "context_len (prefix completion) belongs to the trans_dec (DiP) configuration");
  mdm_model* m = new (std::nothrow) mdm_model();
  if (m == nullptr) return fail(MDM_EINVAL, "out of host memory");
  m->cfg = *cfg;
  m->jf = cfg->njoints * cfg->nfeats;
  m->jf_pad = (m->jf + 3) / 4 * 4;
  m->jf_out = m->jf_pad;
  m->jf_k = (m->jf + 31) / 32 * 32;
  const int64_t d = D, ff = cfg->ff_size, jf = m->jf;
  auto& e = m->expect;
  e["input_process.poseEmbedding.weight"] = d * jf;
  e["input_process.poseEmbedding.bias"] = d;
  for (int l = 0; l < cfg->num_layers; ++l) {
    const std::string p = (cfg->arch == MDM_ARCH_TRANS_DEC ? "seqTransDecoder.layers." : "seqTransEncoder.layers.") +
                          std::to_string(l) + ".";
    if (cfg->arch == MDM_ARCH_TRANS_DEC) {   // nn.TransformerDecoderLayer: + cross-attention over the memory, + norm3
      e[p + "multihead_attn.in_proj_weight"] = 3 * d * d;
      e[p + "multihead_attn.in_proj_bias"] = 3 * d;
      e[p + "multihead_attn.out_proj.weight"] = d * d;
      e[p + "multihead_attn.out_proj.bias"] = d;
      e[p + "norm3.weight"] = d;
      e[p + "norm3.bias"] = d;
    }
    e[p + "self_attn.in_proj_weight"] = 3 * d * d;
    e[p + "self_attn.in_proj_bias"] = 3 * d;
    e[p + "self_attn.out_proj.weight"] = d * d;
    e[p + "self_attn.out_proj.bias"] = d;
    e[p + "linear1.weight"] = ff * d;
    e[p + "linear1.bias"] = ff;
    e[p + "linear2.weight"] = d * ff;
    e[p + "linear2.bias"] = d;
    e[p + "norm1.weight"] = d;
    e[p + "norm1.bias"] = d;
    e[p + "norm2.weight"] = d;
    e[p + "norm2.bias"] = d;
  }
  e["embed_timestep.time_embed.0.weight"] = d * d;
  e["embed_timestep.time_embed.0.bias"] = d;
  e["embed_timestep.time_embed.2.weight"] = d * d;
  e["embed_timestep.time_embed.2.bias"] = d;
  e["embed_text.weight"] = d * cfg->clip_dim;
  e["embed_text.bias"] = d;
  e["output_process.poseFinal.weight"] = jf * d;
  e["output_process.poseFinal.bias"] = jf;
  e["sequence_pos_encoder.pe"] = (int64_t)cfg->max_len * d;
  *out = m;
  return MDM_OK;
}

void mdm_destroy(mdm_model_t* m) { delete m; }

// Run-time options of a handle (include/mdm_hip.h, ABI 9).  The library reads NO environment variable (rounds 3-4 did, on the
// launch path); a value takes effect with the next call -- every call resolves its kernel route once, from the handle.
int mdm_set_option(mdm_model_t* m, int32_t key, int32_t value) {
  if (m == nullptr) return fail(MDM_EINVAL, "mdm_set_option: null model");
  switch (key) {
    case MDM_OPT_SMALL_GEMM_MAX_SEQS:
      if (value < 0) return fail(MDM_EINVAL, "mdm_set_option: MDM_OPT_SMALL_GEMM_MAX_SEQS must be >= 0");
      m->x3s.max_seqs = value;
      return MDM_OK;
    case MDM_OPT_SMALL_GEMM_ROW_TILES:
      if (value < 0 || value > 2) return fail(MDM_EINVAL, "mdm_set_option: MDM_OPT_SMALL_GEMM_ROW_TILES must be 0 (by size), 1 or 2");
      m->x3s.row_tiles = value;
      return MDM_OK;
    case MDM_OPT_DEC_FUSED_XATTN:
      if (value < 0 || value > 3) return fail(MDM_EINVAL, "mdm_set_option: MDM_OPT_DEC_FUSED_XATTN must be 0, 1, 2 or 3");
      m->fused_xattn = value;
      return MDM_OK;
    case MDM_OPT_DEC_FUSED_SELFATTN:
      if (value != 0 && value != 1) return fail(MDM_EINVAL, "mdm_set_option: MDM_OPT_DEC_FUSED_SELFATTN must be 0 or 1");
      m->fused_selfattn = value != 0;
      return MDM_OK;
    case MDM_OPT_ATTN_DIRECT_OUT:
      if (value != 0 && value != 1) return fail(MDM_EINVAL, "mdm_set_option: MDM_OPT_ATTN_DIRECT_OUT must be 0 or 1");
      m->attn_direct = value != 0;
      return MDM_OK;
    case MDM_OPT_ATTN_WIDE:
      if (value != 0 && value != 1) return fail(MDM_EINVAL, "mdm_set_option: MDM_OPT_ATTN_WIDE must be 0 or 1");
      m->attn_wide = value != 0;
      return MDM_OK;
    case MDM_OPT_DEC_TIME_TOKEN:
      if (value != 0 && value != 1) return fail(MDM_EINVAL, "mdm_set_option: MDM_OPT_DEC_TIME_TOKEN must be 0 or 1");
      if (value == 1 && (m->cfg.arch != MDM_ARCH_TRANS_DEC || m->cfg.context_len != 1))
        return fail(MDM_EINVAL, "mdm_set_option: MDM_OPT_DEC_TIME_TOKEN needs a trans_dec model created with context_len = 1 (the class-token row)");
      m->dec_time_token = value != 0;
      return MDM_OK;
    case MDM_OPT_ENC_SHARED_LAYER0:
      if (value != 0 && value != 1) return fail(MDM_EINVAL, "mdm_set_option: MDM_OPT_ENC_SHARED_LAYER0 must be 0 or 1");
      m->enc_shared_l0 = value != 0;
      return MDM_OK;
    default:
      return fail(MDM_EINVAL, "mdm_set_option: unknown key " + std::to_string(key));
  }
}

// ABI 10: y['target_cond'] (model/mdm.py:197-199).  One-shot, caller-owned; see include/mdm_hip.h.
int mdm_set_time_add(mdm_model_t* m, const float* add_dev, int32_t B) {
  if (m == nullptr) return fail(MDM_EINVAL, "mdm_set_time_add: null model");
  if (add_dev != nullptr && B <= 0) return fail(MDM_EINVAL, "mdm_set_time_add: B must be >= 1");
  m->time_add_next = add_dev;
  m->time_add_B = add_dev != nullptr ? B : 0;
  return MDM_OK;
}

int mdm_get_option(const mdm_model_t* m, int32_t key, int32_t* value) {
  if (m == nullptr || value == nullptr) return fail(MDM_EINVAL, "mdm_get_option: null argument");
  switch (key) {
    case MDM_OPT_SMALL_GEMM_MAX_SEQS: *value = m->x3s.max_seqs; return MDM_OK;
    case MDM_OPT_SMALL_GEMM_ROW_TILES: *value = m->x3s.row_tiles; return MDM_OK;
    case MDM_OPT_DEC_FUSED_XATTN: *value = m->fused_xattn; return MDM_OK;
    case MDM_OPT_DEC_FUSED_SELFATTN: *value = m->fused_selfattn ? 1 : 0; return MDM_OK;
    case MDM_OPT_ATTN_DIRECT_OUT: *value = m->attn_direct ? 1 : 0; return MDM_OK;
    case MDM_OPT_ATTN_WIDE: *value = m->attn_wide ? 1 : 0; return MDM_OK;
    case MDM_OPT_DEC_TIME_TOKEN: *value = m->dec_time_token ? 1 : 0; return MDM_OK;
    case MDM_OPT_ENC_SHARED_LAYER0: *value = m->enc_shared_l0 ? 1 : 0; return MDM_OK;
    default: return fail(MDM_EINVAL, "mdm_get_option: unknown key " + std::to_string(key));
  }
}

int mdm_set_weight(mdm_model_t* m, const char* name, const float* dev_ptr, int64_t numel) {
  if (m == nullptr || name == nullptr || dev_ptr == nullptr) return fail(MDM_EINVAL, "mdm_set_weight: null argument");
  auto it = m->expect.find(name);
  if (it == m->expect.end()) return fail(MDM_EINVAL, std::string("unexpected state-dict key: ") + name);
  if (it->second != numel)
    return fail(MDM_EINVAL, std::string("size mismatch for ") + name + ": expected " + std::to_string(it->second) +
                                " elements, got " + std::to_string(numel));
  if ((reinterpret_cast<uintptr_t>(dev_ptr) & 15) != 0) return fail(MDM_EINVAL, std::string(name) + ": pointer must be 16-byte aligned");
  m->w[name] = dev_ptr;
  m->prepared = false;
  return MDM_OK;
}

size_t mdm_const_bytes(const mdm_model_t* m) {
  if (m == nullptr) return 0;
  const size_t D = m->cfg.latent_dim;
  const size_t FF = m->cfg.ff_size;
  if (m->cfg.arch == MDM_ARCH_TRANS_DEC) {
    // padded poseEmbedding, time table + its MLP scratch; per layer the gamma-folded in_proj / q / linear1 (fp32 + 2 vectors
    // each) and the fragment-ordered planes of in_proj, out_proj, q, cross out_proj, linear1, linear2 (4 bytes per weight)
    const size_t fold = align_up(3 * D * D * 4, 256) + align_up(D * D * 4, 256) + align_up(FF * D * 4, 256) +
                        2 * (align_up(3 * D * 4, 256) + align_up(D * 4, 256) + align_up(FF * 4, 256));
    const size_t planes = align_up(3 * D * D * 4, 256) + 3 * align_up(D * D * 4, 256) + 2 * align_up(FF * D * 4, 256);
    // OutputProcess with the last norm3 folded in (the plane path of decoder_pass): fp32 copy, 2 vectors, planes
    const size_t outp = align_up((size_t)m->jf * D * 4, 256) + 2 * align_up((size_t)32 * ((m->jf_out + 31) / 32) * 4, 256) +
                        align_up(x3_packed_weight_elems(m->jf, (int)D) * 4, 256);
    const size_t kv_all = align_up((size_t)m->cfg.num_layers * 2 * D * D * 4, 256) + align_up((size_t)m->cfg.num_layers * 2 * D * 4, 256);
    return 256 /* range flag */ + align_up(D * m->jf_pad * sizeof(float), 256) +
           2 * align_up((size_t)m->cfg.max_len * D * sizeof(float), 256) + (size_t)m->cfg.num_layers * (fold + planes) + outp + kv_all;
  }
  const size_t per_layer = align_up(3 * D * D * 4, 256) + align_up(D * D * 4, 256) + 2 * align_up(FF * D * 4, 256);
  return 256 /* range flag */ + align_up(D * m->jf_pad * sizeof(float), 256) +
         2 * align_up((size_t)m->cfg.max_len * D * sizeof(float), 256) + (size_t)m->cfg.num_layers * per_layer + align_up(x3_packed_weight_elems(m->jf, (int)D) * 4, 256) +
         align_up((size_t)m->jf_out * sizeof(float), 256) +
         // folded-LayerNorm constants: per layer gamma-scaled in_proj / linear1 planes + 2 vectors each; OutputProcess;
         // one fp32 scratch matrix for the scaled weights before they are packed
         (size_t)m->cfg.num_layers * (align_up(3 * D * D * 4, 256) + align_up(FF * D * 4, 256) +
                                      2 * align_up(3 * D * 4, 256) + 2 * align_up(FF * 4, 256)) +
         align_up(x3_packed_weight_elems(m->jf, (int)D) * 4, 256) + 2 * align_up((size_t)32 * ((m->jf_out + 31) / 32) * 4, 256) +
         align_up(std::max<size_t>(3 * D, FF) * D * 4, 256) + align_up((size_t)D * m->jf_k * 4, 256);
}

int mdm_prepare(mdm_model_t* m, void* const_ws, size_t const_ws_bytes, void* stream) {
  ChainGuard chain_guard(stream);
  if (m == nullptr || const_ws == nullptr) return fail(MDM_EINVAL, "mdm_prepare: null argument");
  for (const auto& kv : m->expect)
    if (m->w.find(kv.first) == m->w.end()) return fail(MDM_ESTATE, "missing weight: " + kv.first);
  if (const_ws_bytes < mdm_const_bytes(m)) return fail(MDM_ENOSPC, "mdm_prepare: const workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int D = m->cfg.latent_dim, R = m->cfg.max_len;
  char* base = static_cast<char*>(const_ws);
  // word 0: "a weight left the range of the 16-bit operand planes" (set by the pack kernels below; mdm_weights_in_range)
  m->range_flag = reinterpret_cast<int*>(base);
  base += 256;
#ifdef MDM_EMU
  *m->range_flag = 0;
#else
  if (hipMemsetAsync(m->range_flag, 0, 4, s) != hipSuccess) return fail(MDM_EHIP, "mdm_prepare: hipMemsetAsync failed");
#endif
  m->w_in_pad = reinterpret_cast<float*>(base);
  base += align_up((size_t)D * m->jf_pad * sizeof(float), 256);
  m->time_table = reinterpret_cast<float*>(base);
  base += align_up((size_t)R * D * sizeof(float), 256);
  float* hidden = reinterpret_cast<float*>(base);
  MDM_LAUNCH(pad_rows_kernel, dim3(256), dim3(256), 0, s, m->w_in_pad, m->W("input_process.poseEmbedding.weight"), D,
             m->jf, m->jf_pad);
  if (int rc = rt_launch_status()) return rc;
  // TimestepEmbedder for every possible t (model/mdm.py:323-330): table[t] = W2 silu(W0 pe[t] + b0) + b2
  if (int rc = launch_linear(nullptr, m->W("sequence_pos_encoder.pe"), D, m->W("embed_timestep.time_embed.0.weight"),
                             m->W("embed_timestep.time_embed.0.bias"), nullptr, hidden, R, D, D, ACT_SILU, 0, 1.f, s))
    return rc;
  if (int rc = launch_linear(nullptr, hidden, D, m->W("embed_timestep.time_embed.2.weight"),
                             m->W("embed_timestep.time_embed.2.bias"), nullptr, m->time_table, R, D, D, ACT_NONE, 0,
                             1.f, s))
    return rc;
  if (m->cfg.arch == MDM_ARCH_TRANS_DEC) {   // the DiP decoder: gamma-folded fp32 copies (fp32 skeleton) AND fragment-ordered planes of
                                             // every layer weight (the operand-plane route of the default f16x3 mode)
    // LayerNorm folded into the consumers of its output (gemm_f32.h LnFold)
    base += align_up((size_t)R * D * sizeof(float), 256);
    const int L = m->cfg.num_layers, FFd = m->cfg.ff_size;
    auto take = [&](size_t n) { float* p = reinterpret_cast<float*>(base); base += align_up(n * 4, 256); return p; };
    auto fold_one = [&](const float* w, const float* bias, const float* gamma, const float* beta, int N, float*& wf, float*& cvec,
                        float*& bvec) -> int {
      wf = take((size_t)N * D);
      cvec = take(N);
      bvec = take(N);
      MDM_LAUNCH(fold_layernorm_kernel, dim3((N + 3) / 4), dim3(256), 0, s, w, gamma, beta, bias, wf, cvec, bvec, N, D, N);
      return rt_launch_status();
    };
    m->dec_fold.assign(L, mdm_model::DecFold{});
    for (int l = 0; l < L; ++l) {
      mdm_model::DecFold& F = m->dec_fold[l];
      if (l >= 1)
        if (int rc = fold_one(m->L(l, "self_attn.in_proj_weight"), m->L(l, "self_attn.in_proj_bias"), m->L(l - 1, "norm3.weight"),
                              m->L(l - 1, "norm3.bias"), 3 * D, F.w_in, F.c_in, F.b_in)) return rc;
      if (int rc = fold_one(m->L(l, "multihead_attn.in_proj_weight"), m->L(l, "multihead_attn.in_proj_bias"), m->L(l, "norm1.weight"),
                            m->L(l, "norm1.bias"), D, F.w_q, F.c_q, F.b_q)) return rc;
      if (int rc = fold_one(m->L(l, "linear1.weight"), m->L(l, "linear1.bias"), m->L(l, "norm2.weight"), m->L(l, "norm2.bias"),
                            FFd, F.w_1, F.c_1, F.b_1)) return rc;
    }
    auto make_planes = [&](const float* src, int N, int K, X3Weights& op) -> int {
      const size_t n = x3_packed_weight_elems(N, K);
      p16_t* hi = reinterpret_cast<p16_t*>(base);
      base += align_up(n * 4, 256);
      op = X3Weights{hi, hi + n};
      return launch_pack_weights(src, hi, hi + n, N, K, s, m->range_flag);
    };
    m->dec_planes.assign(L, mdm_model::DecPlanes{});
    for (int l = 0; l < L; ++l) {
      const mdm_model::DecFold& F = m->dec_fold[l];
      mdm_model::DecPlanes& P = m->dec_planes[l];
      if (int rc = make_planes(l >= 1 ? F.w_in : m->L(l, "self_attn.in_proj_weight"), 3 * D, D, P.in_proj)) return rc;
      if (int rc = make_planes(m->L(l, "self_attn.out_proj.weight"), D, D, P.out_proj)) return rc;
      if (int rc = make_planes(F.w_q, D, D, P.q)) return rc;
      if (int rc = make_planes(m->L(l, "multihead_attn.out_proj.weight"), D, D, P.out_proj2)) return rc;
      if (int rc = make_planes(F.w_1, FFd, D, P.linear1)) return rc;
      if (int rc = make_planes(m->L(l, "linear2.weight"), D, FFd, P.linear2)) return rc;
    }
    {  // OutputProcess <- norm3(L-1) (decoder_pass on operand planes: no LayerNorm kernel in front of poseFinal)
      const int jf32 = (m->jf_out + 31) / 32 * 32;
      float* wf = take((size_t)m->jf * D);
      m->c_out = take(jf32);
      m->b_out = take(jf32);
      MDM_LAUNCH(fold_layernorm_kernel, dim3((jf32 + 3) / 4), dim3(256), 0, s, m->W("output_process.poseFinal.weight"),
                 m->L(L - 1, "norm3.weight"), m->L(L - 1, "norm3.bias"), m->W("output_process.poseFinal.bias"), wf, m->c_out,
                 m->b_out, m->jf, D, jf32);
      if (int rc = rt_launch_status()) return rc;
      if (int rc = make_planes(wf, m->jf, D, m->out_planes_f)) return rc;
    }
    // the cross-attention key | value projections of all layers as one [L * 2D][D] matrix (mdm_sample_loop_dec's hoisted projections)
    m->wkv_all = take((size_t)L * 2 * D * D);
    m->bkv_all = take((size_t)L * 2 * D);
    for (int l = 0; l < L; ++l) {
      if (int rc = rt_copy(m->wkv_all + (size_t)l * 2 * D * D, m->L(l, "multihead_attn.in_proj_weight") + (size_t)D * D,
                           (size_t)2 * D * D * sizeof(float), s)) return rc;
      if (int rc = rt_copy(m->bkv_all + (size_t)l * 2 * D, m->L(l, "multihead_attn.in_proj_bias") + D, (size_t)2 * D * sizeof(float), s)) return rc;
    }
    if ((size_t)(base - static_cast<char*>(const_ws)) > const_ws_bytes) return fail(MDM_ENOSPC, "mdm_prepare: const workspace too small");
    m->prepared = true;
    return MDM_OK;
  }
  // hi/lo planes of the encoder weights (always built: the precision mode can be switched afterwards)
  base += align_up((size_t)R * D * sizeof(float), 256);
  const size_t FF = m->cfg.ff_size;
  m->planes.assign(m->cfg.num_layers, mdm_model::LayerPlanes{});
  auto make_planes = [&](const float* src, int N, int K, X3Weights& op) -> int {
    const size_t n = x3_packed_weight_elems(N, K);
    p16_t* hi = reinterpret_cast<p16_t*>(base);
    p16_t* lo = hi + n;
    base += align_up(n * 4, 256);
    op = X3Weights{hi, lo};
    return launch_pack_weights(src, hi, lo, N, K, s, m->range_flag);
  };
  for (int l = 0; l < m->cfg.num_layers; ++l) {
    if (int rc = make_planes(m->L(l, "self_attn.in_proj_weight"), 3 * D, D, m->planes[l].in_proj)) return rc;
    if (int rc = make_planes(m->L(l, "self_attn.out_proj.weight"), D, D, m->planes[l].out_proj)) return rc;
    if (int rc = make_planes(m->L(l, "linear1.weight"), (int)FF, D, m->planes[l].linear1)) return rc;
    if (int rc = make_planes(m->L(l, "linear2.weight"), D, (int)FF, m->planes[l].linear2)) return rc;
  }
  // OutputProcess in split precision: weight rows / bias padded to jf_out (the pad rows are zero)
  if (int rc = make_planes(m->W("output_process.poseFinal.weight"), m->jf, D, m->out_planes)) return rc;
  m->out_bias_pad = reinterpret_cast<float*>(base);
  base += align_up((size_t)m->jf_out * sizeof(float), 256);
  MDM_LAUNCH(pad_rows_kernel, dim3(1), dim3(256), 0, s, m->out_bias_pad, m->W("output_process.poseFinal.bias"), 1, m->jf,
             m->jf_out);
  if (int rc = rt_launch_status()) return rc;
  // ---- LayerNorm folded into its consumers: in_proj(l >= 1) <- norm2(l-1), linear1(l) <- norm1(l), OutputProcess <- norm2(L-1)
  {
    const int L = m->cfg.num_layers;
    float* scratch_w = reinterpret_cast<float*>(base);
    base += align_up(std::max<size_t>(3 * (size_t)D, FF) * D * 4, 256);
    auto take_vec = [&](size_t n) { float* p = reinterpret_cast<float*>(base); base += align_up(n * 4, 256); return p; };
    auto fold_one = [&](const float* w, const float* bias, const float* gamma, const float* beta, int N, int Npad,
                        X3Weights& op, float*& cvec, float*& bvec) -> int {
      cvec = take_vec(Npad);
      bvec = take_vec(Npad);
      MDM_LAUNCH(fold_layernorm_kernel, dim3((Npad + 3) / 4), dim3(256), 0, s, w, gamma, beta, bias, scratch_w, cvec, bvec,
                 N, D, Npad);
      if (int rc = rt_launch_status()) return rc;
      return make_planes(scratch_w, N, D, op);   // stream order: the pack kernel reads scratch_w after the fold kernel
    };
    m->fold.assign(L, mdm_model::LayerFold{});
    for (int l = 0; l < L; ++l) {
      mdm_model::LayerFold& F = m->fold[l];
      if (l >= 1) {
        if (int rc = fold_one(m->L(l, "self_attn.in_proj_weight"), m->L(l, "self_attn.in_proj_bias"),
                              m->L(l - 1, "norm2.weight"), m->L(l - 1, "norm2.bias"), 3 * D, 3 * D, F.in_proj, F.c_qkv, F.b_qkv)) return rc;
      }
      if (int rc = fold_one(m->L(l, "linear1.weight"), m->L(l, "linear1.bias"), m->L(l, "norm1.weight"),
                            m->L(l, "norm1.bias"), (int)FF, (int)FF, F.linear1, F.c_1, F.b_1)) return rc;
    }
    const int jf32 = (m->jf_out + 31) / 32 * 32;
    if (int rc = fold_one(m->W("output_process.poseFinal.weight"), m->W("output_process.poseFinal.bias"),
                          m->L(L - 1, "norm2.weight"), m->L(L - 1, "norm2.bias"), m->jf, jf32, m->out_planes_f, m->c_out,
                          m->b_out)) return rc;
    // InputProcess in split precision: weight [D][jf] zero-padded along K to jf_k, then fragment-ordered planes
    MDM_LAUNCH(pad_rows_kernel, dim3(256), dim3(256), 0, s, scratch_w, m->W("input_process.poseEmbedding.weight"), D, m->jf,
               m->jf_k);
    if (int rc = rt_launch_status()) return rc;
    {
      const size_t n = x3_packed_weight_elems(D, m->jf_k);
      p16_t* hi = reinterpret_cast<p16_t*>(base);
      base += align_up(n * 4, 256);
      m->in_planes = X3Weights{hi, hi + n};
      if (int rc = launch_pack_weights(scratch_w, hi, hi + n, D, m->jf_k, s, m->range_flag)) return rc;
    }
    m->lnfold = true;
  }
  m->prepared = true;
  return MDM_OK;
}

int mdm_weights_in_range(mdm_model_t* m, int32_t* in_range, void* stream) {
  if (int rc = check_ready(m)) return rc;
  if (in_range == nullptr) return fail(MDM_EINVAL, "mdm_weights_in_range: null argument");
  int flag = 0;
#ifdef MDM_EMU
  (void)stream;
  flag = *m->range_flag;
#else
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemcpyAsync(&flag, m->range_flag, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return fail(MDM_EHIP, "mdm_weights_in_range: reading the flag back failed");
#endif
  *in_range = flag == 0 ? 1 : 0;
  return MDM_OK;
}

int mdm_set_precision(mdm_model_t* m, int32_t mode) {
  if (m == nullptr) return fail(MDM_EINVAL, "mdm_set_precision: null model");
  if (mode != MDM_PREC_F32 && mode != MDM_PREC_F16X3) return fail(MDM_EINVAL, "mdm_set_precision: unknown mode");
  if (mode == MDM_PREC_F16X3 && (m->cfg.latent_dim % X3_BK != 0 || m->cfg.ff_size % X3_BK != 0))
    return fail(MDM_EUNSUPPORTED, "f16x3 needs latent_dim and ff_size to be multiples of 32");
  m->precision = mode;
  return MDM_OK;
}

size_t mdm_workspace_bytes(const mdm_model_t* m, int32_t nseq, int32_t nframes) {
  if (m == nullptr || nseq <= 0 || nframes <= 0) return 0;
  return carve(m, nseq, nframes, nullptr).bytes;
}

int mdm_forward(mdm_model_t* m, const float* x, const int64_t* timesteps, const float* text_embed,
                const int32_t* lengths, int32_t B, int32_t T, int32_t branches, float* out, void* ws_dev,
                size_t ws_bytes, void* stream) {
  ChainGuard chain_guard(stream);
  if (int rc = check_ready(m)) return rc;
  TimeAddScope time_add(m, B, "mdm_forward");
  if (time_add.rc) return time_add.rc;
  if (m->cfg.arch != MDM_ARCH_TRANS_ENC) return fail(MDM_ESTATE, "mdm_forward: trans_dec models go through mdm_forward_dec");
  if (x == nullptr || timesteps == nullptr || out == nullptr || ws_dev == nullptr) return fail(MDM_EINVAL, "mdm_forward: null pointer");
  if (B <= 0 || T <= 0 || T + 1 > m->cfg.max_len) return fail(MDM_EINVAL, "mdm_forward: need B >= 1 and 1 <= T < the positional table's length");
  if (branches < 0 || branches > 2) return fail(MDM_EINVAL, "mdm_forward: bad branches");
  if (branches != MDM_BRANCH_UNCOND && text_embed == nullptr) return fail(MDM_EINVAL, "mdm_forward: text_embed required");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nbranch = (branches == MDM_BRANCH_BOTH) ? 2 : 1;
  const int nseq = nbranch * B, S = T + 1, D = m->cfg.latent_dim;
  Workspace ws = carve(m, nseq, T, ws_dev);
  if (ws_bytes < ws.bytes) return fail(MDM_ENOSPC, "mdm_forward: workspace too small");
  const int* len = m->cfg.mask_frames ? lengths : nullptr;
  if (branches != MDM_BRANCH_UNCOND)
    if (int rc = launch_linear(nullptr, text_embed, m->cfg.clip_dim, m->W("embed_text.weight"), m->W("embed_text.bias"), nullptr,
                               ws.cond, B, D, m->cfg.clip_dim, ACT_NONE, 0, 1.f, s)) return rc;
  const int uncond_from = (branches == MDM_BRANCH_UNCOND) ? 0 : 1;
  if (int rc = embed_tokens(m, ws, x, reinterpret_cast<const long long*>(timesteps), /*t_uniform=*/0, ws.cond, B, T, nbranch,
                            uncond_from, s)) return rc;
  if (int rc = encoder(m, ws, nseq, B, S, len, s)) return rc;
  // OutputProcess, plain: every branch's tokens -> [nseq, JF, T]
  if (m->precision == MDM_PREC_F16X3)
    return outproj_x3(m, ws, nseq, B, T, nullptr, 0, out, nullptr, nullptr, NoiseSource{}, nullptr, nullptr, StepCoefs{}, s);
  RowMajorLoader al{m->W("output_process.poseFinal.weight"), D, m->jf, D};
  CfgTokenLoader bl{ws.tok, nullptr, nseq, T, S, D, nseq * T};
  OutProjEpilogue ep{};
  ep.bias = m->W("output_process.poseFinal.bias");
  ep.out = out;
  ep.T = T; ep.JF = m->jf; ep.mode = 0;
  ProfScope ps(&m->prof, MDM_PROF_OUTPROJ, 2.0 * nseq * T * (double)D * m->jf, s);
  launch_gemm_f32(al, bl, ep, m->jf, nseq * T, D, s);
  return rt_launch_status();
}

#include "decoder.h"

size_t mdm_workspace_bytes_dec(const mdm_model_t* m, int32_t nseq, int32_t pred_len, int32_t ntok) {
  if (m == nullptr || nseq <= 0 || pred_len <= 0 || ntok <= 0) return 0;
  return carve_dec(m, nseq, m->cfg.context_len + pred_len, ntok, nseq, nullptr).bytes;
}

size_t mdm_workspace_bytes_dec_loop(const mdm_model_t* m, int32_t nseq, int32_t pred_len, int32_t ntok, int32_t nsteps) {
  if (m == nullptr || nseq <= 0 || pred_len <= 0 || ntok <= 0 || nsteps <= 0) return 0;
  return carve_dec(m, nseq, m->cfg.context_len + pred_len, ntok, nseq, nullptr, nsteps, pred_len).bytes;
}

int mdm_forward_dec(mdm_model_t* m, const float* x, const float* prefix, const int64_t* timesteps, const float* text_tokens,
                    const int32_t* text_lengths, const int32_t* lengths, int32_t B, int32_t pred_len, int32_t ntok,
                    int32_t branches, float* out, void* ws_dev, size_t ws_bytes, void* stream) {
  ChainGuard chain_guard(stream);
  if (int rc = check_ready(m)) return rc;
  TimeAddScope time_add(m, B, "mdm_forward_dec");
  if (time_add.rc) return time_add.rc;
  if (x == nullptr || timesteps == nullptr || out == nullptr || ws_dev == nullptr || text_lengths == nullptr)
    return fail(MDM_EINVAL, "mdm_forward_dec: null pointer");
  if (int rc = check_dec_shapes(m, "mdm_forward_dec", prefix, B, pred_len, ntok)) return rc;
  if (branches < 0 || branches > 2) return fail(MDM_EINVAL, "mdm_forward_dec: bad branches");
  if (branches != MDM_BRANCH_UNCOND && text_tokens == nullptr) return fail(MDM_EINVAL, "mdm_forward_dec: text tokens required");
  const int nseq = ((branches == MDM_BRANCH_BOTH) ? 2 : 1) * B;
  DecWorkspace ws = carve_dec(m, nseq, m->cfg.context_len + pred_len, ntok, B, ws_dev);
  if (ws_bytes < ws.bytes) return fail(MDM_ENOSPC, "mdm_forward_dec: workspace too small");
  return decoder_pass(m, ws, x, prefix, timesteps, text_tokens, text_lengths, lengths, B, pred_len, ntok, branches, out,
                      static_cast<hipStream_t>(stream), DecHoist{});
}

int mdm_sampler_step(const float* x_t, const float* out_cond, const float* out_uncond, const float* scale,
                     const uint8_t* inpaint_mask, const float* inpaint_motion, const float* noise, float* x_prev,
                     float* x0, int32_t B, int32_t per_sample, const mdm_step_t* st, void* stream) {
  ChainGuard chain_guard(stream);
  if (x_t == nullptr || out_cond == nullptr || x_prev == nullptr || st == nullptr) return fail(MDM_EINVAL, "mdm_sampler_step: null pointer");
  if (out_uncond != nullptr && scale == nullptr) return fail(MDM_EINVAL, "mdm_sampler_step: scale required with out_uncond");
  if ((inpaint_mask == nullptr) != (inpaint_motion == nullptr)) return fail(MDM_EINVAL, "mdm_sampler_step: inpainting needs mask and motion");
  if (B <= 0 || per_sample <= 0) return fail(MDM_EINVAL, "mdm_sampler_step: bad shape");
  StepCoefs co{st->a_x0, st->a_xt, st->sigma, st->clip_denoised};
  NoiseSource ns{noise, st->seed, st->sample_base, st->draw, (uint32_t)(st->const_noise != 0)};
  const size_t total = (size_t)B * per_sample;
  const int grid = (int)std::min<size_t>((total + 255) / 256, 2048);
  MDM_LAUNCH(sampler_step_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), x_t, out_cond,
             out_uncond, scale, inpaint_mask, inpaint_motion, x_prev, x0, per_sample, B, co, ns);
  return rt_launch_status();
}

static int launch_randn(float* out, const float* init, const float* eps, float a, float s, int32_t B, int32_t per_sample,
                        uint64_t seed, uint32_t sample_base, uint32_t draw, uint32_t const_noise, void* stream) {
  if (out == nullptr || B <= 0 || per_sample <= 0) return fail(MDM_EINVAL, "mdm_randn: bad argument");
  NoiseSource ns{nullptr, seed, sample_base, draw, const_noise};
  const size_t total = (size_t)B * per_sample;
  const int grid = (int)std::min<size_t>((total + 255) / 256, 2048);
  MDM_LAUNCH(randn_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), out, init, eps, a, s,
             per_sample, B, ns);
  return rt_launch_status();
}

int mdm_randn(float* out, const float* init, const float* eps, float a, float s, int32_t B, int32_t per_sample,
              uint64_t seed, uint32_t sample_base, uint32_t draw, void* stream) {
  ChainGuard chain_guard(stream);
  return launch_randn(out, init, eps, a, s, B, per_sample, seed, sample_base, draw, 0u, stream);
}
#include "loops.h"

#ifdef MDM_PROBES
int mdm_debug_set(int what, int value) {
  // 0 (GEMM ablations), 2 (4-wave workgroups), 6 (sync / pipe probe), 8 (start delay) of gemm_x3.h and 3 (ablations of
  // attention_x3.h): experiments that were removed with their code (lab/README.md) -- refused, so that an old A/B script does not
  // measure the product against itself
  if (what == 0 || what == 2 || what == 3 || what == 6 || what == 8)
    return fail(MDM_EINVAL, "mdm_debug_set: code " + std::to_string(what) + " belonged to a " +
                                (what == 3 ? "attention_x3.h" : "gemm_x3.h") + " experiment that has been removed");
  if (what == 1) g_x3_reuse_planes = value;
  if (what == 4) g_f6_reference = value;
  if (what == 5) g_f6_linear = value;
#ifndef MDM_EMU
  if (what == 9) { x3s_tl_target() = value; x3s_tl_count() = 0; }   // gemm_x3s.h timeline probe: stamp the value-th launch from now
  if (what == 10) { xb_tl_target() = value; xb_tl_count() = 0; }    // xattn_block.h timeline probe
  if (what == 11) { sb_tl_target() = value; sb_tl_count() = 0; }    // selfattn_block.h timeline probe (self and cross launches)
#endif
  return MDM_OK;
}

int mdm_debug_get(int idx, double* out) {   // timeline stamps of the x3s / xattn / selfattn probes
#ifndef MDM_EMU
  if (idx >= 300000) {   // selfattn_block.h timeline stamps (read once at idx == 300000, then served from the host copy)
    static std::vector<unsigned long long> tl(8 * SB_TL_WGS);
    if (idx - 300000 >= 8 * SB_TL_WGS || out == nullptr) return fail(MDM_EINVAL, "mdm_debug_get: bad timeline index");
    if (idx == 300000 && (hipDeviceSynchronize() != hipSuccess ||
                          hipMemcpyFromSymbol(tl.data(), HIP_SYMBOL(g_sb_tl), tl.size() * sizeof(unsigned long long)) != hipSuccess))
      return fail(MDM_EHIP, "mdm_debug_get: reading the timeline failed");
    *out = (double)tl[idx - 300000];
    return MDM_OK;
  }
  if (idx >= 200000) {   // xattn_block.h timeline stamps (read once at idx == 200000, then served from the host copy)
    static std::vector<unsigned long long> tl(8 * XB_TL_WGS);
    if (idx - 200000 >= 8 * XB_TL_WGS || out == nullptr) return fail(MDM_EINVAL, "mdm_debug_get: bad timeline index");
    if (idx == 200000 && (hipDeviceSynchronize() != hipSuccess ||
                          hipMemcpyFromSymbol(tl.data(), HIP_SYMBOL(g_xb_tl), tl.size() * sizeof(unsigned long long)) != hipSuccess))
      return fail(MDM_EHIP, "mdm_debug_get: reading the timeline failed");
    *out = (double)tl[idx - 200000];
    return MDM_OK;
  }
  if (idx >= 100) {   // gemm_x3s.h timeline stamps (read once at idx == 100, then served from the host copy)
    static std::vector<unsigned long long> tl(4 * X3S_TL_WGS);
    if (idx - 100 >= 4 * X3S_TL_WGS || out == nullptr) return fail(MDM_EINVAL, "mdm_debug_get: bad timeline index");
    if (idx == 100 && (hipDeviceSynchronize() != hipSuccess ||
                       hipMemcpyFromSymbol(tl.data(), HIP_SYMBOL(g_x3s_tl), tl.size() * sizeof(unsigned long long)) != hipSuccess))
      return fail(MDM_EHIP, "mdm_debug_get: reading the timeline failed");
    *out = (double)tl[idx - 100];
    return MDM_OK;
  }
  return fail(MDM_EINVAL, "mdm_debug_get: not a timeline index");
#else
  if (out != nullptr) *out = 0.0;
  (void)idx;
  return MDM_OK;
#endif
}
#endif

int mdm_profile_enable(mdm_model_t* m, int on) {
  if (m == nullptr) return fail(MDM_EINVAL, "mdm_profile_enable: null model");
  m->prof.on = on != 0;
  return MDM_OK;
}

int mdm_profile_read(mdm_model_t* m, int32_t category, double* total_ms, int64_t* launches, double* flops) {
  if (m == nullptr || category < 0 || category >= MDM_PROF_NUM) return fail(MDM_EINVAL, "mdm_profile_read: bad argument");
  double ms = 0.0, fl = 0.0;
  int64_t n = 0;
#ifndef MDM_EMU
  for (const auto& r : m->prof.recs) {
    if (r.cat != category) continue;
    if (hipEventSynchronize(r.b) != hipSuccess) return fail(MDM_EHIP, "mdm_profile_read: hipEventSynchronize failed");
    float dt = 0.f;
    if (hipEventElapsedTime(&dt, r.a, r.b) != hipSuccess) return fail(MDM_EHIP, "mdm_profile_read: hipEventElapsedTime failed");
    ms += dt; fl += r.flops; ++n;
  }
#else
  n = m->prof.launches[category];
#endif
  if (total_ms) *total_ms = ms;
  if (launches) *launches = n;
  if (flops) *flops = fl;
  return MDM_OK;
}

int mdm_profile_reset(mdm_model_t* m) {
  if (m == nullptr) return fail(MDM_EINVAL, "mdm_profile_reset: null model");
#ifndef MDM_EMU
  for (auto& r : m->prof.recs) { m->prof.pool.push_back(r.a); m->prof.pool.push_back(r.b); }
  m->prof.recs.clear();
#else
  for (auto& c : m->prof.launches) c = 0;
#endif
  return MDM_OK;
}

int mdm_linear(const float* in, const float* w, const float* bias, const float* res, float* out, int32_t M, int32_t N,
               int32_t K, int32_t act, void* stream) {
  ChainGuard chain_guard(stream);
  if (!in || !w || !bias || !out || M <= 0 || N <= 0 || K <= 0) return fail(MDM_EINVAL, "mdm_linear: bad argument");
  return launch_linear(nullptr, in, K, w, bias, res, out, M, N, K, act, 0, 1.f, static_cast<hipStream_t>(stream));
}

// The weight region is sized for N rounded up to whole 256-column tiles although pack_weight_planes_kernel writes the planes of N
// rounded up to 32 only: every wave of gemm_x3_kernel's last column tile fetches the fragments of its own 32 columns (load_w /
// aim_w_tile do not look at N), so with N % 256 != 0 the waves past the packed rows read up to 7 blocks of 32 rows behind the lo plane
// -- values that are never stored, but bytes that must exist.  (In an engine the planes lie inside the constant workspace; here they
// ended the caller's buffer, and the fetch ran up to 7 * 64 K bytes past it: an illegal address when the buffer ends a mapping.)
size_t mdm_linear_x3_scratch_bytes(int32_t M, int32_t N, int32_t K) {
  const int32_t n_tiles = (N + 255) / 256 * 256;
  return align_up((size_t)M * K * 4, 256) + align_up(x3_packed_weight_elems(n_tiles, K) * 4, 256);
}

int mdm_linear_x3(const float* in, const float* w, const float* bias, const float* res, float* out, int32_t M,
                      int32_t N, int32_t K, int32_t act, void* scratch, size_t scratch_bytes, void* stream) {
  ChainGuard chain_guard(stream);
  if (!in || !w || !bias || !out || !scratch || M <= 0 || N <= 0 || K <= 0) return fail(MDM_EINVAL, "mdm_linear_x3: bad argument");
  if (K % X3_BK != 0) return fail(MDM_EINVAL, "mdm_linear_x3: K must be a multiple of 32");
  if (scratch_bytes < mdm_linear_x3_scratch_bytes(M, N, K)) return fail(MDM_ENOSPC, "mdm_linear_x3: scratch too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  p16_t* ah = static_cast<p16_t*>(scratch);
  p16_t* al = ah + (size_t)M * K;
  p16_t* wh = reinterpret_cast<p16_t*>(static_cast<char*>(scratch) + align_up((size_t)M * K * 4, 256));
  p16_t* wl = wh + x3_packed_weight_elems(N, K);
  if (!g_x3_reuse_planes) {
    if (int rc = launch_split(in, ah, al, (size_t)M * K, s)) return rc;
    if (int rc = launch_pack_weights(w, wh, wl, N, K, s)) return rc;
  }
  return launch_linear_x3(nullptr, X3Operand{ah, al}, X3Weights{wh, wl}, bias, res, out, nullptr, nullptr, M, N, K, act, 0,
                          1.f, 0, s);
}

#ifdef MDM_PROBES
size_t mdm_linear_f16f6_scratch_bytes(int32_t M, int32_t N, int32_t K) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 32 != 0) return 0;
  // A planes | W as fragment-ordered planes (fast kernel) | W as row-major planes (reference kernel)
  return f6_plane_bytes(M, K) + 2 * align_up(x3_packed_weight_elems(N, K) * 2, 256) + f6_plane_bytes(N, K);
}

int mdm_linear_f16f6(const float* in, const float* w, const float* bias, const float* res, float* out, int32_t M,
                     int32_t N, int32_t K, int32_t act, void* scratch, size_t scratch_bytes, void* stream) {
  ChainGuard chain_guard(stream);
  if (!in || !w || !bias || !out || !scratch || M <= 0 || N <= 0 || K <= 0) return fail(MDM_EINVAL, "mdm_linear_f16f6: bad argument");
  if (K % 32 != 0) return fail(MDM_EINVAL, "mdm_linear_f16f6: K must be a multiple of 32");
  if (act != ACT_NONE && act != ACT_GELU && act != ACT_SILU) return fail(MDM_EINVAL, "mdm_linear_f16f6: bad activation");
  if (scratch_bytes < mdm_linear_f16f6_scratch_bytes(M, N, K)) return fail(MDM_ENOSPC, "mdm_linear_f16f6: scratch too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(scratch);
  const F6Planes pa = f6_carve(base, M, K);
  p16_t* wfh = reinterpret_cast<p16_t*>(base + f6_plane_bytes(M, K));
  p16_t* wfl = reinterpret_cast<p16_t*>(base + f6_plane_bytes(M, K) + align_up(x3_packed_weight_elems(N, K) * 2, 256));
  const F6Planes pw = f6_carve(base + f6_plane_bytes(M, K) + 2 * align_up(x3_packed_weight_elems(N, K) * 2, 256), N, K);
  // the production skeleton (gemm_x3_kernel<..., X3_OUT_F32 | X3_F6>) where its epilogues exist; else the one-wave-per-tile reference
  const bool fast = !g_f6_reference && N % 4 == 0 && ((act == ACT_NONE) || (act == ACT_GELU && res == nullptr));
  if (!g_x3_reuse_planes) {
    MDM_LAUNCH(pack_f16f6_kernel, dim3((M * (K / 32) + 255) / 256), dim3(256), 0, s, in, pa, M, K, K);
    if (int rc = rt_launch_status()) return rc;
    if (fast) {
      const int npad = (N + 31) / 32 * 32;
      MDM_LAUNCH(pack_weight_f16f6_kernel, dim3((npad * (K / 32) + 255) / 256), dim3(256), 0, s, w, wfh, wfl, N, K);
    } else {
      MDM_LAUNCH(pack_f16f6_kernel, dim3((N * (K / 32) + 255) / 256), dim3(256), 0, s, w, pw, N, K, K);
    }
    if (int rc = rt_launch_status()) return rc;
  }
  if (fast) {
    X3Call c; c.out = out; c.bias = bias; c.res_f32 = res; c.N = N;
    X3Epilogue ep = x3_epilogue(c);
    ep.acc_scale = 1.f;   // (pack_weight_f16f6_kernel's planes are unscaled: no 2^8 to undo)
    const X3Operand a{reinterpret_cast<const p16_t*>(pa.h16), reinterpret_cast<const p16_t*>(pa.rec)};
    const int rc = launch_gemm_f16f6(a, X3Weights{wfh, wfl}, ep, M, N, K, act, s);
    if (rc == -1 || rc == -3) return lds_fail(rc, "mdm_linear_f16f6");
    if (rc == -2) return fail(MDM_EUNSUPPORTED, "mdm_linear_f16f6: unsupported (activation, residual) combination");
    return rt_launch_status();
  }
  const dim3 grid((N + 31) / 32, (M + 31) / 32);
  if (act == ACT_GELU) MDM_LAUNCH(gemm_f16f6_ref_kernel<ACT_GELU>, grid, dim3(64), 0, s, pa, pw, bias, res, out, M, N, K);
  else if (act == ACT_SILU) MDM_LAUNCH(gemm_f16f6_ref_kernel<ACT_SILU>, grid, dim3(64), 0, s, pa, pw, bias, res, out, M, N, K);
  else MDM_LAUNCH(gemm_f16f6_ref_kernel<ACT_NONE>, grid, dim3(64), 0, s, pa, pw, bias, res, out, M, N, K);
  return rt_launch_status();
}
#endif

int mdm_layernorm(float* x, const float* gamma, const float* beta, int32_t rows, int32_t D, void* stream) {
  ChainGuard chain_guard(stream);
  if (!x || !gamma || !beta || rows <= 0 || D % 256 != 0) return fail(MDM_EINVAL, "mdm_layernorm: bad argument");
  return launch_layernorm(nullptr, x, gamma, beta, rows, D, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int mdm_attention(const float* qkv, float* out, const int32_t* lengths, int32_t nseq, int32_t B, int32_t S, int32_t D,
                  int32_t H, void* stream) {
  ChainGuard chain_guard(stream);
  if (!qkv || !out || nseq <= 0 || B <= 0) return fail(MDM_EINVAL, "mdm_attention: bad argument");
  return launch_attention(nullptr, qkv, out, lengths, nseq, B, S, D, H, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

size_t mdm_attention_x3_scratch_bytes(int32_t nseq, int32_t S, int32_t D) {
  if (nseq <= 0 || S <= 0 || D <= 0) return 0;
  const size_t SP = (size_t)(S + 31) / 32 * 32;
  return (size_t)nseq * SP * D * 12;
}

int mdm_attention_x3(const float* qkv, float* out, const int32_t* lengths, int32_t nseq, int32_t B, int32_t S,
                         int32_t D, int32_t H, void* scratch, size_t scratch_bytes, void* stream) {
  ChainGuard chain_guard(stream);
  if (!qkv || !out || !scratch || nseq <= 0 || B <= 0 || S <= 0 || H <= 0) return fail(MDM_EINVAL, "mdm_attention_x3: bad argument");
  if (D != H * AX_HD) return fail(MDM_EUNSUPPORTED, "attention: head_dim must be 128");
  if (scratch_bytes < mdm_attention_x3_scratch_bytes(nseq, S, D)) return fail(MDM_ENOSPC, "mdm_attention_x3: scratch too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int NKT = (S + 31) / 32, SP = 32 * NKT;
  const size_t plane = (size_t)nseq * SP * D;
  p16_t* q = static_cast<p16_t*>(scratch);
  QkvPlanes qp{q, q + plane, q + 2 * plane, q + 3 * plane, q + 4 * plane, q + 5 * plane, SP, NKT, H};
  const int grid = (int)std::min<size_t>((plane + 255) / 256, 4096);
  if (!g_x3_reuse_planes) {   // mdm_debug_set(1, 1): kernel-only timing, the planes of the previous call are reused
    MDM_LAUNCH(qkv_pack_kernel, dim3(grid), dim3(256), 0, s, qkv, qp, nseq, S, D);
    if (int rc = rt_launch_status()) return rc;
  }
  return launch_attention_x3(nullptr, qp, lengths, nseq, B, S, D, out, nullptr, nullptr, s);
}

#ifdef MDM_PROBES
// mdm_attention_x3 with the kernel form, the lead tokens and the outputs chosen by the caller: fp32 rows and / or hi, lo planes.
// tests/test_*_attention_wide.py hold the wide form against the 4-wave kernel bit for bit.
int mdm_probe_attention_x3(const float* qkv, float* out, void* out_hi, void* out_lo, const int32_t* lengths, int32_t nseq, int32_t B,
                           int32_t S, int32_t D, int32_t H, int32_t lead, int32_t wide, void* scratch, size_t scratch_bytes,
                           void* stream) {
  ChainGuard chain_guard(stream);
  if (!qkv || (!out && !out_hi) || (out_hi == nullptr) != (out_lo == nullptr) || !scratch || nseq <= 0 || B <= 0 || S <= 0 || H <= 0 ||
      lead < 0)
    return fail(MDM_EINVAL, "mdm_probe_attention_x3: bad argument");
  if (D != H * AX_HD) return fail(MDM_EUNSUPPORTED, "attention: head_dim must be 128");
  if (scratch_bytes < mdm_attention_x3_scratch_bytes(nseq, S, D)) return fail(MDM_ENOSPC, "mdm_probe_attention_x3: scratch too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int NKT = (S + 31) / 32, SP = 32 * NKT;
  const size_t plane = (size_t)nseq * SP * D;
  p16_t* q = static_cast<p16_t*>(scratch);
  QkvPlanes qp{q, q + plane, q + 2 * plane, q + 3 * plane, q + 4 * plane, q + 5 * plane, SP, NKT, H};
  MDM_LAUNCH(qkv_pack_kernel, dim3((int)std::min<size_t>((plane + 255) / 256, 4096)), dim3(256), 0, s, qkv, qp, nseq, S, D);
  if (int rc = rt_launch_status()) return rc;
  return launch_attention_x3(nullptr, qp, lengths, nseq, B, S, D, out, static_cast<p16_t*>(out_hi), static_cast<p16_t*>(out_lo), s, lead,
                             /*direct=*/false, wide != 0);
}

// in_proj alone (the non-folded instantiation of layer 0): fp32 tokens [nseq * S][D] and in_proj weights [3D][D] -> the
// attention operand planes, written to `planes_dev` (6 planes of nseq * SP * D 16-bit elements: qh ql kh kl vh vl).
// `scratch_dev`: 4 * nseq * S * D + 12 * D * D bytes.  tools/in_proj_determinism.py compares repeated runs bit for bit.
int mdm_probe_in_proj(const float* tokens, const float* w, const float* bias, void* planes_dev, int32_t nseq, int32_t S,
                      int32_t D, void* scratch_dev, void* stream) {
  ChainGuard chain_guard(stream);
  if (!tokens || !w || !bias || !planes_dev || !scratch_dev || nseq <= 0 || S <= 0 || D % 256 != 0) return fail(MDM_EINVAL, "mdm_probe_in_proj");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t n = (size_t)nseq * S * D;
  p16_t* ah = static_cast<p16_t*>(scratch_dev);
  p16_t* al = ah + n;
  p16_t* wh = al + n;
  p16_t* wl = wh + (size_t)3 * D * D;
  if (!g_x3_reuse_planes) {
    if (int rc = launch_split(tokens, ah, al, n, s)) return rc;
    if (int rc = launch_pack_weights(w, wh, wl, 3 * D, D, s)) return rc;
  }
  const int H = D / AX_HD, NKT = (S + 31) / 32, SP = 32 * NKT;
  const size_t plane = (size_t)nseq * SP * D;
  p16_t* q = static_cast<p16_t*>(planes_dev);
  QkvPlanes qp{q, q + plane, q + 2 * plane, q + 3 * plane, q + 4 * plane, q + 5 * plane, SP, NKT, H};
  return launch_in_proj_x3(nullptr, X3Operand{ah, al}, X3Weights{wh, wl}, bias, qp, nseq, S, D, 0.08838834764831845f, s);
}
#endif

int mdm_recover_from_ric(const float* x, const float* mean, const float* stdv, float* out, int32_t B, int32_t T,
                         int32_t njoints_feat, int32_t joints, void* stream) {
  ChainGuard chain_guard(stream);
  if (!x || !mean || !stdv || !out || B <= 0 || T <= 0 || joints < 1) return fail(MDM_EINVAL, "mdm_recover_from_ric: bad argument");
  if (njoints_feat < 4 + 3 * (joints - 1)) return fail(MDM_EINVAL, "mdm_recover_from_ric: feature width too small for the joint count");
  if (T > 1024) return fail(MDM_EUNSUPPORTED, "mdm_recover_from_ric: at most 1024 frames");
  auto k = &recover_from_ric_kernel;
  MDM_LAUNCH(k, dim3(B), dim3(256), (size_t)3 * T * sizeof(float), static_cast<hipStream_t>(stream), x, mean, stdv, out, T,
             njoints_feat, joints);
  return rt_launch_status();
}

int mdm_rot6d_to_smpl_joints(const float* x, const uint8_t* mask, const float* rest_joints, const int32_t* parents, float* out,
                             int32_t B, int32_t T, int32_t njoints_in, int32_t J, void* stream) {
  if (!x || !rest_joints || !parents || !out) return fail(MDM_EINVAL, "mdm_rot6d_to_smpl_joints: null pointer");
  if (B <= 0 || T <= 0 || J < 1) return fail(MDM_EINVAL, "mdm_rot6d_to_smpl_joints: need B >= 1, T >= 1 and J >= 1");
  if (njoints_in != J + 1)
    return fail(MDM_EINVAL, "mdm_rot6d_to_smpl_joints: njoints_in must be J + 1 (the joint rotations, then the translation row)");
  if (J > kSmplMaxJoints) return fail(MDM_EUNSUPPORTED, "mdm_rot6d_to_smpl_joints: at most 24 joints");
  if (T > 4096 || (int64_t)B * T > (1 << 24)) return fail(MDM_EUNSUPPORTED, "mdm_rot6d_to_smpl_joints: at most 4096 frames and 2^24 frames in all");
  if (parents[0] != -1) return fail(MDM_EINVAL, "mdm_rot6d_to_smpl_joints: parents[0] must be -1 (the root)");
  for (int i = 1; i < J; ++i)
    if (parents[i] < 0 || parents[i] >= i)
      return fail(MDM_EINVAL, "mdm_rot6d_to_smpl_joints: parents[" + std::to_string(i) + "] must lie in [0, " + std::to_string(i) + ")");
  SmplFkTables tab;
  if (smpl_fk_tables(rest_joints, parents, J, tab) < 0) return fail(MDM_EUNSUPPORTED, "mdm_rot6d_to_smpl_joints: tree needs too many live transforms");
  ChainGuard chain_guard(stream);
  auto k = &smpl_joints_kernel;
  MDM_LAUNCH(k, dim3((unsigned)(((int64_t)B * T + kSmplLanes - 1) / kSmplLanes)), dim3(kSmplLanes), 0, static_cast<hipStream_t>(stream),
             x, mask, out, B, T, J, tab);
  return rt_launch_status();
}

}  // extern "C"

namespace {

struct SmplPlan {
  int J, V, Vpad, KP, NA;          // NA: rows of the extended joint list
  bool joints, need_sel, need_mesh;
  size_t feat, aws, delta, allj, mesh;   // workspace extents, floats
};

// Validation shared by mdm_smpl_workspace_bytes and mdm_smpl_forward; 0 or a negative code with the message set.
int smpl_plan(const char* fn, const mdm_smpl_model_t* m, const mdm_smpl_call_t* c, int B, int T, SmplPlan& p) {
  const std::string f = std::string(fn) + ": ";
  if (m == nullptr || c == nullptr) return fail(MDM_EINVAL, f + "null model or call");
  if (B <= 0 || T <= 0) return fail(MDM_EINVAL, f + "need B >= 1 and T >= 1");
  if (T > 4096 || (int64_t)B * T > (1 << 24)) return fail(MDM_EUNSUPPORTED, f + "at most 4096 frames and 2^24 frames in all");
  if (m->J < 1) return fail(MDM_EINVAL, f + "need J >= 1");
  if (m->J > kSmplMaxJoints) return fail(MDM_EUNSUPPORTED, f + "at most 24 joints");
  if (m->V < 1 || m->V > (1 << 20)) return fail(MDM_EINVAL, f + "the vertex count V must lie in [1, 2^20]");
  if (m->n_sel < 0 || m->n_sel > 32) return fail(MDM_EINVAL, f + "n_sel must lie in [0, 32]");
  if (m->n_extra < 0 || m->n_extra > kSmplMaxExtra) return fail(MDM_EINVAL, f + "n_extra must lie in [0, 16]");
  if (m->parents == nullptr) return fail(MDM_EINVAL, f + "null parents");
  if (m->parents[0] != -1) return fail(MDM_EINVAL, f + "parents[0] must be -1 (the root)");
  for (int i = 1; i < m->J; ++i)
    if (m->parents[i] < 0 || m->parents[i] >= i)
      return fail(MDM_EINVAL, f + "parents[" + std::to_string(i) + "] must lie in [0, " + std::to_string(i) + ")");
  if (c->pose_rep < MDM_SMPL_ROT6D || c->pose_rep > MDM_SMPL_ROTQUAT) return fail(MDM_EINVAL, f + "pose_rep must be one of MDM_SMPL_ROT6D .. MDM_SMPL_ROTQUAT");
  if (!c->glob && c->glob_rot_mat == nullptr) return fail(MDM_EINVAL, f + "glob = 0 needs glob_rot_mat");
  if (c->n_points < 0 || c->n_points > kSmplMaxPoints) return fail(MDM_EINVAL, f + "n_points must lie in [0, 64]");
  p.J = m->J;
  p.V = m->V;
  p.Vpad = (m->V + 31) & ~31;
  p.KP = smpl_feat_kp(m->J);
  p.NA = m->J + m->n_sel + m->n_extra;
  p.joints = c->n_points > 0;
  p.need_sel = p.need_mesh = false;
  if (p.joints) {
    if (c->point_map == nullptr) return fail(MDM_EINVAL, f + "n_points > 0 needs point_map");
    if (c->root_point < 0 || c->root_point >= c->n_points) return fail(MDM_EINVAL, f + "root_point must lie in [0, n_points)");
    for (int i = 0; i < c->n_points; ++i) {
      const int s = c->point_map[i];
      if (s < 0 || s >= p.NA)
        return fail(MDM_EINVAL, f + "point_map[" + std::to_string(i) + "] = " + std::to_string(s) + " is outside the joint list of " +
                                    std::to_string(p.NA) + " (J + n_sel + n_extra)");
      if (s >= m->J + m->n_sel) p.need_mesh = true;
      else if (s >= m->J) p.need_sel = true;
    }
  }
  p.feat = (size_t)B * p.KP * T;
  p.aws = (size_t)B * 12 * kSmplMaxJoints * T;
  p.delta = (size_t)B * 3 * T;
  p.allj = (size_t)B * p.NA * 3 * T;
  p.mesh = p.need_mesh ? (size_t)kSkinChunkTiles * kSkinFrames * 3 * p.V : 0;
  return 0;
}

size_t smpl_plan_bytes(const SmplPlan& p) { return (p.feat + p.aws + p.delta + p.allj + p.mesh) * sizeof(float) + 64; }

template <int REP> void launch_smpl_pose(const SmplPoseArgs& a, hipStream_t s) {
  auto k = &smpl_pose_kernel<REP>;
  MDM_LAUNCH(k, dim3((unsigned)(((int64_t)a.B * a.T + kSmplLanes - 1) / kSmplLanes)), dim3(kSmplLanes), 0, s, a);
}

}  // namespace

extern "C" {

size_t mdm_smpl_workspace_bytes(const mdm_smpl_model_t* model, const mdm_smpl_call_t* call, int32_t B, int32_t T) {
  SmplPlan p;
  if (smpl_plan("mdm_smpl_workspace_bytes", model, call, B, T, p) != 0) return 0;
  return smpl_plan_bytes(p);
}

int mdm_smpl_forward(const mdm_smpl_model_t* m, const mdm_smpl_call_t* c, const float* x, const uint8_t* mask, const float* betas,
                     float* out, float* rot_out, int32_t B, int32_t T, int32_t rows_x, int32_t feats_x, void* ws, size_t ws_bytes,
                     void* stream) {
  const char* fn = "mdm_smpl_forward";
  SmplPlan p;
  if (int rc = smpl_plan(fn, m, c, B, T, p)) return rc;
  if (!x || !out || !ws) return fail(MDM_EINVAL, "mdm_smpl_forward: null x, out or workspace");
  if (!m->j0 || !m->jdirs) return fail(MDM_EINVAL, "mdm_smpl_forward: null j0 or jdirs table");
  const bool skin = !p.joints || p.need_mesh;
  if (skin && (!m->blend || !m->weights_t)) return fail(MDM_EINVAL, "mdm_smpl_forward: null blend or weights_t table");
  if (p.need_sel && (!m->sel_blend || !m->sel_weights_t)) return fail(MDM_EINVAL, "mdm_smpl_forward: the map names a selected vertex: null sel_blend or sel_weights_t table");
  if (p.need_mesh && !m->extra_t) return fail(MDM_EINVAL, "mdm_smpl_forward: the map names a regressed joint: null extra_t table");
  const int NR = c->glob ? p.J : p.J - 1;
  const int has_trans = c->translation ? 1 : 0;
  if (rows_x != NR + has_trans)
    return fail(MDM_EINVAL, "mdm_smpl_forward: x has " + std::to_string(rows_x) + " rows; need " + std::to_string(NR) +
                                " rotation rows" + (has_trans ? " and the translation row" : ""));
  if (feats_x != smpl_rep_feats(c->pose_rep))
    return fail(MDM_EINVAL, "mdm_smpl_forward: x has " + std::to_string(feats_x) + " features per row; this pose_rep has " +
                                std::to_string(smpl_rep_feats(c->pose_rep)));
  if (NR < 1) return fail(MDM_EINVAL, "mdm_smpl_forward: no rotation row");
  if (ws_bytes < smpl_plan_bytes(p)) return fail(MDM_ENOSPC, "mdm_smpl_forward: workspace too small (mdm_smpl_workspace_bytes)");
  SmplFkTables tab;
  {
    float zero[kSmplMaxJoints * 3] = {};
    if (smpl_fk_tables(zero, m->parents, p.J, tab) < 0) return fail(MDM_EUNSUPPORTED, "mdm_smpl_forward: tree needs too many live transforms");
  }
  float* w = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws) + 15) & ~(uintptr_t)15);
  float* feat = w;
  float* aws = feat + p.feat;
  float* delta = aws + p.aws;
  float* allj = delta + p.delta;
  float* mesh = allj + p.allj;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);

  SmplPoseArgs pa;
  pa.x = x; pa.mask = mask; pa.betas = betas; pa.j0 = m->j0; pa.jdirs = m->jdirs;
  pa.feat = feat; pa.aws = aws; pa.joints = allj; pa.delta = delta; pa.rot_out = rot_out;
  pa.B = B; pa.T = T; pa.J = p.J; pa.NR = NR; pa.F = feats_x; pa.KP = p.KP; pa.joints_rows = p.NA;
  pa.glob = c->glob ? 1 : 0; pa.has_trans = has_trans; pa.add_trans = has_trans && c->vertstrans ? 1 : 0;
  pa.beta1 = c->beta1;
  for (int i = 0; i < 9; ++i) pa.grot[i] = c->glob ? 0.f : c->glob_rot_mat[i];
  for (int i = 0; i < kSmplMaxJoints; ++i) {
    pa.parent[i] = i < p.J && i > 0 ? m->parents[i] : 0;
    pa.pslot[i] = tab.pslot[i];
    pa.oslot[i] = tab.oslot[i];
  }
  switch (c->pose_rep) {
    case MDM_SMPL_ROT6D: launch_smpl_pose<kRepRot6d>(pa, s); break;
    case MDM_SMPL_ROTVEC: launch_smpl_pose<kRepRotvec>(pa, s); break;
    case MDM_SMPL_ROTMAT: launch_smpl_pose<kRepRotmat>(pa, s); break;
    default: launch_smpl_pose<kRepRotquat>(pa, s); break;
  }
  if (int rc = rt_launch_status()) return rc;

  const int tps = (T + kSkinFrames - 1) / kSkinFrames, ntiles = B * tps;
  SmplSkinArgs sa;
  sa.feat = feat; sa.aws = aws; sa.delta = delta; sa.mask = mask;
  sa.T = T; sa.KP = p.KP; sa.tiles_per_sample = tps;
  auto skin_k = &smpl_skin_kernel;
  if (!p.joints) {                       // 'vertices': the mesh is the output
    sa.blend = m->blend; sa.wt = m->weights_t; sa.out = out; sa.V = p.V; sa.Vpad = p.Vpad;
    sa.tile0 = 0; sa.mode = 0; sa.out_rows = p.V; sa.row_off = 0; sa.finish = 1;
    MDM_LAUNCH(skin_k, dim3(ntiles, (p.Vpad / 32 + kSkinTiles - 1) / kSkinTiles), dim3(kSkinWaves * 64), 0, s, sa);
    return rt_launch_status();
  }
  if (p.need_sel) {                      // the selected vertices, skinned from their gathered tables into the joint list
    sa.blend = m->sel_blend; sa.wt = m->sel_weights_t; sa.out = allj; sa.V = m->n_sel; sa.Vpad = (m->n_sel + 31) & ~31;
    sa.tile0 = 0; sa.mode = 0; sa.out_rows = p.NA; sa.row_off = p.J; sa.finish = 0;
    MDM_LAUNCH(skin_k, dim3(ntiles, 1), dim3(kSkinWaves * 64), 0, s, sa);
    if (int rc = rt_launch_status()) return rc;
  }
  if (p.need_mesh) {                     // the regressed joints: the mesh of 16 frame tiles at a time, then a fixed-order reduction
    sa.blend = m->blend; sa.wt = m->weights_t; sa.out = mesh; sa.V = p.V; sa.Vpad = p.Vpad;
    sa.mode = 1; sa.out_rows = 0; sa.row_off = 0; sa.finish = 0;
    auto extra_k = &smpl_extra_kernel;
    for (int t0 = 0; t0 < ntiles; t0 += kSkinChunkTiles) {
      const int n = std::min(kSkinChunkTiles, ntiles - t0);
      sa.tile0 = t0;
      MDM_LAUNCH(skin_k, dim3(n, (p.Vpad / 32 + kSkinTiles - 1) / kSkinTiles), dim3(kSkinWaves * 64), 0, s, sa);
      MDM_LAUNCH(extra_k, dim3(n, 3, m->n_extra), dim3(256), 0, s, (const float*)mesh, m->extra_t, allj, (int)T, p.V, (int)m->n_extra, tps, t0, p.NA,
                 p.J + m->n_sel);
      if (int rc = rt_launch_status()) return rc;
    }
  }
  SmplPointMap map;
  for (int i = 0; i < kSmplMaxPoints; ++i) map.src[i] = i < c->n_points ? c->point_map[i] : 0;
  auto points_k = &smpl_points_kernel;
  const size_t n = (size_t)B * c->n_points * 3 * T;
  MDM_LAUNCH(points_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)allj, (const float*)delta, mask, out, (int)B, (int)T,
             (int)c->n_points, p.NA, (int)c->root_point, map);
  return rt_launch_status();
}

}  // extern "C"

namespace {

struct EvalPlan {
  int T1, T2;                         // frames after the first / second convolution
  size_t motion, text;                // workspace extents, floats
};

int eval_check_gru(const std::string& f, const char* which, const mdm_eval_gru_t& g, int in_dim) {
  const std::string w = f + which;
  if (g.hidden <= 0 || g.hidden % 256 != 0 || g.hidden > 1024)
    return fail(MDM_EUNSUPPORTED, w + ".hidden must be 256, 512, 768 or 1024 (the step kernel's 8 x 32-deep k split and the LayerNorm rows)");
  if (g.in_dim != in_dim) return fail(MDM_EINVAL, w + ".in_dim must equal the width of what feeds it (" + std::to_string(in_dim) + ")");
  if (g.out <= 0 || g.out % 4 != 0) return fail(MDM_EUNSUPPORTED, w + ".out must be a positive multiple of 4");
  const float* ptrs[] = {g.in_w, g.in_b, g.w_ih, g.b_ih, g.w_hh, g.b_hh, g.h0, g.o1_w, g.o1_b, g.ln_g, g.ln_b, g.o2_w, g.o2_b};
  for (const float* q : ptrs) {
    if (q == nullptr) return fail(MDM_EINVAL, w + ": null weight pointer");
    if ((reinterpret_cast<uintptr_t>(q) & 15) != 0) return fail(MDM_EINVAL, w + ": weight pointers must be 16-byte aligned");
  }
  return 0;
}

// Validation shared by the three mdm_eval_* entry points; 0 or a negative code with the message set.  T or L may be 0 (unused side).
int eval_plan(const char* fn, const mdm_eval_model_t* m, int B, int T, int L, EvalPlan& p) {
  const std::string f = std::string(fn) + ": ";
  if (m == nullptr) return fail(MDM_EINVAL, f + "null model");
  if (B <= 0 || T < 0 || L < 0) return fail(MDM_EINVAL, f + "need B >= 1, T >= 0 and L >= 0");
  if (m->unit_length != 4) return fail(MDM_EUNSUPPORTED, f + "unit_length must be 4 (two stride-2 convolutions)");
  if (m->dim_pose < 5) return fail(MDM_EINVAL, f + "dim_pose must be at least 5 (the last 4 features are not read)");
  if (m->conv_hidden <= 0 || m->conv_hidden % 4 || m->latent <= 0 || m->latent % 4)
    return fail(MDM_EUNSUPPORTED, f + "conv_hidden and latent must be positive multiples of 4");
  if (m->word <= 0 || m->word % 4 || m->pos <= 0) return fail(MDM_EUNSUPPORTED, f + "word must be a positive multiple of 4 and pos positive");
  if (int rc = eval_check_gru(f, "motion", m->motion, m->latent)) return rc;
  if (int rc = eval_check_gru(f, "text", m->text, m->word)) return rc;
  const float* ptrs[] = {m->conv1_w, m->conv1_b, m->conv2_w, m->conv2_b, m->out_w, m->out_b, m->pos_w, m->pos_b};
  for (const float* q : ptrs) {
    if (q == nullptr) return fail(MDM_EINVAL, f + "null weight pointer");
    if ((reinterpret_cast<uintptr_t>(q) & 15) != 0) return fail(MDM_EINVAL, f + "weight pointers must be 16-byte aligned");
  }
  if (T != 0 && T < 4) return fail(MDM_EINVAL, f + "T must be at least 4 frames (one movement step)");
  if (T > (1 << 16) || L > (1 << 16)) return fail(MDM_EUNSUPPORTED, f + "at most 65536 frames / words");
  const int64_t Hm = m->motion.hidden, Ht = m->text.hidden;
  p.T1 = T / 2;                       // floor((T + 2 - 4) / 2) + 1
  p.T2 = p.T1 / 2;
  const int64_t mo = (int64_t)B * ((int64_t)p.T1 * m->conv_hidden + (int64_t)p.T2 * (2 * m->latent + 7 * Hm)) + 5 * (int64_t)B * Hm;
  const int64_t te = (int64_t)B * L * (m->word + 7 * Ht) + 5 * (int64_t)B * Ht;
  // (row counts and offsets inside the GEMMs are 32-bit)
  if ((int64_t)B * std::max(p.T2, L) * 6 * std::max(Hm, Ht) >= (1ll << 31) || (int64_t)B * std::max(T, L) * std::max(m->dim_pose, m->word) >= (1ll << 31))
    return fail(MDM_EUNSUPPORTED, f + "batch too large for one call: chunk the rows (a row's result does not depend on the batch)");
  p.motion = T ? (size_t)mo : 0;
  p.text = L ? (size_t)te : 0;
  return 0;
}

// (launch_gemm_f32_t<false>: the exact-fp32 arithmetic only -- the split-precision forms of these GEMMs are never instantiated)
int eval_linear(const float* in, const float* w, const float* b, float* out, int M, int N, int K, hipStream_t s) {
  RowMajorLoader al{in, K, M, K};
  RowMajorLoader bl{w, K, N, K};
  LeakyEpilogue ep{out, b, N, 0};
  launch_gemm_f32_t<false>(al, bl, ep, M, N, K, s, 0);
  return rt_launch_status();
}

// x [B Tp][g.hidden] (input_emb's output) -> out [B][g.out]: the input projections of all steps, the recurrence, output_net
int eval_gru_encode(const mdm_eval_gru_t& g, const float* emb, const int32_t* lens, int len_div, int max_len, float* gi, float* h,
                    float* o1, float* out, int B, int Tp, hipStream_t s) {
  const int H = g.hidden;
  if (int rc = eval_linear(emb, g.w_ih, g.b_ih, gi, B * Tp, 6 * H, H, s)) return rc;
  float* hb[2] = {h, h + (size_t)B * 2 * H};
  auto init_k = &gru_init_kernel;
  MDM_LAUNCH(init_k, dim3((unsigned)(((size_t)B * 2 * H + 255) / 256)), dim3(256), 0, s, hb[0], g.h0, B, H);
  if (int rc = rt_launch_status()) return rc;
  int steps = max_len > 0 ? std::min(max_len / len_div, Tp) : Tp;
  auto step_k = &gru_step_kernel;
  const dim3 grid(H / 32, (B + 31) / 32, 2);
  for (int st = 0; st < steps; ++st) {
    MDM_LAUNCH(step_k, grid, dim3(GRU_THREADS), 0, s, (const float*)gi, g.w_hh, g.b_hh, (const float*)hb[st & 1], hb[(st + 1) & 1], lens,
               len_div, B, Tp, H, st);
    if (int rc = rt_launch_status()) return rc;
  }
  const float* hl = hb[steps & 1];                      // [B][2H] = cat(gru_last[0], gru_last[1])
  if (int rc = eval_linear(hl, g.o1_w, g.o1_b, o1, B, H, 2 * H, s)) return rc;
  if (int rc = launch_layernorm(nullptr, o1, g.ln_g, g.ln_b, B, H, nullptr, nullptr, s)) return rc;
  LeakyRowLoader al{o1, H, B, H};
  RowMajorLoader bl{g.o2_w, H, g.out, H};
  LeakyEpilogue ep{out, g.o2_b, g.out, 0};
  launch_gemm_f32_t<false>(al, bl, ep, B, g.out, H, s, 0);
  return rt_launch_status();
}

float* eval_ws(void* ws) { return reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws) + 15) & ~(uintptr_t)15); }

}  // namespace

extern "C" {

size_t mdm_eval_workspace_bytes(const mdm_eval_model_t* model, int32_t B, int32_t T, int32_t L) {
  EvalPlan p;
  if (eval_plan("mdm_eval_workspace_bytes", model, B, T, L, p) != 0) return 0;
  return std::max(p.motion, p.text) * sizeof(float) + 64;
}

int mdm_eval_motion_embeddings(const mdm_eval_model_t* m, const float* motions, const int32_t* lens, float* out, int32_t B, int32_t T,
                               int32_t max_len, void* ws, size_t ws_bytes, void* stream) {
  const char* fn = "mdm_eval_motion_embeddings";
  EvalPlan p;
  if (int rc = eval_plan(fn, m, B, T, 0, p)) return rc;
  if (T < 4) return fail(MDM_EINVAL, "mdm_eval_motion_embeddings: T must be at least 4 frames (one movement step)");
  if (!motions || !lens || !out || !ws) return fail(MDM_EINVAL, "mdm_eval_motion_embeddings: null motions, lens, out or workspace");
  if (max_len < 0) return fail(MDM_EINVAL, "mdm_eval_motion_embeddings: max_len must be >= 0");
  if (ws_bytes < p.motion * sizeof(float) + 64) return fail(MDM_ENOSPC, "mdm_eval_motion_embeddings: workspace too small (mdm_eval_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int Hm = m->motion.hidden, C = m->dim_pose - 4, CH = m->conv_hidden, LAT = m->latent;
  float* c1 = eval_ws(ws);
  float* c2 = c1 + (size_t)B * p.T1 * CH;
  float* mv = c2 + (size_t)B * p.T2 * LAT;
  float* emb = mv + (size_t)B * p.T2 * LAT;
  float* gi = emb + (size_t)B * p.T2 * Hm;
  float* h = gi + (size_t)B * p.T2 * 6 * Hm;
  float* o1 = h + (size_t)4 * B * Hm;
  {
    Conv4GatherLoader al{motions, T, p.T1, m->dim_pose, C, B * p.T1};
    RowMajorLoader bl{m->conv1_w, 4 * C, CH, 4 * C};
    LeakyEpilogue ep{c1, m->conv1_b, CH, 1};
    launch_gemm_f32_t<false>(al, bl, ep, B * p.T1, CH, 4 * C, s, 0);
    if (int rc = rt_launch_status()) return rc;
  }
  {
    Conv4GatherLoader al{c1, p.T1, p.T2, CH, CH, B * p.T2};
    RowMajorLoader bl{m->conv2_w, 4 * CH, LAT, 4 * CH};
    LeakyEpilogue ep{c2, m->conv2_b, LAT, 1};
    launch_gemm_f32_t<false>(al, bl, ep, B * p.T2, LAT, 4 * CH, s, 0);
    if (int rc = rt_launch_status()) return rc;
  }
  if (int rc = eval_linear(c2, m->out_w, m->out_b, mv, B * p.T2, LAT, LAT, s)) return rc;
  if (int rc = eval_linear(mv, m->motion.in_w, m->motion.in_b, emb, B * p.T2, Hm, LAT, s)) return rc;
  return eval_gru_encode(m->motion, emb, lens, m->unit_length, max_len > 0 ? max_len : T, gi, h, o1, out, B, p.T2, s);
}

int mdm_eval_text_embeddings(const mdm_eval_model_t* m, const float* word_embs, const float* pos_ohot, const int32_t* cap_lens,
                             float* out, int32_t B, int32_t L, int32_t max_len, void* ws, size_t ws_bytes, void* stream) {
  const char* fn = "mdm_eval_text_embeddings";
  EvalPlan p;
  if (int rc = eval_plan(fn, m, B, 0, L, p)) return rc;
  if (L < 1) return fail(MDM_EINVAL, "mdm_eval_text_embeddings: L must be at least 1 word");
  if (!word_embs || !pos_ohot || !cap_lens || !out || !ws) return fail(MDM_EINVAL, "mdm_eval_text_embeddings: null input, out or workspace");
  if ((reinterpret_cast<uintptr_t>(word_embs) & 15) != 0) return fail(MDM_EINVAL, "mdm_eval_text_embeddings: word_embs must be 16-byte aligned");
  if (max_len < 0) return fail(MDM_EINVAL, "mdm_eval_text_embeddings: max_len must be >= 0");
  if (ws_bytes < p.text * sizeof(float) + 64) return fail(MDM_ENOSPC, "mdm_eval_text_embeddings: workspace too small (mdm_eval_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int Ht = m->text.hidden, W = m->word;
  float* inp = eval_ws(ws);
  float* emb = inp + (size_t)B * L * W;
  float* gi = emb + (size_t)B * L * Ht;
  float* h = gi + (size_t)B * L * 6 * Ht;
  float* o1 = h + (size_t)4 * B * Ht;
  {   // inputs = word_embs + pos_emb(pos_ohot)   (modules.py:338-339)
    ScalarRowLoader al{pos_ohot, m->pos, B * L, m->pos};
    ScalarRowLoader bl{m->pos_w, m->pos, W, m->pos};
    LinearEpilogue ep{inp, m->pos_b, word_embs, W, ACT_NONE, 0, 1.f, nullptr, nullptr};
    launch_gemm_f32_t<false>(al, bl, ep, B * L, W, m->pos, s, 0);
    if (int rc = rt_launch_status()) return rc;
  }
  if (int rc = eval_linear(inp, m->text.in_w, m->text.in_b, emb, B * L, Ht, W, s)) return rc;
  return eval_gru_encode(m->text, emb, cap_lens, 1, max_len > 0 ? max_len : L, gi, h, o1, out, B, L, s);
}

}  // extern "C"

namespace {

// Validation shared by mdm_text_workspace_bytes and mdm_text_encode; 0 or a negative code with the message set (it names the field)
int text_plan(const char* fn, const mdm_text_model_t* m, int B, int L, size_t& floats) {
  const std::string f = std::string(fn) + ": ";
  if (m == nullptr) return fail(MDM_EINVAL, f + "null model");
  if (B < 1) return fail(MDM_EINVAL, f + "B must be at least 1");
  if (L < 1) return fail(MDM_EINVAL, f + "L must be at least 1 word piece");
  if (L > TXT_MAX_L) return fail(MDM_EUNSUPPORTED, f + "L must be at most 128 word pieces (the attention kernel keeps 4 key tiles of 32)");
  if (m->max_pos < 1) return fail(MDM_EINVAL, f + "max_pos must be at least 1");
  if (L > m->max_pos) return fail(MDM_EINVAL, f + "L exceeds max_pos, the rows of the position table (" + std::to_string(m->max_pos) + ")");
  if (m->n_heads < 1 || m->dim != TXT_HD * m->n_heads) return fail(MDM_EUNSUPPORTED, f + "dim must equal 64 * n_heads (heads of 64)");
  if (m->dim > TXT_MAX_DIM) return fail(MDM_EUNSUPPORTED, f + "dim must be at most 1024 (the LayerNorm rows)");
  if (m->hidden < 4 || m->hidden % 4 != 0) return fail(MDM_EUNSUPPORTED, f + "hidden must be a positive multiple of 4");
  if (m->n_layers < 1 || m->n_layers > 16) return fail(MDM_EUNSUPPORTED, f + "n_layers must be between 1 and 16");
  if (m->vocab < 1) return fail(MDM_EINVAL, f + "vocab must be at least 1");
  if (!(m->ln_eps >= 0.f)) return fail(MDM_EINVAL, f + "ln_eps must be >= 0");
  auto check = [&](const float* q, const std::string& name) {
    if (q == nullptr) return fail(MDM_EINVAL, f + "null weight pointer " + name);
    if ((reinterpret_cast<uintptr_t>(q) & 15) != 0) return fail(MDM_EINVAL, f + "weight pointer " + name + " must be 16-byte aligned");
    return 0;
  };
  const float* top[] = {m->word_emb, m->pos_emb, m->emb_ln_g, m->emb_ln_b};
  const char* top_names[] = {"word_emb", "pos_emb", "emb_ln_g", "emb_ln_b"};
  for (int i = 0; i < 4; ++i)
    if (int rc = check(top[i], top_names[i])) return rc;
  if (m->layers == nullptr) return fail(MDM_EINVAL, f + "null layers");
  static const char* layer_names[] = {"qkv_w", "qkv_b", "out_w", "out_b", "sa_ln_g", "sa_ln_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b", "out_ln_g", "out_ln_b"};
  for (int l = 0; l < m->n_layers; ++l) {
    const mdm_text_layer_t& y = m->layers[l];
    const float* ptrs[] = {y.qkv_w, y.qkv_b, y.out_w, y.out_b, y.sa_ln_g, y.sa_ln_b, y.lin1_w, y.lin1_b, y.lin2_w, y.lin2_b, y.out_ln_g, y.out_ln_b};
    for (int i = 0; i < 12; ++i)
      if (int rc = check(ptrs[i], "layers[" + std::to_string(l) + "]." + layer_names[i])) return rc;
  }
  // (row counts and offsets inside the GEMMs are 32-bit)
  if ((int64_t)B * L * std::max<int64_t>(3 * (int64_t)m->dim, m->hidden) >= (1ll << 31))
    return fail(MDM_EUNSUPPORTED, f + "B too large for one call: chunk the prompts (a row's result does not depend on the batch)");
  floats = (size_t)B * L * (5 * (size_t)m->dim + m->hidden);
  return 0;
}

// One dense layer of the encoder on gemm_f32.h's exact-fp32 kernel.  launch_gemm_f32_t sends an output of fewer than 64 x 64 x 4
// elements to its 128-row tiles: a one-prompt call's out_lin and lin2 (12 x 768) would be 6 workgroups walking K = 768 / 3072 alone,
// 138 us a launch and 80 % of the call (profiles/r14a_text_encoder.md).  Those go to the 64-row tiles here -- twice the workgroups;
// both tile shapes sum k in one order, so a row keeps its bits whichever one a batch size selects.
int text_linear(const float* in, const float* w, const float* bias, const float* res, float* out, int M, int N, int K, int act,
                hipStream_t s) {
  if ((size_t)M * N >= 64 * 64 * 4) return launch_linear(nullptr, in, K, w, bias, res, out, M, N, K, act, 0, 1.f, s);
  RowMajorLoader al{in, K, M, K};
  RowMajorLoader bl{w, K, N, K};
  LinearEpilogue ep{out, bias, res, N, act, 0, 1.f, nullptr, nullptr};
  const int tm = (M + 63) / 64, tn = (N + 63) / 64;
  auto kfn = &gemm_f32_kernel<RowMajorLoader, RowMajorLoader, LinearEpilogue, 64, false, 1>;
  MDM_LAUNCH(kfn, dim3(tm * tn), dim3(GEMM_THREADS), gemm_f32_lds_total(64, false), s, al, bl, ep, M, N, K, tn, 0);
  return rt_launch_status();
}

int text_ln(TextLnArgs a, hipStream_t s) {
  auto k = &text_ln_kernel;
  MDM_LAUNCH(k, dim3((unsigned)((a.B * a.L + 3) / 4)), dim3(256), 0, s, a);
  return rt_launch_status();
}

}  // namespace

extern "C" {

size_t mdm_text_workspace_bytes(const mdm_text_model_t* model, int32_t B, int32_t L) {
  size_t floats = 0;
  if (text_plan("mdm_text_workspace_bytes", model, B, L, floats) != 0) return 0;
  return floats * sizeof(float) + 64;
}

int mdm_text_encode(const mdm_text_model_t* m, const int32_t* ids, const int32_t* lens, float* out, int32_t B, int32_t L,
                    int32_t token_major, void* ws, size_t ws_bytes, void* stream) {
  size_t floats = 0;
  if (int rc = text_plan("mdm_text_encode", m, B, L, floats)) return rc;
  if (!ids || !lens || !out || !ws) return fail(MDM_EINVAL, "mdm_text_encode: null ids_dev, lens_dev, out_dev or workspace_dev");
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return fail(MDM_EINVAL, "mdm_text_encode: out_dev must be 16-byte aligned");
  if (ws_bytes < floats * sizeof(float) + 64) return fail(MDM_ENOSPC, "mdm_text_encode: workspace_bytes too small (mdm_text_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int D = m->dim, H = m->n_heads, FF = m->hidden, M = B * L;
  float* x = eval_ws(ws);                      // [M][D] the token rows (residual stream)
  float* qkv = x + (size_t)M * D;              // [M][3D]
  float* ctx = qkv + (size_t)M * 3 * D;        // [M][D]
  float* ffn = ctx + (size_t)M * D;            // [M][FF]
  TextLnArgs ln{nullptr, ids, m->word_emb, m->pos_emb, m->emb_ln_g, m->emb_ln_b, lens, x, B, L, D, m->vocab, m->ln_eps, 0};
  if (int rc = text_ln(ln, s)) return rc;
  ln.ids = nullptr;
  ln.in = x;
  auto attn_k = &text_attn_kernel<false>;
  const int nqt = (L + 31) / 32;
  for (int l = 0; l < m->n_layers; ++l) {
    const mdm_text_layer_t& y = m->layers[l];
    const bool last = l + 1 == m->n_layers;
    if (int rc = text_linear(x, y.qkv_w, y.qkv_b, nullptr, qkv, M, 3 * D, D, ACT_NONE, s)) return rc;
    MDM_LAUNCH(attn_k, dim3((unsigned)(B * H * nqt)), dim3(64), text_attn_lds_bytes(L), s, (const float*)qkv, lens, ctx, (int)L, D, H);
    if (int rc = rt_launch_status()) return rc;
    if (int rc = text_linear(ctx, y.out_w, y.out_b, x, x, M, D, D, ACT_NONE, s)) return rc;    // + x, in place
    ln.gamma = y.sa_ln_g; ln.beta = y.sa_ln_b; ln.out = x; ln.token_major = 0;
    if (int rc = text_ln(ln, s)) return rc;
    if (int rc = text_linear(x, y.lin1_w, y.lin1_b, nullptr, ffn, M, FF, D, ACT_GELU, s)) return rc;
    if (int rc = text_linear(ffn, y.lin2_w, y.lin2_b, x, x, M, D, FF, ACT_NONE, s)) return rc;   // + x, in place
    ln.gamma = y.out_ln_g; ln.beta = y.out_ln_b; ln.out = last ? out : x; ln.token_major = last ? (token_major != 0) : 0;
    if (int rc = text_ln(ln, s)) return rc;
  }
  return MDM_OK;
}

}  // extern "C"

namespace {

// Validation shared by mdm_clip_text_workspace_bytes and mdm_clip_text_encode; 0 or a negative code with the message set (it names the field)
int clip_text_plan(const char* fn, const mdm_clip_text_model_t* m, int B, int L, size_t& floats) {
  const std::string f = std::string(fn) + ": ";
  if (m == nullptr) return fail(MDM_EINVAL, f + "null model");
  if (B < 1) return fail(MDM_EINVAL, f + "B must be at least 1");
  if (L < 1) return fail(MDM_EINVAL, f + "L must be at least 1 token");
  if (L > TXT_MAX_L) return fail(MDM_EUNSUPPORTED, f + "L must be at most 128 tokens (the attention kernel keeps 4 key tiles of 32)");
  if (m->max_pos < 1) return fail(MDM_EINVAL, f + "max_pos must be at least 1");
  if (L > m->max_pos) return fail(MDM_EINVAL, f + "L exceeds max_pos, the rows of the position table (" + std::to_string(m->max_pos) + ")");
  if (m->n_heads < 1 || m->dim != TXT_HD * m->n_heads) return fail(MDM_EUNSUPPORTED, f + "dim must equal 64 * n_heads (heads of 64)");
  if (m->dim > TXT_MAX_DIM) return fail(MDM_EUNSUPPORTED, f + "dim must be at most 1024 (the LayerNorm rows)");
  if (m->mlp < 4 || m->mlp % 4 != 0) return fail(MDM_EUNSUPPORTED, f + "mlp must be a positive multiple of 4");
  if (m->embed < 4 || m->embed % 4 != 0) return fail(MDM_EUNSUPPORTED, f + "embed must be a positive multiple of 4");
  if (m->n_layers < 1 || m->n_layers > 32) return fail(MDM_EUNSUPPORTED, f + "n_layers must be between 1 and 32");
  if (m->vocab < 1) return fail(MDM_EINVAL, f + "vocab must be at least 1");
  auto check = [&](const float* q, const std::string& name) {
    if (q == nullptr) return fail(MDM_EINVAL, f + "null weight pointer " + name);
    if ((reinterpret_cast<uintptr_t>(q) & 15) != 0) return fail(MDM_EINVAL, f + "weight pointer " + name + " must be 16-byte aligned");
    return 0;
  };
  const float* top[] = {m->tok_emb, m->pos_emb, m->lnf_g, m->lnf_b, m->text_proj};
  const char* top_names[] = {"tok_emb", "pos_emb", "lnf_g", "lnf_b", "text_proj"};
  for (int i = 0; i < 5; ++i)
    if (int rc = check(top[i], top_names[i])) return rc;
  if (m->layers == nullptr) return fail(MDM_EINVAL, f + "null layers");
  static const char* layer_names[] = {"ln1_g", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_g", "ln2_b", "fc_w", "fc_b", "proj_w", "proj_b"};
  for (int l = 0; l < m->n_layers; ++l) {
    const mdm_clip_text_layer_t& y = m->layers[l];
    const float* ptrs[] = {y.ln1_g, y.ln1_b, y.qkv_w, y.qkv_b, y.out_w, y.out_b, y.ln2_g, y.ln2_b, y.fc_w, y.fc_b, y.proj_w, y.proj_b};
    for (int i = 0; i < 12; ++i)
      if (int rc = check(ptrs[i], "layers[" + std::to_string(l) + "]." + layer_names[i])) return rc;
  }
  // (row counts and offsets inside the GEMMs are 32-bit)
  if ((int64_t)B * L * std::max<int64_t>(3 * (int64_t)m->dim, m->mlp) >= (1ll << 31) || (int64_t)B * m->embed >= (1ll << 31))
    return fail(MDM_EUNSUPPORTED, f + "B too large for one call: chunk the prompts (a row's result does not depend on the batch)");
  floats = (size_t)B * L * (6 * (size_t)m->dim + m->mlp) + (size_t)B * m->dim;
  return 0;
}

}  // namespace

extern "C" {

size_t mdm_clip_text_workspace_bytes(const mdm_clip_text_model_t* model, int32_t B, int32_t L) {
  size_t floats = 0;
  if (clip_text_plan("mdm_clip_text_workspace_bytes", model, B, L, floats) != 0) return 0;
  return floats * sizeof(float) + 64;
}

int mdm_clip_text_encode(const mdm_clip_text_model_t* m, const int32_t* ids, const int32_t* lens, float* out, int32_t B, int32_t L,
                         void* ws, size_t ws_bytes, void* stream) {
  size_t floats = 0;
  if (int rc = clip_text_plan("mdm_clip_text_encode", m, B, L, floats)) return rc;
  if (!ids || !lens || !out || !ws) return fail(MDM_EINVAL, "mdm_clip_text_encode: null ids_dev, lens_dev, out_dev or workspace_dev");
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return fail(MDM_EINVAL, "mdm_clip_text_encode: out_dev must be 16-byte aligned");
  if (ws_bytes < floats * sizeof(float) + 64) return fail(MDM_ENOSPC, "mdm_clip_text_encode: workspace_bytes too small (mdm_clip_text_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int D = m->dim, H = m->n_heads, FF = m->mlp, M = B * L;
  float* x = eval_ws(ws);                      // [M][D] the residual stream
  float* xn = x + (size_t)M * D;               // [M][D] ln_1(x) / ln_2(x)
  float* qkv = xn + (size_t)M * D;             // [M][3D]
  float* ctx = qkv + (size_t)M * 3 * D;        // [M][D]
  float* ffn = ctx + (size_t)M * D;            // [M][FF]
  float* eot = ffn + (size_t)M * FF;           // [B][D] ln_final of the EOT rows
  auto embed_k = &clip_embed_kernel;
  MDM_LAUNCH(embed_k, dim3((unsigned)((M * (D / 4) + 255) / 256)), dim3(256), 0, s, ids, lens, m->tok_emb, m->pos_emb, x, (int)B, (int)L, D,
             (int)m->vocab);
  if (int rc = rt_launch_status()) return rc;
  TextLnArgs ln{x, nullptr, nullptr, nullptr, nullptr, nullptr, lens, xn, B, L, D, 0, CLIP_LN_EPS, 0};
  auto attn_k = &text_attn_kernel<true>;
  const int nqt = (L + 31) / 32;
  for (int l = 0; l < m->n_layers; ++l) {
    const mdm_clip_text_layer_t& y = m->layers[l];
    ln.gamma = y.ln1_g; ln.beta = y.ln1_b;
    if (int rc = text_ln(ln, s)) return rc;
    if (int rc = text_linear(xn, y.qkv_w, y.qkv_b, nullptr, qkv, M, 3 * D, D, ACT_NONE, s)) return rc;
    MDM_LAUNCH(attn_k, dim3((unsigned)(B * H * nqt)), dim3(64), text_attn_lds_bytes(L), s, (const float*)qkv, lens, ctx, (int)L, D, H);
    if (int rc = rt_launch_status()) return rc;
    if (int rc = text_linear(ctx, y.out_w, y.out_b, x, x, M, D, D, ACT_NONE, s)) return rc;      // + x, in place
    ln.gamma = y.ln2_g; ln.beta = y.ln2_b;
    if (int rc = text_ln(ln, s)) return rc;
    if (int rc = text_linear(xn, y.fc_w, y.fc_b, nullptr, ffn, M, FF, D, ACT_QGELU, s)) return rc;
    if (int rc = text_linear(ffn, y.proj_w, y.proj_b, x, x, M, D, FF, ACT_NONE, s)) return rc;   // + x, in place
  }
  auto eot_k = &clip_eot_ln_kernel;
  MDM_LAUNCH(eot_k, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, (const float*)x, lens, m->lnf_g, m->lnf_b, eot, (int)B, (int)L, D);
  if (int rc = rt_launch_status()) return rc;
  return text_linear(eot, m->text_proj, nullptr, nullptr, out, B, m->embed, D, ACT_NONE, s);
}

}  // extern "C"

namespace {

struct StgcnPlan {
  int Cp;                                    // the input's channels rounded up to a multiple of 4
  int Tin[MDM_STGCN_MAX_BLOCKS + 1];         // frames in front of block b; [n_blocks] = behind the last one
  size_t buf;                                // floats per workspace buffer (three of them)
};

// Validation shared by mdm_stgcn_workspace_bytes and mdm_stgcn_forward; 0 or a negative code with the message set (it names the field)
int stgcn_plan(const char* fn, const mdm_stgcn_model_t* m, int N, int T, StgcnPlan& p) {
  const std::string f = std::string(fn) + ": ";
  if (m == nullptr) return fail(MDM_EINVAL, f + "null model");
  if (N < 1) return fail(MDM_EINVAL, f + "N must be at least 1");
  if (T < 1) return fail(MDM_EINVAL, f + "T must be at least 1 frame");
  if (T > (1 << 16)) return fail(MDM_EUNSUPPORTED, f + "T must be at most 65536 frames");
  if (m->n_blocks < 1 || m->n_blocks > MDM_STGCN_MAX_BLOCKS) return fail(MDM_EUNSUPPORTED, f + "n_blocks must be between 1 and 16");
  if (m->V < 1 || m->V > 64) return fail(MDM_EUNSUPPORTED, f + "V must be between 1 and 64 nodes");
  if (m->K < 1 || m->K > 8) return fail(MDM_EUNSUPPORTED, f + "K must be between 1 and 8 graph kernels");
  if (m->num_class < 1) return fail(MDM_EINVAL, f + "num_class must be at least 1");
  if (m->blocks == nullptr) return fail(MDM_EINVAL, f + "null blocks");
  auto check = [&](const void* q, const std::string& name) {
    if (q == nullptr) return fail(MDM_EINVAL, f + "null weight pointer " + name);
    if ((reinterpret_cast<uintptr_t>(q) & 15) != 0) return fail(MDM_EINVAL, f + "weight pointer " + name + " must be 16-byte aligned");
    return 0;
  };
  const void* top[] = {m->in_scale, m->in_shift, m->fcn_w, m->fcn_b};
  const char* top_names[] = {"in_scale", "in_shift", "fcn_w", "fcn_b"};
  for (int i = 0; i < 4; ++i)
    if (int rc = check(top[i], top_names[i])) return rc;
  if (m->blocks[0].c_in < 1) return fail(MDM_EINVAL, f + "blocks[0].c_in must be at least 1 channel");
  p.Cp = (m->blocks[0].c_in + 3) & ~3;
  int64_t rows = (int64_t)N * T * m->V, widest = rows * p.Cp;
  p.Tin[0] = T;
  int c_prev = p.Cp;
  static const char* names[] = {"gcn_w", "gcn_scale", "gcn_shift", "nbr_idx", "nbr_w", "nbr_cnt", "tcn_w", "tcn_scale", "tcn_shift",
                                "res_w", "res_scale", "res_shift"};
  for (int b = 0; b < m->n_blocks; ++b) {
    const mdm_stgcn_block_t& k = m->blocks[b];
    const std::string w = "blocks[" + std::to_string(b) + "].";
    if (b > 0 && k.c_in != m->blocks[b - 1].c_out) return fail(MDM_EINVAL, f + w + "c_in must equal the c_out of the block in front of it");
    if (k.c_out < 4 || k.c_out % 4 != 0) return fail(MDM_EUNSUPPORTED, f + w + "c_out must be a positive multiple of 4");
    if (k.stride < 1 || k.stride > 4) return fail(MDM_EUNSUPPORTED, f + w + "stride must be between 1 and 4");
    if (k.residual < MDM_STGCN_RES_NONE || k.residual > MDM_STGCN_RES_CONV) return fail(MDM_EINVAL, f + w + "residual must be one of MDM_STGCN_RES_*");
    if (k.residual == MDM_STGCN_RES_IDENTITY && (c_prev != k.c_out || k.stride != 1))
      return fail(MDM_EINVAL, f + w + "an identity residual needs c_in == c_out and stride 1");
    const void* ptrs[] = {k.gcn_w, k.gcn_scale, k.gcn_shift, k.nbr_idx, k.nbr_w, k.nbr_cnt, k.tcn_w, k.tcn_scale, k.tcn_shift,
                          k.res_w, k.res_scale, k.res_shift};
    for (int i = 0; i < (k.residual == MDM_STGCN_RES_CONV ? 12 : 9); ++i)
      if (int rc = check(ptrs[i], w + names[i])) return rc;
    widest = std::max(widest, rows * k.c_out);      // the graph convolution's output: the block's input rows
    p.Tin[b + 1] = (p.Tin[b] - 1) / k.stride + 1;
    rows = (int64_t)N * p.Tin[b + 1] * m->V;
    c_prev = k.c_out;
  }
  if (c_prev > STGCN_MAX_POOL_C) return fail(MDM_EUNSUPPORTED, f + "the last block's c_out must be at most 1024 (the pooling kernel's row)");
  // (row counts and offsets inside the GEMMs are 32-bit)
  if (widest >= (1ll << 31)) return fail(MDM_EUNSUPPORTED, f + "N too large for one call: chunk the samples (a sample's result does not depend on the batch)");
  p.buf = (size_t)widest;
  return 0;
}

// One GEMM of the net: always the 64-row tile (launch_gemm_f32_t's size rule would let the batch choose the tile shape)
template <class AL>
int stgcn_gemm(const AL& al, const float* w, const StgcnEpilogue& ep, int M, int N, int K, hipStream_t s) {
  RowMajorLoader bl{w, K, N, K};
  const int tm = (M + 63) / 64, tn = (N + 63) / 64;
  auto kfn = &gemm_f32_kernel<AL, RowMajorLoader, StgcnEpilogue, 64, false, 1>;
  MDM_LAUNCH(kfn, dim3(tm * tn), dim3(GEMM_THREADS), gemm_f32_lds_total(64, false), s, al, bl, ep, M, N, K, tn, 0);
  return rt_launch_status();
}

}  // namespace

extern "C" {

size_t mdm_stgcn_workspace_bytes(const mdm_stgcn_model_t* model, int32_t N, int32_t T) {
  StgcnPlan p;
  if (stgcn_plan("mdm_stgcn_workspace_bytes", model, N, T, p) != 0) return 0;
  return 3 * p.buf * sizeof(float) + 64;
}

int mdm_stgcn_forward(const mdm_stgcn_model_t* m, const float* x, float* features, float* yhat, int32_t N, int32_t T, void* ws,
                      size_t ws_bytes, void* stream) {
  StgcnPlan p;
  if (int rc = stgcn_plan("mdm_stgcn_forward", m, N, T, p)) return rc;
  if (!x || !features || !yhat || !ws) return fail(MDM_EINVAL, "mdm_stgcn_forward: null x_dev, features_dev, yhat_dev or workspace_dev");
  if ((reinterpret_cast<uintptr_t>(features) & 15) != 0) return fail(MDM_EINVAL, "mdm_stgcn_forward: features_dev must be 16-byte aligned");
  if (ws_bytes < 3 * p.buf * sizeof(float) + 64) return fail(MDM_ENOSPC, "mdm_stgcn_forward: workspace_bytes too small (mdm_stgcn_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int V = m->V;
  float* cur = eval_ws(ws);                   // the block's input  [N Tin V][c_in]
  float* mid = cur + p.buf;                   // relu(BN(gcn))      [N Tin V][c_out]
  float* nxt = mid + p.buf;                   // the block's output [N Tout V][c_out]
  {
    StgcnInputArgs a{x, m->in_scale, m->in_shift, cur, N, V, m->blocks[0].c_in, p.Cp, T};
    auto k = &stgcn_input_kernel;
    MDM_LAUNCH(k, dim3((unsigned)(((size_t)N * T * V * p.Cp + 255) / 256)), dim3(256), 0, s, a);
    if (int rc = rt_launch_status()) return rc;
  }
  int C = p.Cp;
  for (int b = 0; b < m->n_blocks; ++b) {
    const mdm_stgcn_block_t& k = m->blocks[b];
    const int Tin = p.Tin[b], Tout = p.Tin[b + 1], CO = k.c_out;
    const int Min = N * Tin * V, Mout = N * Tout * V;
    {
      GraphMixLoader al{cur, k.nbr_idx, k.nbr_w, k.nbr_cnt, V, C, m->K * C, Min};
      StgcnEpilogue ep{mid, k.gcn_scale, k.gcn_shift, nullptr, CO, V, 1};
      if (int rc = stgcn_gemm(al, k.gcn_w, ep, Min, CO, m->K * C, s)) return rc;
    }
    const float* res = nullptr;
    if (k.residual == MDM_STGCN_RES_IDENTITY) res = cur;
    if (k.residual == MDM_STGCN_RES_CONV) {
      StrideRowLoader al{cur, Tin, Tout, V, C, k.stride, Mout};
      StgcnEpilogue ep{nxt, k.res_scale, k.res_shift, nullptr, CO, 1, 0};
      if (int rc = stgcn_gemm(al, k.res_w, ep, Mout, CO, C, s)) return rc;
      res = nxt;                              // added in place by the temporal GEMM below
    }
    {
      Tap9GatherLoader al{mid, Tin, Tout, V, CO, k.stride, Mout};
      StgcnEpilogue ep{nxt, k.tcn_scale, k.tcn_shift, res, CO, 1, 1};
      if (int rc = stgcn_gemm(al, k.tcn_w, ep, Mout, CO, STGCN_TAPS * CO, s)) return rc;
    }
    std::swap(cur, nxt);
    C = CO;
  }
  StgcnTailArgs a{cur, m->fcn_w, m->fcn_b, features, yhat, p.Tin[m->n_blocks] * V, C, m->num_class};
  auto k = &stgcn_tail_kernel;
  MDM_LAUNCH(k, dim3((unsigned)N), dim3(256), 0, s, a);
  return rt_launch_status();
}

}  // extern "C"

#include "gru_recogniser_api.h"
