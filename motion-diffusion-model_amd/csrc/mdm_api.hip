// mdm_api.hip -- the ONE translation unit of libmdm_hip.so (the C ABI of include/mdm_hip.h): the native counterpart of MDM.forward
// (model/mdm.py:189-283), ClassifierFreeSampleModel.forward (utils/sampler_util.py:27-34) and GaussianDiffusion.p_sample_loop /
// ddim_sample_loop (diffusion/gaussian_diffusion.py:591-727, :876-990).  No torch, no allocation: caller-owned pointers.  This file: the
// includes, the ABI / build-info calls, the forward entry points, the sampler step and randn, the profiler calls and the unit entry points
// (mdm_linear*, mdm_layernorm, mdm_attention*).  Its parts: api_runtime.h, api_launch.h, model_setup.h, encoder.h, decoder.h, loops.h, *_api.h.
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
#include "motion_features.h"
#include "smpl_joints.h"
#include "smpl_mesh.h"
#include "evaluator.h"
#include "text_encoder.h"
#include "clip_text.h"
#include "stgcn.h"
#include "gru_recogniser.h"
#include "metrics.h"
#include "humanml_metrics.h"
#include "frechet.h"
#include "smplify.h"

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
         ";emu=" MDM_BUILD_INFO_EMU ";planes=f16";
}
const char* mdm_last_error(void) { return g_err.c_str(); }

#include "model_setup.h"

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

int mdm_profile_enable(mdm_model_t* m, int on) {
  if (m == nullptr) return fail(MDM_EINVAL, "mdm_profile_enable: null model");
  m->prof.on = on != 0;
  return MDM_OK;
}

int mdm_profile_read(mdm_model_t* m, int32_t category, double* total_ms, int64_t* launches, double* flops) {
  if (m == nullptr || category < 0 || category >= MDM_PROF_NUM) return fail(MDM_EINVAL, "mdm_profile_read: bad argument");
  double ms = 0.0, fl = 0.0;
  int64_t n = 0;
  if (int rc = m->prof.read(category, ms, n, fl)) return rc;
  if (total_ms) *total_ms = ms;
  if (launches) *launches = n;
  if (flops) *flops = fl;
  return MDM_OK;
}

int mdm_profile_reset(mdm_model_t* m) {
  if (m == nullptr) return fail(MDM_EINVAL, "mdm_profile_reset: null model");
  m->prof.reset();
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

}  // extern "C"

// The entry points that are not MDM's own, one file per model (each with its helpers in an anonymous namespace): the probe
// library's, then SMPL, joints to features, the HumanML3D evaluator, the two text encoders, ST-GCN, the GRU recogniser, the
// metrics of the unconstrained, the HumanML3D and the a2m evaluations, the Frechet distance, and the SMPLify fit.
#ifdef MDM_PROBES
#include "probe_api.h"
#endif
#include "smpl_api.h"
#include "motion_features_api.h"
#include "evaluator_api.h"
#include "text_api.h"
#include "stgcn_api.h"
#include "gru_recogniser_api.h"
#include "metrics_api.h"
#include "humanml_metrics_api.h"
#include "frechet_api.h"
#include "smplify_api.h"
