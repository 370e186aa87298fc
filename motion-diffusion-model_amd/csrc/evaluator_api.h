// evaluator_api.h -- part of the ONE translation unit csrc/mdm_api.hip: mdm_eval_workspace_bytes / mdm_eval_motion_embeddings /
// mdm_eval_text_embeddings (include/mdm_hip.h) over the kernels of evaluator.h.
#pragma once
// (included by mdm_api.hip behind its own entry points; relies on its includes, api_runtime.h and `using namespace mdm`)

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
}  // namespace

extern "C" {

size_t mdm_eval_workspace_bytes(const mdm_eval_model_t* model, int32_t B, int32_t T, int32_t L) {
  EvalPlan p;
  if (eval_plan("mdm_eval_workspace_bytes", model, B, T, L, p) != 0) return 0;
  return ws_bytes_of(std::max(p.motion, p.text));
}

int mdm_eval_motion_embeddings(const mdm_eval_model_t* m, const float* motions, const int32_t* lens, float* out, int32_t B, int32_t T,
                               int32_t max_len, void* ws, size_t ws_bytes, void* stream) {
  const char* fn = "mdm_eval_motion_embeddings";
  EvalPlan p;
  if (int rc = eval_plan(fn, m, B, T, 0, p)) return rc;
  if (T < 4) return fail(MDM_EINVAL, "mdm_eval_motion_embeddings: T must be at least 4 frames (one movement step)");
  if (!motions || !lens || !out || !ws) return fail(MDM_EINVAL, "mdm_eval_motion_embeddings: null motions, lens, out or workspace");
  if (max_len < 0) return fail(MDM_EINVAL, "mdm_eval_motion_embeddings: max_len must be >= 0");
  if (ws_bytes < ws_bytes_of(p.motion)) return fail(MDM_ENOSPC, "mdm_eval_motion_embeddings: workspace too small (mdm_eval_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int Hm = m->motion.hidden, C = m->dim_pose - 4, CH = m->conv_hidden, LAT = m->latent;
  float* c1 = ws_floats(ws);
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
  if (ws_bytes < ws_bytes_of(p.text)) return fail(MDM_ENOSPC, "mdm_eval_text_embeddings: workspace too small (mdm_eval_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int Ht = m->text.hidden, W = m->word;
  float* inp = ws_floats(ws);
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
