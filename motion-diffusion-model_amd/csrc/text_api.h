// text_api.h -- part of the ONE translation unit csrc/mdm_api.hip: mdm_text_workspace_bytes / mdm_text_encode over the kernels of
// text_encoder.h and mdm_clip_text_workspace_bytes / mdm_clip_text_encode over those of clip_text.h (include/mdm_hip.h).  One file:
// CLIP runs on text_linear, text_ln and text_attn_kernel.
#pragma once
// (included by mdm_api.hip behind its own entry points; relies on its includes, api_runtime.h and `using namespace mdm`)

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
  const void* top[] = {m->word_emb, m->pos_emb, m->emb_ln_g, m->emb_ln_b};
  static const char* top_names[] = {"word_emb", "pos_emb", "emb_ln_g", "emb_ln_b"};
  if (int rc = check_weight_ptrs(f, top, top_names, 4)) return rc;
  if (m->layers == nullptr) return fail(MDM_EINVAL, f + "null layers");
  static const char* layer_names[] = {"qkv_w", "qkv_b", "out_w", "out_b", "sa_ln_g", "sa_ln_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b", "out_ln_g", "out_ln_b"};
  for (int l = 0; l < m->n_layers; ++l) {
    const mdm_text_layer_t& y = m->layers[l];
    const void* ptrs[] = {y.qkv_w, y.qkv_b, y.out_w, y.out_b, y.sa_ln_g, y.sa_ln_b, y.lin1_w, y.lin1_b, y.lin2_w, y.lin2_b, y.out_ln_g, y.out_ln_b};
    if (int rc = check_weight_ptrs(f, ptrs, layer_names, 12, "layers[" + std::to_string(l) + "].")) return rc;
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
  launch_gemm_f32_rows64(al, bl, ep, M, N, K, s);
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
  return ws_bytes_of(floats);
}

int mdm_text_encode(const mdm_text_model_t* m, const int32_t* ids, const int32_t* lens, float* out, int32_t B, int32_t L,
                    int32_t token_major, void* ws, size_t ws_bytes, void* stream) {
  size_t floats = 0;
  if (int rc = text_plan("mdm_text_encode", m, B, L, floats)) return rc;
  if (!ids || !lens || !out || !ws) return fail(MDM_EINVAL, "mdm_text_encode: null ids_dev, lens_dev, out_dev or workspace_dev");
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return fail(MDM_EINVAL, "mdm_text_encode: out_dev must be 16-byte aligned");
  if (ws_bytes < ws_bytes_of(floats)) return fail(MDM_ENOSPC, "mdm_text_encode: workspace_bytes too small (mdm_text_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int D = m->dim, H = m->n_heads, FF = m->hidden, M = B * L;
  float* x = ws_floats(ws);                      // [M][D] the token rows (residual stream)
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

// ---- the CLIP text tower: pre-LN blocks, causal attention, the EOT row's projection ------------------------------------------------------
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
  const void* top[] = {m->tok_emb, m->pos_emb, m->lnf_g, m->lnf_b, m->text_proj};
  static const char* top_names[] = {"tok_emb", "pos_emb", "lnf_g", "lnf_b", "text_proj"};
  if (int rc = check_weight_ptrs(f, top, top_names, 5)) return rc;
  if (m->layers == nullptr) return fail(MDM_EINVAL, f + "null layers");
  static const char* layer_names[] = {"ln1_g", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_g", "ln2_b", "fc_w", "fc_b", "proj_w", "proj_b"};
  for (int l = 0; l < m->n_layers; ++l) {
    const mdm_clip_text_layer_t& y = m->layers[l];
    const void* ptrs[] = {y.ln1_g, y.ln1_b, y.qkv_w, y.qkv_b, y.out_w, y.out_b, y.ln2_g, y.ln2_b, y.fc_w, y.fc_b, y.proj_w, y.proj_b};
    if (int rc = check_weight_ptrs(f, ptrs, layer_names, 12, "layers[" + std::to_string(l) + "].")) return rc;
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
  return ws_bytes_of(floats);
}

int mdm_clip_text_encode(const mdm_clip_text_model_t* m, const int32_t* ids, const int32_t* lens, float* out, int32_t B, int32_t L,
                         void* ws, size_t ws_bytes, void* stream) {
  size_t floats = 0;
  if (int rc = clip_text_plan("mdm_clip_text_encode", m, B, L, floats)) return rc;
  if (!ids || !lens || !out || !ws) return fail(MDM_EINVAL, "mdm_clip_text_encode: null ids_dev, lens_dev, out_dev or workspace_dev");
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return fail(MDM_EINVAL, "mdm_clip_text_encode: out_dev must be 16-byte aligned");
  if (ws_bytes < ws_bytes_of(floats)) return fail(MDM_ENOSPC, "mdm_clip_text_encode: workspace_bytes too small (mdm_clip_text_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int D = m->dim, H = m->n_heads, FF = m->mlp, M = B * L;
  float* x = ws_floats(ws);                      // [M][D] the residual stream
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
