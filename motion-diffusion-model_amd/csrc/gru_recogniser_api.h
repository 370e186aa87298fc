// gru_recogniser_api.h -- part of the ONE translation unit csrc/mdm_api.hip: mdm_gru_cls_workspace_bytes / mdm_gru_cls_forward
// (include/mdm_hip.h) over the kernels of gru_recogniser.h.
#pragma once
// (included by mdm_api.hip behind its other entry points; relies on its includes, api_runtime.h and `using namespace mdm`)

namespace {

struct GruClsPlan {
  size_t gi, seq, hl;      // floats of the three workspace buffers
  size_t bytes() const { return ws_bytes_of(gi + seq + hl); }
};

// Validation shared by mdm_gru_cls_workspace_bytes and mdm_gru_cls_forward; 0 or a negative code with the message set
int gru_cls_plan(const char* fn, const mdm_gru_cls_model_t* m, int B, int T, GruClsPlan& p) {
  const std::string f = std::string(fn) + ": ";
  if (m == nullptr) return fail(MDM_EINVAL, f + "null model");
  if (B < 1) return fail(MDM_EINVAL, f + "B must be at least 1");
  if (T < 1) return fail(MDM_EINVAL, f + "T must be at least 1 frame");
  if (T > (1 << 16)) return fail(MDM_EUNSUPPORTED, f + "T must be at most 65536 frames");
  if (m->hidden_size != 128 && m->hidden_size != 32)
    return fail(MDM_EUNSUPPORTED, f + "hidden_size must be 128 (or 32, the reduced width): gru_seq_kernel has no other instantiation");
  if (m->num_layers < 1 || m->num_layers > MDM_GRU_CLS_MAX_LAYERS) return fail(MDM_EUNSUPPORTED, f + "num_layers must be between 1 and 4");
  if (m->input_size < 1) return fail(MDM_EINVAL, f + "input_size must be at least 1");
  if (m->mid < 1 || m->mid > GRU_TAIL_MAX) return fail(MDM_EUNSUPPORTED, f + "mid must be between 1 and 64");
  if (m->num_class < 1 || m->num_class > GRU_TAIL_MAX) return fail(MDM_EUNSUPPORTED, f + "num_class must be between 1 and 64");
  static const char* names[] = {"w_ih", "w_hh", "b_ih", "b_hh"};
  for (int l = 0; l < m->num_layers; ++l) {
    const mdm_gru_cls_layer_t& y = m->layers[l];
    const void* ptrs[] = {y.w_ih, y.w_hh, y.b_ih, y.b_hh};
    if (int rc = check_weight_ptrs(f, ptrs, names, 4, "layers[" + std::to_string(l) + "].")) return rc;
  }
  const void* top[] = {m->lin1_w, m->lin1_b, m->lin2_w, m->lin2_b};
  static const char* top_names[] = {"lin1_w", "lin1_b", "lin2_w", "lin2_b"};
  if (int rc = check_weight_ptrs(f, top, top_names, 4)) return rc;
  // (row counts and offsets inside the GEMM are 32-bit)
  const int64_t rows = (int64_t)B * T;
  if (rows * 3 * m->hidden_size >= (1ll << 31) || rows * m->input_size >= (1ll << 31))
    return fail(MDM_EUNSUPPORTED, f + "B too large for one call: chunk the rows (a row's result does not depend on the batch)");
  p.gi = (size_t)rows * 3 * m->hidden_size;
  p.seq = m->num_layers > 1 ? (size_t)rows * m->hidden_size : 0;
  p.hl = (size_t)B * m->hidden_size;
  return 0;
}

// gi = A W_ih^T + b_ih: always the 64-row tile (launch_gemm_f32_t's size rule would let the batch choose the tile shape)
template <class AL, class BL>
int gru_cls_gemm(const AL& al, const BL& bl, const float* bias, float* out, int M, int N, int K, hipStream_t s) {
  LeakyEpilogue ep{out, bias, N, 0};
  launch_gemm_f32_rows64(al, bl, ep, M, N, K, s);
  return rt_launch_status();
}

template <int H>
int gru_cls_seq(const GruSeqArgs& a, hipStream_t s) {
  auto kfn = &gru_seq_kernel<H>;
  MDM_LAUNCH(kfn, dim3((unsigned)((a.B + GRU_SEQ_ROWS - 1) / GRU_SEQ_ROWS)), dim3(H * 4), 0, s, a);
  return rt_launch_status();
}

}  // namespace

extern "C" {

size_t mdm_gru_cls_workspace_bytes(const mdm_gru_cls_model_t* model, int32_t B, int32_t T) {
  GruClsPlan p;
  if (gru_cls_plan("mdm_gru_cls_workspace_bytes", model, B, T, p) != 0) return 0;
  return p.bytes();
}

int mdm_gru_cls_forward(const mdm_gru_cls_model_t* m, const float* x, const int32_t* lens, const float* h0, float* features, float* yhat,
                        int32_t B, int32_t T, void* ws, size_t ws_bytes, void* stream) {
  const char* fn = "mdm_gru_cls_forward";
  GruClsPlan p;
  if (int rc = gru_cls_plan(fn, m, B, T, p)) return rc;
  if (!x || !lens || !h0 || !features || !yhat || !ws)
    return fail(MDM_EINVAL, "mdm_gru_cls_forward: null x_dev, lens_dev, h0_dev, features_dev, yhat_dev or workspace_dev");
  const void* io[] = {x, lens, h0, features, yhat};
  static const char* io_names[] = {"x_dev", "lens_dev", "h0_dev", "features_dev", "yhat_dev"};
  for (int i = 0; i < 5; ++i)
    if ((reinterpret_cast<uintptr_t>(io[i]) & 3) != 0)
      return fail(MDM_EINVAL, std::string(fn) + ": " + io_names[i] + " must be 4-byte aligned");
  if (ws_bytes < p.bytes()) return fail(MDM_ENOSPC, "mdm_gru_cls_forward: workspace_bytes too small (mdm_gru_cls_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int H = m->hidden_size, I = m->input_size, L = m->num_layers;
  float* gi = ws_floats(ws);          // [B T][3H]  the layer's input projections
  float* seq = gi + p.gi;           // [B][T][H]  the layer's outputs: read by the next layer's projection, then overwritten by its recurrence
  float* hl = seq + p.seq;          // [B][H]     the last layer's output at frame len_b - 1
  const int M = B * T;
  for (int l = 0; l < L; ++l) {
    const mdm_gru_cls_layer_t& y = m->layers[l];
    if (l == 0) {
      GruFrameLoader al{x, T, I, M};
      ScalarRowLoader bl{y.w_ih, I, 3 * H, I};
      if (int rc = gru_cls_gemm(al, bl, y.b_ih, gi, M, 3 * H, I, s)) return rc;
    } else {
      RowMajorLoader al{seq, H, M, H};
      RowMajorLoader bl{y.w_ih, H, 3 * H, H};
      if (int rc = gru_cls_gemm(al, bl, y.b_ih, gi, M, 3 * H, H, s)) return rc;
    }
    const bool last = l == L - 1;
    GruSeqArgs a{gi, y.w_hh, y.b_hh, h0 + (size_t)l * B * H, lens, last ? nullptr : seq, last ? hl : nullptr, B, T};
    if (int rc = H == 128 ? gru_cls_seq<128>(a, s) : gru_cls_seq<32>(a, s)) return rc;
  }
  GruTailArgs a{hl, m->lin1_w, m->lin1_b, m->lin2_w, m->lin2_b, features, yhat, H, m->mid, m->num_class};
  auto k = &gru_tail_kernel;
  MDM_LAUNCH(k, dim3((unsigned)B), dim3(64), 0, s, a);
  return rt_launch_status();
}

}  // extern "C"
