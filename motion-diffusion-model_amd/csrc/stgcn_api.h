// stgcn_api.h -- part of the ONE translation unit csrc/mdm_api.hip: mdm_stgcn_workspace_bytes / mdm_stgcn_forward (include/mdm_hip.h) over the
// kernels of stgcn.h.
#pragma once
// (included by mdm_api.hip behind its own entry points; relies on its includes, api_runtime.h and `using namespace mdm`)

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
  const void* top[] = {m->in_scale, m->in_shift, m->fcn_w, m->fcn_b};
  static const char* top_names[] = {"in_scale", "in_shift", "fcn_w", "fcn_b"};
  if (int rc = check_weight_ptrs(f, top, top_names, 4)) return rc;
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
    if (int rc = check_weight_ptrs(f, ptrs, names, k.residual == MDM_STGCN_RES_CONV ? 12 : 9, w)) return rc;
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
  launch_gemm_f32_rows64(al, bl, ep, M, N, K, s);
  return rt_launch_status();
}

}  // namespace

extern "C" {

size_t mdm_stgcn_workspace_bytes(const mdm_stgcn_model_t* model, int32_t N, int32_t T) {
  StgcnPlan p;
  if (stgcn_plan("mdm_stgcn_workspace_bytes", model, N, T, p) != 0) return 0;
  return ws_bytes_of(3 * p.buf);
}

int mdm_stgcn_forward(const mdm_stgcn_model_t* m, const float* x, float* features, float* yhat, int32_t N, int32_t T, void* ws,
                      size_t ws_bytes, void* stream) {
  StgcnPlan p;
  if (int rc = stgcn_plan("mdm_stgcn_forward", m, N, T, p)) return rc;
  if (!x || !features || !yhat || !ws) return fail(MDM_EINVAL, "mdm_stgcn_forward: null x_dev, features_dev, yhat_dev or workspace_dev");
  if ((reinterpret_cast<uintptr_t>(features) & 15) != 0) return fail(MDM_EINVAL, "mdm_stgcn_forward: features_dev must be 16-byte aligned");
  if (ws_bytes < ws_bytes_of(3 * p.buf)) return fail(MDM_ENOSPC, "mdm_stgcn_forward: workspace_bytes too small (mdm_stgcn_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ChainGuard chain_guard(stream);
  const int V = m->V;
  float* cur = ws_floats(ws);                   // the block's input  [N Tin V][c_in]
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
