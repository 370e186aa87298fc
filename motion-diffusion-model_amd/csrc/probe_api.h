// probe_api.h -- part of the ONE translation unit csrc/mdm_api.hip: the entry points of include/mdm_hip_probe.h (libmdm_hip_probe.so
// and the emulator build only; mdm_api.hip includes this file under #ifdef MDM_PROBES).
#pragma once
// (included by mdm_api.hip behind its own entry points; relies on its includes, api_runtime.h and `using namespace mdm`)

extern "C" {

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
  // the timeline probes (common.h): stamp the value-th launch from now of gemm_x3s.h / xattn_block.h / selfattn_block.h (self and cross)
  if (what == 9) x3s_tl_sel() = TimelineSel{value, 0};
  if (what == 10) xb_tl_sel() = TimelineSel{value, 0};
  if (what == 11) sb_tl_sel() = TimelineSel{value, 0};
  return MDM_OK;
}

}  // extern "C"

// Stamp idx - BASE of one kernel's timeline array: read to the host once, at idx == BASE, then served from that copy.
template <int BASE, size_t N> static int timeline_get(const unsigned long long (&arr)[N], int idx, double* out) {
  static std::vector<unsigned long long> tl(N);
  if (idx - BASE >= (int)N || out == nullptr) return fail(MDM_EINVAL, "mdm_debug_get: bad timeline index");
  if (idx == BASE && !rt_timeline_read(tl.data(), arr, N)) return fail(MDM_EHIP, "mdm_debug_get: reading the timeline failed");
  *out = (double)tl[idx - BASE];
  return MDM_OK;
}

extern "C" {

int mdm_debug_get(int idx, double* out) {   // timeline stamps of the selfattn / xattn / x3s probes
  if (idx >= 300000) return timeline_get<300000>(g_sb_tl, idx, out);
  if (idx >= 200000) return timeline_get<200000>(g_xb_tl, idx, out);
  if (idx >= 100) return timeline_get<100>(g_x3s_tl, idx, out);
  return fail(MDM_EINVAL, "mdm_debug_get: not a timeline index");
}

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

}  // extern "C"
