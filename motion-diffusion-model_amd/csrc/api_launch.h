// api_launch.h -- part of the ONE translation unit csrc/mdm_api.hip (the C ABI of libmdm_hip.so); split out of it in round 6
// (source health, no behaviour change).  The encoder workspace and the launchers of the building-block kernels (LayerNorm, attention, the GEMM families).
#pragma once

namespace {

struct Workspace {
  float *tok, *qkv, *att, *ffn, *cond;
  QkvPlanes qp;         // f16x3 mode: the in_proj epilogue writes Q/K/V^T planes over the qkv region
  p16_t *xah, *xal;    // folded-LayerNorm mode: planes of the post-attention pre-norm sum (alias tok)
  float *stat1, *stat2; // folded-LayerNorm mode: per-row partial (sum, sum^2) of xa / of tokh|tokl
  p16_t *tokh, *tokl;  // split planes of tok (f16x3 mode)
  p16_t *atth, *attl;  // alias att: the attention output is only consumed by the out_proj GEMM
  p16_t *ffnh, *ffnl;  // alias ffn: the GELU output is only consumed by the linear2 GEMM
  size_t bytes;
};

// The six operand planes of attention_x3.h over a qkv region of nseq * SP * 3 D floats (SP: S rounded up to whole 32-key tiles)
QkvPlanes carve_qkv_planes(float* qkv, size_t nseq, size_t S, size_t D, int H) {
  const size_t NKT = (S + 31) / 32, SP = 32 * NKT, plane = nseq * SP * D;
  p16_t* q = reinterpret_cast<p16_t*>(qkv);
  QkvPlanes qp{};
  qp.qh = q; qp.SP = (int)SP; qp.NKT = (int)NKT; qp.H = H;
  if (q != nullptr) { qp.ql = q + plane; qp.kh = q + 2 * plane; qp.kl = q + 3 * plane; qp.vh = q + 4 * plane; qp.vl = q + 5 * plane; }
  return qp;
}

Workspace carve(const mdm_model* m, int nseq, int T, void* base) {
  const size_t D = m->cfg.latent_dim, FF = m->cfg.ff_size, S = (size_t)T + 1, M = (size_t)nseq * S;
  size_t off = 0;
  auto take = [&](size_t floats) {
    size_t o = off;
    off += align_up(floats * sizeof(float), 256);
    return base ? reinterpret_cast<float*>(static_cast<char*>(base) + o) : nullptr;
  };
  Workspace w;
  w.tok = take(M * D);
  const size_t NKT = (S + 31) / 32, SP = 32 * NKT;
  w.qkv = take((size_t)nseq * SP * 3 * D);  // fp32 [M][3D] (f32 mode) or six 16-bit planes of nseq*SP*D (f16x3 mode)
  w.att = take(M * D);
  // (at least jf_k floats per row: embed_frames_x3 parks the two pose planes [B*T][jf_k] here, and with ff_size < jf_k = 288 an
  // unguided forward -- nseq = B -- overran the region into ws.cond, which the same launch reads)
  w.ffn = take(M * std::max(FF, (size_t)m->jf_k));
  w.cond = take((size_t)nseq * D);
  float* tp = take(M * D);  // two 16-bit planes = one fp32 array's worth of bytes
  w.tokh = reinterpret_cast<p16_t*>(tp);
  w.tokl = tp ? w.tokh + M * D : nullptr;
  w.atth = reinterpret_cast<p16_t*>(w.att);
  w.attl = w.att ? w.atth + M * D : nullptr;
  w.ffnh = reinterpret_cast<p16_t*>(w.ffn);
  w.ffnl = w.ffn ? w.ffnh + M * FF : nullptr;
  w.xah = reinterpret_cast<p16_t*>(w.tok);
  w.xal = w.tok ? w.xah + M * D : nullptr;
  const size_t parts = (D + 127) / 128;   // per-row partial statistics: per 256 columns (gemm_x3.h) or per 128 (gemm_x3s.h)
  w.stat1 = take(M * parts * 2 + 4);   // (+ 16 bytes: gemm_x3.h stats_dma's last unit of a tile that starts 8-byte aligned)
  w.stat2 = take(M * parts * 2 + 4);
  w.qp = carve_qkv_planes(w.qkv, nseq, S, D, m->cfg.num_heads);
  w.bytes = off;
  return w;
}

int launch_layernorm(Profiler* pf, float* x, const float* g, const float* b, int rows, int D, p16_t* xh, p16_t* xl,
                     hipStream_t s, bool write_f32 = true) {
  ProfScope ps(pf, MDM_PROF_LAYERNORM, 0.0, s);
  const dim3 grid((rows + 3) / 4), block(256);
  switch (D / 256) {
    case 1: { auto k = &layernorm_kernel<1>; MDM_LAUNCH(k, grid, block, 0, s, x, g, b, rows, 1e-5f, xh, xl, (int)write_f32); break; }
    case 2: { auto k = &layernorm_kernel<2>; MDM_LAUNCH(k, grid, block, 0, s, x, g, b, rows, 1e-5f, xh, xl, (int)write_f32); break; }
    case 3: { auto k = &layernorm_kernel<3>; MDM_LAUNCH(k, grid, block, 0, s, x, g, b, rows, 1e-5f, xh, xl, (int)write_f32); break; }
    case 4: { auto k = &layernorm_kernel<4>; MDM_LAUNCH(k, grid, block, 0, s, x, g, b, rows, 1e-5f, xh, xl, (int)write_f32); break; }
    default: return fail(MDM_EUNSUPPORTED, "layernorm: D must be 256, 512, 768 or 1024");
  }
  return rt_launch_status();
}

template <int NKT>
int launch_attention_t(const AttnF32Args& a, float* out, int nseq, int D, int H, p16_t* oh, p16_t* ol, hipStream_t s) {
  auto k = &attention_f32_kernel<NKT>;
  const int nqt = (a.Sq + 31) / 32;
  const size_t lds = attention_lds_bytes(NKT, nqt);
  if (int rc = rt_allow_lds(k, lds)) return rc;
  MDM_LAUNCH(k, dim3(nseq * H), dim3(64 * nqt), lds, s, a, out, D, H, oh, ol);
  return rt_launch_status();
}

// exact-fp32 attention with separate query / key-value sources (attention_f32.h AttnF32Args)
int launch_attention_args(Profiler* pf, const AttnF32Args& a, float* out, int nseq, int D, int H, p16_t* oh, p16_t* ol,
                          hipStream_t s) {
  ProfScope ps(pf, MDM_PROF_ATTENTION, 4.0 * nseq * H * (double)a.Sq * a.Sk * ATT_HD, s);
  if (D != H * ATT_HD) return fail(MDM_EUNSUPPORTED, "attention: head_dim must be 128");
  if (a.Sq < 1 || a.Sk < 1) return fail(MDM_EUNSUPPORTED, "attention: no tokens");
  if (a.Sq > 224 || a.Sk > 224) {   // streaming softmax over 32-key tiles (attention_long.h): any length
    const int nqb = al_query_blocks(a.Sq);
    MDM_LAUNCH(attention_f32_long_kernel, dim3(nseq * H * nqb), dim3(256), al_f32_lds_bytes(), s, a, out, D, H, oh, ol, nqb);
    return rt_launch_status();
  }
  switch ((a.Sk + 31) / 32) {
    case 1: return launch_attention_t<1>(a, out, nseq, D, H, oh, ol, s);
    case 2: return launch_attention_t<2>(a, out, nseq, D, H, oh, ol, s);
    case 3: return launch_attention_t<3>(a, out, nseq, D, H, oh, ol, s);
    case 4: return launch_attention_t<4>(a, out, nseq, D, H, oh, ol, s);
    case 5: return launch_attention_t<5>(a, out, nseq, D, H, oh, ol, s);
    case 6: return launch_attention_t<6>(a, out, nseq, D, H, oh, ol, s);
    default: return launch_attention_t<7>(a, out, nseq, D, H, oh, ol, s);
  }
}

// self-attention over packed qkv rows [nseq*S][3D]; `lead` tokens in front of the frames are never masked
int launch_attention(Profiler* pf, const float* qkv, float* out, const int* lengths, int nseq, int B, int S, int D,
                     int H, p16_t* oh, p16_t* ol, hipStream_t s, int lead = 1, int len_B = 0, int len_b0 = 0) {
  AttnF32Args a{qkv, 3 * D, qkv + D, qkv + 2 * D, 3 * D, S, S, lengths, lead, B};
  a.len_B = len_B;     // `lengths` covers len_B samples, this launch samples len_b0 .. len_b0 + B - 1 of them (0: exactly B)
  a.len_b0 = len_b0;
  return launch_attention_args(pf, a, out, nseq, D, H, oh, ol, s);
}

template <int NKT, bool DIRECT>
int launch_attention_x3_t(const QkvPlanes& qp, const int* lengths, int nseq, int B, int S, int D, float* out, p16_t* oh,
                          p16_t* ol, hipStream_t s, int lead) {
  auto k = &attention_x3_kernel<NKT, DIRECT>;
  const size_t lds = attention_x3_lds_bytes(NKT);
  if (int rc = rt_allow_lds(k, lds)) return rc;
  // two workgroups (query halves) per (sequence, head); the item <-> block mapping pairs blocks b and b + 8 (same XCD),
  // so the number of items is rounded up to a multiple of 8 and surplus workgroups exit
  // persistent workgroups, two per CU (the grid stays a multiple of 16 so that a workgroup keeps its query half)
  const int items = nseq * qp.H, groups = (items + 7) / 8;
  const int grid = std::min(groups * 16, std::max(16, 2 * x3_grid_limit() / 16 * 16));
  MDM_LAUNCH(k, dim3(grid), dim3(256), lds, s, qp, lengths, S, D, B, lead, out, oh, ol, items);
  return rt_launch_status();
}
template <bool DIRECT>
int launch_attention_x3_nkt(const QkvPlanes& qp, const int* lengths, int nseq, int B, int S, int D, float* out, p16_t* oh,
                            p16_t* ol, hipStream_t s, int lead) {
  switch (qp.NKT) {
    case 1: return launch_attention_x3_t<1, DIRECT>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
    case 2: return launch_attention_x3_t<2, DIRECT>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
    case 3: return launch_attention_x3_t<3, DIRECT>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
    case 4: return launch_attention_x3_t<4, DIRECT>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
    case 5: return launch_attention_x3_t<5, DIRECT>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
    case 6: return launch_attention_x3_t<6, DIRECT>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
    default: return launch_attention_x3_t<7, DIRECT>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
  }
}

// the WIDE form (attention_x3.h): one 8-wave workgroup per CU, one (sequence, head) per item, NKT 5 .. 7
template <int NKT>
int launch_attention_x3_wide_t(const QkvPlanes& qp, const int* lengths, int nseq, int B, int S, int D, float* out, p16_t* oh,
                               p16_t* ol, hipStream_t s, int lead) {
  auto k = &attention_x3_kernel_wide<NKT>;
  const size_t lds = (size_t)axw_lds_bytes(NKT);
  if (int rc = rt_allow_lds(k, lds)) return rc;
  const int items = nseq * qp.H;
  const int grid = std::min(items, x3_grid_limit());   // persistent: workgroup b takes items b, b + grid, ...
  MDM_LAUNCH(k, dim3(grid), dim3(AXW_THREADS), lds, s, qp, lengths, S, D, B, lead, out, oh, ol, items);
  return rt_launch_status();
}

// split-precision attention on the operand planes written by the in_proj epilogue (or qkv_pack_kernel)
// `lead` tokens in front of the frames are never masked (trans_enc: the condition token; trans_dec: none -- its `lengths` count the
// context_len prefix frames as frames)
int launch_attention_x3(Profiler* pf, const QkvPlanes& qp, const int* lengths, int nseq, int B, int S, int D, float* out,
                        p16_t* oh, p16_t* ol, hipStream_t s, int lead = 1, bool direct = false, bool wide = true) {
  ProfScope ps(pf, MDM_PROF_ATTENTION, 4.0 * nseq * qp.H * (double)S * S * AX_HD, s);
  if (D != qp.H * AX_HD) return fail(MDM_EUNSUPPORTED, "attention: head_dim must be 128");
  if (S < 1) return fail(MDM_EUNSUPPORTED, "attention: no tokens");
  if (S > 224) {   // streaming softmax over the same operand planes (attention_long.h): any length
    if (qp.NKT != (S + 31) / 32 || qp.SP != 32 * qp.NKT) return fail(MDM_EINVAL, "attention: the operand planes do not match the sequence length");
    const int nqb = al_query_blocks(S);
    MDM_LAUNCH(attention_x3_long_kernel, dim3(nseq * qp.H * nqb), dim3(256), al_x3_lds_bytes(), s, qp, lengths, S, D, B, lead, out, oh, ol, nqb);
    return rt_launch_status();
  }
  if (direct && out == nullptr && oh != nullptr)   // planes straight from the accumulators (attention_x3.h DIRECT)
    return launch_attention_x3_nkt<true>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
  if (wide && qp.NKT >= 5) {   // S >= 129, where the 4-wave kernel runs two workgroups per item (MDM_OPT_ATTN_WIDE)
    if (qp.NKT != (S + 31) / 32 || qp.SP != 32 * qp.NKT) return fail(MDM_EINVAL, "attention: the operand planes do not match the sequence length");
    switch (qp.NKT) {
      case 5: return launch_attention_x3_wide_t<5>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
      case 6: return launch_attention_x3_wide_t<6>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
      default: return launch_attention_x3_wide_t<7>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
    }
  }
  return launch_attention_x3_nkt<false>(qp, lengths, nseq, B, S, D, out, oh, ol, s, lead);
}

// One split-precision GEMM as its caller describes it (gemm_x3.h X3Kind names the epilogue of the folded-LayerNorm stacks).  The
// encoder's and the decoder's LN() set what is constant over a stack; a call site names what differs.
struct X3Call {
  X3Kind kind = X3K_OUT_LN_RES;
  Profiler* pf = nullptr; int prof_cat = MDM_PROF_LINEAR;
  X3Operand a{nullptr, nullptr}; X3Weights w{nullptr, nullptr}; const float* bias = nullptr;
  float* out = nullptr; p16_t* oh = nullptr; p16_t* ol = nullptr; const QkvPlanes* qp = nullptr;   // fp32 rows / planes / Q, K, V^T planes
  int M = 0, N = 0, K = 0, S = 0, D = 0;
  int scale_cols = 0; float col_scale = 1.f;
  const float* astat = nullptr; const float* colsum = nullptr;                                   // FOLD
  X3Operand res{nullptr, nullptr}; const float* rstat = nullptr; const float* rgamma = nullptr; const float* rbeta = nullptr;  // residual
  float* ostat = nullptr;                                                                       // OSTAT
  int parts = 1; float inv_dim = 1.f;
  const float* res_f32 = nullptr; int emb_T = 1, emb_B = 1, emb_nbranch = 1;                     // fp32 residual; EMBED (X3K_EMBED)
  bool small = false;      // the small-row-count kernel (gemm_x3s.h): the whole forward runs on one of the two kernels
  X3sShape shape{1};       // ... and on ONE tile shape of it (x3s_shape(m->x3s, nseq))
  int stat_cols = 256;     // columns per partial of astat / rstat (what the PRODUCER's kernel wrote)
};
// The one place an X3Epilogue (a kernel argument, gemm_x3.h) is filled
X3Epilogue x3_epilogue(const X3Call& c) {
  X3Epilogue ep{};
  ep.out = c.out; ep.bias = c.bias; ep.res = c.res_f32; ep.resh = c.res.hi; ep.resl = c.res.lo; ep.oh = c.oh; ep.ol = c.ol;
  ep.ld = c.N; ep.scale_cols = c.scale_cols; ep.col_scale = c.col_scale;
  if (c.qp != nullptr) ep.qkv = *c.qp;
  ep.S = c.S; ep.D = c.D;
  ep.astat = c.astat; ep.colsum = c.colsum; ep.rstat = c.rstat; ep.rgamma = c.rgamma; ep.rbeta = c.rbeta; ep.ostat = c.ostat;
  ep.stat_parts = c.parts; ep.inv_dim = c.inv_dim; ep.emb_T = c.emb_T; ep.emb_B = c.emb_B; ep.emb_nbranch = c.emb_nbranch;
  ep.stat_cols = c.stat_cols;
  return ep;
}

#ifdef MDM_PROBES
// TEST-ONLY mode (mdm_debug_set(5, 1)): the `f32` mode's encoder GEMMs on the f16f6 kernel, UNFUSED -- operands packed per
// call into a library-owned scratch (the one exception to "the caller owns every buffer": a debug path) -- so that the
// f16f6 arithmetic can be held against the reference's golden trajectories through the product's own seams before the fused
// path exists.  Not a performance path.
int g_f6_linear = 0;
void* g_f6_dbg_scratch = nullptr;
size_t g_f6_dbg_bytes = 0;
int launch_linear_f6_debug(Profiler* pf, const float* in, int ld_in, const float* w, const float* bias, const float* res,
                           float* out, int M, int N, int K, int act, int scale_cols, float col_scale, hipStream_t s) {
  const size_t wfrag = align_up(x3_packed_weight_elems(N, K) * 2, 256);
  const size_t need = f6_plane_bytes(M, K) + 2 * wfrag;
  if (need > g_f6_dbg_bytes) {
    g_f6_dbg_bytes = 0;
    if (int rc = rt_grow(&g_f6_dbg_scratch, need)) return rc;
    g_f6_dbg_bytes = need;
  }
  ProfScope ps(pf, MDM_PROF_LINEAR, 2.0 * M * (double)N * K, s);
  char* base = static_cast<char*>(g_f6_dbg_scratch);
  const F6Planes pa = f6_carve(base, M, K);
  p16_t* wfh = reinterpret_cast<p16_t*>(base + f6_plane_bytes(M, K));
  p16_t* wfl = reinterpret_cast<p16_t*>(base + f6_plane_bytes(M, K) + wfrag);
  MDM_LAUNCH(pack_f16f6_kernel, dim3((M * (K / 32) + 255) / 256), dim3(256), 0, s, in, pa, M, K, ld_in);
  if (int rc = rt_launch_status()) return rc;
  const int npad = (N + 31) / 32 * 32;
  MDM_LAUNCH(pack_weight_f16f6_kernel, dim3((npad * (K / 32) + 255) / 256), dim3(256), 0, s, w, wfh, wfl, N, K);
  if (int rc = rt_launch_status()) return rc;
  X3Call c; c.out = out; c.bias = bias; c.res_f32 = res; c.N = N; c.scale_cols = scale_cols; c.col_scale = col_scale;
  X3Epilogue ep = x3_epilogue(c);
  ep.acc_scale = 1.f;   // (pack_weight_f16f6_kernel's planes are unscaled: no 2^8 to undo)
  const X3Operand a{reinterpret_cast<const p16_t*>(pa.h16), reinterpret_cast<const p16_t*>(pa.rec)};
  const int rc = launch_gemm_f16f6(a, X3Weights{wfh, wfl}, ep, M, N, K, act, s);
  if (rc != 0) return fail(MDM_EUNSUPPORTED, "f16f6 debug mode: launch failed");
  return rt_launch_status();
}
#endif

// x3: the split-precision arithmetic on this (fp32-in-memory) skeleton -- the DiP decoder's GEMMs in the f16x3 mode
int launch_linear(Profiler* pf, const float* in, int ld_in, const float* w, const float* bias, const float* res,
                  float* out, int M, int N, int K, int act, int scale_cols, float col_scale, hipStream_t s, bool x3 = false) {
#ifdef MDM_PROBES
  if (g_f6_linear && K % 32 == 0 && N % 4 == 0 && ld_in % 4 == 0 && (scale_cols % 256 == 0) &&
      (act == ACT_NONE || (act == ACT_GELU && res == nullptr)))
    return launch_linear_f6_debug(pf, in, ld_in, w, bias, res, out, M, N, K, act, scale_cols, col_scale, s);
#endif
  ProfScope ps(pf, MDM_PROF_LINEAR, 2.0 * M * (double)N * K, s);
  if (K % 4 != 0 || ld_in % 4 != 0) return fail(MDM_EINVAL, "linear: K and the row stride must be multiples of 4");
  RowMajorLoader al{in, ld_in, M, K};
  RowMajorLoader bl{w, K, N, K};
  LinearEpilogue ep{out, bias, res, N, act, scale_cols, col_scale, nullptr, nullptr};
  launch_gemm_f32(al, bl, ep, M, N, K, s, x3);
  return rt_launch_status();
}

// linear with LayerNorms folded in (gemm_f32.h LnLinearEpilogue): `a_ln` set = the A operand is a pre-norm sum and w / bias are
// the gamma-folded ones with column sums `colsum`; res_ln set = the residual is LN(res); ostat = where the partial statistics
// of the written rows go (or null)
// (x3: the weights come as the fragment-ordered planes `wp` of the same matrix, gemm_f32.h X3FragB)
int launch_linear_lnfold(Profiler* pf, const float* in, int ld_in, const LnFold& a_ln, const float* w, X3Weights wp,
                         const float* bias, const float* colsum, const float* res, const LnFold& res_ln, float* out,
                         float* ostat, int M, int N, int K, int act, int scale_cols, float col_scale, hipStream_t s, bool x3) {
  ProfScope ps(pf, MDM_PROF_LINEAR, 2.0 * M * (double)N * K, s);
  if (K % 16 != 0 || ld_in % 4 != 0 || N % LN_PART_COLS != 0) return fail(MDM_EINVAL, "linear (LayerNorm fold): bad K / N");
  RowMajorLoader al{in, ld_in, M, K};
  LnLinearEpilogue ep{out, bias, N, act, scale_cols, col_scale, a_ln, colsum, res, res_ln, ostat};
  if (x3 && wp.hi != nullptr) {
    X3FragB bl{wp.hi, wp.lo, (N + 31) / 32, K};
    launch_gemm_f32(al, bl, ep, M, N, K, s, true);
  } else {
    RowMajorLoader bl{w, K, N, K};
    launch_gemm_f32(al, bl, ep, M, N, K, s, x3);
  }
  return rt_launch_status();
}

// f16x3 GEMM on pre-split operands; writes fp32 `out` and/or split planes oh/ol.  seq_len > 0 tells the tiler that
// the M rows are token sequences of that length (tile = whole sequences).
int launch_linear_x3(Profiler* pf, X3Operand a, X3Weights w, const float* bias, const float* res, float* out,
                     p16_t* oh, p16_t* ol, int M, int N, int K, int act, int scale_cols, float col_scale, int seq_len,
                     hipStream_t s, X3Operand res_planes = X3Operand{nullptr, nullptr}) {
  if (K % X3_BK != 0) return fail(MDM_EINVAL, "f16x3 linear: K must be a multiple of 32");
  if (N % 4 != 0) return fail(MDM_EINVAL, "f16x3 linear: N must be a multiple of 4");
  ProfScope ps(pf, MDM_PROF_LINEAR, 2.0 * M * (double)N * K, s);
  X3Call c; c.out = out; c.oh = oh; c.ol = ol; c.bias = bias; c.res_f32 = res; c.res = res_planes; c.N = N;
  c.scale_cols = scale_cols; c.col_scale = col_scale;
  const int rc = launch_gemm_x3(a, w, x3_epilogue(c), M, N, K, act, seq_len, s);
  if (rc == -2) return fail(MDM_EUNSUPPORTED, "f16x3 linear: unsupported (activation, residual, output) combination");
  return rt_launch_status();
}

// in_proj in split precision: tokens -> Q (pre-scaled) / K / V^T operand planes of attention_x3.h
// pair_B > 0: the nseq = 2 pair_B sequences are the two guidance branches of pair_B samples, equal but for token 0 -- one tile per
// sample computes S + 1 rows and writes both sequences' planes (gemm_x3.h PAIR; the caller has checked x3_qkv_pairs)
int launch_in_proj_x3(Profiler* pf, X3Operand a, X3Weights w, const float* bias, const QkvPlanes& qp, int nseq, int S,
                      int D, float qscale, hipStream_t s, int pair_B = 0) {
  if (D % X3_BK != 0) return fail(MDM_EINVAL, "f16x3 in_proj: latent_dim must be a multiple of 32");
  const double rows = pair_B > 0 ? (double)pair_B * (S + 1) : (double)nseq * S;     // the rows actually computed
  ProfScope ps(pf, MDM_PROF_LINEAR, 2.0 * rows * 3.0 * D * (double)D, s);
  X3Call c; c.bias = bias; c.qp = &qp; c.N = 3 * D; c.S = S; c.D = D; c.scale_cols = D; c.col_scale = qscale;
  const int rc = launch_gemm_x3_qkv(a, w, x3_epilogue(c), nseq, S, D, s, pair_B);
  if (rc == -2) return fail(MDM_EUNSUPPORTED, pair_B > 0 ? "f16x3 in_proj: the paired layer-0 launch does not cover this shape"
                                                         : "f16x3 in_proj: sequences longer than 224 tokens");
  return rt_launch_status();
}

// The latency regime (gemm_x3s.h): a forward of at most MDM_OPT_SMALL_GEMM_MAX_SEQS sequences runs its GEMMs on 32 / 64-row tiles --
// and so does EVERY forward whose sequences are longer than gemm_x3.h's 224-row sequence tile (round 6: the row tiles do not care how
// long a sequence is; attention_long.h takes the attention)
inline bool use_small_gemm(const mdm_model* m, int nseq, int S) {
  return m->precision == MDM_PREC_F16X3 && m->lnfold && (nseq <= m->x3s.max_seqs || S > X3_TM) &&
         m->cfg.latent_dim % 128 == 0 && m->cfg.latent_dim % 256 == 0 && m->cfg.ff_size % 256 == 0;
}
int launch_x3_ln(const X3Call& c, hipStream_t s) {
  const X3Kind kind = c.kind;
  const int M = c.M, N = c.N, K = c.K, S = c.S;
  if (K % X3_BK != 0 || N % 4 != 0) return fail(MDM_EINVAL, "f16x3 linear: K % 32 and N % 4 must be 0");
  // partial statistics per row: D / 256 on gemm_x3.h's tiles (<= 4), D / 128 on gemm_x3s.h's (<= 8); D <= 1024 (mdm_create)
  if (c.parts < 1 || c.parts > (c.small ? 8 : 4)) return fail(MDM_EUNSUPPORTED, "folded LayerNorm: too many partial sums per row (D <= 1024)");
  ProfScope ps(c.pf, c.prof_cat, 2.0 * M * (double)N * K, s);
  const X3Epilogue ep = x3_epilogue(c);
  const bool in_proj = kind == X3K_IN_PROJ_FOLD || kind == X3K_IN_PROJ_PLAIN;
  if (c.small) {
    // rows are grouped by sequence only where the epilogue needs (sequence, token) -- in_proj's Q / K / V^T planes, InputProcess's
    // (sample, frame); every other GEMM tiles its M rows CONTIGUOUSLY: 197 tokens are three 64-row tiles plus one of 5 rows, i.e.
    // a quarter of the workgroups of a sequence-aligned launch would do 8 % of a tile's work (B = 6: 37 row tiles instead of 48)
    const int group_rows = in_proj ? S : (kind == X3K_EMBED ? c.emb_T : M);
    const int rc = launch_gemm_x3s(kind, c.shape, c.a, c.w, ep, M, N, K, group_rows, s);
    if (rc == -1 || rc == -3) return lds_fail(rc, "f16x3 linear (small tiles)");
    if (rc == -2) return fail(MDM_EUNSUPPORTED, "f16x3 linear (small tiles): unsupported shape (K must be 288 or a multiple of 256)");
    return rt_launch_status();
  }
  if (kind == X3K_IN_PROJ_PLAIN) {   // layer 0's in_proj without a folded LayerNorm on the sequence-tile kernel: trans_dec's sequence-tile route (decoder.h)
    const int rc6 = launch_gemm_x3_qkv(c.a, c.w, ep, M / S, S, c.D, s);
    if (rc6 != 0) return fail(MDM_EUNSUPPORTED, "f16x3 in_proj: launch failed");
    return rt_launch_status();
  }
  const int rpt = (kind == X3K_IN_PROJ_FOLD) ? S : x3_rows_per_tile(M, kind == X3K_EMBED ? c.emb_T : S);
  const int rc = launch_gemm_x3_ln(kind, c.a, c.w, ep, M, N, K, rpt, s);
  if (rc == -1 || rc == -3) return lds_fail(rc, "f16x3 linear");
  if (rc == -2) return fail(MDM_EUNSUPPORTED, "f16x3 linear: unsupported folded-LayerNorm GEMM kind");
  return rt_launch_status();
}

// fp32 [N][K] weights -> fragment-ordered hi/lo planes (gemm_x3.h header); K % 16 == 0
int launch_pack_weights(const float* src, p16_t* hi, p16_t* lo, int N, int K, hipStream_t s, int* overflow = nullptr) {
  if (K % 16 != 0) return fail(MDM_EINVAL, "pack_weights: K must be a multiple of 16");
  const size_t n = x3_packed_weight_elems(N, K) / 8;
  const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
  MDM_LAUNCH(pack_weight_planes_kernel, dim3(grid), dim3(256), 0, s, src, hi, lo, N, K, overflow);
  return rt_launch_status();
}

int launch_split(const float* src, p16_t* hi, p16_t* lo, size_t n, hipStream_t s) {
  if (n % 4 != 0) return fail(MDM_EINVAL, "split: element count must be a multiple of 4");
  const size_t n4 = n / 4;
  const int grid = (int)std::min<size_t>((n4 + 255) / 256, 4096);
  MDM_LAUNCH(split_planes_kernel, dim3(grid), dim3(256), 0, s, src, hi, lo, n4);
  return rt_launch_status();
}

}  // namespace
