// decoder.h -- part of the ONE translation unit csrc/mdm_api.hip (the C ABI of libmdm_hip.so); split out of it in round 6
// (source health, no behaviour change).  DiP: MDM.forward for arch='trans_dec' (model/mdm.py:85-93, :203-206, :255-283).
#pragma once
// (included inside mdm_api.hip's extern "C" block; everything here sits in anonymous namespaces)

// ---- DiP: trans_dec denoiser: the fp32 skeleton (f32 mode; MDM_OPT_SMALL_GEMM_MAX_SEQS = 0) and, in the
// default f16x3 mode, the operand-plane route with its (sequence, head) attention blocks (decoder_layers_planes) ---------------
namespace {
struct DecWorkspace {
  float *tok, *qkv, *att, *ffn, *mem, *kv, *proj;
  float *stat[2];    // [M][D/32][2] partial LayerNorm statistics of the residual stream (gemm_f32.h LnFold), ping-pong
  // the plane path (decoder_pass_planes): the residual stream as two ping-pong pairs of hi | lo operand planes; the attention
  // outputs and the GELU output as planes over att / ffn; Q / K / V^T planes over qkv
  p16_t *xh[2], *xl[2];
  p16_t *atth, *attl, *ffnh, *ffnl;
  QkvPlanes qp;
  // window loop only (nsteps > 0): what is constant over the steps of one p_sample_loop
  float *out;        // [nseq][J*F*pred_len] model output of the current step
  float *kv_text;    // [nseq*ntok][L][2D]   Wkv_l . (text part of the memory)            (no bias)
  float *kv_time;    // [nsteps][L][2D]      Wkv_l . time_table[timestep of step k] + b_kv_l
  float *time_rows;  // [nsteps][D]          the gathered time-embedding rows
  float *o_text;     // [L][B][D]            Wo_l . (value row of the unconditional sequence's text part) + bo_l   (sequence-tile route
  float *o_time;     // [L][nsteps][D]       Wo_l . (value row of the step's time part)                              under guidance)
  size_t bytes;
};
DecWorkspace carve_dec(const mdm_model* m, int nseq, int S, int ntok, int B, void* base, int nsteps = 0, int pred_len = 0) {
  const size_t D = m->cfg.latent_dim, FF = m->cfg.ff_size, M = (size_t)nseq * S, Mm = (size_t)nseq * ntok;
  size_t off = 0;
  auto take = [&](size_t floats) {
    size_t o = off;
    off += align_up(floats * sizeof(float), 256);
    return base ? reinterpret_cast<float*>(static_cast<char*>(base) + o) : nullptr;
  };
  DecWorkspace w;
  w.tok = take(M * D);
  const size_t NKT = ((size_t)S + 31) / 32, SP = 32 * NKT;
  w.qkv = take((size_t)nseq * SP * 3 * D);   // self-attention: packed q|k|v rows [M][3D] (or six 16-bit planes of nseq*SP*D: the
                                             // plane path); cross-attention: the projected queries [M][D]
  w.att = take(M * D);
  w.ffn = take(M * FF);
  for (int i = 0; i < 2; ++i) {   // two 16-bit planes = one fp32 array's worth of bytes
    float* tp = take(M * D);
    w.xh[i] = reinterpret_cast<p16_t*>(tp);
    w.xl[i] = tp ? w.xh[i] + M * D : nullptr;
  }
  w.atth = reinterpret_cast<p16_t*>(w.att);
  w.attl = w.att ? w.atth + M * D : nullptr;
  w.ffnh = reinterpret_cast<p16_t*>(w.ffn);
  w.ffnl = w.ffn ? w.ffnh + M * FF : nullptr;
  w.qp = carve_qkv_planes(w.qkv, nseq, S, D, m->cfg.num_heads);
  w.mem = take(Mm * D);           // text memory [nseq][ntok][D]
  w.kv = take(Mm * 2 * D);        // its key | value projections of the current layer
  w.proj = take((size_t)ntok * B * D);   // embed_text(enc_text), token-major
  w.stat[0] = take(M * (D / LN_PART_COLS) * 2);
  w.stat[1] = take(M * (D / LN_PART_COLS) * 2);
  w.out = w.kv_text = w.kv_time = w.time_rows = w.o_text = w.o_time = nullptr;
  if (nsteps > 0) {
    const size_t L = m->cfg.num_layers;
    w.out = take((size_t)nseq * m->jf * pred_len);
    w.kv_text = take(L * Mm * 2 * D);
    w.kv_time = take(L * nsteps * 2 * D);
    w.time_rows = take((size_t)nsteps * D);
    w.o_text = take(L * (size_t)B * D);
    w.o_time = take(L * (size_t)nsteps * D);
  }
  w.bytes = off;
  return w;
}
}  // namespace

namespace {
int check_dec_shapes(const mdm_model_t* m, const char* who, const float* prefix, int B, int pred_len, int ntok) {
  const int C = m->cfg.context_len, S = C + pred_len;
  const std::string w(who);
  if (m->cfg.arch != MDM_ARCH_TRANS_DEC) return fail(MDM_ESTATE, w + ": the model was created as trans_enc");
  if ((C > 0) != (prefix != nullptr)) return fail(MDM_EINVAL, w + ": prefix must be given iff context_len > 0");
  if (B <= 0 || pred_len <= 0 || S > m->cfg.max_len) return fail(MDM_EINVAL, w + ": need B >= 1 and context_len + pred_len <= the positional table's length");
  if (ntok <= 0 || ntok > 512) return fail(MDM_EINVAL, w + ": 1 <= text tokens <= 512");
  if (S > m->cfg.max_len) return fail(MDM_EINVAL, w + ": window longer than the positional table");
  return MDM_OK;
}

// One evaluation of the trans_dec denoiser.  hoist_step < 0: the stand-alone forward (memory = text + time built here from
// `timesteps`, projected per layer).  hoist_step = k >= 0: step k of a window loop -- ws.kv_text / ws.kv_time are filled,
// the memory is never materialised and the per-layer memory projection is skipped.
struct DecHoist {         // step k of a window loop: where the hoisted projections of the (whole) batch live
  int step = -1;          // < 0: not hoisted
  int nsteps = 0;
  const float* kv_text = nullptr;   // [nbranch * kv_B * ntok][L][2D]: row stride L * 2D, layer l at + l * 2D
  const float* kv_time = nullptr;   // [nsteps][L][2D]
  int kv_B = 0, kv_b0 = 0;          // this pass covers samples kv_b0 .. kv_b0 + B - 1 of kv_B
  int t_model = 0;                  // the step's model timestep (the class token of MDM_OPT_DEC_TIME_TOKEN needs its table row)
  // the unconditional half's cross-attention block as row constants, hoisted with the projections (null: made per step):
  const float* o_text = nullptr;    // [L][kv_B][D]  Wo_l . v_text(unconditional sequence b) + bo_l
  const float* o_time = nullptr;    // [L][nsteps][D]  Wo_l . v_time(step)
};
// `--emb_trans_dec` (model/mdm.py:256-257, the `humanml-decoder-with-emb-512` checkpoint): the TIMESTEP embedding leads the decoder's
// tgt sequence as a class token.  The library sees it as the one context row of a context_len = 1 model (always a valid key, dropped
// from the output like a prefix frame); the embedding GEMM has written an embedded placeholder frame there -- overwritten here, in
// every branch, with time_embed(t) (+ the target embedding) + pe[0], as fp32 and / or planes.
int dec_time_token_rows(mdm_model_t* m, float* tok, p16_t* th, p16_t* tl, const int64_t* timesteps, const DecHoist& hz, int B, int nseq,
                        int S, hipStream_t s) {
  if (!m->dec_time_token) return MDM_OK;
  const int D = m->cfg.latent_dim;
  ProfScope ps(&m->prof, MDM_PROF_ELEMENTWISE, 0.0, s);
  MDM_LAUNCH(cond_token_kernel, dim3(nseq), dim3(128), 0, s, tok, (const float*)nullptr, (const float*)nullptr,
             (const float*)m->time_table, reinterpret_cast<const long long*>(hz.step >= 0 ? nullptr : timesteps), hz.t_model,
             m->W("sequence_pos_encoder.pe"), B, S, D, 0, (int)m->cfg.max_len, th, tl,
             m->time_add != nullptr ? m->time_add + (size_t)hz.kv_b0 * D : (const float*)nullptr);
  return rt_launch_status();
}
// The sampler update of a window-loop step, handed DOWN to the plane route: its transposing tail kernel (outproj_finish_kernel
// mode 1) then performs guidance combine + inpainting blend + clamp + posterior / DDIM update + inline Philox in place on x, exactly
// as the encoder loop's tail does -- one launch and one [nseq, J, P] round trip through memory fewer per step than
// OutputProcess -> sampler_step_kernel (same arithmetic, element for element).  `done` says whether the route applied it.
struct DecTail {
  const float* scale = nullptr;      // [B] or null (single branch)
  float* x = nullptr;                // [B, J, F, P]: x_t in, x_{t-1} out
  float* x0_out = nullptr;
  NoiseSource ns{};
  const unsigned char* inpaint_mask = nullptr;
  const float* inpaint_motion = nullptr;
  StepCoefs co{};
  bool done = false;
};

// The projected text memory of layer l as this pass sees it: what SelfAttnArgs (CROSS), XattnArgs and AttnF32Args take as their
// key | value source.  Stand-alone forward: ws.kv, projected per layer.  Step of a window loop: the hoisted text part of the whole
// batch, the step's projected time embedding added to every row while it is staged, and the (branch, sample) remap kv_B / kv_b0.
struct DecMemory {
  const float* k; const float* v; int ldkv;
  const float* kadd; const float* vadd;
  int kv_B, kv_b0;
};
DecMemory dec_memory(const mdm_model_t* m, const DecWorkspace& ws, const DecHoist& hz, int l) {
  const int D = m->cfg.latent_dim, L = m->cfg.num_layers;
  DecMemory mem{};
  if (hz.step < 0) {
    mem.k = ws.kv; mem.v = ws.kv + D; mem.ldkv = 2 * D;
  } else {
    const float* kvt = hz.kv_text + (size_t)l * 2 * D;
    const float* row = hz.kv_time + ((size_t)hz.step * L + l) * 2 * D;
    mem.k = kvt; mem.v = kvt + D; mem.ldkv = L * 2 * D; mem.kadd = row; mem.vadd = row + D; mem.kv_B = hz.kv_B; mem.kv_b0 = hz.kv_b0;
  }
  return mem;
}
// exact-fp32 attention of the projected queries q [.][D] over the memory (the three-launch cross-attention and the fp32 skeleton)
int dec_memory_attention(Profiler* pf, const float* q, const DecMemory& mem, int S, int ntok, const int32_t* text_lengths, int B, float* out,
                         int nseq, int D, int H, p16_t* oh, p16_t* ol, hipStream_t s) {
  AttnF32Args a{q, D, mem.k, mem.v, mem.ldkv, S, ntok, text_lengths, 0, B};
  a.kadd = mem.kadd; a.vadd = mem.vadd; a.kv_B = mem.kv_B; a.kv_b0 = mem.kv_b0;
  return launch_attention_args(pf, a, out, nseq, D, H, oh, ol, s);
}

// Which form the two attention blocks of a layer take on the operand-plane route: the rule of include/mdm_hip.h
// (MDM_OPT_SMALL_GEMM_MAX_SEQS, MDM_OPT_DEC_FUSED_SELFATTN, MDM_OPT_DEC_FUSED_XATTN), in the order the header states it.
enum DecSelfForm { DEC_SELF_BLOCK, DEC_SELF_TWO };                       // one kernel per (sequence, head) | in_proj + attention
enum DecCrossForm { DEC_CROSS_SEQHEAD, DEC_CROSS_ONE, DEC_CROSS_THREE };   // (sequence, head) kernel + out_proj | one kernel | three launches
struct DecForms { DecSelfForm self; DecCrossForm cross; };
constexpr int kXattnOneKernelWgs = 144;    // MDM_OPT_DEC_FUSED_XATTN = 3: from this many 32-row tiles on, xattn_block.h's one-kernel block
DecForms dec_forms(int fused_xattn, int fused_selfattn, int D, int S, int ntok, int nseq, bool small, int scols) {
  // the fused forms belong to the row tiles (and the shape rules below say the same: a sequence tile holds 129 .. 224 tokens)
  if (!small) return {DEC_SELF_TWO, DEC_CROSS_THREE};
  const DecSelfForm self = (fused_selfattn && selfattn_block_supported(D, S)) ? DEC_SELF_BLOCK : DEC_SELF_TWO;
  const bool can_sh = crossattn_block_supported(D, S, ntok), can_one = xattn_block_supported(D, ntok) && scols == 128;
  // by size (3): the one-kernel block re-reads all of Wq | Wo per 32-row tile -- it pays once its nseq * ceil(S / 32) workgroups
  // fill the chip (same-box, motions/s, one kernel vs (sequence, head) form: B = 32 per GPU / 128 tiles 598 vs 630, B = 48 / 192 tiles
  // 641 vs 605, B = 64 / 256 tiles 736 vs 707: profiles/r05c section 5)
  const int xb_wgs = nseq * ((S + XB_TR - 1) / XB_TR);
  const int mode = fused_xattn == 3 ? ((xb_wgs >= kXattnOneKernelWgs && can_one) ? 1 : 2) : fused_xattn;
  // a form whose shapes are not covered falls to the OTHER fused form before the three-launch one (an explicit 1 at
  // latent_dim 768 / 1024 used to drop straight to 0 although 2 applies)
  if (mode == 2) return {self, can_sh ? DEC_CROSS_SEQHEAD : (can_one ? DEC_CROSS_ONE : DEC_CROSS_THREE)};
  if (mode == 1) return {self, can_one ? DEC_CROSS_ONE : (can_sh ? DEC_CROSS_SEQHEAD : DEC_CROSS_THREE)};
  return {self, DEC_CROSS_THREE};
}

// The decoder stack on 16-bit operand planes: the f16x3 mode at the sizes the reference's DiP callers run (model/mdm.py:255-270
// under sample/generate.py's autoregressive windows: 2 x 32 sequences of 20 + 40 tokens = 3,840 token rows).  That is the row
// count of the encoder's latency regime, so the six GEMMs of a layer run on gemm_x3s.h's 32 / 64-row tiles straight from planes
// (the fp32 skeleton of gemm_f32.h splits its operands inside the k-loop: 28 us per GEMM at this size), the self-attention on
// attention_x3.h's Q / K / V^T planes, and only the cross-attention -- 24 memory tokens whose keys / values are hoisted fp32 --
// stays on attention_f32.h (fp32 queries in, planes out).  All three LayerNorms of a layer are folded exactly as in the encoder
// (row statistics per 128 columns from the producer, merged by the consumer); the residual stream ping-pongs between two plane
// pairs because a GEMM cannot write the array its residual's statistics are read from.
// Frame masks (tgt_key_padding_mask, model/mdm.py:241-247 -- what DiP.md:181's `--mask_frames` recipe hands over on every call)
// travel as counts / bitmaps into attention_x3.h with lead = 0 since round 5.
// Not taken (the fp32 skeleton below stays): f32 mode, sample groups of the probe build; mdm_set_option(MDM_OPT_SMALL_GEMM_MAX_SEQS,
// 0) forces the skeleton (tests, A/B runs).  There is no upper row count: the alternative
// is not gemm_x3.h's sequence tiles (a 60-token sequence fills a quarter of one) but the skeleton, and the planes win at every
// size measured (B = 32: 544 vs 391 motions/s, B = 64: 660 vs 448; profiles/r04h_dip_planes.md).
// (sequences of 129 .. 224 tokens, more of them than MDM_OPT_SMALL_GEMM_MAX_SEQS: see decoder_layers_planes)
inline bool dec_sequence_tiles(const mdm_model* m, int nseq, int S) {
  return nseq > m->x3s.max_seqs && S > 128 && S <= X3_TM;
}
inline bool dec_on_planes(const mdm_model* m, int M, int S, const DecHoist& hz, int B) {
  (void)M;
  return m->precision == MDM_PREC_F16X3 && m->x3s.max_seqs > 0 &&
         m->cfg.latent_dim % 256 == 0 && m->cfg.ff_size % 256 == 0 && m->out_planes_f.hi != nullptr &&
         (hz.step < 0 || (hz.kv_b0 == 0 && hz.kv_B == B));
}

// Layer l's view of the ping-pong residual planes: X | sX the layer input (and what the cross-attention block writes), Y | sY the other pair
struct DecLayer {
  int l; p16_t *Xh, *Xl, *Yh, *Yl; float *sX, *sY;
  X3Operand X() const { return X3Operand{Xh, Xl}; }
  X3Operand Y() const { return X3Operand{Yh, Yl}; }
};
// One pass of the plane route: the call's shapes, the stack's GEMM constants, and the blocks of a layer as member functions
struct DecStack {
  mdm_model_t* m; const DecWorkspace& ws; const DecHoist& hz; hipStream_t s; Profiler* pf;
  const int32_t* text_lengths; const int32_t* len;   // valid memory tokens [B]; frame mask or null
  int B, nbranch, nseq, S, ntok, D, H, FF, M;
  // Which GEMM kernel: the row tiles of gemm_x3s.h (DiP's windows at every batch size: a 60-token sequence fills a quarter of a
  // sequence tile) -- or, for LONG sequences at LARGE batch, gemm_x3.h's sequence-sized tiles exactly as the encoder chooses them
  // (use_small_gemm): the reference's full-length trans_dec checkpoint (README.md:254 humanml_trans_dec_512_bert-50steps: 196 frames,
  // no prefix, plain p_sample_loop) at the headline batch is the encoder's shape with a cross-attention block per layer.
  bool small; X3sShape shape; int scols, parts; float inv_dim, qscale;

  X3Call LN(X3Kind kind, X3Operand a, X3Weights w, const float* bias, int rows, int N, int K) const {
    X3Call c; c.kind = kind; c.pf = pf; c.a = a; c.w = w; c.bias = bias; c.M = rows; c.N = N; c.K = K; c.S = S; c.D = D;
    c.small = small; c.shape = shape; c.stat_cols = scols; c.parts = parts; c.inv_dim = inv_dim;
    return c;
  }
  SelfAttnArgs seqhead_args() const {   // what both modes of selfattn_block.h's (sequence, head) kernel take from the stack
    SelfAttnArgs a{};
    a.qscale = qscale; a.lead = 0; a.B = B; a.oh = ws.atth; a.ol = ws.attl;
    a.M = M; a.S = S; a.D = D; a.H = H; a.stat_parts = parts; a.stat_cols = scols; a.inv_dim = inv_dim; a.acc_scale = kX3AccScale;
    return a;
  }

  // ---- Y = X' + self_attn(X'), X' = norm3(l-1)(X) (the embedded tokens for l = 0).  Sequences of at most 64 tokens (DiP: 20 + 40):
  // in_proj + attention of a (sequence, head) in one kernel (selfattn_block.h: Q / K / V^T never leave the CU); else in_proj into
  // operand planes + attention_x3.h.
  // share0: a trans_dec tgt sequence carries no condition token (emb_trans_dec: the timestep embedding, the same in both branches), so
  // under guidance the two branches enter layer 0 with IDENTICAL rows and stay identical through its self-attention block (in_proj,
  // attention, out_proj + residual): they part at the first cross-attention.  The sequence-tile route (throughput-bound) runs that
  // block on the conditional half and copies the result; bit-identical to computing it twice.
  int self_attention(const DecLayer& y, DecSelfForm form, bool share0) const {
    const int l = y.l;
    const mdm_model::DecFold& F = m->dec_fold[l];
    const mdm_model::DecPlanes& P = m->dec_planes[l];
    const int M0 = (share0 && l == 0) ? B * S : M;   // the rows this layer's block computes
    const float* b_in = l == 0 ? m->L(l, "self_attn.in_proj_bias") : F.b_in;
    if (form == DEC_SELF_BLOCK) {
      SelfAttnArgs sa = seqhead_args();
      sa.x = y.X(); sa.xstat = l == 0 ? nullptr : y.sX; sa.w = P.in_proj; sa.bias = b_in; sa.colsum = l == 0 ? nullptr : F.c_in;
      sa.lengths = len;
      ProfScope ps(pf, MDM_PROF_LINEAR, 2.0 * M * 3.0 * D * (double)D + 4.0 * nseq * H * (double)S * S * ATT_HD, s);
      const int rc = launch_seqhead_block(sa, l != 0 ? 1 : 0, s);
      if (rc == -1 || rc == -3) return lds_fail(rc, "self-attention block");
      if (rc != 0) return fail(MDM_EUNSUPPORTED, "self-attention block: unsupported shape");
      if (int rc2 = rt_launch_status()) return rc2;
    } else {
      X3Call c = LN(l == 0 ? X3K_IN_PROJ_PLAIN : X3K_IN_PROJ_FOLD, y.X(), P.in_proj, b_in, M0, 3 * D, D);
      c.qp = &ws.qp; c.scale_cols = D; c.col_scale = qscale;
      if (l != 0) { c.astat = y.sX; c.colsum = F.c_in; }
      if (int rc = launch_x3_ln(c, s)) return rc;
      if (int rc = launch_attention_x3(pf, ws.qp, len, share0 && l == 0 ? B : nseq, B, S, D, nullptr, ws.atth, ws.attl, s, /*lead=*/0,
                                       m->attn_direct, m->attn_wide)) return rc;
    }
    X3Call c = LN(l == 0 ? X3K_OUT_PROJ_L0 : X3K_OUT_LN_RES, X3Operand{ws.atth, ws.attl}, P.out_proj, m->L(l, "self_attn.out_proj.bias"), M0, D, D);
    c.oh = y.Yh; c.ol = y.Yl; c.res = y.X(); c.ostat = y.sY;
    if (l >= 1) { c.rstat = y.sX; c.rgamma = m->L(l - 1, "norm3.weight"); c.rbeta = m->L(l - 1, "norm3.bias"); }
    if (int rc = launch_x3_ln(c, s)) return rc;
    if (share0 && l == 0) {   // the unconditional half of layer 0's self-attention block IS the conditional half: copy its rows
      ProfScope ps(pf, MDM_PROF_ELEMENTWISE, 0.0, s);
      if (int rc = rt_copy(y.Yh + (size_t)M0 * D, y.Yh, (size_t)M0 * D * sizeof(p16_t), s)) return rc;
      if (int rc = rt_copy(y.Yl + (size_t)M0 * D, y.Yl, (size_t)M0 * D * sizeof(p16_t), s)) return rc;
      if (int rc = rt_copy(y.sY + (size_t)M0 * parts * 2, y.sY, (size_t)M0 * parts * 2 * sizeof(float), s)) return rc;
    }
    return MDM_OK;
  }

  // ---- X = norm1(Y) + multihead_attn(norm1(Y), memory, memory), in one of three forms (dec_forms).
  // The out_proj GEMM of the (sequence, head) and the three-launch forms: X = att . Wo + bo + norm1(Y), + row statistics, over `rows`
  int cross_out_proj(const DecLayer& y, int rows) const {
    X3Call c = LN(X3K_OUT_LN_RES, X3Operand{ws.atth, ws.attl}, m->dec_planes[y.l].out_proj2, m->L(y.l, "multihead_attn.out_proj.bias"), rows, D, D);
    c.oh = y.Xh; c.ol = y.Xl; c.res = y.Y(); c.rstat = y.sY; c.rgamma = m->L(y.l, "norm1.weight"); c.rbeta = m->L(y.l, "norm1.bias");
    c.ostat = y.sX;
    return launch_x3_ln(c, s);
  }
  // (sequence, head) form: q projection with norm1 folded + attention over the memory in selfattn_block.h's CROSS mode, then out_proj
  int cross_seqhead(const DecLayer& y, const DecMemory& mem) const {
    const mdm_model::DecFold& F = m->dec_fold[y.l];
    SelfAttnArgs ca = seqhead_args();
    ca.x = y.Y(); ca.xstat = y.sY; ca.w = m->dec_planes[y.l].q; ca.bias = F.b_q; ca.colsum = F.c_q; ca.lengths = nullptr;
    ca.mk = mem.k; ca.mv = mem.v; ca.ldkv = mem.ldkv; ca.kadd = mem.kadd; ca.vadd = mem.vadd; ca.kv_B = mem.kv_B; ca.kv_b0 = mem.kv_b0;
    ca.text_lengths = text_lengths; ca.ntok = ntok;
    {
      ProfScope ps(pf, MDM_PROF_LINEAR, 2.0 * M * (double)D * D + 4.0 * M * (double)ntok * D, s);
      const int rc = launch_seqhead_block(ca, 2, s);
      if (rc == -1 || rc == -3) return lds_fail(rc, "cross-attention (sequence, head) kernel");
      if (rc != 0) return fail(MDM_EUNSUPPORTED, "cross-attention (sequence, head) kernel: unsupported shape");
      if (int rc2 = rt_launch_status()) return rc2;
    }
    return cross_out_proj(y, M);
  }
  // One kernel (xattn_block.h: q projection with norm1 folded -> attention over the memory -> out_proj + norm1 residual + row
  // statistics) where its shapes are covered
  int cross_one_kernel(const DecLayer& y, const DecMemory& mem) const {
    const int l = y.l;
    const mdm_model::DecFold& F = m->dec_fold[l];
    const mdm_model::DecPlanes& P = m->dec_planes[l];
    XattnArgs xa{};
    xa.y = y.Y(); xa.ystat = y.sY; xa.wq = P.q; xa.cq = F.c_q; xa.bq = F.b_q; xa.qscale = qscale;
    xa.k = mem.k; xa.v = mem.v; xa.ldkv = mem.ldkv; xa.kadd = mem.kadd; xa.vadd = mem.vadd; xa.kv_B = mem.kv_B; xa.kv_b0 = mem.kv_b0;
    xa.text_lengths = text_lengths; xa.ntok = ntok; xa.B = B;
    xa.wo = P.out_proj2; xa.bo = m->L(l, "multihead_attn.out_proj.bias");
    xa.gamma = m->L(l, "norm1.weight"); xa.beta = m->L(l, "norm1.bias");
    xa.oh = y.Xh; xa.ol = y.Xl; xa.ostat = y.sX; xa.M = M; xa.S = S; xa.inv_dim = inv_dim; xa.acc_scale = kX3AccScale;
    // (profiled as ONE launch of the GEMM class: 2 D^2 per row twice + the attention contractions)
    ProfScope ps(pf, MDM_PROF_LINEAR, 4.0 * M * (double)D * D + 4.0 * M * (double)ntok * D, s);
    const int rc = launch_xattn_block(xa, D, s);
    if (rc == -1 || rc == -3) return lds_fail(rc, "cross-attention block");
    if (rc != 0) return fail(MDM_EUNSUPPORTED, "cross-attention block: unsupported shape");
    return rt_launch_status();
  }
  // skip_uncond (sequence-tile route under guidance): the whole cross-attention block of the unconditional sequences is a row-constant,
  // x' = norm1(y) + (Wo . v + bo), v the sequence's one projected value row.  The route's statistics partials are 256 columns wide
  // (!small) and D / 4 threads fit a workgroup (mdm_create: latent_dim 256 ... 1024), so one small GEMM makes the B vectors o and
  // uncond_xblock_rows_kernel writes the rows Mq .. 2 Mq - 1; the cross out_proj then covers the conditional half only.
  int uncond_rows(const DecLayer& y, const DecMemory& mem, int Mq) const {
    const int l = y.l;
    const float* o1; const float* o2 = nullptr;
    if (hz.step >= 0 && hz.o_text != nullptr && hz.kv_b0 == 0 && hz.kv_B == B) {   // a window loop made the row constants once (loops.h)
      o1 = hz.o_text + (size_t)l * B * D;
      o2 = hz.o_time + ((size_t)l * hz.nsteps + hz.step) * D;
    } else {
      float* vs = ws.tok + (size_t)Mq * D;          // (the projected queries fill the conditional half of ws.tok only)
      float* ov = vs + (size_t)B * D;
      {
        ProfScope ps(pf, MDM_PROF_ELEMENTWISE, 0.0, s);
        const int vseq0 = mem.kv_B > 0 ? mem.kv_B + mem.kv_b0 : B;   // the source sequence of unconditional sequence 0
        MDM_LAUNCH(gather_value_rows_kernel, dim3(B), dim3(128), 0, s, vs, mem.v, (size_t)ntok * mem.ldkv, mem.vadd, D, vseq0);
        if (int rc = rt_launch_status()) return rc;
      }
      if (int rc = launch_linear(pf, vs, D, m->L(l, "multihead_attn.out_proj.weight"), m->L(l, "multihead_attn.out_proj.bias"), nullptr,
                                 ov, B, D, D, ACT_NONE, 0, 1.f, s)) return rc;
      o1 = ov;
    }
    ProfScope ps(pf, MDM_PROF_ELEMENTWISE, 0.0, s);
    MDM_LAUNCH(uncond_xblock_rows_kernel, dim3((Mq + 7) / 8), dim3(D / 4), 0, s, (const p16_t*)y.Yh, (const p16_t*)y.Yl, (const float*)y.sY,
               m->L(l, "norm1.weight"), m->L(l, "norm1.bias"), o1, o2, y.Xh, y.Xl, y.sX, Mq, Mq, S, D, inv_dim);
    return rt_launch_status();
  }
  // Three launches: fp32 queries (pre-scaled) from the small GEMM into ws.tok, the exact-fp32 attention kernel over k | v of the memory,
  // the small GEMM again.  Sequence-tile route under guidance: the unconditional half (branch 1 = sequences B .. 2B-1) needs neither
  // the q projection nor the attention -- every query's output is the sequence's one projected value row (uncond_rows).  -75 us of a
  // 1,138 us layer at B = 128 (profiles/r06h).
  int cross_three_launches(const DecLayer& y, const DecMemory& mem) const {
    const mdm_model::DecFold& F = m->dec_fold[y.l];
    const bool skip_uncond = !small && nbranch == 2;
    const int nseq_q = skip_uncond ? B : nseq, Mq = nseq_q * S;
    float* q32 = ws.tok;   // the projected cross-attention queries [Mq][D]
    X3Call c = LN(X3K_FOLD_F32, y.Y(), m->dec_planes[y.l].q, F.b_q, Mq, D, D);
    c.out = q32; c.astat = y.sY; c.colsum = F.c_q; c.scale_cols = D; c.col_scale = qscale;
    if (int rc = launch_x3_ln(c, s)) return rc;
    if (int rc = dec_memory_attention(pf, q32, mem, S, ntok, text_lengths, B, nullptr, nseq_q, D, H, ws.atth, ws.attl, s)) return rc;
    if (skip_uncond)
      if (int rc = uncond_rows(y, mem, Mq)) return rc;
    return cross_out_proj(y, Mq);
  }

  // ---- Y = norm2(X) + linear2(gelu(linear1(norm2(X))))
  int feed_forward(const DecLayer& y) const {
    const mdm_model::DecFold& F = m->dec_fold[y.l];
    const mdm_model::DecPlanes& P = m->dec_planes[y.l];
    X3Call c1 = LN(X3K_LINEAR1_GELU, y.X(), P.linear1, F.b_1, M, FF, D);
    c1.oh = ws.ffnh; c1.ol = ws.ffnl; c1.astat = y.sX; c1.colsum = F.c_1;
    if (int rc = launch_x3_ln(c1, s)) return rc;
    X3Call c2 = LN(X3K_OUT_LN_RES, X3Operand{ws.ffnh, ws.ffnl}, P.linear2, m->L(y.l, "linear2.bias"), M, D, FF);
    c2.oh = y.Yh; c2.ol = y.Yl; c2.res = y.X(); c2.rstat = y.sX; c2.rgamma = m->L(y.l, "norm2.weight"); c2.rbeta = m->L(y.l, "norm2.bias");
    c2.ostat = y.sY;
    return launch_x3_ln(c2, s);
  }

  // ---- OutputProcess over the completed suffix (mdm.py:278-282) with the last norm3 folded in: every token's features as an
  // fp32 row (in the dead qkv region), then the transposing tail over token rows context_len .. S-1 -- with `tail` (window loop) the
  // step's sampler update in that kernel (the guidance branches are rows b and B + b)
  int output(int cur, int pred_len, float* out, DecTail* tail) const {
    float* out_tok = ws.qkv;
    ProfScope ps(pf, MDM_PROF_OUTPROJ, 2.0 * nseq * pred_len * (double)D * m->jf, s);
    X3Call c = LN(X3K_FOLD_F32, X3Operand{ws.xh[cur], ws.xl[cur]}, m->out_planes_f, m->b_out, M, m->jf_out, D);
    c.pf = nullptr; c.prof_cat = MDM_PROF_OUTPROJ; c.out = out_tok; c.astat = ws.stat[cur]; c.colsum = m->c_out;
    if (int rc = launch_x3_ln(c, s)) return rc;
    if (tail == nullptr)
      return launch_outproj_finish(m, out_tok, nseq, B, S, pred_len, nullptr, 0, out, nullptr, nullptr, NoiseSource{}, nullptr, nullptr,
                                   StepCoefs{}, s);
    tail->done = true;
    return launch_outproj_finish(m, out_tok, nseq, B, S, pred_len, tail->scale, 1, tail->x, tail->x0_out, tail->x, tail->ns,
                                 tail->inpaint_mask, tail->inpaint_motion, tail->co, s);
  }
};

int decoder_layers_planes(mdm_model_t* m, const DecWorkspace& ws, const float* x, const float* prefix, const int64_t* timesteps,
                          const int32_t* text_lengths, const int32_t* len, int B, int pred_len, int ntok, int nbranch, float* out,
                          hipStream_t s, const DecHoist& hz, DecTail* tail) {
  const int S = m->cfg.context_len + pred_len, D = m->cfg.latent_dim, nseq = nbranch * B, M = nseq * S;
  DecStack d{m, ws, hz, s, &m->prof};
  d.text_lengths = text_lengths; d.len = len;
  d.B = B; d.nbranch = nbranch; d.nseq = nseq; d.S = S; d.ntok = ntok; d.D = D; d.H = m->cfg.num_heads; d.FF = m->cfg.ff_size; d.M = M;
  d.small = !dec_sequence_tiles(m, nseq, S);
  d.shape = x3s_shape(m->x3s, (M + 196) / 197);   // the encoder's 32- / 64-row threshold, in its token rows
  d.scols = d.small ? X3S_TN : 256; d.parts = (D + d.scols - 1) / d.scols;
  d.inv_dim = 1.0f / (float)D; d.qscale = 1.0f / sqrtf((float)ATT_HD);
  int cur = 0;   // which plane pair holds the layer input
  // tgt tokens: InputProcess over cat(prefix, x) + positional rows, written as planes (the fp32 copy in ws.tok is not read)
  if (int rc = launch_embed_f32(m, ws.tok, ws.xh[cur], ws.xl[cur], x, prefix, m->cfg.context_len, B, S, /*lead=*/0, nbranch, true, s)) return rc;
  if (int rc = dec_time_token_rows(m, ws.tok, ws.xh[cur], ws.xl[cur], timesteps, hz, B, nseq, S, s)) return rc;
  const DecForms forms = dec_forms(m->fused_xattn, m->fused_selfattn, D, S, ntok, nseq, d.small, d.scols);
  const bool share0 = !d.small && nbranch == 2 && forms.self != DEC_SELF_BLOCK;
  for (int l = 0; l < m->cfg.num_layers; ++l) {
    const DecLayer y{l, ws.xh[cur], ws.xl[cur], ws.xh[cur ^ 1], ws.xl[cur ^ 1], ws.stat[cur], ws.stat[cur ^ 1]};
    if (int rc = d.self_attention(y, forms.self, share0)) return rc;
    if (hz.step < 0) {   // the memory's key | value projection of this layer (a window loop hoists it: loops.h)
      const float* wc = m->L(l, "multihead_attn.in_proj_weight");
      const float* bc = m->L(l, "multihead_attn.in_proj_bias");
      if (int rc = launch_linear(d.pf, ws.mem, D, wc + (size_t)D * D, bc + D, nullptr, ws.kv, nseq * ntok, 2 * D, D, ACT_NONE, 0, 1.f, s, true)) return rc;
    }
    const DecMemory mem = dec_memory(m, ws, hz, l);
    int rc = MDM_OK;
    switch (forms.cross) {
      case DEC_CROSS_SEQHEAD: rc = d.cross_seqhead(y, mem); break;
      case DEC_CROSS_ONE: rc = d.cross_one_kernel(y, mem); break;
      case DEC_CROSS_THREE: rc = d.cross_three_launches(y, mem); break;
    }
    if (rc != MDM_OK) return rc;
    if (int rc2 = d.feed_forward(y)) return rc2;
    cur ^= 1;   // the layer's output (pre-norm3) is the next layer's X
  }
  return d.output(cur, pred_len, out, tail);
}

int decoder_pass(mdm_model_t* m, const DecWorkspace& ws, const float* x, const float* prefix, const int64_t* timesteps,
                 const float* text_tokens, const int32_t* text_lengths, const int32_t* lengths, int B, int pred_len,
                 int ntok, int branches, float* out, hipStream_t s, const DecHoist& hz, DecTail* tail = nullptr) {
  const int C = m->cfg.context_len, S = C + pred_len, D = m->cfg.latent_dim, H = m->cfg.num_heads, FF = m->cfg.ff_size;
  const int nbranch = (branches == MDM_BRANCH_BOTH) ? 2 : 1;
  const int nseq = nbranch * B, M = nseq * S, Mm = nseq * ntok;
  Profiler* pf = &m->prof;
  const int* len = m->cfg.mask_frames ? lengths : nullptr;
  const float qscale = 1.0f / sqrtf((float)ATT_HD);
  const bool x3 = m->precision == MDM_PREC_F16X3;   // GEMM arithmetic (gemm_f32.h X3); attention and LayerNorm statistics stay fp32
  const bool hoisted = hz.step >= 0;

  // ---- text memory: embed_text over every token (cond branch), + time embedding (mdm.py:217-219)
  if (!hoisted && branches != MDM_BRANCH_UNCOND)
    if (int rc = launch_linear(nullptr, text_tokens, m->cfg.clip_dim, m->W("embed_text.weight"), m->W("embed_text.bias"),
                               nullptr, ws.proj, ntok * B, D, m->cfg.clip_dim, ACT_NONE, 0, 1.f, s)) return rc;
  if (!hoisted) {
    ProfScope ps(pf, MDM_PROF_ELEMENTWISE, 0.0, s);
    MDM_LAUNCH(text_memory_kernel, dim3(Mm), dim3(128), 0, s, ws.mem, (const float*)ws.proj, m->W("embed_text.bias"),
               (const float*)m->time_table, reinterpret_cast<const long long*>(timesteps), B, ntok, D,
               (branches == MDM_BRANCH_UNCOND) ? 0 : 1, (int)m->cfg.max_len, m->time_add);
    if (int rc = rt_launch_status()) return rc;
  }
  if (dec_on_planes(m, M, S, hz, B))
    return decoder_layers_planes(m, ws, x, prefix, timesteps, text_lengths, len, B, pred_len, ntok, nbranch, out, s, hz,
                                 (tail != nullptr && (nbranch == 1) == (tail->scale == nullptr)) ? tail : nullptr);
  // ---- tgt tokens: InputProcess over cat(prefix, x) + positional rows (mdm.py:203-206, :239, :259-260); both branches
  if (int rc = launch_embed_f32(m, ws.tok, nullptr, nullptr, x, prefix, C, B, S, /*lead=*/0, nbranch, x3, s)) return rc;
  if (int rc = dec_time_token_rows(m, ws.tok, nullptr, nullptr, timesteps, hz, B, nseq, S, s)) return rc;
  // ---- nn.TransformerDecoder (mdm.py:265; post-norm layers, no final norm).  The three LayerNorms of a layer are folded
  // into the GEMMs around them (gemm_f32.h LnFold): ws.tok holds the PRE-norm sums y, `pend` says which LayerNorm its readers
  // have to apply (none for the embedded tokens entering layer 0); only the last norm3 runs as a kernel, for OutputProcess.
  LnFold pend{};
  int sp = 0;
  auto fold_of = [&](int l, const char* norm) {
    LnFold f;
    f.stat = ws.stat[sp];
    f.gamma = m->L(l, (std::string(norm) + ".weight").c_str());
    f.beta = m->L(l, (std::string(norm) + ".bias").c_str());
    f.parts = D / LN_PART_COLS;
    f.inv_dim = 1.0f / (float)D;
    return f;
  };
  const LnFold none{};
  for (int l = 0; l < m->cfg.num_layers; ++l) {
    const mdm_model::DecFold& F = m->dec_fold[l];
    const mdm_model::DecPlanes& P = m->dec_planes[l];
    const bool folded = pend.stat != nullptr;   // false only for the embedded tokens entering layer 0
    // x = norm1(x + self_attn(x))
    if (int rc = launch_linear_lnfold(pf, ws.tok, D, pend, folded ? F.w_in : m->L(l, "self_attn.in_proj_weight"), P.in_proj,
                                      folded ? F.b_in : m->L(l, "self_attn.in_proj_bias"), folded ? F.c_in : nullptr, nullptr,
                                      none, ws.qkv, nullptr, M, 3 * D, D, ACT_NONE, D, qscale, s, x3)) return rc;
    // (hoisted: `lengths` is the WHOLE batch's array -- counts, then the ABI-7 bitmaps -- and this pass covers samples kv_b0 ..)
    if (int rc = launch_attention(pf, ws.qkv, ws.att, len, nseq, B, S, D, H, nullptr, nullptr, s, /*lead=*/0,
                                  hoisted ? hz.kv_B : 0, hoisted ? hz.kv_b0 : 0)) return rc;
    if (int rc = launch_linear_lnfold(pf, ws.att, D, none, m->L(l, "self_attn.out_proj.weight"), P.out_proj,
                                      m->L(l, "self_attn.out_proj.bias"), nullptr, ws.tok, pend, ws.tok, ws.stat[sp ^ 1], M, D, D,
                                      ACT_NONE, 0, 1.f, s, x3)) return rc;
    sp ^= 1;
    pend = fold_of(l, "norm1");
    // x = norm2(x + multihead_attn(x, memory, memory)): q from the tokens, k | v from the memory (packed in_proj rows)
    const float* wc = m->L(l, "multihead_attn.in_proj_weight");
    const float* bc = m->L(l, "multihead_attn.in_proj_bias");
    if (int rc = launch_linear_lnfold(pf, ws.tok, D, pend, F.w_q, P.q, F.b_q, F.c_q, nullptr, none, ws.qkv, nullptr, M, D, D,
                                      ACT_NONE, D, qscale, s, x3)) return rc;
    if (!hoisted)
      if (int rc = launch_linear(pf, ws.mem, D, wc + (size_t)D * D, bc + D, nullptr, ws.kv, Mm, 2 * D, D, ACT_NONE, 0, 1.f, s, x3)) return rc;
    if (int rc = dec_memory_attention(pf, ws.qkv, dec_memory(m, ws, hz, l), S, ntok, text_lengths, B, ws.att, nseq, D, H, nullptr, nullptr,
                                      s)) return rc;
    if (int rc = launch_linear_lnfold(pf, ws.att, D, none, m->L(l, "multihead_attn.out_proj.weight"), P.out_proj2,
                                      m->L(l, "multihead_attn.out_proj.bias"), nullptr, ws.tok, pend, ws.tok, ws.stat[sp ^ 1], M,
                                      D, D, ACT_NONE, 0, 1.f, s, x3)) return rc;
    sp ^= 1;
    pend = fold_of(l, "norm2");
    // x = norm3(x + linear2(gelu(linear1(x))))
    if (int rc = launch_linear_lnfold(pf, ws.tok, D, pend, F.w_1, P.linear1, F.b_1, F.c_1, nullptr, none, ws.ffn, nullptr, M, FF,
                                      D, ACT_GELU, 0, 1.f, s, x3)) return rc;
    if (int rc = launch_linear_lnfold(pf, ws.ffn, FF, none, m->L(l, "linear2.weight"), P.linear2, m->L(l, "linear2.bias"), nullptr,
                                      ws.tok, pend, ws.tok, ws.stat[sp ^ 1], M, D, FF, ACT_NONE, 0, 1.f, s, x3)) return rc;
    sp ^= 1;
    pend = fold_of(l, "norm3");
  }
  if (pend.stat != nullptr)
    if (int rc = launch_layernorm(pf, ws.tok, pend.gamma, pend.beta, M, D, nullptr, nullptr, s)) return rc;
  // ---- OutputProcess over the completed suffix (mdm.py:278-282): token rows context_len .. S-1 of every sequence
  RowMajorLoader al{m->W("output_process.poseFinal.weight"), D, m->jf, D};
  CfgTokenLoader bl{ws.tok, nullptr, nseq, pred_len, S, D, nseq * pred_len, C};
  OutProjEpilogue ep{};
  ep.bias = m->W("output_process.poseFinal.bias");
  ep.out = out;
  ep.T = pred_len; ep.JF = m->jf; ep.mode = 0;
  ProfScope ps(pf, MDM_PROF_OUTPROJ, 2.0 * nseq * pred_len * (double)D * m->jf, s);
  launch_gemm_f32(al, bl, ep, m->jf, nseq * pred_len, D, s, x3, /*weight_is_a=*/true);
  return rt_launch_status();
}
}  // namespace
