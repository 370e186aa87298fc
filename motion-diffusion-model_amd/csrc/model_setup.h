// model_setup.h -- part of the ONE translation unit csrc/mdm_api.hip (the C ABI of libmdm_hip.so).  The model handle's set-up: mdm_create /
// mdm_destroy, the option table behind mdm_set_option / mdm_get_option, mdm_set_weight, the constant workspace -- carve_const, the one
// statement of its layout, behind mdm_const_bytes and mdm_prepare -- mdm_weights_in_range and mdm_set_precision.
#pragma once
// (included inside mdm_api.hip's extern "C" block: these ARE exported entry points of include/mdm_hip.h; helpers in anonymous namespaces)

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

// ---- Run-time options of a handle (include/mdm_hip.h, ABI 9).  The library reads NO environment variable (rounds 3-4 did, on the
// launch path); a value takes effect with the next call -- every call resolves its kernel route once, from the handle.
namespace {
// One row per MDM_OPT_* key: where the handle stores it, and the range outside of which mdm_set_option fails with "<name> <range>"
struct OptionRow { int32_t key; const char* name; int32_t lo, hi; const char* range; int32_t& (*value)(mdm_model&); };
const OptionRow kOptions[] = {
    {MDM_OPT_SMALL_GEMM_MAX_SEQS, "MDM_OPT_SMALL_GEMM_MAX_SEQS", 0, INT32_MAX, "must be >= 0", [](mdm_model& m) -> int32_t& { return m.x3s.max_seqs; }},
    {MDM_OPT_SMALL_GEMM_ROW_TILES, "MDM_OPT_SMALL_GEMM_ROW_TILES", 0, 2, "must be 0 (by size), 1 or 2", [](mdm_model& m) -> int32_t& { return m.x3s.row_tiles; }},
    {MDM_OPT_DEC_FUSED_XATTN, "MDM_OPT_DEC_FUSED_XATTN", 0, 3, "must be 0, 1, 2 or 3", [](mdm_model& m) -> int32_t& { return m.fused_xattn; }},
    {MDM_OPT_DEC_FUSED_SELFATTN, "MDM_OPT_DEC_FUSED_SELFATTN", 0, 1, "must be 0 or 1", [](mdm_model& m) -> int32_t& { return m.fused_selfattn; }},
    {MDM_OPT_ATTN_DIRECT_OUT, "MDM_OPT_ATTN_DIRECT_OUT", 0, 1, "must be 0 or 1", [](mdm_model& m) -> int32_t& { return m.attn_direct; }},
    {MDM_OPT_DEC_TIME_TOKEN, "MDM_OPT_DEC_TIME_TOKEN", 0, 1, "must be 0 or 1", [](mdm_model& m) -> int32_t& { return m.dec_time_token; }},
    {MDM_OPT_ENC_SHARED_LAYER0, "MDM_OPT_ENC_SHARED_LAYER0", 0, 1, "must be 0 or 1", [](mdm_model& m) -> int32_t& { return m.enc_shared_l0; }},
    {MDM_OPT_ATTN_WIDE, "MDM_OPT_ATTN_WIDE", 0, 1, "must be 0 or 1", [](mdm_model& m) -> int32_t& { return m.attn_wide; }},
};
const OptionRow* option_row(int32_t key) {
  for (const OptionRow& r : kOptions)
    if (r.key == key) return &r;
  return nullptr;
}
}  // namespace

int mdm_set_option(mdm_model_t* m, int32_t key, int32_t value) {
  if (m == nullptr) return fail(MDM_EINVAL, "mdm_set_option: null model");
  const OptionRow* r = option_row(key);
  if (r == nullptr) return fail(MDM_EINVAL, "mdm_set_option: unknown key " + std::to_string(key));
  if (value < r->lo || value > r->hi) return fail(MDM_EINVAL, std::string("mdm_set_option: ") + r->name + " " + r->range);
  if (key == MDM_OPT_DEC_TIME_TOKEN && value == 1 && (m->cfg.arch != MDM_ARCH_TRANS_DEC || m->cfg.context_len != 1))
    return fail(MDM_EINVAL, "mdm_set_option: MDM_OPT_DEC_TIME_TOKEN needs a trans_dec model created with context_len = 1 (the class-token row)");
  r->value(*m) = value;
  return MDM_OK;
}

int mdm_get_option(const mdm_model_t* m, int32_t key, int32_t* value) {
  if (m == nullptr || value == nullptr) return fail(MDM_EINVAL, "mdm_get_option: null argument");
  const OptionRow* r = option_row(key);
  if (r == nullptr) return fail(MDM_EINVAL, "mdm_get_option: unknown key " + std::to_string(key));
  *value = r->value(const_cast<mdm_model_t&>(*m));   // (read only)
  return MDM_OK;
}

// ABI 10: y['target_cond'] (model/mdm.py:197-199).  One-shot, caller-owned; see include/mdm_hip.h.
int mdm_set_time_add(mdm_model_t* m, const float* add_dev, int32_t B) {
  if (m == nullptr) return fail(MDM_EINVAL, "mdm_set_time_add: null model");
  if (add_dev != nullptr && B <= 0) return fail(MDM_EINVAL, "mdm_set_time_add: B must be >= 1");
  m->time_add_next = add_dev;
  m->time_add_B = add_dev != nullptr ? B : 0;
  return MDM_OK;
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

// ---- The constant workspace: every region of the block, once, in 256-byte-aligned steps.  With a null base only `bytes` means something
// (mdm_const_bytes); mdm_prepare carves the caller's block and fills the regions in this order.
namespace {
extern "C++" ConstBlock carve_const(const mdm_model* m, void* base) {   // (returns a C++ type from inside the extern "C" block)
  const size_t D = m->cfg.latent_dim, FF = m->cfg.ff_size, R = m->cfg.max_len, L = m->cfg.num_layers, JF = m->jf;
  const size_t jf32 = (size_t)(m->jf_out + 31) / 32 * 32;
  size_t off = 0;
  auto take = [&](size_t floats) {
    size_t o = off;
    off += align_up(floats * sizeof(float), 256);
    return base ? reinterpret_cast<float*>(static_cast<char*>(base) + o) : nullptr;
  };
  auto take_planes = [&](size_t N, size_t K) {   // hi | lo: two 16-bit planes = one fp32 matrix's worth of bytes
    const size_t n = x3_packed_weight_elems((int)N, (int)K);
    const p16_t* hi = reinterpret_cast<const p16_t*>(take(n));
    return X3Weights{hi, hi ? hi + n : nullptr};
  };
  ConstBlock c;
  // word 0: "a weight left the range of the 16-bit operand planes" (set by the pack kernels; mdm_weights_in_range)
  c.range_flag = reinterpret_cast<int*>(take(64));
  c.w_in_pad = take(D * m->jf_pad);
  c.time_table = take(R * D);
  c.hidden = take(R * D);
  if (m->cfg.arch == MDM_ARCH_TRANS_DEC) {
    c.dec_fold.assign(L, ConstBlock::DecFold{});
    for (size_t l = 0; l < L; ++l) {
      ConstBlock::DecFold& F = c.dec_fold[l];
      if (l >= 1) { F.w_in = take(3 * D * D); F.c_in = take(3 * D); F.b_in = take(3 * D); }
      F.w_q = take(D * D); F.c_q = take(D); F.b_q = take(D);
      F.w_1 = take(FF * D); F.c_1 = take(FF); F.b_1 = take(FF);
    }
    c.dec_planes.assign(L, ConstBlock::DecPlanes{});
    for (ConstBlock::DecPlanes& P : c.dec_planes) {
      P.in_proj = take_planes(3 * D, D); P.out_proj = take_planes(D, D);
      P.q = take_planes(D, D); P.out_proj2 = take_planes(D, D);
      P.linear1 = take_planes(FF, D); P.linear2 = take_planes(D, FF);
    }
    c.wf_out = take(JF * D);
    c.c_out = take(jf32); c.b_out = take(jf32);
    c.out_planes_f = take_planes(JF, D);
    c.wkv_all = take(L * 2 * D * D);
    c.bkv_all = take(L * 2 * D);
  } else {
    c.planes.assign(L, ConstBlock::LayerPlanes{});
    for (ConstBlock::LayerPlanes& P : c.planes) {
      P.in_proj = take_planes(3 * D, D); P.out_proj = take_planes(D, D);
      P.linear1 = take_planes(FF, D); P.linear2 = take_planes(D, FF);
    }
    c.out_planes = take_planes(JF, D);
    c.out_bias_pad = take(m->jf_out);
    c.scratch_w = take(std::max(3 * D, FF) * D);
    c.fold.assign(L, ConstBlock::LayerFold{});
    for (size_t l = 0; l < L; ++l) {
      ConstBlock::LayerFold& F = c.fold[l];
      if (l >= 1) { F.c_qkv = take(3 * D); F.b_qkv = take(3 * D); F.in_proj = take_planes(3 * D, D); }   // (layer 0's in_proj follows no LayerNorm)
      F.c_1 = take(FF); F.b_1 = take(FF); F.linear1 = take_planes(FF, D);
    }
    c.c_out = take(jf32); c.b_out = take(jf32);
    c.out_planes_f = take_planes(JF, D);
    c.in_planes = take_planes(D, m->jf_k);
  }
  c.bytes = off;
  return c;
}

// fp32 [N][K] weights -> the fragment-ordered planes of a carved region (mdm_prepare is the one writer of the block)
int pack_planes(const mdm_model* m, const float* src, int N, int K, X3Weights region, hipStream_t s) {
  return launch_pack_weights(src, const_cast<p16_t*>(region.hi), const_cast<p16_t*>(region.lo), N, K, s, m->range_flag);
}

// A LayerNorm folded into the consumer of its output: wf = w . diag(gamma) [N][D], cvec = its row sums, bvec = bias + w . beta, the
// two vectors zero-padded to Npad
int fold_layernorm(const mdm_model* m, const float* w, const float* bias, const float* gamma, const float* beta, int N, int Npad,
                   float* wf, float* cvec, float* bvec, hipStream_t s) {
  MDM_LAUNCH(fold_layernorm_kernel, dim3((Npad + 3) / 4), dim3(256), 0, s, w, gamma, beta, bias, wf, cvec, bvec, N, m->cfg.latent_dim, Npad);
  return rt_launch_status();
}

// Range flag, the padded poseEmbedding weight and the time table
int prepare_tables(const mdm_model* m, hipStream_t s) {
  const int D = m->cfg.latent_dim, R = m->cfg.max_len;
  if (int rc = rt_zero(m->range_flag, 4, s)) return rc;
  MDM_LAUNCH(pad_rows_kernel, dim3(256), dim3(256), 0, s, m->w_in_pad, m->W("input_process.poseEmbedding.weight"), D,
             m->jf, m->jf_pad);
  if (int rc = rt_launch_status()) return rc;
  // TimestepEmbedder for every possible t (model/mdm.py:323-330): table[t] = W2 silu(W0 pe[t] + b0) + b2
  if (int rc = launch_linear(nullptr, m->W("sequence_pos_encoder.pe"), D, m->W("embed_timestep.time_embed.0.weight"),
                             m->W("embed_timestep.time_embed.0.bias"), nullptr, m->hidden, R, D, D, ACT_SILU, 0, 1.f, s))
    return rc;
  return launch_linear(nullptr, m->hidden, D, m->W("embed_timestep.time_embed.2.weight"), m->W("embed_timestep.time_embed.2.bias"),
                       nullptr, m->time_table, R, D, D, ACT_NONE, 0, 1.f, s);
}

// trans_enc: hi/lo planes of the encoder weights as they are (always built: the precision mode can be switched afterwards), then
// the LayerNorms folded into their consumers: in_proj(l >= 1) <- norm2(l-1), linear1(l) <- norm1(l), OutputProcess <- norm2(L-1)
int prepare_encoder(mdm_model* m, hipStream_t s) {
  const int D = m->cfg.latent_dim, FF = m->cfg.ff_size, L = m->cfg.num_layers;
  for (int l = 0; l < L; ++l) {
    const mdm_model::LayerPlanes& P = m->planes[l];
    if (int rc = pack_planes(m, m->L(l, "self_attn.in_proj_weight"), 3 * D, D, P.in_proj, s)) return rc;
    if (int rc = pack_planes(m, m->L(l, "self_attn.out_proj.weight"), D, D, P.out_proj, s)) return rc;
    if (int rc = pack_planes(m, m->L(l, "linear1.weight"), FF, D, P.linear1, s)) return rc;
    if (int rc = pack_planes(m, m->L(l, "linear2.weight"), D, FF, P.linear2, s)) return rc;
  }
  // OutputProcess in split precision: weight rows / bias padded to jf_out (the pad rows are zero)
  if (int rc = pack_planes(m, m->W("output_process.poseFinal.weight"), m->jf, D, m->out_planes, s)) return rc;
  MDM_LAUNCH(pad_rows_kernel, dim3(1), dim3(256), 0, s, m->out_bias_pad, m->W("output_process.poseFinal.bias"), 1, m->jf,
             m->jf_out);
  if (int rc = rt_launch_status()) return rc;
  // every fold goes through scratch_w; stream order: the pack kernel reads scratch_w after the fold kernel wrote it
  for (int l = 0; l < L; ++l) {
    const mdm_model::LayerFold& F = m->fold[l];
    if (l >= 1) {
      if (int rc = fold_layernorm(m, m->L(l, "self_attn.in_proj_weight"), m->L(l, "self_attn.in_proj_bias"), m->L(l - 1, "norm2.weight"),
                                  m->L(l - 1, "norm2.bias"), 3 * D, 3 * D, m->scratch_w, F.c_qkv, F.b_qkv, s)) return rc;
      if (int rc = pack_planes(m, m->scratch_w, 3 * D, D, F.in_proj, s)) return rc;
    }
    if (int rc = fold_layernorm(m, m->L(l, "linear1.weight"), m->L(l, "linear1.bias"), m->L(l, "norm1.weight"), m->L(l, "norm1.bias"),
                                FF, FF, m->scratch_w, F.c_1, F.b_1, s)) return rc;
    if (int rc = pack_planes(m, m->scratch_w, FF, D, F.linear1, s)) return rc;
  }
  if (int rc = fold_layernorm(m, m->W("output_process.poseFinal.weight"), m->W("output_process.poseFinal.bias"),
                              m->L(L - 1, "norm2.weight"), m->L(L - 1, "norm2.bias"), m->jf, (m->jf_out + 31) / 32 * 32, m->scratch_w,
                              m->c_out, m->b_out, s)) return rc;
  if (int rc = pack_planes(m, m->scratch_w, m->jf, D, m->out_planes_f, s)) return rc;
  // InputProcess in split precision: weight [D][jf] zero-padded along K to jf_k, then fragment-ordered planes
  MDM_LAUNCH(pad_rows_kernel, dim3(256), dim3(256), 0, s, m->scratch_w, m->W("input_process.poseEmbedding.weight"), D, m->jf,
             m->jf_k);
  if (int rc = rt_launch_status()) return rc;
  if (int rc = pack_planes(m, m->scratch_w, D, m->jf_k, m->in_planes, s)) return rc;
  m->lnfold = true;
  return MDM_OK;
}

// trans_dec (DiP): gamma-folded fp32 copies (kept: the fp32 skeleton runs on them) AND fragment-ordered planes of every layer weight
// (the operand-plane route of the default f16x3 mode); LayerNorm folded into the consumers of its output (gemm_f32.h LnFold)
int prepare_decoder(mdm_model* m, hipStream_t s) {
  const int D = m->cfg.latent_dim, FF = m->cfg.ff_size, L = m->cfg.num_layers;
  for (int l = 0; l < L; ++l) {
    const mdm_model::DecFold& F = m->dec_fold[l];
    if (l >= 1)
      if (int rc = fold_layernorm(m, m->L(l, "self_attn.in_proj_weight"), m->L(l, "self_attn.in_proj_bias"), m->L(l - 1, "norm3.weight"),
                                  m->L(l - 1, "norm3.bias"), 3 * D, 3 * D, F.w_in, F.c_in, F.b_in, s)) return rc;
    if (int rc = fold_layernorm(m, m->L(l, "multihead_attn.in_proj_weight"), m->L(l, "multihead_attn.in_proj_bias"),
                                m->L(l, "norm1.weight"), m->L(l, "norm1.bias"), D, D, F.w_q, F.c_q, F.b_q, s)) return rc;
    if (int rc = fold_layernorm(m, m->L(l, "linear1.weight"), m->L(l, "linear1.bias"), m->L(l, "norm2.weight"), m->L(l, "norm2.bias"),
                                FF, FF, F.w_1, F.c_1, F.b_1, s)) return rc;
  }
  for (int l = 0; l < L; ++l) {
    const mdm_model::DecFold& F = m->dec_fold[l];
    const mdm_model::DecPlanes& P = m->dec_planes[l];
    if (int rc = pack_planes(m, l >= 1 ? F.w_in : m->L(l, "self_attn.in_proj_weight"), 3 * D, D, P.in_proj, s)) return rc;
    if (int rc = pack_planes(m, m->L(l, "self_attn.out_proj.weight"), D, D, P.out_proj, s)) return rc;
    if (int rc = pack_planes(m, F.w_q, D, D, P.q, s)) return rc;
    if (int rc = pack_planes(m, m->L(l, "multihead_attn.out_proj.weight"), D, D, P.out_proj2, s)) return rc;
    if (int rc = pack_planes(m, F.w_1, FF, D, P.linear1, s)) return rc;
    if (int rc = pack_planes(m, m->L(l, "linear2.weight"), D, FF, P.linear2, s)) return rc;
  }
  // OutputProcess <- norm3(L-1) (decoder_pass on operand planes: no LayerNorm kernel in front of poseFinal)
  if (int rc = fold_layernorm(m, m->W("output_process.poseFinal.weight"), m->W("output_process.poseFinal.bias"),
                              m->L(L - 1, "norm3.weight"), m->L(L - 1, "norm3.bias"), m->jf, (m->jf_out + 31) / 32 * 32, m->wf_out,
                              m->c_out, m->b_out, s)) return rc;
  if (int rc = pack_planes(m, m->wf_out, m->jf, D, m->out_planes_f, s)) return rc;
  // the cross-attention key | value projections of all layers as one [L * 2D][D] matrix (mdm_sample_loop_dec's hoisted projections)
  for (int l = 0; l < L; ++l) {
    if (int rc = rt_copy(m->wkv_all + (size_t)l * 2 * D * D, m->L(l, "multihead_attn.in_proj_weight") + (size_t)D * D,
                         (size_t)2 * D * D * sizeof(float), s)) return rc;
    if (int rc = rt_copy(m->bkv_all + (size_t)l * 2 * D, m->L(l, "multihead_attn.in_proj_bias") + D, (size_t)2 * D * sizeof(float), s)) return rc;
  }
  return MDM_OK;
}
}  // namespace

size_t mdm_const_bytes(const mdm_model_t* m) { return m == nullptr ? 0 : carve_const(m, nullptr).bytes; }

int mdm_prepare(mdm_model_t* m, void* const_ws, size_t const_ws_bytes, void* stream) {
  ChainGuard chain_guard(stream);
  if (m == nullptr || const_ws == nullptr) return fail(MDM_EINVAL, "mdm_prepare: null argument");
  for (const auto& kv : m->expect)
    if (m->w.find(kv.first) == m->w.end()) return fail(MDM_ESTATE, "missing weight: " + kv.first);
  ConstBlock c = carve_const(m, const_ws);
  if (const_ws_bytes < c.bytes) return fail(MDM_ENOSPC, "mdm_prepare: const workspace too small");
  static_cast<ConstBlock&>(*m) = std::move(c);   // from here on: launches over the carved regions, nothing else
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = prepare_tables(m, s)) return rc;
  if (int rc = m->cfg.arch == MDM_ARCH_TRANS_DEC ? prepare_decoder(m, s) : prepare_encoder(m, s)) return rc;
  m->prepared = true;
  return MDM_OK;
}

int mdm_weights_in_range(mdm_model_t* m, int32_t* in_range, void* stream) {
  if (int rc = check_ready(m)) return rc;
  if (in_range == nullptr) return fail(MDM_EINVAL, "mdm_weights_in_range: null argument");
  int flag = 0;
  if (int rc = rt_read_back(&flag, m->range_flag, 4, static_cast<hipStream_t>(stream))) return rc;
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
