/* mdm_hip.h -- C ABI of libmdm_hip.so: the MI355X (gfx950) implementation of MDM's DDPM sampling hot path.
 *
 * The upstream project (GuyTevet/motion-diffusion-model) has no FFI: its boundary is three Python
 * duck-typed seams.  This header is the native layer *beneath* those seams; each entry
 * point names the reference interface it replaces (paths relative to the upstream tree).  The Python
 * mirror of the seams lives in motion-diffusion-model_amd/ and INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pointer named *_dev / documented "device" is a caller-owned HIP device pointer (e.g. memory of
 *     a torch tensor); the library never allocates, frees or retains tensor memory except the weight
 *     pointers registered with mdm_set_weight (which must stay valid while the model is used);
 *   - all work is enqueued asynchronously on the hipStream_t passed as `stream` (void* to keep this header
 *     free of HIP types); nothing synchronises the device;
 *   - every function returns MDM_OK (0) or a negative MDM_E* code; mdm_last_error() gives the message of the
 *     calling thread's last failure.  No C++ exception crosses the ABI;
 *   - a model handle may be used from one thread / one stream at a time.
 *   - CONCURRENCY: ONE chain of this library's kernels per device.  The library itself enforces it: every call that
 *     enqueues kernels takes a per-device lock for the duration of the (asynchronous) enqueue and, when the previous call
 *     on this device used a DIFFERENT stream, makes `stream` wait (hipStreamWaitEvent) for the event recorded behind
 *     that call's kernels.  Two model handles, two streams or two host threads on one GPU therefore run their kernels
 *     back to back, never side by side.  Why: in the f16x3 mode the DiP path's small eight-wave GEMM returns rare wrong
 *     values (one 16-lane row of one register reads as zero) when a workgroup of a DIFFERENT kernel that uses LDS is
 *     resident on the same CU at the same time -- measured with this library's own chains on side streams AND with another
 *     library's fused attention kernels (scaled-dot-product attention) on a foreign stream (17 of 60 DiP window loops differed); never on disjoint CUs,
 *     never in the f32 mode, and not on the encoder path (trans_enc: its kernels own a CU's whole LDS; 0 of 120 forwards
 *     beside the same foreign stream).  Not cache coherence, not kernel ordering (profiles/r03g_dip_groups.md); and NOT a
 *     wait-state hazard that a disassembly can show: round 6 pointed the static auditor that found round 5's
 *     `v_fma_mix -> v_mfma` hazard (tools/hazard_audit.py: VALU write -> MFMA read, MFMA write -> VALU / memory read or
 *     overwrite, every kernel, fall-through paths) at the SLP build that corrupts -- 12,806 v_pk_{add,mul,fma}_f32, 0 sites, hipcc
 *     pads its packed instructions exactly like its plain ones (profiles/r06b_slp_hazard_audit.md).  The cause stays
 *     unidentified -- looked for with the tool, not found.  What cures it is building without packed fp32 VALU math (-fno-slp-vectorize, the
 *     way __graft_entry__.build() builds this library: 0 of 520 window loops in the regimes that corrupted 100 of 520).
 *     PRECAUTION FOR CALLERS, because the effect is not understood: while mdm_forward_dec / mdm_sample_loop_dec work is in
 *     flight on a device and the results matter, keep other LDS-using kernels off it; never build the library with SLP
 *     vectorisation if they cannot be kept off (mdm_build_info() says how a binary was built; the loaders check it).  The
 *     encoder calls need no such care.
 *   - hipGraph CAPTURE: supported for a loop that stays on ONE stream (since ABI 8 a same-stream call makes no HIP runtime
 *     call besides its kernel launches and device-to-device copies: the per-device guard is a host mutex).  The warm-up may have
 *     run on ANOTHER stream (graph-capture helpers of ML frameworks capture on a side stream of their own): since ABI 9 the guard asks hipStreamIsCapturing and
 *     skips its cross-stream event while `stream` is being captured (tests/test_gpu_round5.py replays such a capture).  Run one
 *     warm-up call of the SAME shapes (batch, frames, text tokens) first: a kernel instantiation opts in to its dynamic LDS on first
 *     use, and a first use on a capturing stream is refused with MDM_EUNSUPPORTED (round 6; it used to issue the function-attribute
 *     call inside the capture).  Keep mdm_profile_enable off, and order the
 *     graph's REPLAYS against other users of the device yourself.  Not supported: a capture that contains calls from two
 *     different streams.
 *   - all tensors are fp32, dense, in the reference's layouts: poses [B, njoints, nfeats, T] (T contiguous).
 */
#ifndef MDM_HIP_H
#define MDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDM_OK 0
#define MDM_EINVAL (-1)   /* bad argument / shape                              */
#define MDM_ESTATE (-2)   /* missing weight, mdm_prepare not called, ...       */
#define MDM_ENOSPC (-3)   /* workspace too small                               */
#define MDM_EHIP (-4)     /* a HIP runtime call failed                         */
#define MDM_EUNSUPPORTED (-5)

#define MDM_ABI_VERSION 10

typedef struct mdm_model mdm_model_t;

#define MDM_ARCH_TRANS_ENC 0  /* model/mdm.py:75-84: nn.TransformerEncoder, condition token in front of the frames   */
#define MDM_ARCH_TRANS_DEC 1  /* model/mdm.py:85-93: nn.TransformerDecoder over a text-token memory (DiP, DiP.md)    */

/* Hyper-parameters of model/mdm.py:11-135 (data_rep='hml_vec', cond_mode='text'). */
typedef struct mdm_config {
  int32_t njoints;      /* 263  (utils/model_util.py:43)                        */
  int32_t nfeats;       /* 1                                                    */
  int32_t latent_dim;   /* 512  (utils/parser_util.py:106); multiple of 256     */
  int32_t ff_size;      /* 1024 (utils/model_util.py:63); multiple of 32        */
  int32_t num_layers;   /* 8                                                    */
  int32_t num_heads;    /* 4  -> head dim must be 128                           */
  int32_t clip_dim;     /* 512: width of y['text_embed']                        */
  int32_t max_len;      /* rows of the positional table `sequence_pos_encoder.pe` (5000) */
  int32_t mask_frames;  /* args.mask_frames (model/mdm.py:48, :243)             */
  int32_t arch;         /* MDM_ARCH_TRANS_ENC (0, default) | MDM_ARCH_TRANS_DEC  */
  int32_t context_len;  /* trans_dec: prefix frames of the completion task (model/mdm.py:59, :203-206); 0 otherwise.
                         * With MDM_ARCH_TRANS_DEC, clip_dim is the width of the text-token embeddings (768, DistilBERT:
                         * model/mdm.py:121-127), emb_policy is 'add' and emb_trans_dec is False (the DiP configuration) */
} mdm_config_t;

int mdm_abi_version(void);
/* How the binary was built, as "key=value;..." -- "slp=off|on;probes=0|1;emu=0|1;planes=f16|bf16".  "slp=off" means the
 * library was compiled with -fno-slp-vectorize -DMDM_NO_SLP=1 (no packed fp32 VALU math), the only build in which the DiP path
 * is immune to the co-residency corruption described under CONCURRENCY above; the Python loader (_native.py) and the ctypes
 * stub of INTEGRATION.md refuse any other product library unless MDM_ALLOW_SLP_BUILD=1 is set (A/B experiments).  ABI 8. */
const char* mdm_build_info(void);
const char* mdm_last_error(void);

/* MDM(...) constructor (model/mdm.py:11-135) -- shapes only, no weights yet. */
int mdm_create(const mdm_config_t* cfg, mdm_model_t** out);
void mdm_destroy(mdm_model_t* m);

/* Run-time options of a model handle (ABI 9).  The library reads NO environment variable: everything that steers which kernels
 * a call runs is either derived from the shapes or set here, per handle, and takes effect with the next call (a call resolves
 * its route once; set options between calls, not from another thread during one).  No counterpart in the reference.
 *   MDM_OPT_SMALL_GEMM_MAX_SEQS   up to how many token sequences (B, or 2B under guidance) a forward runs its GEMMs on the
 *                                 32 / 64-row tiles of the latency regime (csrc/gemm_x3s.h) instead of the sequence-sized tiles
 *                                 (csrc/gemm_x3.h).  Default 80 (the measured cross-over, profiles/r05k_crossovers.md).  0: never -- which also sends the
 *                                 trans_dec (DiP) decoder to its fp32-skeleton route (csrc/gemm_f32.h).  The parity tests use it
 *                                 to hold every route against the reference's fixtures.  A trans_dec forward of MORE sequences than
 *                                 this leaves the row tiles only where its sequences are 129 .. 224 tokens long: there it runs on
 *                                 the sequence tiles with in_proj + attention and the three-launch cross-attention (the fused forms
 *                                 below belong to the row tiles), and under guidance computes layer 0's self-attention block once
 *                                 and the unconditional half's cross-attention as row constants.
 *   MDM_OPT_SMALL_GEMM_ROW_TILES  0 (default): 32-row tiles up to 12 sequences, 64-row tiles above; 1 / 2: pin 32 / 64 rows.
 *   MDM_OPT_DEC_FUSED_XATTN       the cross-attention block of a trans_dec layer on the operand-plane route -- query projection with
 *                                 norm1 folded, attention over the text memory, out_proj + residual + row statistics (model/mdm.py:
 *                                 85-93, :263-265).  3 (default): by size -- 2 below 144 32-row tiles (DiP's 32 motions per GPU: 120), 1
 *                                 from there on.  2: projection + attention of a (sequence, head) in one kernel
 *                                 (csrc/selfattn_block.h, CROSS mode: windows and memories of at most 64 tokens), then the out_proj
 *                                 GEMM; 1: the whole block as ONE kernel (csrc/xattn_block.h: latent_dim 256 / 512, <= 96 memory
 *                                 tokens); 0: as three launches around the exact-fp32 attention kernel (round 4's form).  An explicit
 *                                 1 or 2 whose shapes are not covered takes the other fused form if that one applies, else 0.
 *   MDM_OPT_DEC_FUSED_SELFATTN    1 (default): in_proj + self-attention of a trans_dec layer on the operand-plane route run as ONE
 *                                 kernel per (sequence, head) for sequences of at most 64 tokens (csrc/selfattn_block.h: DiP's 20 + 40);
 *                                 0: in_proj into Q / K / V^T planes + the attention kernel (two launches; A/B and tests). */
#define MDM_OPT_SMALL_GEMM_MAX_SEQS 1
#define MDM_OPT_SMALL_GEMM_ROW_TILES 2
#define MDM_OPT_DEC_FUSED_XATTN 3
#define MDM_OPT_DEC_FUSED_SELFATTN 4
/*   MDM_OPT_ATTN_DIRECT_OUT       the split-precision self-attention kernel (csrc/attention_x3.h) writes its output planes straight from
 *                                 the accumulators and requests the next (sequence, head)'s first key tiles in front of those stores,
 *                                 instead of staging the output through its LDS ring (A/B of round 5: profiles/r05e_attention_direct.md). */
#define MDM_OPT_ATTN_DIRECT_OUT 5
/*   MDM_OPT_DEC_TIME_TOKEN        a MODEL-STRUCTURE switch (ABI 10; set once, before the first forward): `--emb_trans_dec` (model/mdm.py:101,
 *                                 :245-247, :256-257, :269-270 -- the `humanml-decoder-with-emb-512` checkpoint): the timestep embedding
 *                                 leads the trans_dec tgt sequence as a class token.  Create the model with context_len = 1 -- that row
 *                                 is the class token: always a valid key, dropped from the output like a prefix frame -- pass a
 *                                 `prefix_dev` of B zero frames [B, njoints, nfeats, 1] (a placeholder; the library overwrites the row it
 *                                 embeds to with time_embed(t) (+ the mdm_set_time_add row) + pe[0] in every branch), and count the row
 *                                 in `lengths_dev` as context rows are.  0 (default): context rows are embedded prefix frames (DiP). */
#define MDM_OPT_DEC_TIME_TOKEN 6
/*   MDM_OPT_ENC_SHARED_LAYER0     1 (default): under guidance (MDM_BRANCH_BOTH) layer 0's in_proj of the trans_enc stack computes the
 *                                 Q / K / V rows of a sample's frame tokens ONCE and writes them to both branches' operand planes --
 *                                 the two sequences of a sample differ only in token 0, the condition token, which rides in a pad
 *                                 row of the sample's 208-row tile (csrc/gemm_x3.h PAIR).  Same products in the same order: results
 *                                 are bit-identical.  Taken on the sequence-tile route of the f16x3 mode for sequences of at most
 *                                 207 tokens; every other forward, and 0 (A/B and tests), runs one tile per sequence. */
#define MDM_OPT_ENC_SHARED_LAYER0 7
/*   MDM_OPT_ATTN_WIDE             1 (default): from 129 tokens on (five to seven 32-key tiles; up to 224) the split-precision self-attention
 *                                 runs as ONE 8-wave workgroup per (sequence, head) -- a wave per query tile, the remaining waves copy
 *                                 the K / V^T tiles into LDS for all of them -- instead of two 4-wave workgroups that each stream all of
 *                                 K and V^T (csrc/attention_x3.h).  Same arithmetic in the same order: results are bit-identical.
 *                                 0 (A/B and tests): the 4-wave kernel at every length.  MDM_OPT_ATTN_DIRECT_OUT = 1 selects the
 *                                 4-wave kernel's direct form whatever this option says. */
#define MDM_OPT_ATTN_WIDE 8
int mdm_set_option(mdm_model_t* m, int32_t key, int32_t value);
int mdm_get_option(const mdm_model_t* m, int32_t key, int32_t* value);

/* y['target_cond'] -- the target-location condition of the `--multi_target_cond` checkpoints (model/mdm.py:197-199; the target-conditioned
 * DiP of DiP.md:105) -- reaches the denoiser as a per-sample vector ADDED TO THE TIMESTEP EMBEDDING, in every guidance branch
 * (`time_emb += mask_cond(embed_target_cond(...), force_mask=y.get('target_uncond'))`): through it into the condition token of the
 * trans_enc sequence (mdm.py:219-220, :251) or into every row of the trans_dec text memory (:217-219, :263-265).  The embedding
 * itself (a SiLU MLP over <= 8 joints x 4 numbers per sample, model/mdm.py:399-479) does not depend on x or t: the host evaluates it
 * once per loop, like the text encoder, and binds the result here (ABI 10):
 *   add_dev  [B, latent_dim] fp32, caller-owned, alive until the consuming call's work on its stream is done; NULL clears a binding.
 * ONE-SHOT: the next mdm_forward / mdm_forward_dec / mdm_sample_loop / mdm_sample_loop_dec call on this handle consumes the binding
 * (and fails with MDM_EINVAL, consuming it, if its batch is not B); calls after it run without one.  Under MDM_BRANCH_BOTH / guidance,
 * row b is added to sample b of both branches.  A force-masked target (y['target_uncond']) is simply no binding. */
int mdm_set_time_add(mdm_model_t* m, const float* add_dev, int32_t B);

/* load_state_dict (utils/model_util.py:8-15): register the device pointer of one state-dict tensor under
 * its REFERENCE key, e.g. "seqTransEncoder.layers.3.self_attn.in_proj_weight".  `numel` is checked against
 * the shape the config implies.  The positional table is registered as "sequence_pos_encoder.pe"
 * ([max_len, latent_dim], computed by the host exactly as model/mdm.py:301-305 does). */
int mdm_set_weight(mdm_model_t* m, const char* name, const float* dev_ptr, int64_t numel);

/* Bytes of the caller-owned, model-lifetime device block that holds everything mdm_prepare derives from the weights: the padded
 * poseEmbedding weight and the time-MLP table TimestepEmbedder(pe[t]) for every t (model/mdm.py:316-330), the fragment-ordered 16-bit
 * hi | lo planes of every layer weight, the weights with their LayerNorm folded in (planes, column sums, biases; trans_dec: fp32 copies
 * too) and, for trans_dec, the stacked cross-attention K | V projections of all layers.  Exactly what mdm_prepare writes: one layout
 * (csrc/model_setup.h carve_const) gives this size and carves the block.  Depends on the mdm_config_t only. */
size_t mdm_const_bytes(const mdm_model_t* m);
/* Validates that every weight is present and (re)builds the derived tables.  Call again after weights change. */
int mdm_prepare(mdm_model_t* m, void* const_ws_dev, size_t const_ws_bytes, void* stream);

/* Range check of the split-precision weight planes.  The f16x3 arithmetic carries every weight matrix (and every
 * LayerNorm-gamma-folded weight matrix: gamma[k] * W[n][k]) as fp16 hi + lo planes of w * 2^8, i.e. it needs
 * |w| < 255.9 (activations: |x| <= 65504, checked on the samples by the Python seam).  mdm_prepare's pack kernels record a
 * violation in a device flag; this call reads it back (ONE stream synchronisation -- call it once after mdm_prepare).
 * *in_range = 1: every plane is finite; 0: use MDM_PREC_F32 for this checkpoint (the Python seam raises and says so).
 * No counterpart in the reference (its fp32 `addmm`s have fp32's range). */
int mdm_weights_in_range(mdm_model_t* m, int32_t* in_range, void* stream);

/* Arithmetic of the model's dense contractions:
 *   MDM_PREC_F32     exact fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere: bit-for-bit an fp32 fma chain; the on-device
 *                    parity reference (157 TFLOP/s peak);
 *   MDM_PREC_F16X3   default: operands split into fp16 hi + lo planes (11 + 11 significant bits), three fp16 MFMA products
 *                    per fp32 product (hi*hi + hi*lo + lo*hi), fp32 accumulation: ~2^-22 relative per product while the
 *                    operands stay inside fp16's range (|x| <= 2 * 65504; 2^-25 absolute below 2^-14) -- on the reference's
 *                    golden trajectories this is the fp32 re-association floor (2.5 PFLOP/s fp16 peak / 3 passes).
 * In MDM_PREC_F16X3 every GEMM of MDM.forward runs on the split kernel -- in_proj / out_proj / linear1 / linear2, the
 * 263-wide InputProcess / OutputProcess projections (K resp. N padded) -- and so do the attention contractions (QK^T, PV),
 * on planes written by the in_proj epilogue.  LayerNorm statistics, GELU, softmax, the time / text embeddings and the
 * sampler update are fp32 in both modes.  May be called any time after mdm_create. */
#define MDM_PREC_F32 0
#define MDM_PREC_F16X3 1
int mdm_set_precision(mdm_model_t* m, int32_t mode);

/* Per-call activation workspace for `nseq` token sequences (B, or 2B under classifier-free guidance)
 * of `nframes` frames each. */
size_t mdm_workspace_bytes(const mdm_model_t* m, int32_t nseq, int32_t nframes);

#define MDM_BRANCH_COND 0    /* y['uncond'] absent/False                     */
#define MDM_BRANCH_UNCOND 1  /* y['uncond'] == True  (model/mdm.py:155-156, :208) */
#define MDM_BRANCH_BOTH 2    /* both, batched: out = [cond(B) ; uncond(B)]   */

/* MDM.forward(x, timesteps, y)  (model/mdm.py:189-283).
 *   x_dev          [B, njoints, nfeats, T]
 *   timesteps_dev  [B] int64
 *   text_embed_dev [B, clip_dim] = y['text_embed'][0]; may be NULL for MDM_BRANCH_UNCOND
 *   lengths_dev    the key-padding mask of model/mdm.py:241-247 (`~y['mask']` -> src_key_padding_mask), in one of two forms:
 *                  [B] int32 valid-FRAME COUNTS when every y['mask'] row is a prefix mask (what data_loaders/tensors.py:3-8
 *                  builds; the kernels' fast path), or -- since ABI 7 -- [9 B] int32 for arbitrary masks: lengths[b] >= 0 is
 *                  sample b's count as before, lengths[b] == -1 says that its mask is the BITMAP in the eight words
 *                  lengths[B + 8 b .. B + 8 b + 7] (bit j of word i set: frame 32 i + j is a valid key; frames >= T ignored);
 *                  the condition token is always a valid key.  NULL = no key-padding mask (all frames valid, or
 *                  mask_frames == 0).  The same two forms hold wherever this header says `lengths_dev`
 *   T              1 <= T < cfg.max_len (the positional table, model/mdm.py:55; the condition token takes one row).  Up to 223
 *                  frames the attention keeps a query's scores in registers (exact softmax); longer sequences run the GEMMs on row
 *                  tiles at every batch size and the attention with a streaming softmax (csrc/attention_long.h, round 6).  A
 *                  BITMAP covers 256 frames: frames beyond it are masked -- use counts for longer prefix masks
 *   out_dev        [B or 2B, njoints, nfeats, T]                                                   */
int mdm_forward(mdm_model_t* m, const float* x_dev, const int64_t* timesteps_dev, const float* text_embed_dev,
                const int32_t* lengths_dev, int32_t B, int32_t T, int32_t branches, float* out_dev, void* ws_dev,
                size_t ws_bytes, void* stream);

/* MDM.forward for MDM_ARCH_TRANS_DEC (model/mdm.py:189-283 with is_prefix_comp, text_encoder_type='bert' or 'clip').  Arithmetic as
 * mdm_set_precision says: in MDM_PREC_F16X3 (default) the whole decoder stack runs on fp16 hi/lo operand planes -- the small-tile
 * split-precision GEMMs, the split-precision self-attention, all three LayerNorms of a layer folded -- with or without a frame
 * mask; exact fp32 MFMA in MDM_PREC_F32.
 *   x_dev            [B, njoints, nfeats, pred_len]      the window being denoised
 *   prefix_dev       [B, njoints, nfeats, context_len]   y['prefix'] (NULL iff context_len == 0)
 *   timesteps_dev    [B] int64
 *   text_tokens_dev  [ntok, B, clip_dim]  = y['text_embed'][0] (DistilBERT last_hidden_state, token-major as
 *                    bert_encode_text returns it, model/mdm.py:180-187); may be NULL for MDM_BRANCH_UNCOND
 *   text_lengths_dev [B] int32: tokens of each prompt (y['text_embed'][1] is a suffix pad mask: the tokenizer pads on the
 *                    right, model/BERT/BERT_encoder.py:28-30) -- the memory_key_padding_mask of mdm.py:265
 *   lengths_dev      the tgt_key_padding_mask of model/mdm.py:241-247 over the context_len + pred_len window, in the two forms
 *                    of mdm_forward's lengths_dev ([B] counts, or [9 B] counts + bitmaps) -- here the counts / bits INCLUDE the
 *                    context_len prefix frames (always valid, mdm.py:203-206) and there is no condition token -- or NULL
 *   out_dev          [B or 2B, njoints, nfeats, pred_len]  the completed suffix (mdm.py:278-279)              */
size_t mdm_workspace_bytes_dec(const mdm_model_t* m, int32_t nseq, int32_t pred_len, int32_t ntok);
int mdm_forward_dec(mdm_model_t* m, const float* x_dev, const float* prefix_dev, const int64_t* timesteps_dev,
                    const float* text_tokens_dev, const int32_t* text_lengths_dev, const int32_t* lengths_dev, int32_t B,
                    int32_t pred_len, int32_t ntok, int32_t branches, float* out_dev, void* ws_dev, size_t ws_bytes,
                    void* stream);

/* One fused sampler update given model outputs (the tail of GaussianDiffusion.p_sample / ddim_sample,
 * diffusion/gaussian_diffusion.py:489-541, :729-779, incl. ClassifierFreeSampleModel's combine
 * utils/sampler_util.py:34 and the inpainting blend :300-304):
 *   x0     = out_uncond ? out_uncond + scale[b]*(out_cond - out_uncond) : out_cond
 *   x0     = inpaint_mask ? (mask ? motion : x0) : x0 ;  clamp to [-1,1] if clip_denoised
 *   x_prev = a_x0*x0 + a_xt*x_t + sigma*eps,   eps = noise_dev ? noise_dev : Philox(seed, sample, draw)
 * a_x0/a_xt/sigma are the host-folded per-step scalars (posterior_mean_coef1/2, exp(.5*log_var)*[t!=0]). */
typedef struct mdm_step {
  float a_x0, a_xt, sigma;
  int32_t clip_denoised;
  uint64_t seed;         /* Philox key                                           */
  uint32_t sample_base;  /* global index of local sample 0 (shard-invariant RNG) */
  uint32_t draw;         /* draw index: 0 = x_T, 1+k = k-th loop iteration       */
  int32_t const_noise;   /* 1: eps of sample 0 for every sample (gaussian_diffusion.py:527-528) */
} mdm_step_t;

int mdm_sampler_step(const float* x_t_dev, const float* out_cond_dev, const float* out_uncond_dev,
                     const float* scale_dev, const uint8_t* inpaint_mask_dev, const float* inpaint_motion_dev,
                     const float* noise_dev, float* x_prev_dev, float* x0_dev, int32_t B, int32_t per_sample,
                     const mdm_step_t* step, void* stream);

/* th.randn(*shape) / q_sample (gaussian_diffusion.py:691, :226-244, :693-700) from the counter-based stream:
 *   out = init ? a*init + s*eps : eps,  eps = eps_dev ? eps_dev : Philox(seed, sample_base+b, draw).     */
int mdm_randn(float* out_dev, const float* init_dev, const float* eps_dev, float a, float s, int32_t B,
              int32_t per_sample, uint64_t seed, uint32_t sample_base, uint32_t draw, void* stream);

/* GaussianDiffusion.p_sample_loop / ddim_sample_loop (diffusion/gaussian_diffusion.py:591-727, :876-990)
 * over ClassifierFreeSampleModel(MDM) (or bare MDM when scale_dev == NULL), entirely on `stream`:
 * per step  InputProcess GEMM -> condition token -> 8 encoder layers -> OutputProcess GEMM whose epilogue
 * performs the CFG combine + posterior/DDIM update in place on x.  Host arrays are indexed by the
 * (respaced) diffusion index i = start_index .. 0. */
typedef struct mdm_sample_params {
  int32_t B, T;
  int32_t num_timesteps;        /* length of the host tables below                                   */
  int32_t start_index;          /* first i (= num_timesteps-1-skip_timesteps)                        */
  const float* a_x0;            /* host [num_timesteps]                                              */
  const float* a_xt;            /* host [num_timesteps]                                              */
  const float* sigma;           /* host [num_timesteps]  (0 at i == 0)                               */
  const int32_t* timestep_map;  /* host [num_timesteps]: model timestep for index i (respace.py:125-130) */
  const float* text_embed_dev;  /* [B, clip_dim] or NULL (unconditional)                             */
  const float* scale_dev;       /* [B] guidance scale y['scale'], NULL = no CFG (single branch)      */
  const int32_t* lengths_dev;   /* [B] or NULL                                                       */
  const uint8_t* inpaint_mask_dev;   /* [B,J,F,T] or NULL  (y['inpainting_mask'])                    */
  const float* inpaint_motion_dev;   /* [B,J,F,T] or NULL  (y['inpainted_motion'])                   */
  const float* noise_dev;       /* [nsteps, B,J,F,T] injected per-step noise, NULL = Philox          */
  uint64_t seed;
  uint32_t sample_base;
  int32_t clip_denoised;
  int32_t force_uncond;         /* 1: y['uncond']=True for the single-branch case                    */
  float* x0_dev;                /* optional: pred_xstart of the last executed step                   */
  const int32_t* dump_steps;    /* host, ascending loop indices k to snapshot (p_sample_loop dump_steps) */
  int32_t num_dump;
  float* dump_dev;              /* [num_dump, B,J,F,T]                                               */
  int32_t const_noise;          /* p_sample const_noise=True (gaussian_diffusion.py:527-528): every sample receives the
                                 * step noise of (global) sample 0 -- noise[[0]].repeat(B, 1, 1, 1)     */
} mdm_sample_params_t;

/* x_dev [B,J,F,T]: in = x at index start_index (x_T, or q_sample(init) -- see mdm_randn), out = sample. */
int mdm_sample_loop(mdm_model_t* m, const mdm_sample_params_t* p, float* x_dev, void* ws_dev, size_t ws_bytes,
                    void* stream);

/* The same loop over the MDM_ARCH_TRANS_DEC (DiP) denoiser: one call = one p_sample_loop over a prediction window
 * (sample/generate.py's autoregressive loop calls it once per window with the previous window's tail as y['prefix']).
 * `loop.T` is pred_len and `loop.text_embed_dev` the token-major text tokens [ntok, B, clip_dim] of mdm_forward_dec.
 * What does not change over the steps of a window is computed once per call: embed_text over the tokens and, per layer,
 * the key | value projections of the text part of the cross-attention memory; a step adds its projected timestep
 * embedding (one [2D] row per layer) while the attention kernel stages K / V.  The sampler update runs in place on x. */
typedef struct mdm_sample_dec_params {
  mdm_sample_params_t loop;
  int32_t ntok;
  const float* prefix_dev;           /* [B, njoints, nfeats, context_len]; NULL iff context_len == 0 */
  const int32_t* text_lengths_dev;   /* [B] tokens per prompt                                        */
} mdm_sample_dec_params_t;
size_t mdm_workspace_bytes_dec_loop(const mdm_model_t* m, int32_t nseq, int32_t pred_len, int32_t ntok, int32_t nsteps);
int mdm_sample_loop_dec(mdm_model_t* m, const mdm_sample_dec_params_t* p, float* x_dev, void* ws_dev, size_t ws_bytes,
                        void* stream);

/* Opt-in per-launch timing, for bench.py's roofline line.  While enabled, every kernel the model launches is
 * bracketed by a hipEvent pair on the launch stream and bucketed by kernel class; mdm_profile_read waits for
 * the events of one class and returns their summed duration, the launch count and the ALGORITHMIC flops of
 * those launches (2MNK per GEMM, 4 S^2 hd per (sequence, head) of attention; 0 for the HBM-bound classes).
 * (The CPU emulation of the test suite has no events: it reports the launch counts, with times and flops 0.)
 * The event records perturb the stream slightly, so throughput is always timed with profiling off. */
#define MDM_PROF_LINEAR 0       /* encoder GEMMs: in_proj, out_proj, linear1, linear2 */
#define MDM_PROF_ATTENTION 1
#define MDM_PROF_LAYERNORM 2
#define MDM_PROF_EMBED 3        /* InputProcess GEMM                                  */
#define MDM_PROF_OUTPROJ 4      /* OutputProcess GEMM (+ fused sampler update)        */
#define MDM_PROF_ELEMENTWISE 5  /* condition token, Philox noise                      */
#define MDM_PROF_NUM 6
int mdm_profile_enable(mdm_model_t* m, int on);
int mdm_profile_read(mdm_model_t* m, int32_t category, double* total_ms, int64_t* launches, double* flops);
int mdm_profile_reset(mdm_model_t* m);
/* Building blocks, exported for the parity tests and for callers that compose their own layers.
 *   mdm_linear:    out[M,N] = act(in[M,K] . w[N,K]^T + bias) (+ res)     act: 0 none, 1 gelu(erf), 2 silu
 *   mdm_layernorm: in-place LayerNorm over rows of D (eps 1e-5)
 *   mdm_attention: softmax(QK^T + keypad) V per (sequence, head) on a packed [nseq*S, 3D] qkv buffer whose
 *                  Q columns are pre-scaled by 1/sqrt(head_dim); lengths as in mdm_forward (indexed seq % B). */
int mdm_linear(const float* in_dev, const float* w_dev, const float* bias_dev, const float* res_dev, float* out_dev,
               int32_t M, int32_t N, int32_t K, int32_t act, void* stream);
/*   mdm_linear_x3: the same contract as mdm_linear computed by the split-precision kernel (K % 32 == 0);
 *                      `scratch_dev` (mdm_linear_x3_scratch_bytes) receives the 16-bit hi / lo planes of both operands. */
size_t mdm_linear_x3_scratch_bytes(int32_t M, int32_t N, int32_t K);
int mdm_linear_x3(const float* in_dev, const float* w_dev, const float* bias_dev, const float* res_dev,
                      float* out_dev, int32_t M, int32_t N, int32_t K, int32_t act, void* scratch_dev,
                      size_t scratch_bytes, void* stream);
int mdm_layernorm(float* x_dev, const float* gamma_dev, const float* beta_dev, int32_t rows, int32_t D, void* stream);
int mdm_attention(const float* qkv_dev, float* out_dev, const int32_t* lengths_dev, int32_t nseq, int32_t B,
                  int32_t S, int32_t D, int32_t H, void* stream);
/*   mdm_attention_x3: the same contract computed by the split-precision kernel the f16x3 mode uses (QK^T and PV
 *                  as three 16-bit MFMA products each, fp32 softmax); `scratch_dev` receives the Q/K/V^T hi / lo planes. */
size_t mdm_attention_x3_scratch_bytes(int32_t nseq, int32_t S, int32_t D);
int mdm_attention_x3(const float* qkv_dev, float* out_dev, const int32_t* lengths_dev, int32_t nseq, int32_t B,
                         int32_t S, int32_t D, int32_t H, void* scratch_dev, size_t scratch_bytes, void* stream);

/* Post-sampling transform of sample/generate.py:160-166, on the device:
 *   data = x * std + mean                         (data_loaders/humanml/data/dataset.py:132-133 inv_transform)
 *   recover_from_ric(data, joints)                (data_loaders/humanml/scripts/motion_process.py:437-452, :366-385)
 * x_dev [B, njoints_feat, 1, T] (the sampler's output, normalised HumanML3D features: 263 wide, 22 joints; KIT 251 / 21),
 * mean_dev / std_dev [njoints_feat], out_dev [B, joints, 3, T] -- the layout generate.py:166 produces by permute. */
int mdm_recover_from_ric(const float* x_dev, const float* mean_dev, const float* std_dev, float* out_dev, int32_t B,
                         int32_t T, int32_t njoints_feat, int32_t joints, void* stream);

/* The inverse of mdm_recover_from_ric, on the device: joint positions -> HumanML3D / KIT feature vectors (additive to ABI 10;
 * kernels: csrc/motion_features.h).  Restates
 *   extract_features(positions, feet_thre, ...)   (data_loaders/humanml/scripts/motion_process.py:43-170)
 *   process_file(positions, feet_thre)            (motion_process.py:173-355; uniform_skeleton :17-40)
 *   Skeleton.inverse_kinematics_np / forward_kinematics_np   (data_loaders/humanml/common/skeleton.py:55-104, :129-150)
 * and the quaternion helpers they use (data_loaders/humanml/common/quaternion.py: qbetween, qnormalize, qmul, qinv, qrot,
 * quaternion_to_cont6d).  The foot contacts are computed in fp32 exactly as numpy computes them on fp32 positions (bit-exact flags);
 * everything else in fp64, rounded once at the store.  Where the reference's qbetween crosses along the frame axis for a clip of
 * exactly 3 frames (its cross product is called without an axis), this call crosses over xyz.
 *
 * The skeleton tables are HOST data (utils/paramUtil.py:4-55; motion_process.py:460-466, :506-512): the kinematic chains -- chain 0
 * starts at the root, joint 0; every other chain at a joint an earlier chain reaches; every other joint is reached once --, the raw
 * offsets (unit axes), the face joints in the reference's list order, the foot joints, the two leg bones of the retargeting ratio. */
#define MDM_SKEL_MAX_JOINTS 22
#define MDM_SKEL_MAX_CHAINS 8
#define MDM_SKEL_MAX_CHAIN_LEN 8
typedef struct mdm_skeleton {
  int32_t joints;                                            /* J <= 22                                   */
  int32_t n_chains;
  int32_t chain_len[MDM_SKEL_MAX_CHAINS];
  int32_t chains[MDM_SKEL_MAX_CHAINS][MDM_SKEL_MAX_CHAIN_LEN];
  float raw_offsets[MDM_SKEL_MAX_JOINTS][3];
  int32_t face_joints[4];                                    /* face_joint_indx: r_hip, l_hip, sdr_r, sdr_l */
  int32_t fid_r[2], fid_l[2];
  int32_t l_idx1, l_idx2;
} mdm_skeleton_t;

#define MDM_J2F_LAYOUT_BJ3T 0   /* joints_dev [B, J, 3, T]: what mdm_recover_from_ric emits */
#define MDM_J2F_LAYOUT_BTJ3 1   /* joints_dev [B, T, J, 3]: the reference's per-clip layout  */

/* process_file's steps, each selectable (all off: extract_features on the positions as they are):
 *   tgt_offsets   HOST [J][3] or null: uniform_skeleton -- IK with the unsmoothed forward, the root scaled by the leg-length ratio of
 *                 frame 0, FK along these offsets (what Skeleton.get_offsets_joints returns for the target clip);
 *   floor         subtract the minimum y over all valid frames and joints of the clip;
 *   origin_xz     move the root's xz of frame 0 to the origin;
 *   face_z        rotate the clip so that frame 0 faces +Z.
 * mean_dev / std_dev [F] or both null: the output is (x - mean) / std.  global_dev / ric_dev, optional [B, J, 3, T]: the positions
 * the features were taken from (process_file's global_positions) and the rotation-invariant positions of every valid frame (its
 * third result); zeros beyond a clip's length. */
typedef struct mdm_joints_to_features_call {
  int32_t layout;
  int32_t floor, origin_xz, face_z;
  double feet_thre;                                          /* 0.002 HumanML3D, 0.05 KIT                  */
  const float* tgt_offsets;
  const float* mean_dev;
  const float* std_dev;
  float* global_dev;
  float* ric_dev;
} mdm_joints_to_features_call_t;

/* joints_dev as `layout` says, fp32; lengths HOST [B] or null (every clip has T frames), 2 <= lengths[b] <= T; out_dev
 * [B, F, 1, T - 1] with F = 12 J - 1 (263 for 22 joints, 251 for 21): frames >= lengths[b] - 1 of a clip are exact zeros, and nothing
 * read beyond lengths[b] influences a valid frame.  ws_dev (mdm_joints_to_features_workspace_bytes) holds the canonicalised
 * positions in fp64; it may be null when no step of process_file is selected.  T <= 1024 (MDM_EUNSUPPORTED beyond: a clip's forward
 * vectors are staged in LDS for the 161-tap temporal filter).  The frame counts travel as kernel arguments, 64 clips a launch: no
 * allocation, no copy, capture-safe. */
size_t mdm_joints_to_features_workspace_bytes(int32_t B, int32_t T, int32_t joints);
int mdm_joints_to_features(const mdm_skeleton_t* skeleton, const mdm_joints_to_features_call_t* call, const float* joints_dev,
                           const int32_t* lengths, float* out_dev, int32_t B, int32_t T, int32_t F, void* ws_dev, size_t ws_bytes,
                           void* stream);

/* Post-sampling transform of the rot6d (action-to-motion) families, on the device: the SMPL joint positions of
 *   model.rot2xyz(x, mask, pose_rep='rot6d', glob=True, translation=True, jointstype='smpl', vertstrans=True, beta=0)
 * (model/rotation2xyz.py:17-90, utils/rotation_conversions.py rotation_6d_to_matrix, smplx lbs batch_rigid_transform).
 * x_dev [B, njoints_in = J + 1, 6, T] (the sampler's output: J joint rotations in 6D, then the translation row, of which the
 * first 3 features are read); mask_dev [B, T] uint8 (nullptr: every frame valid; a masked frame's rotations are not read and
 * its joints are 0 before the translation is added); rest_joints [J * 3] HOST array, the rest-pose joints
 * J_regressor . v_template; parents [J] HOST array, parents[0] = -1 and 0 <= parents[i] < i (SMPL's kintree_table[0]);
 * out_dev [B, J, 3, T]: posed joint minus posed root plus (translation_t - translation_0).  J <= 24, T <= 4096.
 * The tables travel as kernel arguments: no device allocation, capture-safe. */
int mdm_rot6d_to_smpl_joints(const float* x_dev, const uint8_t* mask_dev, const float* rest_joints, const int32_t* parents,
                             float* out_dev, int32_t B, int32_t T, int32_t njoints_in, int32_t J, void* stream);

/* The full SMPL body pass of model/rotation2xyz.py:17-92 over model/smpl.py:64-97 and smplx's lbs, on the device: shape blend,
 * pose blend shapes, linear blend skinning of every vertex, joints regressed from the mesh; every pose_rep, jointstype, betas and
 * glob_rot the reference accepts (additive to ABI 10; kernels: csrc/smpl_mesh.h).
 *
 * The model tables are caller-owned fp32 DEVICE arrays, prepared once per model (mdm_amd/smpl_mesh.py does it):
 *   j0         [J][3]                the rest joints of the mean shape, J_regressor . v_template
 *   jdirs      [J][3][10]            their shape directions, J_regressor . shapedirs
 *   blend      [3][KP][Vpad]         B'_c[k][v]: rows 0 .. (J-1)*9 - 1 posedirs, then the 10 shapedirs, then v_template, then zeros;
 *                                    KP = ((J - 1) * 9 + 10 + 1) rounded up to 4, Vpad = V rounded up to 32, zero beyond V
 *   weights_t  [24][Vpad]            the skinning weights transposed, zero beyond J and V
 *   sel_blend, sel_weights_t         the same two tables gathered at the n_sel vertices that follow the J joints in smplx's joint
 *                                    list (VertexJointSelector), Vpad = n_sel rounded up to 32; may be null when n_sel = 0
 *   extra_t    [V][n_extra]          J_regressor_extra transposed; may be null when n_extra = 0
 *   parents    [J] HOST              parents[0] = -1, 0 <= parents[i] < i                                         J <= 24 */
typedef struct mdm_smpl_model {
  const float* j0;
  const float* jdirs;
  const float* blend;
  const float* weights_t;
  const float* sel_blend;
  const float* sel_weights_t;
  const float* extra_t;
  const int32_t* parents;
  int32_t J, V, n_sel, n_extra;
} mdm_smpl_model_t;

#define MDM_SMPL_ROT6D 0   /* pose_rep: features per rotation row 6, 3, 9, 4 */
#define MDM_SMPL_ROTVEC 1
#define MDM_SMPL_ROTMAT 2
#define MDM_SMPL_ROTQUAT 3

/* One call's arguments (rotation2xyz.py:17-19).  n_points = 0: jointstype 'vertices', out_dev [B, V, 3, T], no root subtraction.
 * n_points >= 1 (at most 64): a joints family, out_dev [B, n_points, 3, T]; point_map (HOST) indexes smplx's joint list extended
 * as model/smpl.py:86-96 does -- 0 .. J-1 the posed joints, J .. J+n_sel-1 the selected vertices, then the n_extra regressed
 * joints -- and root_point is the POINT whose position is subtracted (JOINTSTYPE_ROOT).  Only what the map names is computed. */
typedef struct mdm_smpl_call {
  int32_t pose_rep;            /* MDM_SMPL_*                                                                     */
  int32_t glob;                /* 0: glob_rot_mat is every frame's global orient, every rotation row is a body joint */
  int32_t translation;         /* 1: the last row of x holds the translation in its first 3 features              */
  int32_t vertstrans;          /* 1 (with translation): add translation_t - translation_0                          */
  int32_t n_points;
  int32_t root_point;
  const int32_t* point_map;    /* HOST [n_points]                                                                  */
  const float* glob_rot_mat;   /* HOST [9], row-major; read when glob = 0                                          */
  float beta1;                 /* betas_dev = null: betas = (0, beta1, 0, ...) for every frame                      */
} mdm_smpl_call_t;

/* Bytes of workspace mdm_smpl_forward needs; 0 on a bad argument (mdm_last_error says which).  The bound, in floats:
 *   B * T * (KP + 12 * 24 + 3 + 3 * (J + n_sel + n_extra))     pose features, relative transforms, offsets, joint list
 *   + 16 * 32 * 3 * V                                           only when the map names a regressed joint: the mesh of 16 tiles
 *                                                               of 32 frames at a time (42 MB at V = 6890), whatever B and T are */
size_t mdm_smpl_workspace_bytes(const mdm_smpl_model_t* model, const mdm_smpl_call_t* call, int32_t B, int32_t T);

/* x_dev [B, rows_x, feats_x, T]: rows_x = (glob ? J : J - 1) + (translation ? 1 : 0) and feats_x = the pose_rep's feature count.
 * mask_dev [B, T] uint8 or null (every frame valid): a masked frame is 0 before the root subtraction and the translation add.
 * betas_dev [B, 10, T] or null.  rot_out_dev [B, T, rows of rotations, 3, 3] or null: the rotation matrices of the rows of x
 * (valid frames only are written).  workspace_dev: 16-byte aligned, at least mdm_smpl_workspace_bytes.  No device allocation, no
 * synchronisation, every kernel on `stream`: capture-safe.  T <= 4096, B * T <= 2^24. */
int mdm_smpl_forward(const mdm_smpl_model_t* model, const mdm_smpl_call_t* call, const float* x_dev, const uint8_t* mask_dev,
                     const float* betas_dev, float* out_dev, float* rot_out_dev, int32_t B, int32_t T, int32_t rows_x,
                     int32_t feats_x, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The HumanML3D / KIT evaluator (eval/eval_humanml.py): the networks behind EvaluatorMDMWrapper.get_co_embeddings and
 * get_motion_embeddings (data_loaders/humanml/networks/evaluator_wrapper.py:121-187; modules.py:79-98 MovementConvEncoder,
 * :311-350 TextEncoderBiGRUCo, :353-386 MotionEncoderBiGRUCo), in exact fp32 (additive to ABI 10; kernels: csrc/evaluator.h).
 * Every weight is a caller-owned, 16-byte aligned fp32 DEVICE array, prepared once per model (mdm_amd/evaluator.py does it).
 *
 * One BiGRU encoder (`gru` + `output_net` of either module, with the `input_emb` in front):
 *   in_w [H][in_dim], in_b [H]        input_emb
 *   w_ih [6H][H], b_ih [6H]           weight_ih_l0 then weight_ih_l0_reverse (gate rows r, z, n each), and the biases likewise
 *   w_hh [2][3H][H], b_hh [2][3H]     weight_hh_l0, weight_hh_l0_reverse
 *   h0   [2][H]                       the module's learned `hidden`, broadcast over the batch
 *   o1_w [H][2H], o1_b [H]            output_net.0
 *   ln_g, ln_b [H]                    output_net.1 (LayerNorm, eps 1e-5); output_net.2 is LeakyReLU(0.2)
 *   o2_w [out][H], o2_b [out]         output_net.3
 * H (hidden) must be 256, 512, 768 or 1024; in_dim and out positive multiples of 4. */
typedef struct mdm_eval_gru {
  const float* in_w; const float* in_b;
  const float* w_ih; const float* b_ih;
  const float* w_hh; const float* b_hh;
  const float* h0;
  const float* o1_w; const float* o1_b;
  const float* ln_g; const float* ln_b;
  const float* o2_w; const float* o2_b;
  int32_t in_dim, hidden, out;
} mdm_eval_gru_t;

/* conv1_w [conv_hidden][4][dim_pose - 4] and conv2_w [latent][4][conv_hidden]: the Conv1d(., ., 4, 2, 1) weights with the tap axis
 * moved in front of the input channels (k = tap * C_in + c); out_w [latent][latent] is MovementConvEncoder.out_net.
 * pos_w [word][pos] / in_w of `text` [H][word]: TextEncoderBiGRUCo.pos_emb / input_emb.  motion.in_dim = latent, text.in_dim = word;
 * conv_hidden, latent and word positive multiples of 4; dim_pose >= 5 (263 HumanML3D, 251 KIT: the last 4 features are not read);
 * unit_length = 4, the time reduction of the two convolutions (m_lens // unit_length are the recurrent lengths). */
typedef struct mdm_eval_model {
  const float* conv1_w; const float* conv1_b;
  const float* conv2_w; const float* conv2_b;
  const float* out_w; const float* out_b;
  const float* pos_w; const float* pos_b;
  mdm_eval_gru_t motion;
  mdm_eval_gru_t text;
  int32_t dim_pose, conv_hidden, latent, word, pos, unit_length;
} mdm_eval_model_t;

/* Bytes of workspace the larger of the two calls below needs for B sequences of T frames (motion) and L words (text); either of
 * T and L may be 0 when that call is not made.  0 on a bad argument (mdm_last_error says which).  In floats, per call:
 *   motion: B (T/2 conv_hidden + T/4 (2 latent + 7 H)) + 5 B H        text: B L (word + 7 H) + 5 B H                              */
size_t mdm_eval_workspace_bytes(const mdm_eval_model_t* model, int32_t B, int32_t T, int32_t L);

/* motions_dev [B, T, dim_pose] (T >= 4), lens_dev [B] int32 FRAME counts -> out_dev [B, motion.out]: movement encoder, then the
 * BiGRU over the first lens[b] / unit_length of the T / 4 movement steps of row b, then output_net.  Rows come out in the order
 * they went in (the reordering by length of the reference's wrapper is the caller's).  max_len: an upper bound of lens[] known to
 * the host (the recurrence runs max_len / unit_length steps, at most T / 4), or 0 for T.  A row whose length is below unit_length
 * takes no step and a length beyond T is clamped: the callers refuse both on the host -- the lengths are not read back here.
 * No device allocation, no synchronisation, every kernel on `stream`: capture-safe. */
int mdm_eval_motion_embeddings(const mdm_eval_model_t* model, const float* motions_dev, const int32_t* lens_dev, float* out_dev,
                               int32_t B, int32_t T, int32_t max_len, void* workspace_dev, size_t workspace_bytes, void* stream);

/* word_embs_dev [B, L, word], pos_ohot_dev [B, L, pos], cap_lens_dev [B] int32 -> out_dev [B, text.out]: input_emb(word_embs +
 * pos_emb(pos_ohot)), the BiGRU over the first cap_lens[b] words of row b, output_net.  max_len as above, in words. */
int mdm_eval_text_embeddings(const mdm_eval_model_t* model, const float* word_embs_dev, const float* pos_ohot_dev,
                             const int32_t* cap_lens_dev, float* out_dev, int32_t B, int32_t L, int32_t max_len,
                             void* workspace_dev, size_t workspace_bytes, void* stream);

/* The DistilBERT text encoder of the `text_encoder_type='bert'` checkpoints (model/BERT/BERT_encoder.py: HF DistilBertModel, eval mode):
 * token ids -> last_hidden_state, in exact fp32 (additive to ABI 10; kernels: csrc/text_encoder.h).
 *   x0 = LN(word_emb[id] + pos_emb[t]);  per layer: q, k, v = x W^T + b, heads of 64, p = softmax(q k^T / 8 over keys t' < lens[b]),
 *   x = LN(ctx Wo^T + bo + x), x = LN(gelu_erf(x W1^T + b1) W2^T + b2 + x);  every LN with ln_eps (DistilBERT: 1e-12).
 * Every weight is a caller-owned, 16-byte aligned fp32 DEVICE array, prepared once per model (mdm_amd/text_encoder.py does it).
 *
 * One layer (HF names under transformer.layer.N):
 *   qkv_w [3 dim][dim], qkv_b [3 dim]     attention.q_lin, k_lin, v_lin stacked in that order, the q rows (weight AND bias) already
 *                                         multiplied by 1/8 = 1/sqrt(64)
 *   out_w [dim][dim], out_b [dim]         attention.out_lin          sa_ln_g, sa_ln_b [dim]     sa_layer_norm
 *   lin1_w [hidden][dim], lin1_b [hidden] ffn.lin1                   lin2_w [dim][hidden], lin2_b [dim]   ffn.lin2
 *   out_ln_g, out_ln_b [dim]              output_layer_norm */
typedef struct mdm_text_layer {
  const float* qkv_w; const float* qkv_b;
  const float* out_w; const float* out_b;
  const float* sa_ln_g; const float* sa_ln_b;
  const float* lin1_w; const float* lin1_b;
  const float* lin2_w; const float* lin2_b;
  const float* out_ln_g; const float* out_ln_b;
} mdm_text_layer_t;

/* word_emb [vocab][dim], pos_emb [max_pos][dim], emb_ln_g / emb_ln_b [dim]: embeddings.word_embeddings, position_embeddings,
 * LayerNorm.  layers: a HOST array of n_layers structs.  dim == 64 n_heads and dim <= 1024; hidden a positive multiple of 4;
 * 1 <= n_layers <= 16; vocab >= 1; max_pos >= 1. */
typedef struct mdm_text_model {
  const float* word_emb; const float* pos_emb;
  const float* emb_ln_g; const float* emb_ln_b;
  const mdm_text_layer_t* layers;
  int32_t n_layers, dim, n_heads, hidden, vocab, max_pos;
  float ln_eps;
} mdm_text_model_t;

/* Bytes of workspace mdm_text_encode needs for B prompts padded to L word pieces; 0 on a bad argument (mdm_last_error says which).
 * In floats: B L (5 dim + hidden)  -- the token rows, their q | k | v, the attention output and the feed-forward's hidden rows --
 * plus 64 bytes. */
size_t mdm_text_workspace_bytes(const mdm_text_model_t* model, int32_t B, int32_t L);

/* ids_dev [B, L] int32 (right-padded prompts), lens_dev [B] int32 valid word pieces per prompt -> out_dev [B, L, dim], or
 * [L, B, dim] with token_major != 0 (what the decoder's memory wants).  Rows at or beyond a length are written as zeros; the ids
 * behind a length are not read, and a valid row does not depend on L, on B or on the other prompts (bit for bit).
 * 1 <= L <= min(128, max_pos).  lens[b] in [1, L] and ids < vocab are the caller's duty (a host tokenizer made them; an id outside
 * the table is clamped into it, a length outside [0, L] likewise).  workspace_dev: at least mdm_text_workspace_bytes.
 * 7 launches per layer and one for the embeddings.  No device allocation, no synchronisation, every kernel on `stream`: capture-safe. */
int mdm_text_encode(const mdm_text_model_t* model, const int32_t* ids_dev, const int32_t* lens_dev, float* out_dev, int32_t B,
                    int32_t L, int32_t token_major, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The ST-GCN action recogniser of the UESTC evaluation (eval/a2m/stgcn_eval.py -> eval/a2m/recognition/models/stgcn.py, ten blocks,
 * V = 24, 6 input channels) and of the unconstrained evaluation (eval/unconstrained/evaluate.py -> eval/unconstrained/models/stgcn.py,
 * six blocks, V = 15, 3 input channels): eval mode, one person per sample, no length mask (the reference applies none), in exact fp32
 * (additive to ABI 10; kernels: csrc/stgcn.h).  One entry point serves both networks: the network is a HOST array of block
 * descriptors.  Every weight is a caller-owned, 16-byte aligned DEVICE array prepared once per model (mdm_amd/stgcn.py does it);
 * "BN" below is BatchNorm2d in eval mode folded with the bias in front of it: scale = gamma / sqrt(var + eps),
 * shift = (bias - mean) scale + beta, formed in fp64 and rounded once.
 *
 * One block (reference names under st_gcn_networks.N), with A_b = A * edge_importance[N] of shape [K][V][V] and c_in_p = c_in
 * rounded up to a multiple of 4 (only the first block's c_in may need it; the pad columns of its weights are zero):
 *   gcn_w   [c_out][K][c_in_p]     gcn.conv.weight [K c_out][c_in] with the k axis moved behind c_out (contraction index k c_in_p + ci)
 *   gcn_scale [c_out]              tcn.0 (BN)
 *   gcn_shift [V][c_out]           (sum_k gcn.conv.bias[k c_out + c] sum_v A_b[k][v][w] - mean[c]) scale[c] + beta[c]   per node w
 *   nbr_idx [K][V][8] int32, nbr_w [K][V][8], nbr_cnt [K][V] int32
 *                                  the non-zero A_b[k][v][w] of each (k, w): the v's in ascending order, their values, how many
 *                                  (at most MDM_STGCN_MAX_NEIGHBOURS; idx < V; entries behind cnt are not read; a count or an index
 *                                  outside its range is clamped into it)
 *   tcn_w   [c_out][9][c_out]      tcn.2.weight [c_out][c_out][9][1] tap-major (contraction index tap c_out + c)
 *   tcn_scale, tcn_shift [c_out]   tcn.3 (BN) with tcn.2.bias
 *   residual                       MDM_STGCN_RES_NONE; _IDENTITY (c_in == c_out, stride 1: the block's input is added);
 *                                  _CONV: res_w [c_out][c_in_p] (residual.0.weight), res_scale, res_shift [c_out] (residual.1 with
 *                                  residual.0.bias)
 * The block computes  y = relu(BN(gcn(x)));  out = relu(BN(conv9x1_stride(y)) + residual(x)),  T_out = (T - 1) / stride + 1. */
#define MDM_STGCN_RES_NONE 0
#define MDM_STGCN_RES_IDENTITY 1
#define MDM_STGCN_RES_CONV 2
#define MDM_STGCN_MAX_BLOCKS 16
#define MDM_STGCN_MAX_NEIGHBOURS 8

typedef struct mdm_stgcn_block {
  const float* gcn_w; const float* gcn_scale; const float* gcn_shift;
  const int32_t* nbr_idx; const float* nbr_w; const int32_t* nbr_cnt;
  const float* tcn_w; const float* tcn_scale; const float* tcn_shift;
  const float* res_w; const float* res_scale; const float* res_shift;   /* MDM_STGCN_RES_CONV only, else null */
  int32_t c_in, c_out, stride, residual;
} mdm_stgcn_block_t;

/* blocks: a HOST array of n_blocks (1 .. MDM_STGCN_MAX_BLOCKS) descriptors; blocks[0].c_in is the input's channel count C (any
 * positive number), every other c_in equals the c_out in front of it, every c_out is a positive multiple of 4 and the last one at
 * most 1024; stride 1 .. 4.  V nodes (1 .. 64), K graph kernels (1 .. 8).  in_scale / in_shift [V C]: data_bn (BatchNorm1d over the
 * V C channels, eval mode) as x scale + shift.  fcn_w [num_class][c_out of the last block], fcn_b [num_class]: the 1 x 1 `fcn`. */
typedef struct mdm_stgcn_model {
  const mdm_stgcn_block_t* blocks;
  const float* in_scale; const float* in_shift;
  const float* fcn_w; const float* fcn_b;
  int32_t n_blocks, V, K, num_class;
} mdm_stgcn_model_t;

/* Bytes of workspace mdm_stgcn_forward needs for N samples of T frames; 0 on a bad argument (mdm_last_error says which).  In floats:
 * three buffers of  max(N T V c_in_p of block 0, max over blocks of N T_b V c_out_b)  -- a block's input, the graph convolution's
 * output and the block's output, T_b the block's INPUT frames -- plus 64 bytes. */
size_t mdm_stgcn_workspace_bytes(const mdm_stgcn_model_t* model, int32_t N, int32_t T);

/* x_dev [N, V, C, T] (the reference's batch["output"] / batch["x"]: T contiguous) -> features_dev [N, c_out of the last block], the
 * mean over the last block's T' V positions, and yhat_dev [N, num_class], the logits.  A sample's results do not depend on N or on
 * its row (bit for bit): one tile shape, one k order, fixed neighbour and pooling orders.  N >= 1, 1 <= T <= 65536, and
 * N T V times the widest row below 2^31 (chunk the samples otherwise).  Launches: 1 + per block 2 (3 with a convolutional
 * residual) + 1.  No device allocation, no synchronisation, every kernel on `stream`: capture-safe. */
int mdm_stgcn_forward(const mdm_stgcn_model_t* model, const float* x_dev, float* features_dev, float* yhat_dev, int32_t N, int32_t T,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* The HumanAct12 GRU action recogniser behind A2MEvaluation (eval/a2m/gru_eval.py -> eval/a2m/action2motion/models.py:6-61,
 * MotionDiscriminator / MotionDiscriminatorForFID): nn.GRU(input_size, hidden_size, num_layers) over the frames, the last layer's
 * output at frame lengths[b] - 1, features = tanh(linear1(.)), yhat = linear2(features); exact fp32 (additive to ABI 10; kernels:
 * csrc/gru_recogniser.h).  Every weight is a caller-owned, 16-byte aligned DEVICE array in PyTorch's own layout:
 *   layers[l].w_ih [3 H][I] (l = 0) or [3 H][H], w_hh [3 H][H], b_ih, b_hh [3 H]     recurrent.{weight,bias}_{ih,hh}_l<l>, gates r | z | n
 *   lin1_w [mid][H], lin1_b [mid], lin2_w [num_class][mid], lin2_b [num_class]       linear1, linear2
 * hidden_size 128 (the published checkpoint; 32 is built as the reduced width of the emulator tests), num_layers 1 .. 4, input_size
 * any positive number (72 for HumanAct12, 54 for NTU-13), mid (30) and num_class 1 .. 64. */
#define MDM_GRU_CLS_MAX_LAYERS 4

typedef struct mdm_gru_cls_layer {
  const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh;
} mdm_gru_cls_layer_t;

typedef struct mdm_gru_cls_model {
  mdm_gru_cls_layer_t layers[MDM_GRU_CLS_MAX_LAYERS];      /* the first num_layers are read */
  const float* lin1_w; const float* lin1_b; const float* lin2_w; const float* lin2_b;
  int32_t input_size, hidden_size, num_layers, mid, num_class;
} mdm_gru_cls_model_t;

/* Bytes of workspace mdm_gru_cls_forward needs for B sequences of T frames; 0 on a bad argument (mdm_last_error says which).  In
 * floats: B T 3 H (a layer's input projections) + B T H (a layer's outputs; only with num_layers > 1) + B H, plus 64 bytes. */
size_t mdm_gru_cls_workspace_bytes(const mdm_gru_cls_model_t* model, int32_t B, int32_t T);

/* x_dev [B, I, T] (the reference's [bs, njoints, nfeats, T]: T contiguous), lens_dev int32 [B], h0_dev [num_layers, B, H] (the
 * reference's `hidden_unit`) -> features_dev [B, mid] (what MotionDiscriminatorForFID returns) and yhat_dev [B, num_class] (what
 * MotionDiscriminator returns).  lens_dev is read on the device and clamped to [1, T] (the reference wraps a zero length to the
 * last frame and fails beyond T); frames behind a row's length are not read.  A row's results do not depend on B, on its position
 * or on the other rows' lengths (bit for bit).  Refused with a message: a null pointer; a weight that is not 16-byte aligned or an
 * x_dev / lens_dev / h0_dev / features_dev / yhat_dev that is not 4-byte aligned; B or T < 1; a hidden_size without an
 * instantiation; num_layers outside 1 .. 4; a workspace below mdm_gru_cls_workspace_bytes; B T 3 H >= 2^31 (chunk the rows).
 * Launches: per layer one GEMM and ONE recurrence kernel (all T steps; no cross-workgroup synchronisation), + 1.  Joins the
 * one-chain-per-device guard (CONCURRENCY).  No device allocation, no synchronisation, every kernel on `stream`: capture-safe. */
int mdm_gru_cls_forward(const mdm_gru_cls_model_t* model, const float* x_dev, const int32_t* lens_dev, const float* h0_dev,
                        float* features_dev, float* yhat_dev, int32_t B, int32_t T, void* workspace_dev, size_t workspace_bytes,
                        void* stream);

/* The text tower of OpenAI CLIP (clip/model.py CLIP.encode_text; ViT-B/32 conditions the `text_encoder_type='clip'` checkpoints):
 * token ids -> text_embed, in exact fp32 (additive to ABI 10; kernels: csrc/clip_text.h, csrc/text_encoder.h).
 *   x = tok_emb[id] + pos_emb[t];  per layer (pre-LN, eps 1e-5): x += out(attn(ln_1(x))), causal (query t sees the keys t' <= t),
 *   heads of 64, scores / 8;  x += proj(quick_gelu(fc(ln_2(x)))), quick_gelu(v) = v sigmoid(1.702 v);
 *   out[b] = ln_final(x[b, lens[b] - 1]) text_proj^T, lens[b] - 1 being the prompt's EOT (upstream: argmax of the ids).
 * Every weight is a caller-owned, 16-byte aligned fp32 DEVICE array, prepared once per model (mdm_amd/clip_text.py does it).
 *
 * One layer (OpenAI names under transformer.resblocks.N):
 *   ln1_g, ln1_b [dim]                    ln_1                       ln2_g, ln2_b [dim]         ln_2
 *   qkv_w [3 dim][dim], qkv_b [3 dim]     attn.in_proj_weight / in_proj_bias, the q rows (weight AND bias) already multiplied by 1/8
 *   out_w [dim][dim], out_b [dim]         attn.out_proj
 *   fc_w [mlp][dim], fc_b [mlp]           mlp.c_fc                   proj_w [dim][mlp], proj_b [dim]   mlp.c_proj */
typedef struct mdm_clip_text_layer {
  const float* ln1_g; const float* ln1_b;
  const float* qkv_w; const float* qkv_b;
  const float* out_w; const float* out_b;
  const float* ln2_g; const float* ln2_b;
  const float* fc_w; const float* fc_b;
  const float* proj_w; const float* proj_b;
} mdm_clip_text_layer_t;

/* tok_emb [vocab][dim], pos_emb [max_pos][dim]: token_embedding.weight, positional_embedding.  lnf_g / lnf_b [dim]: ln_final.
 * text_proj [embed][dim]: text_projection TRANSPOSED (upstream keeps [dim][embed]).  layers: a HOST array of n_layers structs.
 * dim == 64 n_heads and dim <= 1024; mlp and embed positive multiples of 4; 1 <= n_layers <= 32; vocab >= 1; max_pos >= 1. */
typedef struct mdm_clip_text_model {
  const float* tok_emb; const float* pos_emb;
  const float* lnf_g; const float* lnf_b;
  const float* text_proj;
  const mdm_clip_text_layer_t* layers;
  int32_t n_layers, dim, n_heads, mlp, vocab, max_pos, embed;
} mdm_clip_text_model_t;

/* Bytes of workspace mdm_clip_text_encode needs for B prompts padded to L tokens; 0 on a bad argument (mdm_last_error says which).
 * In floats: B L (6 dim + mlp) + B dim  -- the residual rows, their LayerNorm, q | k | v, the attention output, the mlp's hidden rows
 * and the normalised EOT rows -- plus 64 bytes. */
size_t mdm_clip_text_workspace_bytes(const mdm_clip_text_model_t* model, int32_t B, int32_t L);

/* ids_dev [B, L] int32, lens_dev [B] int32 (tokens per prompt up to and including its EOT) -> out_dev [B, embed].  The ids behind a
 * length are not read, and a prompt's row does not depend on L, on B or on the other prompts (bit for bit); pass L = max(lens),
 * not the tokenizer's context length.  1 <= L <= min(128, max_pos).  lens[b] in [1, L] and ids < vocab are the caller's duty (a
 * host tokenizer made them; an id outside the table is clamped into it, a length outside [1, L] likewise).  Refused with a message:
 * a null model or pointer, a weight or out_dev that is not 16-byte aligned (named), dim != 64 n_heads, dim > 1024, L > max_pos,
 * B L times the widest row >= 2^31 (chunk the prompts), a workspace below mdm_clip_text_workspace_bytes.
 * Launches: one for the embedding, 7 per layer, two for ln_final over the EOT rows and the projection.  Joins the
 * one-chain-per-device guard (CONCURRENCY).  No device allocation, no synchronisation, every kernel on `stream`: capture-safe. */
int mdm_clip_text_encode(const mdm_clip_text_model_t* model, const int32_t* ids_dev, const int32_t* lens_dev, float* out_dev,
                         int32_t B, int32_t L, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- The metrics of the unconstrained evaluation (eval/unconstrained/evaluate.py) on feature matrices [rows, D], fp32, row-major,
 * on the device: improved precision / recall, KID, the FID statistics, diversity.  (Additive to ABI 10.)
 *
 * Common to the five calls: every pointer is a device pointer; feature matrices and fp32 / int32 arrays 4-byte aligned (rows take
 * 16-byte loads when D % 4 == 0 and the matrix lies on a 16-byte boundary), fp64 outputs 8-byte aligned; D >= 1; rows * D < 2^31.
 * Refused with a message (mdm_last_error) before anything is launched: a null or misaligned pointer, a size out of range, a
 * workspace below mdm_metrics_workspace_bytes.  Index tables are trusted to be in range.  Distances are sum_j (a_j - b_j)^2 in fp32,
 * one fixed order over j for every pair (never the Gram form): d2 of two rows is the same bits in every call, at every position, and
 * exactly 0 for equal rows.  No atomics; every sum in one fixed order: repeated calls return the same bits.  Each call joins the
 * one-chain-per-device guard (CONCURRENCY).  No device allocation, no synchronisation, every kernel on `stream`: capture-safe. */
#define MDM_METRICS_KNN_RADIUS 0
#define MDM_METRICS_MANIFOLD_MEMBERS 1
#define MDM_METRICS_GATHER_DIST 2
#define MDM_METRICS_POLY_MMD 3
#define MDM_METRICS_FEATURE_STATS 4
#define MDM_METRICS_RETRIEVAL_RANKS 5
#define MDM_METRICS_DIST_MATRIX 6
#define MDM_METRICS_CONFUSION 7

/* Bytes of workspace of the call `kind` (MDM_METRICS_*) on `rows` rows; 0 on a bad argument (mdm_last_error says which).
 * MDM_METRICS_POLY_MMD: rows = the subset size m, subsets = S; 2 S ceil(m / 64) 16 doubles plus 64 bytes; subsets * rows < 2^31 and
 * subsets < 65536 (chunk the subsets: a subset's result does not depend on the others).  Every other kind: 64 bytes, `subsets` ignored. */
size_t mdm_metrics_workspace_bytes(int32_t kind, int32_t rows, int32_t subsets);

/* radius2_dev[i] = the (k+1)-th smallest squared distance from row i of a_dev [N, D] to the rows of a_dev, row i itself included
 * (np.partition(distances, k)[k] of precision_recall.py, squared).  1 <= k <= 7, N >= k + 1.  One launch. */
int mdm_knn_radius(const float* a_dev, int32_t N, int32_t D, int32_t k, float* radius2_dev, void* workspace_dev, size_t workspace_bytes,
                   void* stream);

/* member_dev[b] (uint8) = 1 if a row a' of a_dev [NA, D] has d2(b_dev[b], a') <= radius2_dev[a'], else 0, for the NB rows of b_dev;
 * count_dev (int32) = their sum.  The comparison is in the squared domain, on the values mdm_knn_radius compares.  Two launches. */
int mdm_manifold_members(const float* a_dev, const float* radius2_dev, int32_t NA, const float* b_dev, int32_t NB, int32_t D,
                         uint8_t* member_dev, int32_t* count_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* dist_dev[p] = || x[first_dev[p]] - x[second_dev[p]] || for P >= 1 index pairs into x_dev [N, D]; mean_dev (fp64) = their mean,
 * added in fp64 in a fixed order.  Two launches. */
int mdm_gather_dist(const float* x_dev, int32_t N, int32_t D, const int32_t* first_dev, const int32_t* second_dev, int32_t P,
                    float* dist_dev, double* mean_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* kid.py polynomial_mmd with the `unbiased` estimator for S subsets at once: subset s is X = g_dev[idx_g_dev[s]] and
 * Y = r_dev[idx_r_dev[s]] (index tables [S, m] int32), K = (gamma <x, y> + coef0)^degree with <x, y> in exact fp32 (k ascending) and
 * everything behind it in fp64; mmd2_dev[s] and var_dev[s] (fp64; var at `var_at_m` >= 2) from _mmd2_and_variance's sums.
 * m >= 3, degree >= 1.  No m x m matrix is written.  Two launches. */
int mdm_poly_mmd(const float* g_dev, int32_t Ng, const float* r_dev, int32_t Nr, int32_t D, const int32_t* idx_g_dev,
                 const int32_t* idx_r_dev, int32_t S, int32_t m, double gamma, double coef0, int32_t degree, int32_t var_at_m,
                 double* mmd2_dev, double* var_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* mu_dev [D] = the column means, sigma_dev [D, D] = the covariance (two-pass, centred, divisor N - 1: np.cov(rowvar=False)) of
 * x_dev [N, D], both in fp64.  N >= 2, D * D < 2^31.  Two launches. */
int mdm_feature_stats(const float* x_dev, int32_t N, int32_t D, double* mu_dev, double* sigma_dev, void* workspace_dev,
                      size_t workspace_bytes, void* stream);

/* ---- The metrics of the HumanML3D / KIT evaluation (data_loaders/humanml/utils/metrics.py: R-precision, matching score, the
 * distance matrix) and the a2m family's accuracy (eval/a2m/ * /accuracy.py), on device features.  (Additive to ABI 10.)  The common
 * rules of the five calls above hold: the same distance statement, the same refusals before any launch, the one-chain guard, no
 * device allocation, no synchronisation, capture-safe.
 *
 * mdm_retrieval_ranks: q_dev (texts) and c_dev (motions) are [N, D]; group_offsets_dev [n_groups + 1] (int32, ascending, [0] == 0,
 * [n_groups] == N) cuts the rows into the reference's batches, each of 1 .. max_group_rows rows (sizes may differ).  Row i of a group
 * [b, e):  diag_dev[i] = sqrt(d2(q_i, c_i));  rank_dev[i] = #{j in [b, e): d2(q_i, c_j) < d2(q_i, c_i)} + #{j in [b, i): d2(q_i, c_j) ==
 * d2(q_i, c_i)}, the position of i in a stable ascending sort of row i of the group's distance matrix (np.argsort + calculate_top_k
 * whenever the row has no tie).  topk_count_dev[k] (int64, k < top_k, 1 <= top_k <= 16) = #{i: rank[i] <= k} (top_k_mat.sum(axis=0)
 * over all groups); diag_sum_dev (fp64) = the sum of diag in row order.  The table is read on the device and clamped there (offsets
 * into [0, N], ends to their begins, sizes to max_group_rows): a corrupt table gives wrong ranks, never an access out of bounds; rows
 * that no group covers are not written.  A row's rank and diag do not depend on the other groups.  Two launches. */
int mdm_retrieval_ranks(const float* q_dev, const float* c_dev, int32_t N, int32_t D, const int32_t* group_offsets_dev,
                        int32_t n_groups, int32_t max_group_rows, int32_t top_k, int32_t* rank_dev, float* diag_dev,
                        int64_t* topk_count_dev, double* diag_sum_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* out_dev[i][j] = sqrt(d2(a_dev[i], b_dev[j])) for a_dev [NA, D], b_dev [NB, D], out_dev [NA, NB] fp32 (euclidean_distance_matrix
 * without the Gram form's cancellation: exactly 0 for equal rows, never NaN for finite rows).  NA * NB < 2^31.  One launch. */
int mdm_dist_matrix(const float* a_dev, int32_t NA, const float* b_dev, int32_t NB, int32_t D, float* out_dev, void* workspace_dev,
                    size_t workspace_bytes, void* stream);

/* pred_dev[n] = argmax_c yhat_dev[n][c] for yhat_dev [N, C]: the lowest index among equal maxima, a NaN counts as the maximum and the
 * first NaN wins (what the reference's `.max(dim=1).indices` returns on the host).  confusion_dev [C, C] (int64): [labels_dev[n]][pred_dev[n]] += 1 -- the call ADDS to
 * the matrix, which the caller zeroes once and may then feed batch by batch (integer atomics: the result does not depend on their
 * order).  A label outside [0, C) is not counted; it adds 1 to bad_dev (int32, also accumulated).  N * C, C * C < 2^31.  One launch. */
int mdm_confusion(const float* yhat_dev, const int32_t* labels_dev, int32_t N, int32_t C, int32_t* pred_dev, int64_t* confusion_dev,
                  int32_t* bad_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- The Frechet distance of two Gaussians on the device (calculate_frechet_distance of eval/a2m/action2motion/fid.py and
 * data_loaders/humanml/utils/metrics.py), in fp64, from the statistics mdm_feature_stats writes.  (Additive to ABI 10.)
 *
 * Tr sqrtm(sigma1 sigma2) = sum_i sqrt(lambda_i(M)), M = S^T sigma2 S, S = V diag(sqrt(max(w, 0))), sigma1 = V diag(w) V^T: two
 * symmetric eigen-solves (two-sided cyclic Jacobi on a round-robin schedule; the first with vectors) and two D x D x D products on
 * v_mfma_f64_16x16x4_f64 between them.  Both covariances are taken by their symmetric parts (s_ij + s_ji) / 2.  No complex
 * arithmetic, no division by a small eigenvalue, no eps retry: a singular product is finite.  D <= 64 (rounded up to even): each
 * solve is one launch of one workgroup; above: one launch per round of D - 1 (D odd: D) rounds per sweep, 30 sweeps enqueued, every
 * launch behind the first sweep that rotated nothing returns at once (convergence is detected on the device; nothing is read back).
 *
 * result4_dev (fp64): [0] = |mu1 - mu2|^2 + Tr sigma1 + Tr sigma2 - 2 [1];  [1] = sum_i sqrt(max(lambda_i, 0));  [2] = min w / max w
 * of sigma1;  [3] = min lambda / max lambda of M (a spectrum without a positive value: 0 when it is all zero, -inf when it holds a
 * negative one).  sweeps2_dev (int32): per solve, the sweeps that performed a rotation; 30: the solve did not converge, and then
 * result4_dev is NaN, never a plausible number.  Every sum is fp64 in a fixed order; the only atomics count rotations: repeated
 * calls return the same bits.  Refused with a message before anything is launched: a null pointer, an fp64 pointer off an 8-byte
 * boundary, D outside 1 .. 1024, a missing workspace, one below mdm_frechet_workspace_bytes (MDM_ENOSPC).  Joins the
 * one-chain-per-device guard (CONCURRENCY).  No device allocation, no synchronisation, every kernel on `stream`: capture-safe after
 * one warm-up call of a D <= 64 outside the capture (the one-workgroup solve opts in to 66 KB of LDS at its first use). */

/* Bytes of workspace of mdm_frechet_distance at D features: 64 + 1 KB + 16 KB + seven fp64 matrices of D (rounded up to even)
 * squared; 0 for D < 1 or D > 1024 (mdm_last_error says so). */
size_t mdm_frechet_workspace_bytes(int32_t D);

int mdm_frechet_distance(const double* mu1_dev, const double* sigma1_dev, const double* mu2_dev, const double* sigma2_dev, int32_t D,
                         double* result4_dev, int32_t* sweeps2_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- SMPLify: fitting SMPL to 22 generated joints per frame (visualize/simplify_loc2rot.py joints2smpl over
 * visualize/joints2smpl/src/smplify.py SMPLify3D, use_lbfgs=True, use_collision=False, joints_category="AMASS", seq_ind = 0).
 * (Additive to ABI 10.)
 *
 * The losses read the 24 skeleton joints only, and those depend on the 24 rotations and on rest joints that are affine in the betas:
 * no vertex is computed.  One kernel launch per closure evaluation returns the loss, its analytic gradient in the optimiser's flat
 * layout and, from a fixed-order reduction (no atomics), the loss, max|g| and g . d; the host runs the control flow of
 * PyTorch 2.10's optim.LBFGS.step with line_search_fn='strong_wolfe' on those scalars and reads them from pinned memory after
 * every evaluation and every new direction.  mdm_smplify_value_grad and mdm_smplify_fit therefore SYNCHRONISE with `stream`, cannot be
 * captured into a hipGraph (refused with MDM_EUNSUPPORTED on a capturing stream) and hold the one-chain-per-device guard
 * (CONCURRENCY) for the whole call.  Every host loop is counted: a call ends whatever the data is.
 *
 * Flat layout of the variables, T frames: step 1 (camera_fitting_loss_3d) [global_orient T x 3 | camera_t T x 3]; step 2
 * (body_fitting_loss_3d) [body_pose T x 69 | betas T x 10 | global_orient T x 3 | camera_t T x 3] -- the order of the reference's
 * parameter lists.  Frames are [T][22][3] joints, conf [22]. */
typedef struct {
  const float* j0;                  /* [24][3]      J_regressor . v_template                                  (device, 16-byte aligned) */
  const float* jdirs;               /* [24][3][10]  J_regressor . shapedirs                                                             */
  const float* means;               /* [8][69]      the mixture prior's means (prior.py MaxMixturePrior)                                */
  const float* precisions;          /* [8][69][69]  its precisions: the float32 inverses of the float32 covariances                     */
  const float* neg_log_nll_weights; /* [8]          -log(nll_weights)                                                                   */
  const int32_t* parents;           /* [24]         host; parents[0] = -1, parents[i] < i                                               */
} mdm_smplify_model_t;

typedef struct {
  int32_t num_iters;        /* 150: max_iter of both optimisers (max_eval = num_iters * 5 / 4)                    */
  int32_t history;          /* 100: history_size, at most 128                                                     */
  int32_t stage1_calls;     /* 10:  step() calls of the camera optimiser                                          */
  int32_t stage2_calls;     /* num_iters: step() calls of the body optimiser                                      */
  double step_size;         /* 1e-2: lr                                                                           */
  double tolerance_grad;    /* 1e-7                                                                               */
  double tolerance_change;  /* 1e-9                                                                               */
  double joint_weight;      /* 600   (all weights enter squared, as in customloss.py)                             */
  double sigma;             /* 100   gmof                                                                         */
  double pose_prior_weight; /* 4.78 * 1.5                                                                         */
  double angle_prior_weight;/* 15.2                                                                               */
  double shape_prior_weight;/* 5                                                                                  */
  double pose_preserve_weight; /* 5                                                                               */
  double depth_weight;      /* 100   camera_fitting_loss_3d; its term counts four times (the reference's broadcast) */
} mdm_smplify_call_t;

/* Bytes of workspace of both calls below at T frames (1 <= T <= 4096): the vectors, five gradient buffers and 2 * history pairs of
 * 85 T floats each; 0 on a bad argument (mdm_last_error says which). */
size_t mdm_smplify_workspace_bytes(const mdm_smplify_model_t* model, const mdm_smplify_call_t* call, int32_t T);

/* The loss of step `stage` (1 or 2) and its gradient at the point x_dev (flat layout).  fixed_pose_dev [T][69]: step 1 the body pose,
 * step 2 preserve_pose; fixed_betas_dev [T][10] and cam_est_dev [T][3] (guess_init_3d): step 1 only.  dir_dev: a direction in the
 * flat layout, or null.  Writes grad_dev (flat), terms_dev [T][6] (step 2: joints, prior, angle, shape, preserve, total; step 1:
 * joints, depth -- counted once --, 0, 0, 0, total), joints_dev [T][24][3] (the model joints without the camera; may be null) and on
 * the host scalars_host[3] = loss, max|g|, g . dir.  A frame's terms and gradient are the same bits at every position and T.  A
 * non-finite pose, betas, j3d or conf is refused with MDM_EINVAL before any output is written; a loss, gradient or g . dir that is
 * not finite for another reason (the camera block of x, cam_est, the fixed pose of step 2, dir) is refused with MDM_EINVAL behind
 * the evaluation: the device outputs are written, scalars_host is not.  Two launches, two reads. */
int mdm_smplify_value_grad(const mdm_smplify_model_t* model, const mdm_smplify_call_t* call, int32_t stage, const float* x_dev,
                           const float* dir_dev, const float* fixed_pose_dev, const float* fixed_betas_dev, const float* cam_est_dev,
                           const float* j3d_dev, const float* conf_dev, int32_t T, float* grad_dev, float* terms_dev, float* joints_dev,
                           float* scalars_host, void* workspace_dev, size_t workspace_bytes, void* stream);

/* SMPLify3D.__call__: from init_pose_dev [T][72] (global orient, then body pose) and init_betas_dev [T][10], the camera guess, step 1
 * and step 2.  Writes pose_out_dev [T][72], betas_out_dev [T][10], cam_out_dev [T][3], joints_out_dev [T][24][3] (the fitted model
 * joints, without the camera) and thetas_out_dev [25][6][T] (simplify_loc2rot.py:108-112: rot6d of the pose through
 * axis_angle_to_matrix, row 24 = (j3d[:, 0], 0, 0, 0)), and on the host stats_host[6] = function evaluations, iterations and final
 * loss of step 1, then of step 2 (its final loss as SMPLify3D reports it, pose_preserve_weight 0).  Once a step() call returns at
 * its first max|g| <= tolerance_grad check the stage ends: every later call would evaluate the same point and return too.  A
 * non-finite input is refused with MDM_EINVAL before any output is written. */
int mdm_smplify_fit(const mdm_smplify_model_t* model, const mdm_smplify_call_t* call, const float* init_pose_dev,
                    const float* init_betas_dev, const float* j3d_dev, const float* conf_dev, int32_t T, float* pose_out_dev,
                    float* betas_out_dev, float* cam_out_dev, float* joints_out_dev, float* thetas_out_dev, double* stats_host,
                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* The line search of mdm_smplify_fit (PyTorch's _strong_wolfe, c1 = 1e-4, c2 = 0.9) on a recorded objective, host only:
 * evaluation i returns f_seq[i] and gtd_seq[i] whatever step it asks for, and the step it asked for is written to t_seq[i].  Starts
 * at step t0 from (f0, gtd0) with max|d| = d_norm.  float32_tensors != 0: g . d and max|d| are 0-dim float32 tensors as in the fit
 * (every value derived from them is rounded to float, as PyTorch does); 0: everything in double.  Returns the number of evaluations,
 * the final step and its loss. */
int mdm_smplify_strong_wolfe(const double* f_seq, const double* gtd_seq, int32_t n_seq, double t0, double f0, double gtd0, double d_norm,
                             double tolerance_change, int32_t max_ls, int32_t float32_tensors, double* t_seq, int32_t* n_evals,
                             double* t_final, double* f_final);

#ifdef __cplusplus
}
#endif
#endif /* MDM_HIP_H */
