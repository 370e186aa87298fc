// Split-precision ("f16x3"; round 1: "bf16x3") MFMA GEMM for the encoder's dense contractions:
//     C[m][n] = sum_k A[m][k] * W[n][k],   A = Ah + Al,  W = Wh + Wl  (fp16 planes: common.h split_p16)
//             ~ sum_k  Ah*Wh + Ah*Wl + Al*Wh            three fp16 MFMA passes, fp32 accumulate.
//
// Why: the reference computes these `addmm`s in fp32 (model/mdm.py:77-84 -> torch TransformerEncoderLayer) and
// BASELINE's parity bar is 1e-3 max-abs over a 50-step guided trajectory.  gfx950 has no TF32; exact-fp32 MFMA
// peaks at 157 TFLOP/s, fp16 / bf16 MFMA at 2.5 PFLOP/s, so three 16-bit passes carry a ~2^-22- (fp16) / ~2^-16- (bf16) relative fp32 product at up to
// ~5x the fp32 rate.  Replaces in_proj / out_proj / linear1 / linear2 and,
// with K / N padded, InputProcess and OutputProcess (rows a12, a16); the LayerNorms between them are folded into the
// epilogues (X3Epilogue).  The exact-fp32 kernel (gemm_f32.h) remains the `f32` mode.
//
// Data layout.  Activations: two 16-bit planes [rows][K] (hi, lo), K contiguous, written by the PRODUCING kernel's
// epilogue.  Weights: split ONCE (mdm_prepare), as hi / lo of w * 2^8 (common.h kX3WeightScale; the epilogue scales the
// accumulators back), and stored in MFMA-FRAGMENT order
//     Wp[plane][n/32][k/16][lane 0..63][8]      lane = (n%32) + 32*((k%16)/8),  element j = k%8
// so the B-operand fragment of one wave for one 16-deep k sub-step is ONE contiguous, perfectly coalesced 1 KB
// global_load_dwordx4 -- weights never pass through LDS (a wave's 32 output columns are private to it, so staging them
// in LDS bought nothing and cost an LDS-DMA write plus an LDS read per byte).
//
// Machine mapping (gfx950).  One PERSISTENT workgroup of eight waves per CU works on 256-column tiles whose row extent is a whole
// number of token sequences (S = 197 -> one sequence per tile), so the headline shape (256 sequences, N in {512, 1024, 1536}) gives
// every CU exactly N/256 equal tiles; each wave owns 32 output columns x all rows of the tile.  Two k-loops exist:
//   * the PIPELINED loop (X3_PIPE; 208-row tiles, an even number of 32-deep k steps: every encoder GEMM but InputProcess) runs
//     the whole tile on v_mfma_f32_16x16x32_f16: per wave 13 row slices of 16 x 2 column halves of f32x4 accumulators (104 VGPRs),
//     the A fragment of a slice one ds_read_b128 per plane, the W fragments read from the same fragment-ordered planes through a
//     per-lane remap.  Every stream runs AHEAD of the matrix work: A in four LDS stages (A(g+3) is issued during step g; each wave
//     retires its own pieces of A(g+1) with a COUNTED vmcnt in the middle of the step, then one bare s_barrier -- no drain --
//     makes them visible), W in four register slots (two column halves x step parity) refilled in place for step g+2, the fragment reads two elements
//     ahead across step and stage boundaries: the pipeline never restarts inside a tile (details at the k-loop);
//   * the STEP-SYNCHRONOUS loop (InputProcess, K = 288: nine steps; odd step counts; 224-row tiles) runs on v_mfma_f32_32x32x16_f16,
//     7 row sub-tiles of 32 (112 VGPRs) or, on 208-row tiles (X3_T16), six plus one 16-row sub-tile on 16x16x32: two LDS stages,
//     A(g+1) and W(g+1) fetched during step g, every step closed by vmcnt(0) and one barrier.
// While this kernel runs the chip sits at its power limit (zero-filled operands: +16-22 %) and the costs of the parts add up
// instead of overlapping -- MFMA-only 141 us + epilogue stores 25-40 + fragment reads / barriers 18 + loads 32 = 230 us for
// in_proj (profiles/r01c_final.md).  What pays is less work and fewer bytes.
//   * A tile: global -> LDS by global_load_lds_dwordx4, BK = 32, stages of Ah|Al [224][32] = 28 KB; the pieces a
//     wave issues per step ride BETWEEN the MFMA units; the stream has its own (tile, k) cursor ahead of the matrix work and
//     rolls over into the workgroup's next tile, so the pipeline never drains at a tile boundary;
//   * LDS image: row-major, 64-byte rows, 16-byte chunk index XOR-swizzled with x3_swz((row>>2)&3), x3_swz = (0, 2, 3, 1) (below):
//     one image whose ds_read_b128 lane groups are conflict-free on the 16x16x32 read pattern AND on both 32x32x16 ones (rounds
//     1-7 XORed with (row>>2)&3 itself: conflict-free on 32x32x16 only, 2-way on the 16x16x32 reads round 7 moved the tile to);
//     LDS-DMA writes lane-linearly, so the swizzle is applied to the per-lane SOURCE address and to the reads
//     (cdna_hip_programming.md rule 21).  Fragment reads are issued through untracked inline-asm ds_reads retired by
//     counted lgkmcnt waits (common.h lds_read16): hipcc only ever emits lgkmcnt(0) beside an LDS-DMA;
//   * XCD-aware tile order keeps the workgroups that share an activation row panel on one XCD's L2.
//
// Retired forms (measured, written up and removed from this file; lab/README.md names the last commit that has them):
//   * four waves on 224 x 128 tiles, two workgroups per CU: 302 vs 307 motions/s (profiles/r01c_final.md), and the start delay
//     that ran a CU's two workgroups in anti-phase: 0.0 % (profiles/r05h_dephase.md);
//   * four waves x 64 columns, one wave per SIMD ("wide"): 12-18 % slower per launch, in_proj spilled (profiles/r04d_wide.md);
//   * the pipelined loop on 32x32x16 MFMAs: in_proj 251 vs 232 us per launch, headline -8.4 % (profiles/r07a_m16.md);
//   * the timing ablations and cycle counters of rounds 1-3 (profiles/r01c_final.md, profiles/r03c_ab.md);
//   * the epilogue that reads its patch one round ahead: neutral here (profiles/r05j_epilogue_ahead.md); gemm_x3s.h keeps its own.
#pragma once
#include "attention_x3.h"  // QkvPlanes: the in_proj epilogue writes the attention kernel's operand planes
#include "common.h"
#include "gemm_f32.h"  // ACT_* enums

namespace mdm {

constexpr int X3_TM = 224, X3_BK = 32;
// The A-stage swizzle: the 16-byte chunk c of row `row` is stored at chunk c ^ x3_swz((row >> 2) & 3) of its 64-byte LDS row.  ONE
// helper for the LDS-DMA source address and for every fragment read, so that the two cannot drift apart.  A ds_read_b128 is
// served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32 for the upper half; MI355X_MICROARCH.md, LDS): 16 lanes
// x 16 bytes over 64 banks x 4 bytes, conflict-free when the 16 (row & 3, stored chunk) pairs differ.
//   16x16x32 reads  lane -> (row lane & 15, chunk lane >> 4): a group holds row quads q = 0, 3 with chunk c and q = 1, 2 with c ^ 1;
//                   stored chunks f(0), f(3), f(1) ^ 1, f(2) ^ 1 (^ c) must differ -- the identity gives 0, 3, 0, 3: 2-way
//                   (measured: SQ_LDS_BANK_CONFLICT 1.79 M -> 22.4 M per in_proj launch, profiles/r07a_m16.md);
//   32x32x16 reads  lane -> (row lane & 31, chunk 2 ksub + (lane >> 5)): a group holds q = 0, 3, 5, 6 or 1, 2, 4, 7 (mod 4: all
//                   four) with ONE chunk; any permutation f works.
// f = (0, 2, 3, 1) is one of the eight permutations that are 1-way on all three patterns (tests/test_host_lds_swizzle.py).
__host__ __device__ constexpr int x3_swz(int q) { return (((q ^ (q >> 1)) & 1) << 1) | (q >> 1); }
static_assert(x3_swz(0) == 0 && x3_swz(1) == 2 && x3_swz(2) == 3 && x3_swz(3) == 1, "A-stage swizzle permutation");
constexpr int X3_NWAVE = 8;                                      // waves per workgroup, each owning 32 output columns
constexpr int X3_TN = 32 * X3_NWAVE;                             // 224 x 256 tiles, one workgroup per CU
constexpr int X3_MSUB = X3_TM / 32;                              // 7 row sub-tiles
constexpr int X3_A_BYTES = X3_TM * X3_BK * 2;                    // one A plane tile: 14336
constexpr int X3_A_STAGE = 2 * X3_A_BYTES;                       // Ah|Al: 28672
constexpr int X3_A_RING = 2;                                     // stages of the step-synchronous k-loop
constexpr int X3_PIPE_RING = 4;                                  // stages of the pipelined k-loop (PIPE): A runs 3 steps ahead
// Counted vmcnt waits of the pipelined loop, whose queue holds per step and wave  A(g+3) x nA | W(g+2) x 4  (nA >= 3: the 26 groups
// of a 208-row tile dealt to eight waves).  The queue retires in issue order across both kinds of operation it holds (LDS-DMA pieces
// of A, VGPR loads of W), so a count is the number of YOUNGER operations of either kind:
//   step start, slots W(g):  younger = A(g+2) + W(g+1) = 3 + 4
//   middle, own A(g+1):      younger = W(g) + A(g+2) + W(g+1) = 4 + 3 + 4
// (the start-of-step wait already retires A(g+1), which is older than W(g); the middle wait states the need).  If only operations
// of the SAME kind were assumed to retire in order, the counts would be 4 (W(g+1)) and 3 (A(g+2)).
constexpr int X3M_WAIT_WS = 7, X3M_WAIT_MID = 11;
constexpr int x3_patch_base(int ring) { return ring * X3_A_STAGE; }   // 57344 (2 stages) / 114688 (4)
constexpr int X3_PATCH_BYTES = 8 * 32 * 4;                       // per wave: 8 rows x 32 columns fp32
constexpr int X3_TAB_BYTES = X3_TM * 8;                          // one (mean, rstd) table of the tile's rows
// LDS after the patches: the (mean, rstd) table of the tile's rows (FOLD or RES == 3: a kernel has one of them) and the
// raw partial sums it is built from (<= 4 partials per row: 7 KB, the LDS-DMA lands whole KBs), both double-buffered by
// tile parity, then the per-wave partial sums of OSTAT
constexpr int x3_tab_base(int ring) { return x3_patch_base(ring) + X3_NWAVE * X3_PATCH_BYTES; }
constexpr int X3_RAW_BYTES = 7 * 1024;
constexpr int x3_raw_base(int ring) { return x3_tab_base(ring) + 2 * X3_TAB_BYTES; }      // tables: 2 (tile parity)
constexpr int x3_part_base(int ring) { return x3_raw_base(ring) + 2 * X3_RAW_BYTES; }    // raw partials: 2 (parity)
// last: the epilogue's per-column vectors of the tile (bias, folded column sums, residual gamma, beta: 4 x 256 floats),
// fetched by LDS-DMA one tile ahead, double-buffered by tile parity
constexpr int X3_CVEC_BYTES = 4 * 1024;
constexpr int x3_cvec_base(bool ln, int ring) { return ln ? x3_part_base(ring) + X3_NWAVE * X3_TAB_BYTES : x3_tab_base(ring); }
constexpr int x3_lds_bytes(bool ln, int ring) { return x3_cvec_base(ln, ring) + 2 * X3_CVEC_BYTES; }
// two stages: 73728, with the LayerNorm tables 105984; four stages (pipelined): 131072 / 163328 of the CU's 163840
static_assert(x3_lds_bytes(false, X3_A_RING) == 73728 && x3_lds_bytes(true, X3_A_RING) == 105984, "LDS of the step-synchronous form");
static_assert(x3_lds_bytes(false, X3_PIPE_RING) == 131072 && x3_lds_bytes(true, X3_PIPE_RING) == 163328, "LDS of the pipelined form");
constexpr int X3_A_GROUPS = X3_A_STAGE / 1024;                   // 28 LDS-DMA wave-instructions per stage
constexpr int X3_A_PIECES = (X3_A_GROUPS + X3_NWAVE - 1) / X3_NWAVE;   // 4 per wave and step

struct X3Operand {   // activations: [rows][K] planes
  const p16_t* hi;
  const p16_t* lo;
};
struct X3Weights {   // fragment-ordered planes (see header); rows padded to a multiple of 32
  const p16_t* hi;
  const p16_t* lo;
};
inline size_t x3_packed_weight_elems(int N, int K) { return (size_t)((N + 31) / 32 * 32) * K; }

// v = act(acc + bias[n]) * (n < scale_cols ? col_scale : 1) + (res ? res[m][n] : 0) -> fp32 out and/or split planes,
// or (OUT_QKV) the attention operand planes of attention_x3.h.
struct X3Epilogue {
  float* out;        // [M][ld] or null
  const float* bias;
  const float* res;  // RES == 1: fp32 residual [M][ld]; may alias out
  const p16_t* resh;  // RES == 2: the residual as hi/lo planes [M][ld] (value = hi + lo)
  const p16_t* resl;
  p16_t* oh;        // [M][ld] split planes or null
  p16_t* ol;
  int ld;
  int scale_cols;
  float col_scale;
  QkvPlanes qkv;     // OUT_QKV only
  int S, D;          // OUT_QKV only: tokens per sequence (= rows per tile), model width (N = 3 D)
  // ---- LayerNorm folded into the GEMMs around it (no LayerNorm kernel, no normalised copy of the residual stream):
  // the producer of a pre-norm sum x (out_proj / linear2, OSTAT) writes x as planes plus, per row and column tile, the
  // partial statistics (sum x, sum (x - tile mean)^2) over its columns; every consumer merges them into mean / rstd
  // (Chan's pairwise update: no E[x^2] - mean^2 cancellation).  OSTAT needs N % 256 == 0.
  //   FOLD  the A operand is x itself and the weights were pre-multiplied by gamma (mdm_prepare), so
  //         W.LN(x) + b = rstd * (W'.x - mean * colsum) + b'       with colsum[n] = sum_k W'[n][k], b' = b + W.beta
  //   RES 3 the residual is LN(x) = (x - mean) * rstd * gamma + beta, rebuilt on the fly from x's planes
  const float* astat;    // FOLD: partial sums of the A rows [M][stat_parts][2]
  const float* colsum;   // FOLD: [N]
  const float* rstat;    // RES == 3: partial sums of the residual rows [M][stat_parts][2]
  const float* rgamma;   // RES == 3: [ld]
  const float* rbeta;
  float* ostat;          // OSTAT: [M][tiles_n][2] partial sums of the rows this launch writes
  int stat_parts;        // partials per row in astat / rstat
  float inv_dim;         // 1 / (normalised width) for astat / rstat
  // ---- EMBED (InputProcess, mdm.py:343-349 + :251-252): GEMM row m = (b, t) of [B*T]; the value gets the positional row
  // res[(1 + t) * ld + n] added and is written, as planes, to token row b*S + 1 + t of every branch (S = emb_T + 1)
  int emb_T, emb_B, emb_nbranch;
  float acc_scale = kX3AccScale;   // accumulators -> value: undoes the 2^8 the weight planes carry (common.h kX3WeightScale)
  int stat_cols = 256;             // columns each partial of astat / rstat covers: 256 (this kernel's OSTAT), 128 (gemm_x3s.h)
  int pair_B = 0;                  // PAIR (OUT_QKV): samples per guidance branch -- tile b also serves sequence pair_B + b (kernel header)
};

constexpr bool x3_has_col_scale(int act, int res) { return act == 0 && (res == 0 || res == 1); }

// exact-GELU with erf from Abramowitz-Stegun 7.1.26 (|err| < 1.5e-7, i.e. fp32-rounding class): one v_exp, one v_rcp
// and a 5-term Horner chain instead of the ~40-instruction libm erff; used only in this split-precision path.  (Round 3 tried
// the odd rational x P(x^2) / Q(x^2) on |x| <= 4 -- ten packed FMAs and a single v_rcp per element, |err| < 4.5e-7: same-box
// A/B 0.35 % SLOWER over the whole sampling loop, profiles/r03c_ab.md; not kept.)
__device__ __forceinline__ float gelu_erf_fast(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = rcp_fast(1.0f + 0.3275911f * z);
  float p = 1.061405429f;
  p = p * t - 1.453152027f;
  p = p * t + 1.421413741f;
  p = p * t - 0.284496736f;
  p = p * t + 0.254829592f;
  const float erfc_z = p * t * exp_fast(-z * z);
  const float erf_abs = 1.0f - erfc_z;
  return 0.5f * x * (1.0f + copysignf(erf_abs, x));
}

// fp32 [N][K] -> fragment-ordered hi/lo planes (rows >= N zero).  One thread per 8 consecutive k of one row.
// `overflow` (device int, may be null): set to 1 when a hi element is not a finite 16-bit number, i.e. |w * 2^8| left the
// plane format's range (fp16: |w| >= 255.9) -- such a matrix cannot be carried by the split arithmetic (mdm_weights_in_range).
__global__ __launch_bounds__(256) void pack_weight_planes_kernel(const float* __restrict__ w, p16_t* __restrict__ hi,
                                                                 p16_t* __restrict__ lo, int N, int K, int* overflow) {
  const int npad = (N + 31) / 32 * 32, k8n = K / 8;
  const size_t total = (size_t)npad * k8n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / k8n), k8 = (int)(i - (size_t)n * k8n);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (n < N) ? w[(size_t)n * K + 8 * k8 + j] * kX3WeightScale : 0.f;
    p16x8 h8, l8;
    split8(v, h8, l8);
    if (overflow != nullptr) {
      bool bad = false;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float back = p16_to_f32((p16_t)h8[j]);
        bad = bad || !(fabsf(back) <= 3.0e38f);   // inf or NaN (also when the fp32 weight itself is not finite)
      }
      if (bad) *overflow = 1;   // benign race: every writer stores the same value
    }
    const int kstep = k8 >> 1, half = k8 & 1, lane = (n & 31) + 32 * half;
    const size_t o = (((size_t)(n >> 5) * (K / 16) + kstep) * 64 + lane) * 8;
    *reinterpret_cast<p16x8*>(hi + o) = h8;
    *reinterpret_cast<p16x8*>(lo + o) = l8;
  }
}

// epilogue rounds (8 rows each) of row sub-tile t: 4, or 2 for the 16-row last sub-tile; and how many rounds' worth of
// residual loads are younger than sub-tile t's when RR sub-tiles are kept in flight + in use
constexpr int x3_res_rounds(int t, bool t16) { return (t16 && t == X3_MSUB - 1) ? 2 : 4; }
constexpr int x3_res_younger_rounds(int t, int rr, bool t16) {
  int n = 0;
  for (int q = t + 1; q <= t + rr - 1 && q < X3_MSUB; ++q) n += x3_res_rounds(q, t16);
  return n;
}

// The A load stream: which tile of this workgroup and which k step it fetches next, and the per-lane source element
// offsets of the wave's LDS-DMA pieces for that tile.
struct X3Cursor {
  int v;        // virtual tile id (blockIdx.x + j * gridDim.x)
  int k;        // next k step
  uint32_t off[X3_A_PIECES];
};

// The kernel's options: ACT (gemm_f32.h ACT_*), RES and one word of X3_* flags.
// RES: 0 = no residual, 1 = fp32 residual, 2 = residual held as 16-bit hi/lo planes, 3 = LayerNorm of such planes.
enum : unsigned {
  X3_OUT_F32 = 1u << 0,      // output: fp32 [M][ld]
  X3_OUT_PLANES = 1u << 1,   //         hi/lo planes [M][ld]
  X3_OUT_QKV = 1u << 2,      //         the attention kernel's operand planes (in_proj)
  X3_FOLD = 1u << 3,         // the LayerNorm of the A rows is folded into this GEMM
  X3_OSTAT = 1u << 4,        // writes the partial row statistics of its output
  X3_EMBED = 1u << 5,        // InputProcess: positional rows, planes to the token rows of every branch
  X3_T16 = 1u << 6,          // 208-row tile
  X3_F6 = 1u << 7,           // the f16f6 arithmetic on the step-synchronous loop
  X3_PIPE = 1u << 8,         // the pipelined k-loop on 16x16x32 MFMAs
  X3_PAIR = 1u << 9,         // one tile serves both guidance branches of a sample
};
// FOLD / OSTAT / RES == 3: LayerNorm folded into the GEMMs (X3Epilogue).
// T16: the tile is 208 rows -- six 32-row sub-tiles plus ONE 16-row sub-tile (rows 192-207) on v_mfma_f32_16x16x32_f16 --
// for row extents <= 208 (S = 197: 11 pad rows instead of 27, i.e. 6.5 of 7 units of matrix work and 13 of 14 A groups).
// The 16-row sub-tile needs the wave's W fragments in the 16x16x32 operand layout; they are derived from the 32x32x16
// fragments in registers by two lane swaps per dword (common.h frag32_to_frag16), not fetched a second time.
// F6: the k-loop runs the "f16f6" arithmetic of gemm_f16f6.h on the same skeleton -- plane 0 holds fp16 values, plane 1 the MX-FP6
// records, the weight planes come from pack_weight_f16f6_kernel; units are ordered sub-tile-major so that a sub-tile's two
// 16-byte record reads (k sub-steps 0 and 1) meet in ONE scaled MFMA; 2 + 1 MFMAs per sub-tile and step instead of 6.
// PIPE (round 7): the pipelined loop with the WHOLE 208-row tile on v_mfma_f32_16x16x32_f16 -- 13 row slices x 2 column halves of
// f32x4 accumulators per wave (see the k-loop below).
// PAIR (round 8, layer 0's in_proj under guidance): sequences b and pair_B + b of the 2 pair_B the planes hold differ only in token 0
// (the condition token; the frame tokens are written once to both by the embedding GEMM), so ONE tile serves both: tile rows
// 0 .. S-1 are sequence b, tile row S -- a pad row of the 208-row tile, S <= 207 -- is loaded from token 0 of sequence pair_B + b.
// The epilogue writes row 0 to sequence b, rows 1 .. S-1 to both and row S to token 0 of sequence pair_B + b: every Q / K / V^T
// element keeps its products and their order, a row's position in the tile does not enter them.  M, the grid and the k-loop (its
// stages, piece dealing and counted waits) are those of a pair_B-sequence launch; only one lane's source offset per plane differs.
template <int ACT, int RES, unsigned FLAGS>
__global__ __launch_bounds__(64 * X3_NWAVE, 2) void gemm_x3_kernel(X3Operand A, X3Weights W, X3Epilogue ep, int M, int N, int K,
                                                                   int rows_per_tile, int tiles_n, int total) {
  MDM_DYN_SMEM(unsigned char, lds);
  constexpr bool OUT_F32 = (FLAGS & X3_OUT_F32) != 0, OUT_PLANES = (FLAGS & X3_OUT_PLANES) != 0, OUT_QKV = (FLAGS & X3_OUT_QKV) != 0;
  constexpr bool FOLD = (FLAGS & X3_FOLD) != 0, OSTAT = (FLAGS & X3_OSTAT) != 0, EMBED = (FLAGS & X3_EMBED) != 0;
  constexpr bool T16 = (FLAGS & X3_T16) != 0, F6 = (FLAGS & X3_F6) != 0, PIPE = (FLAGS & X3_PIPE) != 0, PAIR = (FLAGS & X3_PAIR) != 0;
  static_assert(FLAGS < (X3_PAIR << 1), "unknown flag");
  static_assert((int)OUT_F32 + (int)OUT_PLANES + (int)OUT_QKV == 1, "exactly one output form");
  static_assert(RES >= 0 && RES <= 3 && !(OUT_QKV && RES != 0), "in_proj has no residual");
  static_assert(!(FOLD && RES == 3), "one (mean, rstd) table: of the A rows or of the residual rows");
  static_assert(!OSTAT || OUT_PLANES, "row statistics are written next to the planes they describe");
  static_assert(!EMBED || (OUT_PLANES && RES == 1 && !PIPE), "InputProcess: fp32 positional rows, planes out, step-synchronous loop");
  static_assert(!PIPE || (T16 && !F6), "the pipelined k-loop exists for 208-row (T16) tiles");
  static_assert(!F6 || (!T16 && OUT_F32 && !FOLD && !OSTAT), "the f16f6 k-loop: 224-row tiles, plain fp32-out epilogues");
  static_assert(!PAIR || (PIPE && OUT_QKV && !FOLD), "the paired tile: layer 0's in_proj (no folded LayerNorm) on the pipelined loop");
  constexpr int RINGN = PIPE ? X3_PIPE_RING : X3_A_RING;   // A stages in LDS
  constexpr int NT32 = T16 ? X3_MSUB - 1 : X3_MSUB;     // 32-row sub-tiles
  constexpr int NROUNDS = 4 * NT32 + (T16 ? 2 : 0);     // epilogue rounds of 8 rows
  using Cursor = X3Cursor;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = wave_index(tid);
  const int r = lane & 31, h = lane >> 5;
  const int nk = K / X3_BK;
  const int gstride = (int)gridDim.x;

  auto tile_origin = [&](int v, int& m0, int& n0) {
    const int lid = xcd_remap(v, total);
    const int tile_m = lid / tiles_n, tile_n = lid - tile_m * tiles_n;
    m0 = tile_m * rows_per_tile;
    n0 = tile_n * X3_TN;
  };

  // ---- LDS-DMA sources.  A stage image = 28 groups of 1 KB (16 rows x 64 B): groups 0-13 Ah, 14-27 Al.  Wave w issues
  // groups w, w+8, w+16, w+24.  Lane -> (row = lane>>2, stored chunk = lane&3); the logical k-chunk it fetches is
  // stored ^ x3_swz((row>>2)&3) = (lane&3) ^ x3_swz((lane>>4)&3).  Rows past the tile / matrix are clamped (never stored).
  const int schunk = (lane & 3) ^ x3_swz((lane >> 4) & 3);
  auto aim_a = [&](Cursor& c) {
    int m0, n0;
    tile_origin(c.v, m0, n0);
#pragma unroll
    for (int i = 0; i < X3_A_PIECES; ++i) {
      // PIPE: the 26 groups a 208-row tile reads (13 per plane) are dealt round-robin: piece j = wid + 8 i -> group j (hi) /
      // j + 1 (lo, stage groups 14..26); waves 0 and 1 issue four pieces per step, the others three
      const int jj = min(wid + X3_NWAVE * i, 25);
      const int q = PIPE ? (jj < 13 ? jj : jj + 1) : min(wid + X3_NWAVE * i, X3_A_GROUPS - 1);
      const int ga = (q < 14) ? q : q - 14;
      int arow = min(m0 + ga * 16 + (lane >> 2), M - 1);
      if constexpr (PAIR) {   // tile row S: token 0 of the other branch's sequence (rows_per_tile == S, M == pair_B * S)
        if (ga * 16 + (lane >> 2) == rows_per_tile) arow = m0 + M;
      }
      c.off[i] = (uint32_t)arow * (uint32_t)K + schunk * 8;
    }
  };
  auto piece_a = [&](const Cursor& c, int i, int buf) {
    if constexpr (PIPE) {
      const int j = wid + X3_NWAVE * i;
      const int q = j < 13 ? j : j + 1;
      if (j < 26) glds16(((q < 14) ? A.hi : A.lo) + c.off[i] + c.k * X3_BK, lds + buf * X3_A_STAGE + q * 1024);
    } else {
      const int q = wid + X3_NWAVE * i;
      if (q < X3_A_GROUPS && !(T16 && (q == 13 || q == 27)))   // T16: rows 208-223 of the stage are never read
        glds16(((q < 14) ? A.hi : A.lo) + c.off[i] + c.k * X3_BK, lds + buf * X3_A_STAGE + q * 1024);
    }
  };
  // past its last tile the stream simply re-fetches that tile (one wasted stage per workgroup): no "anything left to
  // load" branches in the step body
  auto advance_a = [&](Cursor& c) {
    if (++c.k == nk) {
      c.k = 0;
      if (c.v + gstride < total) { c.v += gstride; aim_a(c); }
    }
  };

  // ---- W fragments of this wave for k step `k` of tile `v`: four 16-byte loads per lane, each a contiguous 1 KB per wave
  const size_t wk16 = (size_t)(K / 16);
  auto load_w = [&](int v, int k, p16x8 (&fh)[2], p16x8 (&fl)[2]) {
    int m0, n0;
    tile_origin(v, m0, n0);
    const size_t nb = (size_t)((n0 >> 5) + wid);
    const size_t o = ((nb * wk16 + 2 * (size_t)k) * 64 + lane) * 8;
    fh[0] = *reinterpret_cast<const p16x8*>(W.hi + o);
    fl[0] = *reinterpret_cast<const p16x8*>(W.lo + o);
    fh[1] = *reinterpret_cast<const p16x8*>(W.hi + o + 512);
    fl[1] = *reinterpret_cast<const p16x8*>(W.lo + o + 512);
  };

  // ---- fragment read offsets (bytes inside a plane tile): row*64 + ((ksub*2 + h) ^ sw)*16, sw = x3_swz((row>>2)&3)
  const int sw = x3_swz((r >> 2) & 3);
  const int fa = r * 64;                 // + t*2048 per row sub-tile
  // 16-row sub-tile (T16): lane -> (row 192 + (lane&15), k chunk lane>>4)
  const int r16 = lane & 15, g16 = lane >> 4;
  const int fa16 = (192 + r16) * 64 + ((g16 ^ x3_swz((r16 >> 2) & 3)) * 16);
  const LdsAddr lds_base = lds_addr_of(lds);

  int v = (int)blockIdx.x;
  if (v >= total) return;
  Cursor ca{v, 0, {}};
  aim_a(ca);
  int wv = v, wkk = 0;   // the W stream's (tile, k): one step ahead of the MFMAs, like the A stream

  // Pipeline invariant: at the top of global step g the LDS holds A(g) [landed, visible] and the registers wh/wl hold
  // W(g).  During the step A(g+1) is issued into the other stage (its previous content A(g-1) was last read before the
  // barrier that ended step g-1) and W(g+1) is fetched into wnh/wnl; the step ends with vmcnt(0) + one barrier.
  // LayerNorm row statistics: LDS-DMA of the producer's partial sums of the 224 rows starting at m0 (contiguous:
  // [row][part][2] floats) into raw buffer `par`; waves 0..npieces-1 move 1 KB each
  auto stats_dma = [&](int m0s, int par) {
    const float* st = FOLD ? ep.astat : ep.rstat;
    const int npieces = (X3_TM * ep.stat_parts * 8 + 1023) / 1024;
    for (int pc = wid; pc < npieces; pc += X3_NWAVE) {      // (<= 7 pieces)
      // A 16-byte unit keeps its place in the table (unit u of the tile = floats 4u .. 4u+3 behind the tile's first row) as long
      // as it holds any float of the matrix; units entirely past it read a valid address instead.  With an odd number of
      // partials per row (D = 256, 768) a tile that starts on an odd row is only 8-byte aligned and its last unit may straddle
      // the end of the array by up to 12 bytes: the workspace carves every statistics array with 16 spare bytes for this
      // (api_launch.h carve).  (Round 3 clamped straddling units to the last 16 bytes of the array, which moved the last row's
      // partials to the wrong table slot: wrong last token row for D = 256 when the last tile starts on an odd row.)
      const long long total_f = (long long)M * ep.stat_parts * 2;
      long long fo = (long long)m0s * ep.stat_parts * 2 + 4LL * (64 * pc + lane);
      if (fo >= total_f) fo = 0;                                       // rows past the matrix: any valid address
      glds16(st + fo, lds + x3_raw_base(RINGN) + par * X3_RAW_BYTES + pc * 1024);
    }
  };
  // the epilogue's per-column vectors of the tile starting at column n0c -> LDS buffer `par`: wave 0 bias, wave 1 folded
  // column sums (FOLD), waves 2 / 3 residual gamma / beta (RES == 3); 1 KB = the tile's 256 columns each (columns past N:
  // clamped source, never stored)
  constexpr bool LN_ANY = FOLD || OSTAT || RES == 3;
  auto cvec_dma = [&](int n0c, int par) {
    const float* src = nullptr;
    if (wid == 0) src = ep.bias;
    if constexpr (FOLD) { if (wid == 1) src = ep.colsum; }
    if constexpr (RES == 3) { if (wid == 2) src = ep.rgamma; if (wid == 3) src = ep.rbeta; }
    if (src != nullptr) glds16(src + min(n0c + 4 * lane, N - 4), lds + x3_cvec_base(LN_ANY, RINGN) + par * X3_CVEC_BYTES + wid * 1024);
  };
  {
    int m0f, n0f;
    tile_origin(v, m0f, n0f);
    if constexpr (FOLD || RES == 3) stats_dma(m0f, 0);
    cvec_dma(n0f, 0);
  }
  p16x8 wh[2], wl[2], wnh[2], wnl[2];
  // PIPE: the W stream lives in four slots (slot 2 * (step parity) + column half; hi and lo plane fragment each), refilled
  // IN PLACE for two steps later behind the step's last MFMA -- 32 VGPRs, one step of cover
  p16x8 wsh[4] = {}, wsl[4] = {};   // (zero: the first refill formally reads its slot)
  uint32_t wso = 0;           // element offset of the W stream's current step inside the fragment-ordered planes
  uint32_t wtile = 0;         // ... of its tile's first step (wave-uniform): changes only when the stream enters a new tile
  auto aim_w_tile = [&]() {
    int m0w, n0w;
    tile_origin(wv, m0w, n0w);
    wtile = (uint32_t)((n0w >> 5) + wid) * (uint32_t)wk16 * 512u;
  };
  // the fragment-ordered planes serve the 16x16x32 B operand of column half c through a per-lane remap -- lane l reads block
  // k/16 = 2 step + (l >> 5), slot 16 c + (l & 15) + 32 ((l >> 4) & 1): every 16 lanes one contiguous 256 bytes; column half 1 lies
  // 128 elements behind half 0
  const uint32_t lane_wo = (uint32_t)((lane >> 5) * 512 + ((lane & 15) + 32 * ((lane >> 4) & 1)) * 8);
  auto aim_w = [&]() { wso = wtile + (uint32_t)wkk * 1024u + lane_wo; };
  auto advance_w = [&]() {
    if (++wkk == nk) {
      wkk = 0;
      if (wv + gstride < total) { wv += gstride; aim_w_tile(); }
    }
  };
  auto load_w_half = [&](int c, auto q_tag) __attribute__((always_inline)) {   // in-place refill of slot q (common.h gload16_refill)
    constexpr int q = decltype(q_tag)::value;
    const uint32_t o = wso + 128u * (uint32_t)c;
    gload16_refill(wsh[q], W.hi + o);
    gload16_refill(wsl[q], W.lo + o);
  };
  auto wait_all_slots = [&]() __attribute__((always_inline)) {
    vmem_wait<0>(wsh[0], wsl[0], wsh[1], wsl[1], wsh[2], wsl[2], wsh[3], wsl[3]);
  };
  int gs = 0;                 // PIPE: global k-step counter of this workgroup (stage of step g = g & 3)
  if constexpr (PIPE) {
    // A(0), A(1), A(2) into stages 0..2 and W(0), W(1) into the four slots; everything landed and visible before step 0
#pragma unroll
    for (int st = 0; st < 3; ++st) {
#pragma unroll
      for (int i = 0; i < X3_A_PIECES; ++i) piece_a(ca, i, st);
      advance_a(ca);
    }
    aim_w_tile();
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      aim_w();
      if (st == 0) { load_w_half(0, std::integral_constant<int, 0>{}); load_w_half(1, std::integral_constant<int, 1>{}); }
      else { load_w_half(0, std::integral_constant<int, 2>{}); load_w_half(1, std::integral_constant<int, 3>{}); }
      advance_w();
    }
    wait_all_slots();
    wg_barrier();
  } else {
#pragma unroll
    for (int i = 0; i < X3_A_PIECES; ++i) piece_a(ca, i, 0);
    advance_a(ca);
    load_w(wv, wkk, wh, wl);
    wait_vmem_all();
    wg_barrier();
  }

  int abuf = 0;
  int tile_parity = 0;
  for (; v < total; v += gstride, tile_parity ^= 1) {
    int m0, n0;
    tile_origin(v, m0, n0);
    f32x16 acc[NT32];            // step-synchronous loop: [row sub-tile]
    f32x4 acc16[2];              // ... T16: rows 192-207 x columns 0-15 / 16-31
    constexpr int NS16 = 2 * X3_MSUB - 1;                   // PIPE: 13 row slices of 16
    f32x4 accm_[PIPE ? NS16 : 1][2];                        // PIPE: [row slice][column half], 104 VGPRs
    if constexpr (PIPE) {
#pragma unroll
      for (int s = 0; s < NS16; ++s) accm_[s][0] = accm_[s][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
      for (int t = 0; t < NT32; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
      acc16[0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc16[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int ncol0 = n0 + wid * 32;                     // this wave's first column (wave-uniform)
    // this tile's per-column epilogue vectors are in LDS buffer `tile_parity` (requested one tile ago / in the prologue: no
    // global-load latency in front of the epilogue); the next tile's are requested in this tile's SECOND k step (below),
    // i.e. behind a workgroup barrier every wave reaches only after its epilogue of the previous tile -- whose vectors
    // live in the buffer being refilled -- and land under the rest of this tile's k-loop
    const float* const cvec = reinterpret_cast<const float*>(lds + x3_cvec_base(LN_ANY, RINGN) + tile_parity * X3_CVEC_BYTES);
    const int kt_cvec = nk > 1 ? 1 : 0;
    if (nk == 1) wg_barrier();   // single-step contractions: no k-step barrier in front of the request
    // row statistics (mean, rstd) of this tile's rows, built HERE -- where the accumulators are not live yet -- from the
    // producer's partial sums, which an LDS-DMA issued one tile ago (or in the kernel prologue) has already landed; the
    // next tile's partials are requested now and land under this tile's k-loop.  Tables and raw buffers alternate with
    // the tile parity: a fast wave may build table j+1 while a slow one still reads table j in its epilogue.
    constexpr bool LN_TABS = FOLD || RES == 3;
    float2* const stab = reinterpret_cast<float2*>(lds + x3_tab_base(RINGN) + tile_parity * X3_TAB_BYTES);
    if constexpr (LN_TABS) {
      if (tid < X3_TM) {
        // rows of the tile past the matrix (the last sequence's pad rows) have no statistics: their raw slots hold whatever the
        // clamped DMA fetched -- for an odd M with one partial per row two floats BEHIND the buffer (uninitialised workspace:
        // a NaN there went through these rows' V^T pad keys, 0 * NaN, into the whole sequence) -- so they get (0, 0): every
        // folded value of such a row is then the finite constant b' / beta
        int m0t, n0t;
        tile_origin(v, m0t, n0t);
        const bool pad_row = m0t + tid >= M;
        const float* sraw = reinterpret_cast<const float*>(lds + x3_raw_base(RINGN) + tile_parity * X3_RAW_BYTES);
        // partials are (sum, CENTRED sum of squares about the partial's own mean) of X3_TN columns each; merged by Chan's
        // formula -- no E[x^2] - mean^2 cancellation when a row's mean is large against its spread
        float s1 = 0.f;
        for (int p = 0; p < ep.stat_parts; ++p) s1 += sraw[(tid * ep.stat_parts + p) * 2];
        const float mean = s1 * ep.inv_dim;
        const float pcols = (float)ep.stat_cols, inv_pcols = 1.0f / pcols;   // columns per partial (256, or 128 from gemm_x3s.h)
        float m2 = 0.f;
        for (int p = 0; p < ep.stat_parts; ++p) {
          const float dm = sraw[(tid * ep.stat_parts + p) * 2] * inv_pcols - mean;
          m2 += sraw[(tid * ep.stat_parts + p) * 2 + 1] + pcols * dm * dm;
        }
        const float var = m2 * ep.inv_dim;
        stab[tid] = pad_row ? make_float2(0.f, 0.f) : make_float2(mean, rsqrt_fast(var + 1e-5f));
      }
      // the NEXT tile's partials are requested BEHIND the table build: hipcc drains the vector-memory queue in front of the
      // build's LDS reads (an LDS-DMA may be pending), and issued first, this request -- a fresh HBM / L2 round trip -- was what
      // it waited for at every tile start (round 3; the other raw buffer is the target, the build does not touch it)
      if (v + gstride < total) {
        int m0n, n0n;
        tile_origin(v + gstride, m0n, n0n);
        stats_dma(m0n, tile_parity ^ 1);
      }
    }
    float2* const atab = stab;   // FOLD: statistics of the A rows;  RES == 3: of the residual rows (a kernel has one)
    float2* const rtab = stab;
    if constexpr (PIPE) {
      // ================= pipelined k-loop on v_mfma_f32_16x16x32_f16 =================
      // What the step-synchronous loop below pays per 32-deep step -- a full vmcnt(0) drain of loads issued at most one step
      // earlier, a rendezvous of all eight waves behind it, and a cold restart of the fragment-read pipeline (measured: a
      // step takes ~2.8 us against 1.3 us of matrix work) -- is removed by running every stream AHEAD of the matrix work:
      //   * A: four LDS stages.  During step g the pieces of A(g+3) are issued (into the stage A(g-1) lived in); each wave
      //     retires its own pieces of A(g+1) with a COUNTED vmcnt at the step's middle, then one bare s_barrier -- no drain --
      //     makes them visible, and from there on the fragment reads of step g+1 may begin: the element pipeline never restarts
      //     inside a tile;
      //   * W: four register slots refilled in place by untracked loads retired with counted waits that name the slot (hipcc
      //     would drain the LDS-DMA queue for a tracked load).
      // Other operations that land in the vector-memory queue (column vectors, row statistics, the previous tile's stores) only
      // make the counted waits (X3M_WAIT_*) stricter: the queue retires in order.
      // The matrix work is 13 elements per 32-deep step, one per 16-row slice s: two ds_read_b128 (Ah, Al of rows 16 s + (lane & 15),
      // k chunk lane >> 4 -- the T16 read pattern, conflict-free under x3_swz) and six MFMAs, the three products of each column half
      // interleaved (acc[s][0], acc[s][1], ...: the two chains hide each other's dependency).  Under the power limit the 16x16x32
      // shape delivers more FLOP/s than 32x32x16 at the same cycles per FLOP (MI355X_MICROARCH.md, "DVFS give-back").
      //   * both W column halves of step g are read by every element, so slots W0 / W1 of the step are refilled together for
      //     g + 2 behind its last MFMA (cover: one step);
      //   * fragment ring: element e uses slot e % 3, the last element slot 3 -- 13 is not a multiple of 3, and the reads of the
      //     next step's elements 0 / 1 (slots 0 / 1), issued at elements 11 / 12, must not land on a slot still in use.
      constexpr int NE = NS16, DEPTH = 2, RING = DEPTH + 1, XB = NE / 2;
      auto slot = [](int e) constexpr { return e == NE - 1 ? RING : e % RING; };
      //   * the ring is read IN PLACE (common.h lds_refill16): its registers are never an MFMA destination
      p16x8 ah[RING + 1] = {}, al[RING + 1] = {};
      const LdsAddr lane_a = lds_base + fa16 - 192 * 64;   // slice s: + s * 1024 (the swizzle x3_swz((row >> 2) & 3) does not depend on s)
      auto issue_reads = [&](auto e_tag, uint32_t stg) __attribute__((always_inline)) {
        constexpr int e = decltype(e_tag)::value;
        lds_refill16<e * 1024>(ah[slot(e)], lane_a + stg * X3_A_STAGE);
        lds_refill16<X3_A_BYTES + e * 1024>(al[slot(e)], lane_a + stg * X3_A_STAGE);
      };
      auto pipe_step = [&](auto par_tag) __attribute__((always_inline)) {
        constexpr int PAR = decltype(par_tag)::value, W0 = 2 * PAR, W1 = 2 * PAR + 1;
        const uint32_t cur = (uint32_t)gs & 3u, nxt = (uint32_t)(gs + 1) & 3u, fill = (uint32_t)(gs + 3) & 3u;
        // slots W(g) (issued at the end of step g-2) landed
        vmem_wait<X3M_WAIT_WS>(wsh[W0], wsl[W0], wsh[W1], wsl[W1]);
        static_for<NE>([&](auto e_tag) __attribute__((always_inline)) {
          constexpr int e = decltype(e_tag)::value;
          // ---- 1. reads of the element DEPTH ahead (past the step: elements 0, 1 of step g+1, from the next stage)
          if constexpr (e + DEPTH < NE) issue_reads(std::integral_constant<int, e + DEPTH>{}, cur);
          else issue_reads(std::integral_constant<int, e + DEPTH - NE>{}, nxt);
          // ---- 2. the middle of the step: own pieces of A(g+1) landed, then the rendezvous makes them visible
          if constexpr (e == XB) {
            vmem_wait<X3M_WAIT_MID>(wsh[W0], wsl[W0], wsh[W1], wsl[W1]);
            sched_fence();
            wg_barrier_nodrain();   // A(g+1) visible to every wave; every wave is past step g-1, whose stage A(g+3) refills
            sched_fence();
          }
          // ---- 3. this element's reads retired (those of the DEPTH younger elements stay in flight)
          lds_wait<2 * DEPTH>(ah[slot(e)], al[slot(e)]);
          sched_fence();  // the MFMAs below must not be hoisted above the wait (rule 18)
          // ---- 4. matrix work: per column half al*wh, ah*wl, ah*wh (the product order of every form)
#pragma unroll
          for (int c = 0; c < 2; ++c) accm_[e][c] = mfma16_p16(al[slot(e)], wsh[W0 + c], accm_[e][c]);
#pragma unroll
          for (int c = 0; c < 2; ++c) accm_[e][c] = mfma16_p16(ah[slot(e)], wsl[W0 + c], accm_[e][c]);
#pragma unroll
          for (int c = 0; c < 2; ++c) accm_[e][c] = mfma16_p16(ah[slot(e)], wsh[W0 + c], accm_[e][c]);
          sched_fence();
          // ---- 5. one LDS-DMA piece of A(g+3) rides behind each of the elements that follow the barrier
          if constexpr (e >= XB && e < XB + X3_A_PIECES) piece_a(ca, e - XB, (int)fill);
          sched_fence();
        });
        // both W slots of the step are free: refill in place for g+2; then both streams move on
        aim_w();
        load_w_half(0, std::integral_constant<int, W0>{});
        load_w_half(1, std::integral_constant<int, W1>{});
        advance_w();
        advance_a(ca);
        ++gs;
      };
      // prime the fragment pipeline of this tile: its first stage was made visible by the previous step's barrier / the prologue
      static_for<DEPTH>([&](auto d_tag) __attribute__((always_inline)) { issue_reads(d_tag, (uint32_t)gs & 3u); });
      for (int kt = 0; kt < nk; kt += 2) {
        pipe_step(std::integral_constant<int, 0>{});
        // the next tile's per-column vectors: behind step 0's barrier, which every wave reaches only after its epilogue of
        // the previous tile (whose vectors live in the buffer being refilled)
        if (kt == 0 && v + gstride < total) {
          int m0n, n0n;
          tile_origin(v + gstride, m0n, n0n);
          cvec_dma(n0n, tile_parity ^ 1);
        }
        pipe_step(std::integral_constant<int, 1>{});
      }
      // the tile's last step has run two elements ahead like every other (ONE step body): those fragments belong to the next
      // tile's first step, whose pipeline is primed afresh behind the epilogue -- retire and drop them
      lds_wait<0>(ah[0], al[0], ah[1], al[1]);
      // the epilogue must not meet a W slot whose load is still in flight (a spill would save the stale register); hipcc
      // drains the queue in front of the epilogue's first LDS read anyway (LDS-DMA pending)
      wait_all_slots();
    } else {
    // ================= step-synchronous k-loop on v_mfma_f32_32x32x16_f16 =================
    for (int kt = 0; kt < nk; ++kt) {
      if (kt == kt_cvec && v + gstride < total) {
        int m0n, n0n;
        tile_origin(v + gstride, m0n, n0n);
        cvec_dma(n0n, tile_parity ^ 1);
      }
      // W(g+1): advance the W stream and fetch (past the last tile: re-fetch, like the A stream)
      if (++wkk == nk) {
        wkk = 0;
        if (wv + gstride < total) wv += gstride;
      }
      load_w(wv, wkk, wnh, wnl);
      // 14 units per stage (2 k sub-steps x 7 row sub-tiles), each = 2 A-fragment reads + 3 MFMAs, software-pipelined
      // DEPTH units deep: the reads of unit u+DEPTH are issued, then a COUNTED wait (2*DEPTH younger reads may stay in
      // flight) retires unit u's, then its 3 MFMAs go.  One LDS-DMA piece of A(g+1) rides behind each of the first four.
      constexpr int DEPTH = 2, RING = DEPTH + 1;  // fragment-read lookahead in units
      p16x8 ah[RING], al[RING];
      // per-lane LDS byte addresses of this stage's fragments for k sub-step 0 / 1 (the XOR swizzle moves with ks)
      const LdsAddr sa0 = lds_base + abuf * X3_A_STAGE + fa;
      const LdsAddr aaddr[2] = {sa0 + ((h ^ sw) * 16), sa0 + (((2 + h) ^ sw) * 16)};
#define X3_RD_A(dst, plane, t, ks) lds_read16<(plane) * X3_A_BYTES + (t) * 2048>(dst, aaddr[ks])
      // T16: the 16-row sub-tile's A fragments (one per plane covers the whole 32-deep step) are read FIRST, so they are
      // older than every unit's reads and retired by unit 0's wait; its W fragments come from wh / wl by lane swaps
      p16x8 a16h, a16l, w16h[2], w16l[2];
      if constexpr (T16) {
        const LdsAddr a16addr = lds_base + abuf * X3_A_STAGE + fa16;
        lds_read16<0>(a16h, a16addr);
        lds_read16<X3_A_BYTES>(a16l, a16addr);
        w16h[0] = wh[0]; w16h[1] = wh[1];
        w16l[0] = wl[0]; w16l[1] = wl[1];
        frag32_to_frag16(w16h[0], w16h[1]);
        frag32_to_frag16(w16l[0], w16l[1]);
      }
      constexpr int NU = 2 * NT32;  // units per stage
      p16x8 f6_hold = {0, 0, 0, 0, 0, 0, 0, 0};   // F6 only
      static_for<NU + DEPTH>([&](auto u_tag) __attribute__((always_inline)) {
        constexpr int u = decltype(u_tag)::value;
        if constexpr (u < NU) {
          constexpr int ks = F6 ? (u & 1) : u / NT32, t = F6 ? (u >> 1) : u - ks * NT32;
          X3_RD_A(ah[u % RING], 0, t, ks);
          X3_RD_A(al[u % RING], 1, t, ks);
        }
        if constexpr (u >= DEPTH) {
          constexpr int uv = u - DEPTH, ks = F6 ? (uv & 1) : uv / NT32, t = F6 ? (uv >> 1) : uv - ks * NT32;
          // reads allowed to stay in flight: those of the (up to) DEPTH younger units
          constexpr int younger = 2 * ((NU - 1 - uv) < DEPTH ? (NU - 1 - uv) : DEPTH);
          if constexpr (T16 && uv == 0) lds_wait<younger>(ah[uv % RING], al[uv % RING], a16h, a16l);
          else lds_wait<younger>(ah[uv % RING], al[uv % RING]);
          sched_fence();  // the MFMAs below must not be hoisted above the wait (rule 18)
          if constexpr (F6) {
            // main term on fp16; the record's first 16 bytes (code dwords c0-c3) wait in f6_hold for the second read
            // (c4, c5, scale) of the same sub-tile, then ONE scaled MFMA adds both cross terms of the 32-k block
            if constexpr (ks == 0) {
              f6_hold = al[uv % RING];
              acc[t] = mfma_f16(__builtin_bit_cast(f16x8, ah[uv % RING]), __builtin_bit_cast(f16x8, wh[0]), acc[t]);
            } else {
              acc[t] = mfma_f16(__builtin_bit_cast(f16x8, ah[uv % RING]), __builtin_bit_cast(f16x8, wh[1]), acc[t]);
              const u32x4 c0 = __builtin_bit_cast(u32x4, f6_hold), c1 = __builtin_bit_cast(u32x4, al[uv % RING]);
              const u32x4 w0 = __builtin_bit_cast(u32x4, wl[0]), w1 = __builtin_bit_cast(u32x4, wl[1]);
              const i32x8 a6 = {(int)c0[0], (int)c0[1], (int)c0[2], (int)c0[3], (int)c1[0], (int)c1[1], 0, 0};
              const i32x8 w6 = {(int)w0[0], (int)w0[1], (int)w0[2], (int)w0[3], (int)w1[0], (int)w1[1], 0, 0};
              acc[t] = mfma_mx_fp6(a6, w6, acc[t], (int)c1[2], (int)w1[2]);
            }
          } else {
            acc[t] = mfma_p16(al[uv % RING], wh[ks], acc[t]);
            acc[t] = mfma_p16(ah[uv % RING], wl[ks], acc[t]);
            acc[t] = mfma_p16(ah[uv % RING], wh[ks], acc[t]);
            if constexpr (T16 && uv == 0) {
#pragma unroll
              for (int cb = 0; cb < 2; ++cb) {
                acc16[cb] = mfma16_p16(a16l, w16h[cb], acc16[cb]);
                acc16[cb] = mfma16_p16(a16h, w16l[cb], acc16[cb]);
                acc16[cb] = mfma16_p16(a16h, w16h[cb], acc16[cb]);
              }
            }
          }
          sched_fence();  // keep the same-accumulator triple back to back (no filler inside)
          if constexpr (uv < X3_A_PIECES) piece_a(ca, uv, abuf ^ 1);
          sched_fence();
        }
      });
#undef X3_RD_A
      advance_a(ca);
      wait_vmem_all();
      wg_barrier();
      abuf ^= 1;
      wh[0] = wnh[0]; wh[1] = wnh[1]; wl[0] = wnl[0]; wl[1] = wnl[1];
    }
    }   // !PIPE

    // ---- epilogue.  In the accumulator layout a lane owns ONE column and 16 rows of each 32x32 sub-tile, which would
    // mean 4-byte (fp32) / 2-byte (planes) stores: the store tail is issue-bound (cdna_hip_programming.md T21).  So
    // each wave transposes 8 rows x 32 columns at a time (accumulator registers 4g..4g+3 of both lane halves) through
    // its private 1 KB LDS patch -- disjoint from the A stages, which already hold the next tile's first stage
    // -- and writes 16 bytes per lane: lane -> (row = lane>>3, 4 consecutive columns).
    [&]() __attribute__((always_inline)) {
        // epilogue scope: every lane-derived index below is rebuilt from an OPAQUE copy of the lane id, so that hipcc cannot
        // compute the epilogue's per-round offsets once, in front of the tile loop, and carry them (24 VGPRs of hoisted
        // store offsets, spilled in the in_proj instantiation) through every k-loop.  (A lambda called in place, not a plain
        // block: hipcc schedules 21 of the 28 instantiations differently for the block, and every measurement of this kernel
        // was taken on this form.)
    int lane_e = lane;
    opaque_v(lane_e);
    const int r = lane_e & 31, h = lane_e >> 5, r16 = lane_e & 15, g16 = lane_e >> 4;
    const int m_end = min(M, m0 + rows_per_tile);
    float* patch = reinterpret_cast<float*>(lds + x3_patch_base(RINGN)) + wid * (X3_PATCH_BYTES / 4);  // [8][32] fp32
    const int prow = lane_e >> 3, pc4 = (lane_e & 7) * 4;
    const int n4 = ncol0 + pc4;                          // first of this lane's 4 columns in the row layout
    // per-lane column vectors of the row-major side: bias (or folded bias), Q scale, folded column sums, residual gamma/beta
    const int cl4 = wid * 32 + pc4;                      // this lane's first column inside the tile
    const float4 b4 = ld4(cvec + cl4);
    // column scale (in_proj's Q columns; scale_cols is a multiple of the tile width): only the instantiations without an
    // activation and without a plane residual carry one (the launcher refuses it elsewhere) -- two packed multiplies per round
    constexpr bool COL_SCALE = x3_has_col_scale(ACT, RES);
    const float mult4 = (COL_SCALE && n4 < ep.scale_cols) ? ep.col_scale : 1.f;
    float4 c4 = zero4(), g4 = zero4(), be4 = zero4();
    if constexpr (FOLD) c4 = ld4(cvec + 256 + cl4);
    if constexpr (RES == 3) {
      g4 = ld4(cvec + 512 + cl4);
      be4 = ld4(cvec + 768 + cl4);
    }
    // the same in the accumulator layout (lane -> column r of the wave's 32): V^T path
    const float bias = cvec[wid * 32 + r];
    float csum = 0.f;
    if constexpr (FOLD) csum = cvec[256 + wid * 32 + r];
    // accumulator values of one round, row-major, -> the GEMM's value:  fold / bias, activation, Q scale
    const float accs = ep.acc_scale;
    // RES == 3: the rebuilt LayerNorm residual's beta is a per-column constant like the bias -- added with it
    const float4 bb4 = RES == 3 ? make_float4(b4.x + be4.x, b4.y + be4.y, b4.z + be4.z, b4.w + be4.w) : b4;
    auto finish4 = [&](float4 v4, float2 st) __attribute__((always_inline)) {
      v4.x *= accs; v4.y *= accs; v4.z *= accs; v4.w *= accs;
      if constexpr (FOLD) {
        v4.x = st.y * (v4.x - st.x * c4.x) + bb4.x; v4.y = st.y * (v4.y - st.x * c4.y) + bb4.y;
        v4.z = st.y * (v4.z - st.x * c4.z) + bb4.z; v4.w = st.y * (v4.w - st.x * c4.w) + bb4.w;
      } else {
        v4.x += bb4.x; v4.y += bb4.y; v4.z += bb4.z; v4.w += bb4.w;
      }
      if (ACT == ACT_GELU) { v4.x = gelu_erf_fast(v4.x); v4.y = gelu_erf_fast(v4.y); v4.z = gelu_erf_fast(v4.z); v4.w = gelu_erf_fast(v4.w); }
      else if (ACT == ACT_SILU) { v4.x = silu(v4.x); v4.y = silu(v4.y); v4.z = silu(v4.z); v4.w = silu(v4.w); }
      if constexpr (COL_SCALE) { v4.x *= mult4; v4.y *= mult4; v4.z *= mult4; v4.w *= mult4; }
      return v4;
    };
    // row statistics of the rows a lane finishes in round j (FOLD: of the A rows, RES == 3: of the residual rows).  Read ONE
    // ROUND AHEAD, next to the patch read: fetched where it is used, each round paid a second, exposed LDS round trip
    // (the wave-level fences keep it behind the next round's patch writes)
    auto row_stats = [&](auto j_tag) __attribute__((always_inline)) {
      constexpr int j = decltype(j_tag)::value;
      if constexpr (LN_TABS && j < NROUNDS) return stab[(j / 4) * 32 + 8 * (j % 4) + prow];
      else return make_float2(0.f, 1.f);
    };
    // 28 rounds (row sub-tile t, register group g): raw accumulators -> patch -> 16-byte row-major read.  Round j+1's
    // patch writes are issued between round j's read and its stores, so the LDS round trip of one round hides under
    // the VALU work of the next (a wave's LDS operations execute in order).
    auto patch_write = [&](auto j_tag) __attribute__((always_inline)) {
      constexpr int j = decltype(j_tag)::value, t = j / 4, g = j % 4;
      if constexpr (PIPE) {
        // 16x16 accumulators: round j = rows 8 (j % 2) .. + 7 of slice j / 2, held by the lanes with lane >> 5 == j % 2 (as below)
        if constexpr (j < NROUNDS) {
          if (h == j % 2) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
              for (int e = 0; e < 4; ++e) patch[((e + 4 * (g16 & 1)) << 5) + 16 * cb + r16] = accm_[j / 2][cb][e];
          }
        }
      } else if constexpr (j < 4 * NT32) {
#pragma unroll
        for (int e = 0; e < 4; ++e) patch[((e + 4 * h) << 5) + r] = acc[t][4 * g + e];
      } else if constexpr (T16 && j < NROUNDS) {
        // 16-row sub-tile, rows 8g .. 8g+7 = accumulator rows 4*(lane>>4) + e of the lanes with lane>>5 == g
        if (h == g) {
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int e = 0; e < 4; ++e) patch[((e + 4 * (g16 & 1)) << 5) + 16 * cb + r16] = acc16[cb][e];
        }
      }
    };

    if (OUT_QKV) {
      // in_proj -> attention operand planes (attention_x3.h).  rows_per_tile == S: tile row == token, tile_m == sequence.
      // Pad tokens (S <= token < SP): V^T pads are written with whatever finite values the neighbouring activation rows
      // produce (the attention kernel multiplies them by p == 0 exactly); Q / K pad rows are never read by it and are not
      // stored in the last sub-tile (masking every round cost 112 hoisted lane masks, 280 spilled SGPRs).
      const int Dm = ep.D, SPq = ep.qkv.SP, Hq = ep.qkv.H;
      int ncol_e = ncol0, m0_e = m0;
      // opaque copies: keeps hipcc from computing the epilogue's 64-bit store addresses BEFORE the k-loop and carrying
      // them (spilled) across it
      opaque_s(ncol_e, m0_e);
      const int which = ncol_e / Dm, hcol = ncol_e - which * Dm, head = hcol >> 7, d0 = hcol & 127;
      const size_t shq = (size_t)(m0_e / rows_per_tile) * Hq + head;
      if (ncol0 < N) {
        if (which == 2) {
          // V^T: accumulator registers 8 s2 .. 8 s2 + 7 of a lane ARE positions 8h .. 8h+7 of 16-key group s2
          p16_t* vhp = ep.qkv.vh + ((shq * ep.qkv.NKT) * AX_HD + d0 + r) * 32 + 8 * h;
          p16_t* vlp = ep.qkv.vl + ((shq * ep.qkv.NKT) * AX_HD + d0 + r) * 32 + 8 * h;
          const int nkt = ep.qkv.NKT;
          if constexpr (PIPE) {
            // 16x16 accumulators: keys 16 s + 4 (lane >> 4) + e of slice s = key tile s / 2, 16-key group s % 2, positions
            // 4 ((g16 >> 1) + 2 (g16 & 1)) + e of the group (the T16 store below, on every slice); keys 208-223 are never written
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
              const int cl = 16 * cb + r16;                      // this lane's column inside the wave's 32
              const float b16 = cvec[wid * 32 + cl];
              const float c16 = FOLD ? cvec[256 + wid * 32 + cl] : 0.f;
              const size_t o0 = (shq * ep.qkv.NKT * AX_HD + d0 + cl) * 32 + 4 * ((g16 >> 1) + 2 * (g16 & 1));
              auto vfin = [&](float a) __attribute__((always_inline)) { return a * accs + b16; };   // (!FOLD: one expression for both uses)
              // PAIR: key 0 of sequence pair_B + b is tile row S -- register S & 3 of slice S >> 4 in the lane of this column whose
              // lane >> 4 is (S >> 2) & 3.  Every lane finishes that register of its own (the slice and the register are wave-uniform:
              // no dynamic register index), then the lanes that hold keys 0-3 fetch it across the wave and store it WITH their
              // keys 1-3, in one 8-byte store per plane: no byte of the other sequence is written twice.
              float u0 = 0.f;
              size_t po = 0;
              if constexpr (PAIR) {
                const int sS = ep.S >> 4, eS = ep.S & 3;
#pragma unroll
                for (int s = 0; s < NS16; ++s) {
                  if (s == sS) {
                    const f32x4 a = accm_[s][cb];
                    u0 = vfin(eS == 0 ? a[0] : eS == 1 ? a[1] : eS == 2 ? a[2] : a[3]);
                  }
                }
                u0 = lane_bcast(u0, r16 + 16 * ((ep.S >> 2) & 3));
                po = (size_t)ep.pair_B * Hq * ep.qkv.NKT * (AX_HD * 32);
              }
#pragma unroll
              for (int s = 0; s < NS16; ++s) {
                if ((s >> 1) < nkt) {
                  float vv[4];
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
                    if constexpr (FOLD) {
                      const float2 st = atab[16 * s + 4 * g16 + e];
                      vv[e] = st.y * (accm_[s][cb][e] * accs - st.x * c16) + b16;
                    } else {
                      vv[e] = vfin(accm_[s][cb][e]);
                    }
                  }
                  const size_t o = o0 + (size_t)(s >> 1) * (AX_HD * 32) + 16 * (s & 1);
                  split4_store(ep.qkv.vh + o, ep.qkv.vl + o, make_float4(vv[0], vv[1], vv[2], vv[3]));
                  if constexpr (PAIR) {   // the same keys of sequence pair_B + b (pad keys, tile row S among them, stay finite)
                    const float k0 = (s == 0 && g16 == 0) ? u0 : vv[0];
                    split4_store(ep.qkv.vh + po + o, ep.qkv.vl + po + o, make_float4(k0, vv[1], vv[2], vv[3]));
                  }
                }
              }
            }
          } else {
#pragma unroll
          for (int t = 0; t < NT32; ++t) {
            if (t < nkt) {
#pragma unroll
              for (int s2 = 0; s2 < 2; ++s2) {
                float vv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                  if constexpr (FOLD) {
                    const float2 st = atab[32 * t + mfma_row(8 * s2 + j, h)];
                    vv[j] = st.y * (acc[t][8 * s2 + j] * accs - st.x * csum) + bias;
                  } else {
                    vv[j] = acc[t][8 * s2 + j] * accs + bias;
                  }
                }
                p16x8 vh8, vl8;
                split8(vv, vh8, vl8);
                *reinterpret_cast<p16x8*>(vhp + t * (AX_HD * 32) + 16 * s2) = vh8;
                *reinterpret_cast<p16x8*>(vlp + t * (AX_HD * 32) + 16 * s2) = vl8;
              }
            }
          }
          if constexpr (T16) {
            // keys 192 + 4*(lane>>4) + e of key tile 6, 16-key group 0: positions 4*((g16>>1) + 2*(g16&1)) + e; the group-1
            // half of the tile (keys 208-223) is never written -- the attention kernel skips it
            if (NT32 < nkt) {
#pragma unroll
              for (int cb = 0; cb < 2; ++cb) {
                const int cl = 16 * cb + r16;                      // this lane's column inside the wave's 32
                const float b16 = lane_bcast(bias, cl);
                const float c16 = FOLD ? lane_bcast(csum, cl) : 0.f;
                float vv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  if constexpr (FOLD) {
                    const float2 st = atab[192 + 4 * g16 + e];
                    vv[e] = st.y * (acc16[cb][e] * accs - st.x * c16) + b16;
                  } else {
                    vv[e] = acc16[cb][e] * accs + b16;
                  }
                }
                const size_t o = ((shq * ep.qkv.NKT + NT32) * AX_HD + d0 + cl) * 32 + 4 * ((g16 >> 1) + 2 * (g16 & 1));
                split4_store(ep.qkv.vh + o, ep.qkv.vl + o, make_float4(vv[0], vv[1], vv[2], vv[3]));
              }
            }
          }
          }   // !PIPE
        } else {
          // Q / K rows: one base pointer per plane, 32-bit offsets
          p16_t* dh = (which == 0 ? ep.qkv.qh : ep.qkv.kh) + shq * SPq * AX_HD + d0 + pc4;
          p16_t* dl = (which == 0 ? ep.qkv.ql : ep.qkv.kl) + shq * SPq * AX_HD + d0 + pc4;
          // sub-tiles that hold rows to store; PAIR: rows 0 .. S (S a multiple of 32: tile row S opens one more than the planes' NKT)
          const int nkt = PAIR ? (ep.S + 32) / 32 : ep.qkv.NKT;
          // PAIR: the same rows of sequence pair_B + b (rows 1 .. S-1 as they are, tile row S as its token 0)
          const size_t pq = PAIR ? (size_t)ep.pair_B * Hq * SPq * AX_HD : 0;
          patch_write(std::integral_constant<int, 0>{});
          float2 st_cur = row_stats(std::integral_constant<int, 0>{});
          static_for<NROUNDS>([&](auto j_tag) __attribute__((always_inline)) {
            constexpr int j = decltype(j_tag)::value, t = j / 4, g = j % 4;
            wave_lds_fence();
            float4 v4 = ld4(&patch[prow * 32 + pc4]);
            const float2 st_next = row_stats(std::integral_constant<int, j + 1>{});
            wave_lds_fence();
            patch_write(std::integral_constant<int, j + 1>{});
            const float2 st = st_cur;
            st_cur = st_next;
            if (t < nkt) {
              const int tok = 32 * t + 8 * g + prow;
              v4 = finish4(v4, st);
              // tokens past the sequence (only the last sub-tile can hold any when the tile is one sequence of more than
              // 192 tokens) are not stored: the attention kernel never reads Q / K pad rows
              if constexpr (PAIR) {
                // (tile row S is another sequence's token here: no pad row of sequence b is stored in any sub-tile)
                if (tok < ep.S) split4_store(dh + tok * AX_HD, dl + tok * AX_HD, v4);
                if ((unsigned)(tok - 1) < (unsigned)ep.S) {
                  const int tok2 = tok == ep.S ? 0 : tok;
                  split4_store(dh + pq + tok2 * AX_HD, dl + pq + tok2 * AX_HD, v4);
                }
              } else {
                if (t < X3_MSUB - 1 || tok < ep.S) split4_store(dh + tok * AX_HD, dl + tok * AX_HD, v4);
              }
            }
          });
        }
      }
    } else {
      // residual tile: streamed two row sub-tiles ahead of its use through untracked loads (common.h gload16_async);
      // rows past the matrix are clamped (loaded, never stored)
      constexpr bool HAS_RES = RES != 0;
      constexpr bool RES_PLANES = RES == 2 || RES == 3;
      // plane rows of this tile (output and residual) are addressed through clipped windows (common.h ClipWin): byte offset
      // of a lane's 4 columns in tile row `prow`, plus a wave-uniform row term per round
      static_assert(!(EMBED && RES_PLANES), "the EMBED epilogue takes an fp32 residual");
      constexpr bool CLIP_OUT = OUT_PLANES && !EMBED;
      const uint32_t pitch2 = (uint32_t)ep.ld * 2u;
      const uint32_t voff0 = n4 < N ? ((uint32_t)prow * (uint32_t)ep.ld + (uint32_t)n4) * 2u : CLIP_OFF;
      ClipWin w_oh = {}, w_ol = {}, w_rh = {}, w_rl = {};
      {
        int m0_e = m0;
        opaque_s(m0_e);   // (opaque: keeps the windows from being built, and carried, in front of the k-loop)
        const size_t row0 = (size_t)m0_e * ep.ld;
        if constexpr (CLIP_OUT) {
          const uint32_t bytes = (uint32_t)(m_end - m0_e) * pitch2;
          w_oh = clip_win(ep.oh + row0, bytes);
          w_ol = clip_win(ep.ol + row0, bytes);
        }
        if constexpr (RES_PLANES) {
          const uint32_t bytes = (uint32_t)min(M - m0_e, X3_TM) * pitch2;
          w_rh = clip_win(ep.resh + row0, bytes);
          w_rl = clip_win(ep.resl + row0, bytes);
        }
      }
      constexpr int RR = (RES == 3) ? 2 : 3;   // residual sub-tiles in flight + in use (RES == 3 sits at the VGPR limit)
      f32x4 rr[RR][4];       // RES == 1
      u32x2 rh[RR][4], rl[RR][4];  // RES == 2 / 3
      auto res_issue = [&](auto t_tag) __attribute__((always_inline)) {
        constexpr int t = decltype(t_tag)::value;
        if constexpr (HAS_RES && t < X3_MSUB) {
#pragma unroll
          for (int g = 0; g < x3_res_rounds(t, T16); ++g) {
            if constexpr (RES == 1) {
              const int m = min(m0 + t * 32 + 8 * g + prow, M - 1);
              const size_t o = (size_t)(EMBED ? 1 + m % ep.emb_T : m) * ep.ld + (n4 < N ? n4 : 0);   // EMBED: positional row
              gload16_async(rr[t % RR][g], ep.res + o);
            } else {
              const uint32_t o = voff0 + (uint32_t)(t * 32 + 8 * g) * pitch2;   // past the matrix: reads 0, never stored
              clip_load8_async(rh[t % RR][g], w_rh, o);
              clip_load8_async(rl[t % RR][g], w_rl, o);
            }
          }
        }
      };
      auto res_wait = [&](auto t_tag) __attribute__((always_inline)) {
        constexpr int t = decltype(t_tag)::value;
        // loads of the younger sub-tiles already requested (the only ones allowed to stay in flight)
        constexpr int ahead = x3_res_younger_rounds(t, RR, T16);
        if constexpr (RES == 1) {
          vmem_wait<ahead>(rr[t % RR][0], rr[t % RR][1], rr[t % RR][2], rr[t % RR][3]);
        } else if constexpr (RES_PLANES) {
          vmem_wait<2 * ahead>(rh[t % RR][0], rh[t % RR][1], rh[t % RR][2], rh[t % RR][3], rl[t % RR][0], rl[t % RR][1],
                               rl[t % RR][2], rl[t % RR][3]);
        }
      };
      res_issue(std::integral_constant<int, 0>{});
      if constexpr (RR == 3) res_issue(std::integral_constant<int, 1>{});
      float2* part = reinterpret_cast<float2*>(lds + x3_part_base(RINGN)) + wid * X3_TM;   // OSTAT: this column block's partials
      patch_write(std::integral_constant<int, 0>{});
      float2 st_cur = row_stats(std::integral_constant<int, 0>{});
      static_for<NROUNDS>([&](auto j_tag) __attribute__((always_inline)) {
        constexpr int j = decltype(j_tag)::value, t = j / 4, g = j % 4;
        if constexpr (HAS_RES && g == 0) {
          res_issue(std::integral_constant<int, t + RR - 1>{});
          res_wait(std::integral_constant<int, t>{});
        }
        wave_lds_fence();
        float4 v4 = ld4(&patch[prow * 32 + pc4]);
        const float2 st_next = row_stats(std::integral_constant<int, j + 1>{});
        wave_lds_fence();
        patch_write(std::integral_constant<int, j + 1>{});
        const float2 st = st_cur;
        st_cur = st_next;
        const int row_in_tile = t * 32 + 8 * g + prow;
        v4 = finish4(v4, st);
        if constexpr (RES == 1) {
          const f32x4 q4 = rr[t % RR][g];
          v4.x += q4[0]; v4.y += q4[1]; v4.z += q4[2]; v4.w += q4[3];
        } else if constexpr (RES_PLANES) {
          // x = hi + lo (RES == 3: minus the row mean, times rstd * gamma; beta rides in the bias vector bb4): the planes are
          // converted inside the adds (common.h f16_half_plus), the mean leaves before anything is scaled
          const u32x2 a = rh[t % RR][g], b = rl[t % RR][g];
          const float c0 = RES == 3 ? -st.x : 0.f;
          const float d0 = f16_half_plus<0>(b[0], f16_half_plus<0>(a[0], c0));
          const float d1 = f16_half_plus<1>(b[0], f16_half_plus<1>(a[0], c0));
          const float d2 = f16_half_plus<0>(b[1], f16_half_plus<0>(a[1], c0));
          const float d3 = f16_half_plus<1>(b[1], f16_half_plus<1>(a[1], c0));
          if constexpr (RES == 3) {
            v4.x = fmaf(d0, st.y * g4.x, v4.x); v4.y = fmaf(d1, st.y * g4.y, v4.y);
            v4.z = fmaf(d2, st.y * g4.z, v4.z); v4.w = fmaf(d3, st.y * g4.w, v4.w);
          } else {
            v4.x += d0; v4.y += d1; v4.z += d2; v4.w += d3;
          }
        }
        if constexpr (OSTAT) {   // partial (sum, centred sum of squares) of this row over the wave's 32 columns
          const float s1 = sum_lanes8((v4.x + v4.y) + (v4.z + v4.w));
          const float mw = s1 * (1.0f / 32.0f);
          const float dx = v4.x - mw, dy = v4.y - mw, dz = v4.z - mw, dw = v4.w - mw;
          const float m2 = sum_lanes8((dx * dx + dy * dy) + (dz * dz + dw * dw));
          if ((lane_e & 7) == 0) part[row_in_tile] = make_float2(s1, m2);
        }
        if constexpr (CLIP_OUT) split4_store_clip(w_oh, w_ol, voff0 + (uint32_t)(t * 32 + 8 * g) * pitch2, v4);
        if constexpr (EMBED || OUT_F32) {
          const int m = m0 + row_in_tile;
          if (m < m_end && n4 < N) {  // N % 4 == 0
            if constexpr (EMBED) {
              const int bb = m / ep.emb_T, tt = m - bb * ep.emb_T;
              for (int br = 0; br < ep.emb_nbranch; ++br) {
                const size_t o = ((size_t)(br * ep.emb_B + bb) * (ep.emb_T + 1) + 1 + tt) * ep.ld + n4;
                split4_store(ep.oh + o, ep.ol + o, v4);
              }
            } else {
              st4(ep.out + (size_t)m * ep.ld + n4, v4);
            }
          }
        }
      });
    }
    }();   // epilogue scope
    if constexpr (OSTAT && !OUT_QKV) {   // rows x column blocks partials -> one (sum, M2) pair per row and column tile
        const int m_end = min(M, m0 + rows_per_tile);
        wg_barrier();
        if (tid < X3_TM && m0 + tid < m_end) {
          const float2* pp = reinterpret_cast<const float2*>(lds + x3_part_base(RINGN));
          float s1 = 0.f;
#pragma unroll
          for (int w8 = 0; w8 < X3_NWAVE; ++w8) s1 += pp[w8 * X3_TM + tid].x;
          const float mt = s1 * (1.0f / X3_TN);     // OSTAT launches have N % X3_TN == 0: every block contributes 32 columns
          float m2 = 0.f;
#pragma unroll
          for (int w8 = 0; w8 < X3_NWAVE; ++w8) {
            const float2 v = pp[w8 * X3_TM + tid];
            const float dm = v.x * (1.0f / 32.0f) - mt;
            m2 += v.y + 32.0f * dm * dm;
          }
          *reinterpret_cast<float2*>(ep.ostat + ((size_t)(m0 + tid) * tiles_n + n0 / X3_TN) * 2) = make_float2(s1, m2);
        }
      }
  }
  wait_vmem_all();  // the stream's last (unused) LDS-DMA stage must land before this workgroup's LDS is released
}

#ifndef MDM_X3_KERNEL_ONLY   // (register-pressure studies compile single instantiations of the kernel without the launchers)
// rows per block tile: a whole number of sequences when the row space is sequence-structured (keeps the tile count a
// multiple of the sequence count -> no ragged last wave of workgroups), else the full 224.
inline int x3_rows_per_tile(int M, int seq_len) {
  if (seq_len > 0 && seq_len <= X3_TM && M % seq_len == 0) return (X3_TM / seq_len) * seq_len;
  return X3_TM;
}

// persistent grid: one workgroup per CU
inline int x3_grid_limit() {
  const int cus = rt_cu_count();   // (the emulator's 3 comes back as it is: a grid that small walks through the tile roll-over paths)
  return cus >= 8 ? cus / 8 * 8 : cus;  // xcd_remap keeps a workgroup on one XCD only if the stride is a multiple of 8
}

template <int ACT, int RES, unsigned FLAGS>
inline int launch_gemm_x3_w(const X3Operand& A, const X3Weights& W, const X3Epilogue& ep, int M, int N, int K,
                                int rpt, hipStream_t stream) {
  constexpr bool T16 = (FLAGS & X3_T16) != 0, PIPE = (FLAGS & X3_PIPE) != 0, PAIR = (FLAGS & X3_PAIR) != 0;
  constexpr bool LN = (FLAGS & (X3_FOLD | X3_OSTAT)) != 0 || RES == 3;
  constexpr int RINGN = PIPE ? X3_PIPE_RING : X3_A_RING;
  const int tiles_m = (M + rpt - 1) / rpt, tiles_n = (N + X3_TN - 1) / X3_TN;
  const int total = tiles_m * tiles_n;
  auto kfn = &gemm_x3_kernel<ACT, RES, FLAGS>;
  if (T16 && rpt > X3_TM - 16) return -2;
  if (PAIR && (rpt + 1 > X3_TM - 16 || ep.pair_B < 1 || M != ep.pair_B * rpt)) return -2;   // tile row S must exist; one tile per sample
  if (PIPE && (K / X3_BK) % 2 != 0) return -2;   // the pipelined k-loop is unrolled over step pairs
  if (!x3_has_col_scale(ACT, RES) && ep.scale_cols > 0) return -2;   // (this instantiation compiles the column scale out)
  {   // every form needs more than the 64 KB a kernel gets unasked
    static bool configured[kMaxDevices] = {};  // per instantiation and device (the attribute belongs to the device's code object)
    if (const int rc = rt_dyn_lds_once(kfn, x3_lds_bytes(LN, RINGN), configured, stream)) return rc;
  }
  const int grid = std::min(total, x3_grid_limit());
  MDM_LAUNCH(kfn, dim3(grid), dim3(64 * X3_NWAVE), x3_lds_bytes(LN, RINGN), stream, A, W, ep, M, N, K, rpt, tiles_n, total);
  return 0;
}

// The GEMMs of the folded-LayerNorm stacks (encoder.h, decoder.h): which epilogue a launch_x3_ln call (api_launch.h) runs.  The two
// dispatchers -- launch_gemm_x3_ln_t here, launch_gemm_x3s_rt in gemm_x3s.h -- map a kind to its kernel instantiation.
enum X3Kind : int {
  X3K_IN_PROJ_FOLD = 0,    // in_proj, A = pre-norm sum        FOLD -> attention operand planes
  X3K_OUT_PROJ_L0 = 1,     // out_proj of layer 0              residual = plain planes, writes planes + row statistics
  X3K_OUT_LN_RES = 2,      // out_proj (l >= 1) / linear2      residual = LayerNorm rebuilt from planes, writes planes + row statistics
  X3K_LINEAR1_GELU = 3,    // linear1                          FOLD + GELU -> planes
  X3K_FOLD_F32 = 4,        // OutputProcess (trans_dec: also the cross-attention q projection)   FOLD -> fp32
  X3K_EMBED = 5,           // InputProcess                     + positional rows, planes to the token rows of every branch (EMBED)
  X3K_IN_PROJ_PLAIN = 6,   // in_proj of layer 0               no folded LayerNorm -> attention operand planes (gemm_x3s.h's tiles;
                           //                                  on this kernel's launch_x3_ln goes through launch_gemm_x3_qkv)
};
// TILE: the tile form (X3_T16, X3_PIPE), which launch_gemm_x3_ln chooses by shape
template <unsigned TILE>
inline int launch_gemm_x3_ln_t(X3Kind kind, const X3Operand& A, const X3Weights& W, const X3Epilogue& ep, int M, int N,
                                   int K, int rpt, hipStream_t s) {
  switch (kind) {
    case X3K_IN_PROJ_FOLD: return launch_gemm_x3_w<ACT_NONE, /*RES*/ 0, X3_OUT_QKV | X3_FOLD | TILE>(A, W, ep, M, N, K, rpt, s);
    case X3K_OUT_PROJ_L0: return launch_gemm_x3_w<ACT_NONE, /*RES*/ 2, X3_OUT_PLANES | X3_OSTAT | TILE>(A, W, ep, M, N, K, rpt, s);
    case X3K_OUT_LN_RES: return launch_gemm_x3_w<ACT_NONE, /*RES*/ 3, X3_OUT_PLANES | X3_OSTAT | TILE>(A, W, ep, M, N, K, rpt, s);
    case X3K_LINEAR1_GELU: return launch_gemm_x3_w<ACT_GELU, /*RES*/ 0, X3_OUT_PLANES | X3_FOLD | TILE>(A, W, ep, M, N, K, rpt, s);
    case X3K_FOLD_F32: return launch_gemm_x3_w<ACT_NONE, /*RES*/ 0, X3_OUT_F32 | X3_FOLD | TILE>(A, W, ep, M, N, K, rpt, s);
    case X3K_EMBED:   // InputProcess: K = 288 is nine steps -- always the step-synchronous loop
      return launch_gemm_x3_w<ACT_NONE, /*RES*/ 1, X3_OUT_PLANES | X3_EMBED | (TILE & X3_T16)>(A, W, ep, M, N, K, rpt, s);
    default: return -2;
  }
}
// 208-row tiles whenever the row extent of a tile fits (S = 197 does); on them the pipelined loop wherever it exists (an even
// number of 32-deep k steps; not InputProcess)
inline int launch_gemm_x3_ln(X3Kind kind, const X3Operand& A, const X3Weights& W, const X3Epilogue& ep, int M, int N,
                                 int K, int rpt, hipStream_t s) {
  if (rpt <= X3_TM - 16) {
    if (kind != X3K_EMBED && (K / X3_BK) % 2 == 0) return launch_gemm_x3_ln_t<X3_T16 | X3_PIPE>(kind, A, W, ep, M, N, K, rpt, s);
    return launch_gemm_x3_ln_t<X3_T16>(kind, A, W, ep, M, N, K, rpt, s);
  }
  return launch_gemm_x3_ln_t<0u>(kind, A, W, ep, M, N, K, rpt, s);
}

// runtime (act, res, outputs) -> one of the instantiations the encoder needs (224-row tiles, step-synchronous loop)
inline int launch_gemm_x3(const X3Operand& A, const X3Weights& W, const X3Epilogue& ep, int M, int N, int K, int act,
                              int seq_len, hipStream_t s) {
  const bool res = ep.res != nullptr, f32 = ep.out != nullptr, pl = ep.oh != nullptr;
  const int rpt = x3_rows_per_tile(M, seq_len);
  if (ep.resh != nullptr) {  // residual stream held as planes (the model's f16x3 mode)
    if (act == ACT_NONE && !res && f32 && !pl) return launch_gemm_x3_w<ACT_NONE, /*RES*/ 2, X3_OUT_F32>(A, W, ep, M, N, K, rpt, s);
    return -2;
  }
  if (act == ACT_NONE && !res && f32 && !pl) return launch_gemm_x3_w<ACT_NONE, /*RES*/ 0, X3_OUT_F32>(A, W, ep, M, N, K, rpt, s);
  if (act == ACT_NONE && res && f32 && !pl) return launch_gemm_x3_w<ACT_NONE, /*RES*/ 1, X3_OUT_F32>(A, W, ep, M, N, K, rpt, s);
  if (act == ACT_GELU && !res && !f32 && pl) return launch_gemm_x3_w<ACT_GELU, /*RES*/ 0, X3_OUT_PLANES>(A, W, ep, M, N, K, rpt, s);
  if (act == ACT_GELU && !res && f32 && !pl) return launch_gemm_x3_w<ACT_GELU, /*RES*/ 0, X3_OUT_F32>(A, W, ep, M, N, K, rpt, s);
  if (act == ACT_GELU && res && f32 && !pl) return launch_gemm_x3_w<ACT_GELU, /*RES*/ 1, X3_OUT_F32>(A, W, ep, M, N, K, rpt, s);
  if (act == ACT_SILU && !res && f32 && !pl) return launch_gemm_x3_w<ACT_SILU, /*RES*/ 0, X3_OUT_F32>(A, W, ep, M, N, K, rpt, s);
  return -2;
}

#ifdef MDM_PROBES
// The f16f6 building block (mdm_linear_f16f6): plain fp32-out epilogues on the F6 k-loop, 224-row tiles
inline int launch_gemm_f16f6(const X3Operand& A, const X3Weights& W, const X3Epilogue& ep, int M, int N, int K, int act,
                             hipStream_t s) {
  const bool res = ep.res != nullptr;
  if (act == ACT_NONE && !res) return launch_gemm_x3_w<ACT_NONE, /*RES*/ 0, X3_OUT_F32 | X3_F6>(A, W, ep, M, N, K, X3_TM, s);
  if (act == ACT_NONE && res) return launch_gemm_x3_w<ACT_NONE, /*RES*/ 1, X3_OUT_F32 | X3_F6>(A, W, ep, M, N, K, X3_TM, s);
  if (act == ACT_GELU && !res) return launch_gemm_x3_w<ACT_GELU, /*RES*/ 0, X3_OUT_F32 | X3_F6>(A, W, ep, M, N, K, X3_TM, s);
  return -2;
}
#endif

// Does a guided in_proj launch (2 B sequences of S tokens) take the paired tile (kernel header, PAIR)?  Only the pipelined loop
// has it, and tile row S must exist; everything else runs one tile per sequence.
inline bool x3_qkv_pairs(int S, int D) { return S + 1 <= X3_TM - 16 && (D / X3_BK) % 2 == 0; }

// in_proj: tokens [nseq*S][D] x W [3D][D] -> the attention operand planes; one sequence per tile (tile row == token).
// pair_B > 0 (nseq == 2 pair_B, x3_qkv_pairs): one tile per SAMPLE, written to both of its sequences.
inline int launch_gemm_x3_qkv(const X3Operand& A, const X3Weights& W, const X3Epilogue& ep, int nseq, int S, int D,
                                  hipStream_t s, int pair_B = 0) {
  if (S > X3_TM) return -2;
  if (pair_B > 0) {
    if (nseq != 2 * pair_B || !x3_qkv_pairs(S, D)) return -2;
    X3Epilogue ep2 = ep;
    ep2.pair_B = pair_B;
    return launch_gemm_x3_w<ACT_NONE, /*RES*/ 0, X3_OUT_QKV | X3_T16 | X3_PIPE | X3_PAIR>(A, W, ep2, pair_B * S, 3 * D, D, S, s);
  }
  if (S <= X3_TM - 16) {
    if ((D / X3_BK) % 2 == 0) return launch_gemm_x3_w<ACT_NONE, /*RES*/ 0, X3_OUT_QKV | X3_T16 | X3_PIPE>(A, W, ep, nseq * S, 3 * D, D, S, s);
    return launch_gemm_x3_w<ACT_NONE, /*RES*/ 0, X3_OUT_QKV | X3_T16>(A, W, ep, nseq * S, 3 * D, D, S, s);
  }
  return launch_gemm_x3_w<ACT_NONE, /*RES*/ 0, X3_OUT_QKV>(A, W, ep, nseq * S, 3 * D, D, S, s);
}

#endif  // MDM_X3_KERNEL_ONLY

}  // namespace mdm
