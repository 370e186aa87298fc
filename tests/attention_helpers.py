"""Checker of the four attention kernels (csrc/attention_f32.h, attention_x3.h and the two streaming kernels of attention_long.h) at
kernel level, through mdm_attention / mdm_attention_x3: input builders for seven score regimes, an independent builder of the ABI's
`lengths` array (counts and per-sample bitmaps), the fp64 and fp32 references, the bound, and the one case runner that
tests/test_gpu_attention_kernels.py (MI355X) and tests/test_emu_attention_kernels.py (CPU wave emulator) share.

The bound.  err = max-abs of a kernel's output against reference_fp64; e_ref = max-abs of reference_fp32 against reference_fp64 ON THE
SAME CASE, computed when the test runs; floor(S) = the smallest non-zero e_ref among the `flat` cases of that S (no mask, and counts
[S - 1, S // 2]), for the cases whose fp32 reference happens to be exact (ties, a single valid key).  A parity assertion is

    err <= k * max(e_ref, floor(S))

with k per kernel family from profiles/r10a_attention_parity.md: twice the worst ratio measured over the whole matrix on the emulator
and on the MI355X, rounded up to an integer.  No fixed tolerance: a flat softmax leaves the fp32 reference 5-7e-7 from fp64, a peaked
one 1-2e-5, scores around +-100 5-9e-5.

Cases with a bound of their own, derived from the number formats (see count_zero_bounds / ties_bound): count 0 and a one-token sequence
(every output row is V[0] of its head) and `ties` (every output row is the mean of the valid V rows)."""
import math

import numpy as np
import torch

from helpers import memo

HD = 128
GUARD_ROWS = 64
SENTINEL = -7777.25                     # what the guard rows behind `out` hold before and after a call

# k of `err <= k * max(e_ref, floor)`: profiles/r10a_attention_parity.md (worst measured ratio per family, doubled, rounded up).
# "exact" = the kernels that keep every score tile in registers (S <= 224), "long" = the streaming kernels of attention_long.h.
K_BOUND = {("f32", "exact"): 4, ("f32", "long"): 4, ("x3", "exact"): 7, ("x3", "long"): 7}

PROFILES = ("flat", "peaked", "offset_pos", "offset_neg", "ascending", "descending", "ties")
OFFSET_C = 100.0                        # offset_pos / offset_neg: every score carries +-c
RAMP_Q, RAMP_K = 2.0, 20.0              # ascending / descending: the scores rise (fall) by RAMP_Q * RAMP_K = 40 over the sequence


def family(S):
    return "exact" if S <= 224 else "long"


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_qkv(seed, nseq, S, H, profile):
    """fp32 [nseq * S, 3 * H * 128], Q pre-scaled by 1 / sqrt(128) (the ABI's contract).  Every value stays far inside the fp16 hi
    plane's range (|x| < 40; tests/test_gpu_round2.py::test_fp16_planes_keep_subnormals_and_fail_loudly_out_of_range: 65504)."""
    assert profile in PROFILES
    rng = np.random.default_rng([seed, nseq, S, H, PROFILES.index(profile)])
    q, k, v = (rng.standard_normal((nseq, S, H, HD)) for _ in range(3))
    q /= math.sqrt(HD)
    u = rng.standard_normal((nseq, 1, H, HD))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)                    # one unit direction per (sequence, head)
    if profile == "peaked":
        q *= 8.0
    elif profile in ("offset_pos", "offset_neg"):
        sign = 1.0 if profile == "offset_pos" else -1.0
        q += sign * math.sqrt(OFFSET_C) * u
        k += math.sqrt(OFFSET_C) * u
    elif profile in ("ascending", "descending"):
        ramp = np.arange(S, dtype=np.float64) / max(S - 1, 1)
        if profile == "descending":
            ramp = 1.0 - ramp
        q += RAMP_Q * u
        k += RAMP_K * ramp[None, :, None, None] * u
    elif profile == "ties":
        k[:] = k[:, :1]
    D = H * HD
    qkv = np.concatenate([t.reshape(nseq * S, D) for t in (q, k, v)], axis=1)
    return np.ascontiguousarray(qkv, dtype=np.float32)


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
COUNT_SPECS = ("count0", "count1", "count31", "count32", "count33", "countS-1", "countS+5")
BITMAP_SPECS = ("bits_zero", "bits_last", "bits_alt", "bits_from63")
MASK_SPECS = COUNT_SPECS + BITMAP_SPECS + ("mixed", "none")


def _count_of(spec, S):
    return {"count0": 0, "count1": 1, "count31": 31, "count32": 32, "count33": 33, "countS-1": S - 1, "countS+5": S + 5}[spec]


def _words(frames_valid):
    """bool [F <= 256] -> eight int32 words, bit j of word i = frame 32 i + j (include/mdm_hip.h)."""
    assert frames_valid.size <= 256
    w = np.zeros(8, np.uint32)
    for f in np.flatnonzero(frames_valid):
        w[f >> 5] |= np.uint32(1) << np.uint32(f & 31)
    return w.view(np.int32)


def make_lengths(B, S, spec):
    """-> (the int32 `lengths` array in the ABI's format or None, bool [B, S] key validity).  Key 0 (the lead token) is always valid and
    frame f is key f + 1.  Forms: None / "none"; ("counts", [c, ...]) cycled over the samples; one of COUNT_SPECS (every sample the same
    count); one of BITMAP_SPECS (every sample count -1 and a bitmap; bits_alt: even frames for even samples, odd for odd ones);
    "mixed": samples cycle through [count S // 2, alternating bitmap, full count S - 1].  Arrays with a bitmap carry the words of the
    count rows too, as mdm_amd/mdm.py frame_mask_lengths writes them (the kernels read a row's words only behind a count of -1)."""
    F = S - 1
    frames = np.zeros((B, F), bool)
    counts = np.zeros(B, np.int64)
    if spec is None or spec == "none":
        return None, np.ones((B, S), bool)
    if isinstance(spec, tuple) or spec in COUNT_SPECS:
        cs = list(spec[1]) if isinstance(spec, tuple) else [_count_of(spec, S)]
        for b in range(B):
            counts[b] = cs[b % len(cs)]
            frames[b, :min(F, int(counts[b]))] = True
        lengths = counts.astype(np.int32)
    else:
        assert F <= 256, "bitmaps describe at most 256 frames"
        for b in range(B):
            counts[b] = -1
            if spec == "bits_zero":
                pass
            elif spec == "bits_last":
                frames[b, F - 1] = True
            elif spec == "bits_alt":
                frames[b, b % 2::2] = True
            elif spec == "bits_from63":
                frames[b, 63:] = True
            elif spec == "mixed":
                kind = b % 3
                if kind == 0:
                    counts[b] = S // 2
                    frames[b, :S // 2] = True
                elif kind == 1:
                    frames[b, ::2] = True
                else:
                    counts[b] = F
                    frames[b, :] = True
            else:
                raise ValueError(spec)
        lengths = np.concatenate([counts.astype(np.int32)] + [_words(frames[b]) for b in range(B)])
    valid = np.concatenate([np.ones((B, 1), bool), frames], axis=1)
    return np.ascontiguousarray(lengths, dtype=np.int32), valid


# ---- references -----------------------------------------------------------------------------------------------------------------------
def _reference(qkv, valid, H, dtype):
    """softmax(q k^T + mask) v per (sequence, head) in plain torch on the CPU; sequence s takes row s % B of `valid`."""
    B, S = valid.shape
    D = H * HD
    t = torch.from_numpy(qkv).to(dtype)
    nseq = t.shape[0] // S
    q, k, v = (x.reshape(nseq, S, H, HD).transpose(1, 2) for x in t.split(D, dim=-1))
    mask = torch.zeros(B, S, dtype=dtype).masked_fill(~torch.from_numpy(valid), float("-inf"))
    sc = q @ k.transpose(-1, -2) + mask[torch.arange(nseq) % B][:, None, None, :]
    return (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(nseq * S, D).numpy()


def reference_fp64(qkv, valid, H):
    return _reference(qkv, valid, H, torch.float64)


def reference_fp32(qkv, valid, H):
    return _reference(qkv, valid, H, torch.float32)


def maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def case_refs(seed, nseq, B, S, H, profile, spec):
    """(qkv, lengths, valid, fp64 reference, e_ref) of one case: built once per process, shared by the tests that need it, never
    written to."""
    def build():
        qkv = make_qkv(seed, nseq, S, H, profile)
        lengths, valid = make_lengths(B, S, spec)
        ref = reference_fp64(qkv, valid, H)
        e_ref = maxabs(reference_fp32(qkv, valid, H), ref)
        for a in (qkv, ref, valid) + (() if lengths is None else (lengths,)):
            a.setflags(write=False)
        return qkv, lengths, valid, ref, e_ref
    return memo(("attn_case", seed, nseq, B, S, H, profile, str(spec)), build)


def floor_of(S):
    """The smallest non-zero e_ref among the `flat` cases of this S (nseq = 2, H = 2: no mask, counts [S - 1, S // 2]).  0.0 only for
    S == 1, where every case is exact and the one-token bound applies instead."""
    def build():
        es = [case_refs(0, 2, 2, S, 2, "flat", spec)[4] for spec in (None, ("counts", [S - 1, S // 2]))]
        es = [e for e in es if e > 0.0]
        return min(es) if es else 0.0
    return memo(("attn_floor", S), build)


# ---- bounds derived from the number formats -------------------------------------------------------------------------------------------
def split_residual(v):
    """|v - (hi + lo)| of the fp16 operand split, hi = rne16(v), lo = rne16(v - hi), restated in numpy exactly as
    tests/test_gpu_round4.py::test_operand_split_is_bit_exact_fp16_hi_plus_lo pins the kernels' planes."""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return np.abs(v.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))


def count_zero_bounds(v):
    """One valid key: p = 1 for it and exp(-inf) = 0 for the others, sum = 1, so every output row is V[0] of its head.
    f32 kernel: 1 * v + 0 * (finite) in fp32 -- bit for bit.  f16x3 kernel: the one probability is p0 = exp(10 ln 2), 2^10 up to the
    rounding of the exponential, split as hi + lo; the output is (v_hi + v_lo) p0 / p0 up to a few roundings of 2^-24 |v|: off by the
    split's residual, at most 2^-22 |v|, plus those roundings -- inside 2^-21 max|v| (hi + lo keep 22 bits; the residual is checked
    against the restated split right here)."""
    bound = 2.0 ** -21 * float(np.abs(v).max())
    assert float(split_residual(v).max()) <= bound
    return 0.0, bound


def ties_bound(v_rows, kernel):
    """All K rows equal: the scores of a query are computed by the same operations on the same numbers, so they are equal, every valid
    p is exp(0) (one common p0 ~ 2^10 in the f16x3 kernels, which cancels in 1 / sum), the sum is n p0.  What remains is a fp32 sum of n
    values of V in some order, |error| <= (n - 1) u sum|v_j|, one rounding of 1 / n and one of the product (2 u |out|): per output
    column at most (n + 1) u mean_j|v_j|, with u = 2^-23, one whole ulp per addition, since an MFMA's multi-term accumulation is not
    documented to round every partial sum to nearest -- and in the f16x3 kernels the split residual of V, at most 2^-21 max_j|v_j|
    (count_zero_bounds).  The streaming kernels add one rounding per key tile for the running sum and the rescaling by c = 1: covered
    by the same first-order term with n + 1 + n / 32.  v_rows: the valid V rows [n, d] -> the bound per column [d]."""
    n = v_rows.shape[0]
    u = 2.0 ** -23
    b = (n + 1 + n / 32.0) * u * np.abs(v_rows.astype(np.float64)).mean(axis=0)
    if kernel == "x3":
        b = b + 2.0 ** -21 * np.abs(v_rows.astype(np.float64)).max(axis=0)
    return b


# ---- running a case -------------------------------------------------------------------------------------------------------------------
class GpuBackend:
    """mdm_attention / mdm_attention_x3 of the product library on cuda:0.  `out` gets GUARD_ROWS rows of SENTINEL behind it and starts
    as NaN; the f16x3 scratch starts as 0xFF bytes (a NaN in every 16-bit plane)."""
    name = "gpu"

    def __init__(self, lib, device="cuda:0"):
        self.lib, self.dev = lib, device

    def run(self, kernel, qkv, lengths, nseq, B, S, H):
        D = H * HD
        key = ("attn_dev", id(qkv))
        qd = memo(key, lambda: (qkv, torch.tensor(qkv).to(self.dev)))[1]      # (the host array is kept alive with its copy)
        ld = torch.tensor(lengths).to(self.dev) if lengths is not None else None
        out = torch.full((nseq * S + GUARD_ROWS, D), float("nan"), device=self.dev)
        out[nseq * S:] = SENTINEL
        stream = torch.cuda.current_stream().cuda_stream
        lp = ld.data_ptr() if ld is not None else None
        if kernel == "f32":
            self.lib.check(self.lib.mdm_attention(qd.data_ptr(), out.data_ptr(), lp, nseq, B, S, D, H, stream), "mdm_attention")
        else:
            nb = self.lib.mdm_attention_x3_scratch_bytes(nseq, S, D)
            scratch = torch.full((nb,), 0xFF, dtype=torch.uint8, device=self.dev)
            self.lib.check(self.lib.mdm_attention_x3(qd.data_ptr(), out.data_ptr(), lp, nseq, B, S, D, H, scratch.data_ptr(), nb,
                                                     stream), "mdm_attention_x3")
        torch.cuda.synchronize()
        return out.cpu().numpy()


class EmuBackend:
    """The same two entry points of the CPU wave emulator's library (tests/emu), on numpy buffers prepared the same way."""
    name = "emu"

    def __init__(self, lib):
        self.lib = lib

    def run(self, kernel, qkv, lengths, nseq, B, S, H):
        D = H * HD
        out = np.full((nseq * S + GUARD_ROWS, D), np.nan, np.float32)
        out[nseq * S:] = SENTINEL
        lp = lengths.ctypes.data if lengths is not None else None
        if kernel == "f32":
            self.lib.check(self.lib.mdm_attention(qkv.ctypes.data, out.ctypes.data, lp, nseq, B, S, D, H, None), "mdm_attention")
        else:
            nb = self.lib.mdm_attention_x3_scratch_bytes(nseq, S, D)
            scratch = np.full(nb, 0xFF, np.uint8)
            self.lib.check(self.lib.mdm_attention_x3(qkv.ctypes.data, out.ctypes.data, lp, nseq, B, S, D, H, scratch.ctypes.data, nb,
                                                     None), "mdm_attention_x3")
        return out


KERNELS = ("f32", "x3")


def run_kernel(backend, kernel, qkv, lengths, nseq, B, S, H):
    """One call with the memory contracts checked: the guard rows behind `out` untouched, rows [0, nseq * S) finite (so no pad row, pad
    key or unwritten byte of the poisoned scratch reached them).  -> out[:nseq * S]."""
    full = backend.run(kernel, qkv, lengths, nseq, B, S, H)
    guard = full[nseq * S:]
    assert guard.shape[0] == GUARD_ROWS and np.array_equal(guard, np.full_like(guard, SENTINEL)), f"{kernel}: wrote behind row nseq * S"
    out = full[:nseq * S]
    assert np.isfinite(out).all(), f"{kernel}: {int((~np.isfinite(out)).sum())} non-finite outputs"
    return out


def check_parity(backend, nseq, B, S, H, profile, spec, seed=0, kernels=KERNELS):
    """Both kernels on one case against fp64 under `err <= k * max(e_ref, floor(S))`; the figures are printed before anything is
    asserted.  -> {kernel: err / max(e_ref, floor)}."""
    qkv, lengths, valid, ref, e_ref = case_refs(seed, nseq, B, S, H, profile, spec)
    scale = max(e_ref, floor_of(S))
    assert scale > 0.0
    outs, ratios, failed = {}, {}, []
    for kernel in kernels:
        try:
            outs[kernel] = run_kernel(backend, kernel, qkv, lengths, nseq, B, S, H)
        except AssertionError as e:
            failed.append(str(e))
            continue
        err = maxabs(outs[kernel], ref)
        ratios[kernel] = err / scale
        print(f"[attention] {backend.name} kernel={kernel} family={family(S)} profile={profile} S={S} nseq={nseq} H={H} mask={spec} "
              f"err={err:.3e} e_ref={e_ref:.3e} floor={floor_of(S):.3e} ratio={ratios[kernel]:.3f} k={K_BOUND[(kernel, family(S))]}")
    assert not failed, failed
    for kernel in kernels:
        assert ratios[kernel] <= K_BOUND[(kernel, family(S))], (kernel, ratios[kernel])
    return ratios


def check_single_key(backend, nseq, B, S, H, spec, profile="flat", seed=0):
    """Cases with one valid key per sequence (count 0, an all-zero bitmap, S == 1): every output row is V[0] of its head."""
    qkv, lengths, valid, _, _ = case_refs(seed, nseq, B, S, H, profile, spec)
    assert (valid.sum(axis=1) == 1).all()
    D = H * HD
    v0 = qkv.reshape(nseq, S, 3 * D)[:, :1, 2 * D:]
    want = np.broadcast_to(v0, (nseq, S, D)).reshape(nseq * S, D)
    b_f32, b_x3 = count_zero_bounds(v0)
    out32 = run_kernel(backend, "f32", qkv, lengths, nseq, B, S, H)
    out3 = run_kernel(backend, "x3", qkv, lengths, nseq, B, S, H)
    print(f"[attention] {backend.name} single key S={S} mask={spec}: f32 max-abs vs V[0] = {maxabs(out32, want):.3e} (bound 0), "
          f"f16x3 = {maxabs(out3, want):.3e} (bound {b_x3:.3e})")
    assert np.array_equal(out32.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert maxabs(out3, want) <= b_x3


def check_ties(backend, nseq, B, S, H, spec, seed=0):
    """`ties` against the fp64 mean of the valid V rows, per output column under ties_bound."""
    qkv, lengths, valid, _, _ = case_refs(seed, nseq, B, S, H, "ties", spec)
    D = H * HD
    v = qkv.reshape(nseq, S, 3 * D)[:, :, 2 * D:]
    outs = {kernel: run_kernel(backend, kernel, qkv, lengths, nseq, B, S, H).reshape(nseq, S, D) for kernel in KERNELS}
    worst = {}
    for kernel in KERNELS:
        worst[kernel] = 0.0
        for s in range(nseq):
            rows = v[s, valid[s % B]]
            err = np.abs(outs[kernel][s].astype(np.float64) - rows.astype(np.float64).mean(axis=0)[None]).max(axis=0)
            worst[kernel] = max(worst[kernel], float((err / ties_bound(rows, kernel)).max()))
    print(f"[attention] {backend.name} ties S={S} mask={spec}: worst error / derived bound: " +
          ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))
    for kernel in KERNELS:
        assert worst[kernel] <= 1.0, (kernel, worst[kernel])
