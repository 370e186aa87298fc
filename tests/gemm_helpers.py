"""Checker of the GEMM kernels at kernel level -- mdm_linear (csrc/gemm_f32.h: exact fp32, 64x64 and 128x128 tiles), mdm_linear_x3
(csrc/gemm_x3.h: three fp16 MFMA products, 224-row x 256-column tiles, 32 k per step) -- of mdm_layernorm, and of the encoder's GEMM
routes (csrc/gemm_x3s.h row tiles, csrc/gemm_x3.h sequence tiles with the LayerNorms folded into their epilogues, the paired layer-0
launch) through one-layer models: input builders for six operand regimes, the fp64 and fp32 references, the bound, and the case runners
that tests/test_gpu_gemm_kernels.py / tests/test_gpu_encoder_routes.py (MI355X) and tests/test_emu_gemm_kernels.py /
tests/test_emu_encoder_routes.py (CPU wave emulator) share.  Nothing here is derived from the code under test.

The bound.  err = max-abs of a kernel's output against the fp64 reference; e_ref = max-abs of the torch fp32 reference of the same
expression against fp64 ON THE SAME CASE, computed when the test runs; floor = the smallest non-zero e_ref among the `flat` cases of
that (N, K) (for the cases whose fp32 reference happens to be exact or nearly so: `tiny`).  A parity assertion is

    err <= k * max(e_ref, floor)

with k per kernel from profiles/r11a_gemm_parity.md (K_BOUND).  `integer` has no tolerance: every product and partial sum is exact in
fp32 and in the split arithmetic, so the kernel must equal the fp64 result bit for bit.  `tiny` carries a second bound derived from the
fp16 plane format (tiny_bound).

The memory contracts, checked on every call: GUARD_ROWS rows of SENTINEL in front of and behind `out` (and around the rows of
mdm_layernorm) come back untouched, `out` starts as NaN and comes back finite, the scratch of mdm_linear_x3 starts as 0xFF bytes (a NaN
in every 16-bit plane: the pad rows of the fragment-ordered weight planes, N padded to 32, must be written before they are read, and
must not reach a column < N)."""
import math

import numpy as np
import torch

from helpers import memo

GUARD_ROWS = 16
SENTINEL = -7777.25

MDM_OK, MDM_EINVAL, MDM_EUNSUPPORTED = 0, -1, -5
ACT_NONE, ACT_GELU, ACT_SILU = 0, 1, 2

# k of `err <= k * max(e_ref, floor)`: profiles/r11a_gemm_parity.md.  Derived before anything was measured (see there): the fp32
# kernels differ from the reference in the association of the k-sum only -- 3, the factor tests/test_gpu_round2.py
# test_hostile_weights_forward_and_loop already allows fp32 against fp32; f16x3 carries ~2^-22 per product where fp32 carries 2^-24
# -- 6, the same test's factor for the split.  The measured worst ratios (emulator and MI355X) sit below both.
K_BOUND = {"f32": 3, "x3": 6, "layernorm": 3, "route_f32": 3, "route_x3": 6}

REGIMES = ("flat", "wide", "offset", "cancel", "tiny", "integer")
OFFSET_C = 100.0
TINY = 1.0e-6
CANCEL_EPS = 2.0e-3          # w[2j+1] = -w[2j] (1 - eps): the dot product is eps / 2 of sum |a w|


def maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def make_operands(M, N, K, regime, seed=0):
    """-> a [M, K], w [N, K], bias [N], res [M, N], fp32, deterministic in (seed, M, N, K, regime).  Every a stays inside the fp16 hi
    plane's range (65504) and every w below 255.9 (the weight planes hold w * 2^8 as fp16)."""
    assert regime in REGIMES and K % 2 == 0
    rng = np.random.default_rng([seed, M, N, K, REGIMES.index(regime)])
    a, w = rng.standard_normal((M, K)), rng.standard_normal((N, K)) / math.sqrt(K)
    b, r = rng.standard_normal(N), rng.standard_normal((M, N))
    if regime == "wide":
        # an exponent drawn per element from [-10, 10]: a dynamic range of 2^+-10 inside every 32-wide k block of both operands; three
        # rows of w ten times the rest (oracle/synth.py synth_state_dict_hostile); w as a whole 2^-7 down, so that 5 sigma of a tenfold
        # row at K = 32 (5 * 0.18 * 2^10 * 10 * 2^-7 = 71) stays in the weight planes' range
        a *= 2.0 ** rng.integers(-10, 11, (M, K))
        w *= 2.0 ** (rng.integers(-10, 11, (N, K)) - 7)
        w[rng.permutation(N)[:3]] *= 10.0
    elif regime == "offset":
        a += OFFSET_C                       # the hi plane carries the offset (fp16 spacing 2^-4 at 100), the lo plane the signal
    elif regime == "cancel":
        # pairs of equal a against w, -w (1 - eps) with one sign per pair common to a and w: every product of a pair is +|a w| then
        # -|a w| (1 - eps), so a row's dot product is eps / 2 = 1e-3 of sum |a w| while the operands themselves carry mixed signs
        s = np.where(rng.random(K // 2) < 0.5, -1.0, 1.0)
        a[:, 0::2] = np.abs(a[:, 0::2]) * s
        a[:, 1::2] = a[:, 0::2]
        w[:, 0::2] = np.abs(w[:, 0::2]) * s
        w[:, 1::2] = -w[:, 0::2] * (1.0 - CANCEL_EPS)
    elif regime == "tiny":
        a *= TINY                           # |a| < 6.1e-5: hi is fp16-subnormal and lo at most one subnormal step
        b *= TINY
        r *= TINY
    elif regime == "integer":
        a, w = rng.integers(-8, 9, (M, K)), rng.integers(-8, 9, (N, K))
        b, r = rng.integers(-8, 9, N), rng.integers(-8, 9, (M, N))
        assert K * 64 + 16 < 2 ** 24 // 256, "a * (w * 2^8) must stay exact in the fp32 accumulators"
    out = tuple(np.ascontiguousarray(t, dtype=np.float32) for t in (a, w, b, r))
    assert np.abs(out[0]).max() < 65504.0 and np.abs(out[1]).max() < 255.0
    return out


def _reference(a, w, b, r, act, dtype):
    a, w, b = (torch.from_numpy(t).to(dtype) for t in (a, w, b))
    v = a @ w.t() + b
    if act == ACT_GELU:
        v = torch.nn.functional.gelu(v)             # erf form
    elif act == ACT_SILU:
        v = torch.nn.functional.silu(v)
    if r is not None:
        v = v + torch.from_numpy(r).to(dtype)
    return v.numpy()


def linear_case(M, N, K, regime, act=ACT_NONE, res=False, seed=0):
    """(a, w, bias, res or None, fp64 reference, e_ref) of one case: built once per process, shared, never written to."""
    def build():
        a, w, b, r = make_operands(M, N, K, regime, seed)
        r = r if res else None
        ref = _reference(a, w, b, r, act, torch.float64)
        e_ref = maxabs(_reference(a, w, b, r, act, torch.float32), ref)
        for t in (a, w, b, ref) + (() if r is None else (r,)):
            t.setflags(write=False)
        return a, w, b, r, ref, e_ref
    return memo(("gemm_case", M, N, K, regime, act, res, seed), build)


def floor_of(N, K):
    """The smallest non-zero e_ref among the `flat` cases of this (N, K): M = 33 rows, no activation, without and with a residual."""
    def build():
        es = [linear_case(33, N, K, "flat", ACT_NONE, res)[5] for res in (False, True)]
        return min(e for e in es if e > 0.0)
    return memo(("gemm_floor", N, K), build)


def tiny_bound(w, ref):
    """`tiny` (|a| ~ 1e-6, far below fp16's smallest normal 6.1e-5): hi = rne16(a) lies on the subnormal grid of spacing 2^-24 and
    lo = rne16(a - hi) is 0 or one step, so hi + lo misses a by at most 2^-25 per element whatever the kernel does with lo: an output
    is off by at most 2^-25 sum_k |w[n, k]|, plus fp32 roundings of values of the output's size (2^-20 |out| covers K <= 1024 of them
    many times over).  A flushed hi plane would be off by max |a . w| ~ 4e-6, about twenty times this at K = 96."""
    return 2.0 ** -25 * float(np.abs(w.astype(np.float64)).sum(axis=1).max()) + 2.0 ** -20 * float(np.abs(ref).max())


# ---- the tile form mdm_linear takes, from the shape rule of csrc/gemm_f32.h launch_gemm_f32_t --------------------------------------
def f32_tile_form(M, N):
    """64: 64x64 tiles when the 128x128 tiling has fewer than 512 tiles and the output at least 16384 elements; 128 otherwise."""
    tiles128 = ((M + 127) // 128) * ((N + 127) // 128)
    return 64 if tiles128 < 512 and M * N >= 16384 else 128


# ---- backends -------------------------------------------------------------------------------------------------------------------------
class GpuBackend:
    """The product library on cuda:0."""
    name = "gpu"

    def __init__(self, lib, device="cuda:0"):
        self.lib, self.dev = lib, device

    def _dev(self, arr):
        if arr is None:
            return None
        return memo(("gemm_dev", id(arr)), lambda: (arr, torch.tensor(arr).to(self.dev)))[1]     # (keeps the host array alive)

    def linear(self, kernel, a, w, b, r, M, N, K, act):
        ad, wd, bd, rd = (self._dev(t) for t in (a, w, b, r))
        full = torch.full((M + 2 * GUARD_ROWS, N), float("nan"), device=self.dev)
        full[:GUARD_ROWS] = SENTINEL
        full[GUARD_ROWS + M:] = SENTINEL
        out_ptr = full.data_ptr() + GUARD_ROWS * N * 4
        stream = torch.cuda.current_stream().cuda_stream
        rp = rd.data_ptr() if rd is not None else None
        if kernel == "f32":
            rc = self.lib.mdm_linear(ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), rp, out_ptr, M, N, K, act, stream)
        else:
            nb = self.lib.mdm_linear_x3_scratch_bytes(M, N, K)
            scratch = torch.full((max(nb, 1),), 0xFF, dtype=torch.uint8, device=self.dev)
            rc = self.lib.mdm_linear_x3(ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), rp, out_ptr, M, N, K, act, scratch.data_ptr(),
                                        nb, stream)
        torch.cuda.synchronize()
        return rc, full.cpu().numpy()

    def layernorm(self, x_full, gamma, beta, rows, D):
        xd = torch.tensor(x_full).to(self.dev)
        gd, bd = torch.tensor(gamma).to(self.dev), torch.tensor(beta).to(self.dev)
        rc = self.lib.mdm_layernorm(xd.data_ptr() + GUARD_ROWS * D * 4, gd.data_ptr(), bd.data_ptr(), rows, D,
                                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, xd.cpu().numpy()


class EmuBackend:
    """The same entry points of the CPU wave emulator's library (tests/emu), on numpy buffers prepared the same way."""
    name = "emu"

    def __init__(self, lib):
        self.lib = lib

    def linear(self, kernel, a, w, b, r, M, N, K, act):
        full = np.full((M + 2 * GUARD_ROWS, N), np.nan, np.float32)
        full[:GUARD_ROWS] = SENTINEL
        full[GUARD_ROWS + M:] = SENTINEL
        out_ptr = full.ctypes.data + GUARD_ROWS * N * 4
        rp = r.ctypes.data if r is not None else None
        if kernel == "f32":
            rc = self.lib.mdm_linear(a.ctypes.data, w.ctypes.data, b.ctypes.data, rp, out_ptr, M, N, K, act, None)
        else:
            nb = self.lib.mdm_linear_x3_scratch_bytes(M, N, K)
            scratch = np.full(max(nb, 1), 0xFF, np.uint8)
            rc = self.lib.mdm_linear_x3(a.ctypes.data, w.ctypes.data, b.ctypes.data, rp, out_ptr, M, N, K, act, scratch.ctypes.data,
                                        nb, None)
        return rc, full

    def layernorm(self, x_full, gamma, beta, rows, D):
        x = np.array(x_full, np.float32)
        rc = self.lib.mdm_layernorm(x.ctypes.data + GUARD_ROWS * D * 4, gamma.ctypes.data, beta.ctypes.data, rows, D, None)
        return rc, x


def _guards_untouched(full, rows, what):
    for name, g in (("in front of", full[:GUARD_ROWS]), ("behind", full[GUARD_ROWS + rows:])):
        assert g.shape[0] == GUARD_ROWS and np.array_equal(g, np.full_like(g, SENTINEL)), f"{what}: wrote {name} its rows"


# ---- running a GEMM case --------------------------------------------------------------------------------------------------------------
def run_linear(backend, kernel, M, N, K, regime, act=ACT_NONE, res=False, seed=0):
    """One call with the memory contracts checked -> out [M, N]."""
    a, w, b, r, _, _ = linear_case(M, N, K, regime, act, res, seed)
    rc, full = backend.linear(kernel, a, w, b, r, M, N, K, act)
    what = f"{kernel} ({M}, {N}, {K}) {regime} act={act} res={res}"
    assert rc == MDM_OK, f"{what}: rc = {rc}"
    _guards_untouched(full, M, what)
    out = full[GUARD_ROWS:GUARD_ROWS + M]
    assert np.isfinite(out).all(), f"{what}: {int((~np.isfinite(out)).sum())} non-finite outputs"
    return out


def check_linear(backend, kernel, M, N, K, regime, act=ACT_NONE, res=False, seed=0):
    """One kernel on one case against fp64: bit for bit on `integer`, else `err <= k * max(e_ref, floor(N, K))` (and tiny_bound); the
    figures are printed before anything is asserted.  -> err / max(e_ref, floor)."""
    a, w, b, r, ref, e_ref = linear_case(M, N, K, regime, act, res, seed)
    out = run_linear(backend, kernel, M, N, K, regime, act, res, seed)
    err = maxabs(out, ref)
    form = f32_tile_form(M, N) if kernel == "f32" else 224
    head = f"[gemm] {backend.name} kernel={kernel} tile={form} regime={regime} M={M} N={N} K={K} act={act} res={int(res)}"
    if regime == "integer":
        assert act == ACT_NONE and e_ref == 0.0, "the integer regime is exact in fp32 by construction"
        bad = np.argwhere(out.astype(np.float64) != ref)
        print(f"{head} err={err:.3e} (bound 0) ratio=0 mismatches={len(bad)}" + (f" first at (m, n) = {tuple(bad[0])}" if len(bad) else ""))
        assert len(bad) == 0, f"{len(bad)} outputs differ from the exact result, first at (m, n) = {tuple(bad[0])}, max {err}"
        return 0.0
    scale = max(e_ref, floor_of(N, K))
    ratio = err / scale
    print(f"{head} err={err:.3e} e_ref={e_ref:.3e} floor={floor_of(N, K):.3e} ratio={ratio:.3f} k={K_BOUND[kernel]}")
    assert ratio <= K_BOUND[kernel], (kernel, ratio)
    if regime == "tiny" and act == ACT_NONE:
        tb = tiny_bound(w, ref)
        print(f"{head} tiny: err / plane-format bound = {err / tb:.3f}")
        assert err <= tb, (err, tb)
    return ratio


def check_linear_refused(backend, kernel, M, N, K, act, res, want_rc):
    """A call the ABI must refuse: the return code, and `out` (NaN) and its guards exactly as they were."""
    a, w, b, r, _, _ = linear_case(M, N, K, "flat", ACT_NONE, True)
    rc, full = backend.linear(kernel, a, w, b, r if res else None, M, N, K, act)
    print(f"[gemm] {backend.name} kernel={kernel} M={M} N={N} K={K} act={act} res={int(res)}: rc = {rc} (want {want_rc})")
    assert rc == want_rc, (rc, want_rc)
    _guards_untouched(full, M, "refused call")
    assert np.isnan(full[GUARD_ROWS:GUARD_ROWS + M]).all(), "a refused call wrote to out"


# ---- mdm_layernorm --------------------------------------------------------------------------------------------------------------------
LN_REGIMES = ("normal", "mean1e3", "constant", "outlier")


def layernorm_case(rows, D, regime, seed=0):
    """(x, gamma, beta, fp64 reference, e_ref).  normal: N(0.5, 3) (tests/test_gpu_parity.py test_mdm_layernorm); mean1e3: mean 1000,
    std 1 (E[x^2] - mean^2 in fp32 would lose every digit of the variance); constant: each row one dyadic constant whose partial sums
    are all exact in fp32, so the variance is exactly 0 and the output exactly beta; outlier: one channel 300 times the rest."""
    def build():
        assert regime in LN_REGIMES
        rng = np.random.default_rng([seed, rows, D, LN_REGIMES.index(regime)])
        x = rng.standard_normal((rows, D))
        if regime == "normal":
            x = 3.0 * x + 0.5
        elif regime == "mean1e3":
            x = x + 1000.0
        elif regime == "constant":
            x = np.broadcast_to(((np.arange(rows) % 13) - 6.0)[:, None] * 0.25, (rows, D))      # multiples of 1/4, |c| <= 1.5
        elif regime == "outlier":
            x[:, int(rng.integers(D))] *= 300.0
        x = np.ascontiguousarray(x, dtype=np.float32)
        gamma = np.ascontiguousarray(rng.standard_normal(D), dtype=np.float32)
        beta = np.ascontiguousarray(rng.standard_normal(D), dtype=np.float32)
        f = torch.nn.functional.layer_norm
        ref = f(torch.from_numpy(x).double(), (D,), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), 1e-5).numpy()
        e_ref = maxabs(f(torch.from_numpy(x), (D,), torch.from_numpy(gamma), torch.from_numpy(beta), 1e-5).numpy(), ref)
        for t in (x, gamma, beta, ref):
            t.setflags(write=False)
        return x, gamma, beta, ref, e_ref
    return memo(("ln_case", rows, D, regime, seed), build)


def ln_floor_of(D):
    """The smallest non-zero e_ref among the `normal` cases of this D (1 and 64 rows)."""
    return memo(("ln_floor", D), lambda: min(e for e in (layernorm_case(n, D, "normal")[4] for n in (1, 64)) if e > 0.0))


def check_layernorm(backend, rows, D, regime):
    x, gamma, beta, ref, e_ref = layernorm_case(rows, D, regime)
    x_full = np.full((rows + 2 * GUARD_ROWS, D), SENTINEL, np.float32)
    x_full[GUARD_ROWS:GUARD_ROWS + rows] = x
    rc, full = backend.layernorm(x_full, gamma, beta, rows, D)
    what = f"layernorm rows={rows} D={D} {regime}"
    assert rc == MDM_OK, f"{what}: rc = {rc}"
    _guards_untouched(full, rows, what)
    out = full[GUARD_ROWS:GUARD_ROWS + rows]
    assert np.isfinite(out).all(), what
    err = maxabs(out, ref)
    if regime == "constant":
        print(f"[gemm] {backend.name} kernel=layernorm regime=constant rows={rows} D={D} err={err:.3e} (bound 0: exactly beta) ratio=0")
        assert np.array_equal(ref, np.broadcast_to(beta.astype(np.float64), ref.shape))
        assert np.array_equal(out.view(np.uint32), np.ascontiguousarray(np.broadcast_to(beta, out.shape)).view(np.uint32))
        return 0.0
    scale = max(e_ref, ln_floor_of(D))
    ratio = err / scale
    print(f"[gemm] {backend.name} kernel=layernorm regime={regime} rows={rows} D={D} err={err:.3e} e_ref={e_ref:.3e} "
          f"floor={ln_floor_of(D):.3e} ratio={ratio:.3f} k={K_BOUND['layernorm']}")
    assert ratio <= K_BOUND["layernorm"], ratio
    return ratio


# ---- encoder routes on one-layer models -----------------------------------------------------------------------------------------------
# name -> (precision, engine options).  small / small64: csrc/gemm_x3s.h on 32- / 64-row tiles; seq: csrc/gemm_x3.h sequence tiles
# (pipelined; above 224 tokens its plain row tiles); seq_shared1 / seq_shared0: the same under guidance with and without the paired
# layer-0 in_proj; f32: the exact-fp32 mode's one route.
ROUTES = {"small": ("f16x3", {}),
          "small64": ("f16x3", {"small_gemm_row_tiles": 2}),
          "seq": ("f16x3", {"small_gemm_max_seqs": 0}),
          "seq_shared1": ("f16x3", {"small_gemm_max_seqs": 0, "enc_shared_layer0": 1}),
          "seq_shared0": ("f16x3", {"small_gemm_max_seqs": 0, "enc_shared_layer0": 0}),
          "f32": ("f32", {})}
ROUTE_TS = (1, 31, 32, 63, 64, 65, 206, 207, 223, 230)      # S = T + 1 tokens: the 32- / 64-row tile edges, the paired launch's last
                                                            # length (S = 207) and first refusal, the last length on sequence tiles
                                                            # (S = 224) and the first on row tiles


def route_guided(route):
    return route.startswith("seq_shared")


def route_model_case(weights, D, ff, B, T, lengths, guided, seed=0):
    """(sd, x, t, y, fp64 oracle output, e_ref of the fp32 oracle) of one forward of a one-layer model."""
    def build():
        from helpers import orc
        from oracle.synth import synth_state_dict, synth_state_dict_hostile, synth_y, synth_y_hostile
        hostile = weights == "hostile"
        sd = memo(("route_sd", weights, D, ff), lambda: (synth_state_dict_hostile if hostile else synth_state_dict)(
            seed=0, latent_dim=D, ff_size=ff, num_layers=1))
        y = (synth_y_hostile if hostile else synth_y)(B, T, seed=seed + 2, lengths=list(lengths) if lengths else None)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, 263, 1, T, generator=g)
        t = torch.tensor([49, 0, 13][:B])
        fwd = orc.cfg_forward if guided else orc.mdm_forward
        H = D // 128
        ref = fwd(sd, x, t, y, num_heads=H, dtype=torch.float64)
        e_ref = maxabs(fwd(sd, x, t, y, num_heads=H), ref)
        return sd, x, t, y, ref, e_ref
    return memo(("route_case", weights, D, ff, B, T, tuple(lengths) if lengths else None, guided, seed), build)


def route_floor_of(D, ff):
    """The smallest non-zero e_ref among the plain-weight, unguided B = 1 cases of this width at T = 31 and 64."""
    return memo(("route_floor", D, ff), lambda: min(e for e in (route_model_case("plain", D, ff, 1, T, None, False)[5]
                                                               for T in (31, 64)) if e > 0.0))


def _route_model(sd, D, ff, device, guided, native_lib, prec):
    """tests/helpers.py make_pair with a feed-forward width of its own (the reference pins 1024; the narrow model here has 256)."""
    from mdm_amd import model_util
    from mdm_amd.cfg_sampler import ClassifierFreeSampleModel
    over = {"pos_embed_max_len": 512} if native_lib is not None else {}       # (the emulator's short positional table, as make_pair)
    args = model_util.default_args(diffusion_steps=50, layers=1, latent_dim=D, **over)
    model, _ = model_util.create_model_and_diffusion(args, _native_lib=native_lib, num_heads=D // 128, precision=prec, ff_size=ff)
    model_util.load_model_wo_clip(model, sd)
    if guided:
        model = ClassifierFreeSampleModel(model)
    model.to(device)
    model.eval()
    return model


def check_route(engine_options, route, device, native_lib, weights, D, ff, B, T, lengths=None, guided=None):
    """One forward of a one-layer model on one route against the fp64 oracle under `err <= k * max(e_ref, floor)`; -> the ratio."""
    from helpers import to_dev
    prec, opts = ROUTES[route]
    guided = route_guided(route) if guided is None else guided
    sd, x, t, y, ref, e_ref = route_model_case(weights, D, ff, B, T, lengths, guided)
    engine_options(**opts)
    # one model (and so one engine: mdm_amd/mdm.py keys it by the options) per route, weight set and width, whatever the shape
    model = memo(("route_model", route, weights, D, ff, guided, str(device), native_lib is not None),
                 lambda: _route_model(sd, D, ff, device, guided, native_lib, prec))
    out = model(x.to(device), t.to(device), y=to_dev(dict(y), device))
    eng = model.model.engine() if guided else model.engine()
    for k, v in opts.items():
        assert eng.get_option(k) == v, (k, v)
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    err = maxabs(out.cpu(), ref)
    kind = "route_f32" if prec == "f32" else "route_x3"
    scale = max(e_ref, route_floor_of(D, ff))
    ratio = err / scale
    where = "emu" if native_lib is not None else "gpu"
    print(f"[gemm] {where} kernel=route:{route} weights={weights} D={D} ff={ff} B={B} T={T} lengths={lengths} guided={int(guided)} "
          f"err={err:.3e} e_ref={e_ref:.3e} floor={route_floor_of(D, ff):.3e} ratio={ratio:.3f} k={K_BOUND[kind]}")
    assert ratio <= K_BOUND[kind], (route, ratio)
    return ratio
