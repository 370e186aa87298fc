"""Checker of the trans_dec (DiP) decoder's routes -- csrc/decoder.h decoder_layers_planes / decoder_pass and the window loop of
csrc/loops.h -- through ONE-layer models against the fp64 oracle (oracle/dip_oracle.py with dtype=float64): the case builder, the
bound, the rule that says which kernel form a call must take, the launch-count table that proves it did, and the runners that
tests/test_gpu_decoder_routes.py (MI355X) and tests/test_emu_decoder_routes.py (CPU wave emulator) share.  Modelled on the encoder's
route checker (tests/gemm_helpers.py check_route); maxabs, memo and K_BOUND are that file's.  Nothing here is derived from the code
under test.

The bound.  err = max-abs of the product's output against the fp64 oracle; e_ref = max-abs of the fp32 oracle against the fp64 one
ON THE SAME CASE; floor(D, ff, guided) = the smallest non-zero e_ref among the plain-weight B = 1 cases of that width and guidance
mode at the windows 20 + 40 and 0 + 64 with a 24-token prompt.  A parity assertion is

    err <= k * max(e_ref, floor)

with k = K_BOUND["route_x3"] = 6 for every f16x3 route (the fp32-skeleton route runs f16x3 arithmetic in its GEMMs) and
K_BOUND["route_f32"] = 3 for the `f32` precision (profiles/r11a_gemm_parity.md).  The floor is per guidance mode because the guided
output is ou + 7.5 (oc - ou): its fp32 error is about ten times the unguided one, and it is needed because a one-key softmax is exact
(the one-token memory, the one-frame window: e_ref about five times below ordinary windows).

Which form ran.  The decoder falls from one kernel form to another without a word, so a case table can believe it covers a form that
never ran.  expected_form restates the documented rule (include/mdm_hip.h: MDM_OPT_SMALL_GEMM_MAX_SEQS, MDM_OPT_DEC_FUSED_XATTN,
MDM_OPT_DEC_FUSED_SELFATTN) as a pure function of (D, S, ntok, nseq, precision, options); FORM_LAUNCHES says how many launches per
profiler class (include/mdm_hip.h MDM_PROF_*) a ONE-LAYER stand-alone forward of each form makes; every check runs one profiled
forward (Engine.profile) and compares the counters with the table, then runs the parity forward with profiling off.  A window loop
is proved on its own as well: one profiled call of the loop against loop_launches (steps x the per-step launches + the hoisted ones).

Forms with equal counts (so a test must not rely on the counters to tell them apart -- the option that decides is pinned by the
route and read back from the engine):
  * (self-attention block, three-launch cross-attention) and (two-launch self-attention, (sequence, head) cross-attention): 7 GEMM-
    class launches and 1 attention launch each.  The first needs dec_fused_selfattn = 1, the second 0: never both in one route.
  * unguided, with the three-launch cross-attention: row tiles and sequence tiles (the sequence tiles know no other cross-attention
    form).  The `seqtiles` route therefore leaves dec_fused_xattn at its default, under which row tiles at 129 .. 224 tokens take the
    one-kernel block (latent_dim 256 / 512, <= 96 memory tokens) -- one GEMM-class launch and one attention launch fewer -- and it is
    run at those widths and memories only.  Under guidance the sequence tiles add four launches of their own (see FORM_LAUNCHES)."""

import torch

from gemm_helpers import K_BOUND, maxabs
from helpers import memo

# name -> (precision, engine options)
ROUTES = {"planes32": ("f16x3", {"small_gemm_row_tiles": 1}),
          "planes64": ("f16x3", {"small_gemm_row_tiles": 2}),
          "x2": ("f16x3", {"dec_fused_xattn": 2}),
          "x1": ("f16x3", {"dec_fused_xattn": 1}),
          "x0": ("f16x3", {"dec_fused_xattn": 0}),
          "sa0": ("f16x3", {"dec_fused_selfattn": 0}),
          "x0sa0": ("f16x3", {"dec_fused_xattn": 0, "dec_fused_selfattn": 0}),
          "seqtiles": ("f16x3", {"small_gemm_max_seqs": 1}),       # B >= 2 (or B = 1 under guidance) exceeds it
          "skeleton": ("f16x3", {"small_gemm_max_seqs": 0}),
          "f32": ("f32", {}),
          "bysize": ("f16x3", {})}                                 # the library's defaults: dec_fused_xattn = 3
OPTION_DEFAULTS = {"small_gemm_max_seqs": 80, "small_gemm_row_tiles": 0, "dec_fused_xattn": 3, "dec_fused_selfattn": 1}
WINDOW_S = (1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 224, 225)       # S = C + P
MEMORY_NTOK = (1, 31, 32, 33, 64, 65, 96, 97, 230)


# ---- which form a call takes: include/mdm_hip.h ---------------------------------------------------------------------------------------
def expected_form(D, S, ntok, nseq, prec, opts):
    """-> (self-attention form, cross-attention form, GEMM tiling) of a trans_dec call; S counts the context rows (the class token of
    MDM_OPT_DEC_TIME_TOKEN is one), nseq = B, or 2B under guidance.
      tiling   `skeleton`: the f32 precision, and MDM_OPT_SMALL_GEMM_MAX_SEQS = 0 (fp32 activations in memory, in_proj + attention,
               q projection + attention + out_proj); `seq`: more sequences than MDM_OPT_SMALL_GEMM_MAX_SEQS, each of 129 .. 224
               tokens (in_proj + attention, the three-launch cross-attention: the fused forms belong to the row tiles); else `row`
      self     `block` (MDM_OPT_DEC_FUSED_SELFATTN = 1 and at most 64 tokens), else `two` launches
      cross    MDM_OPT_DEC_FUSED_XATTN: 3 = 2 below 144 32-row tiles, 1 from there on; 2 = `seqhead` (windows and memories of at
               most 64 tokens); 1 = `one` kernel (latent_dim 256 / 512, at most 96 memory tokens); an explicit or by-size 1 / 2 whose
               shapes are not covered takes the other fused form if that applies, else -- and with 0 -- `three` launches."""
    o = {**OPTION_DEFAULTS, **opts}
    if prec == "f32" or o["small_gemm_max_seqs"] == 0:
        return ("two", "three", "skeleton")
    if nseq > o["small_gemm_max_seqs"] and 129 <= S <= 224:
        return ("two", "three", "seq")
    sa = "block" if o["dec_fused_selfattn"] == 1 and S <= 64 else "two"
    can_seqhead = S <= 64 and ntok <= 64
    can_one = D in (256, 512) and ntok <= 96
    mode = o["dec_fused_xattn"]
    if mode == 3:
        mode = 1 if nseq * ((S + 31) // 32) >= 144 else 2
    if mode == 2:
        xa = "seqhead" if can_seqhead else ("one" if can_one else "three")
    elif mode == 1:
        xa = "one" if can_one else ("seqhead" if can_seqhead else "three")
    else:
        xa = "three"
    return (sa, xa, "row")


# Launches of a one-layer stand-alone forward, per profiler class (linear, attention, layernorm, elementwise); embed and outproj are 1
# in every form.  Common to all forms: the text memory (1 elementwise; the class token of MDM_OPT_DEC_TIME_TOKEN adds 1), the memory's
# key | value projection (1 linear), linear1 and linear2 (2 linear).
#   self-attention   block: the block + out_proj (2 linear);             two: in_proj + out_proj (2 linear) and 1 attention
#   cross-attention  seqhead: the (sequence, head) kernel + out_proj (2 linear);   one: 1 linear;
#                    three: q projection + out_proj (2 linear) and 1 attention
#   skeleton         in_proj, out_proj, q, k | v, out_proj, linear1, linear2 (7 linear), 2 attention, and the one LayerNorm kernel the
#                    stack runs (the last norm3, in front of OutputProcess); the plane routes fold it (0 layernorm)
#   seq, guided      layer 0's self-attention block runs on the conditional half and is copied (share0: 1 elementwise); the
#                    unconditional half's cross-attention is a row constant (skip_uncond: the value rows gathered and written,
#                    2 elementwise, through one small out_proj GEMM, 1 linear)
_SA = {"block": (2, 0), "two": (2, 1)}
_XA = {"seqhead": (2, 0), "one": (1, 0), "three": (2, 1)}


def form_launches(form, guided, class_token):
    sa, xa, tiling = form
    ew = 1 + int(class_token)
    if tiling == "skeleton":
        return {"linear": 7, "attention": 2, "layernorm": 1, "elementwise": ew, "embed": 1, "outproj": 1}
    lin = 1 + 2 + _SA[sa][0] + _XA[xa][0]
    att = _SA[sa][1] + _XA[xa][1]
    if tiling == "seq" and guided:
        lin, ew = lin + 1, ew + 3
    return {"linear": lin, "attention": att, "layernorm": 0, "elementwise": ew, "embed": 1, "outproj": 1}


def loop_launches(form, guided, nsteps):
    """Launches of one window loop (mdm_sample_loop_dec) of `nsteps` steps on a one-layer model without the class token.
      once per window  the text memory and the gather of the steps' time-embedding rows (2 elementwise; one gather covers 64 steps);
                       the memory's key | value projection split in its text part and its per-step rows (kv_text, kv_time: 2 linear);
                       on sequence tiles under guidance the unconditional half's row constants in their two parts (o_text, o_time:
                       2 linear)
      per step         the stand-alone forward's launches without the text memory (1 elementwise) and the memory's key | value
                       projection (1 linear); on sequence tiles under guidance also without skip_uncond's gather and its small
                       out_proj GEMM (1 elementwise, 1 linear: hoisted); the sampler update rides in the tail of OutputProcess on
                       the plane routes (DecTail: no launch) and is a kernel of its own behind the fp32 skeleton (1 elementwise)
    A loop that left its route -- the planes for the skeleton (one LayerNorm launch a step), the hoisted row constants for the
    per-step ones -- shows in these counts where a stand-alone forward on the same engine would not."""
    assert 1 <= nsteps <= 64
    tiling = form[2]
    per = form_launches(form, guided, False)
    hoisted_o = tiling == "seq" and guided
    per["linear"] -= 1 + int(hoisted_o)
    per["elementwise"] -= 1 + int(hoisted_o)
    per["elementwise"] += int(tiling == "skeleton")
    got = {k: nsteps * v for k, v in per.items()}
    got["linear"] += 2 + 2 * int(hoisted_o)
    got["elementwise"] += 2
    return got


FORM_LAUNCHES = {(f, g): form_launches(f, g, False)
                 for f in [(sa, xa, "row") for sa in _SA for xa in _XA] + [("two", "three", "seq"), ("two", "three", "skeleton")]
                 for g in (False, True)}


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def _sd(weights, D, ff, variant):
    from oracle.synth import synth_dip_state_dict, synth_dip_state_dict_hostile
    build = synth_dip_state_dict_hostile if weights == "hostile" else synth_dip_state_dict
    return memo(("dec_sd", weights, D, ff, variant),
                lambda: build(seed=0, latent_dim=D, ff_size=ff, num_layers=1, bert_dim=512 if variant == "clip" else 768))


def _y(weights, B, C, P, text_lengths, lengths, holes, variant, seed):
    from oracle.synth import synth_dip_y, synth_dip_y_hostile
    hostile = weights == "hostile"
    y = (synth_dip_y_hostile if hostile else synth_dip_y)(B, P, max(C, 1), seed=seed + 2, text_lengths=list(text_lengths),
                                                          lengths=list(lengths) if lengths else None)
    if C == 0:
        y.pop("prefix")
    else:
        y["prefix"] = y["prefix"][..., :C].contiguous()
    if variant == "clip":       # ONE memory token per sample, no memory pad mask (model/mdm.py:261-262)
        g = torch.Generator().manual_seed(seed + 3)
        y["text_embed"] = torch.randn(1, B, 512, generator=g) * (20.0 if hostile else 1.0)
    if holes:                   # the bitmap form of `lengths`: interior frames and frame 0 of the last sample
        assert P >= 6 and C + P <= 256
        n = int(lengths[B - 1]) if lengths else P
        y["mask"] = y["mask"].clone()
        y["mask"][B - 1, 0, 0, sorted({0, n // 3, n // 2})] = False
    return y


def _kw(D, C, variant, dtype):
    return dict(context_len=C, num_heads=D // 128, mask_frames=True, dtype=dtype, emb_trans_dec=variant == "class_token")


def _timesteps(B):
    return torch.tensor([(49, 0, 13)[b % 3] for b in range(B)])


def case(weights, D, ff, B, C, P, text_lengths, lengths, holes, guided, variant, seed=0):
    """(sd, x, t, y, fp64 reference, e_ref) of one forward of a one-layer decoder: built once per process, shared, never written to.
    variant: `bert` (token memory with a pad mask), `clip` (one memory token), `class_token` (emb_trans_dec; C must be 0)."""
    assert variant in ("bert", "clip", "class_token") and (variant != "class_token" or C == 0)

    def build():
        from helpers import dip
        sd = _sd(weights, D, ff, variant)
        y = _y(weights, B, C, P, text_lengths, lengths, holes, variant, seed)
        x = torch.randn(B, 263, 1, P, generator=torch.Generator().manual_seed(seed))
        t = _timesteps(B)
        fwd = dip.dip_cfg_forward if guided else dip.dip_forward
        ref = fwd(sd, x, t, y, **_kw(D, C, variant, torch.float64))
        e_ref = maxabs(fwd(sd, x, t, y, **_kw(D, C, variant, torch.float32)), ref)
        return sd, x, t, y, ref, e_ref
    return memo(("dec_case", weights, D, ff, B, C, P, tuple(text_lengths), tuple(lengths) if lengths else None, bool(holes),
                 bool(guided), variant, seed), build)


def loop_case(weights, D, ff, B, C, P, text_lengths, lengths, guided, variant, steps, inpaint=False, skip=0, seed=0):
    """(sd, y, noise sequence, fp64 reference, e_ref) of one window loop (p_sample_loop with an injected noise sequence) over a
    `steps`-step cosine schedule.  inpaint: an inpainting mask over the first four features and the first quarter of the frames, and
    clip_denoised=True (the blend and the clamp of gaussian_diffusion.py:300-304, :347-353 ahead of the posterior step).  skip:
    skip_timesteps (:693-700) -- the loop starts from q_sample(0, t = steps - 1 - skip, x_T) and runs steps - skip steps.  Without
    either the reference is oracle/dip_oracle.py dip_sample_loop; with one, the same loop composed from the oracle's own pieces
    (oracle/mdm_oracle.py q_sample, predict_x0, ddpm_step around dip_forward / dip_cfg_forward)."""
    def build():
        from helpers import dip, orc
        sd = _sd(weights, D, ff, variant)
        y = _y(weights, B, C, P, text_lengths, lengths, False, variant, seed)
        g = torch.Generator().manual_seed(seed + 8)
        shape = (B, 263, 1, P)
        seq = [torch.randn(*shape, generator=g) for _ in range(1 + steps)]
        if inpaint:
            m = torch.zeros(shape, dtype=torch.bool)
            m[:, :4] = True
            m[..., : max(P // 4, 1)] = True
            y["inpainting_mask"] = m
            y["inpainted_motion"] = torch.randn(*shape, generator=g)
        tab = orc.Tables(orc.named_betas("cosine", steps))

        def run(dtype):
            kw = _kw(D, C, variant, dtype)
            if not inpaint and not skip:
                return dip.dip_sample_loop(sd, tab, shape, y, seq[0], seq[1:], cfg=guided, **kw)
            pe = orc.positional_table(5000, D, dtype)
            fwd = dip.dip_cfg_forward if guided else dip.dip_forward
            img = seq[0].to(dtype)
            if skip:
                img = orc.q_sample(tab, torch.zeros_like(img), torch.full((B,), steps - 1 - skip, dtype=torch.long), img)
            for k, i in enumerate(range(steps - skip)[::-1]):
                t = torch.full((B,), i, dtype=torch.long)
                x0 = orc.predict_x0(lambda xx, tt, yy: fwd(sd, xx, tt, yy, pe=pe, **kw), img, t, y, clip_denoised=bool(inpaint))
                img = orc.ddpm_step(tab, img, x0, t, seq[1 + k].to(dtype))
            return img
        ref = run(torch.float64)
        return sd, y, seq, ref, maxabs(run(torch.float32), ref)
    return memo(("dec_loop", weights, D, ff, B, C, P, tuple(text_lengths), tuple(lengths) if lengths else None, bool(guided), variant,
                 steps, bool(inpaint), skip, seed), build)


def floor_of(D, ff, guided):
    """The smallest non-zero e_ref among the plain-weight B = 1 cases of this width and guidance mode: windows 20 + 40 and 0 + 64, a
    24-token prompt."""
    return memo(("dec_floor", D, ff, bool(guided)),
                lambda: min(e for e in (case("plain", D, ff, 1, C, P, (24,), None, False, guided, "bert")[5]
                                        for C, P in ((20, 40), (0, 64))) if e > 0.0))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _model(sd, D, ff, C, variant, steps, device, native_lib, prec):
    """tests/helpers.py make_pair for the decoder, with a feed-forward width of its own (as tests/gemm_helpers.py _route_model)."""
    from mdm_amd import model_util
    over = {"pos_embed_max_len": 512} if native_lib is not None else {}       # (the emulator's short positional table, as make_pair)
    args = model_util.default_args(diffusion_steps=steps, layers=1, latent_dim=D, arch="trans_dec", mask_frames=True,
                                   text_encoder_type="clip" if variant == "clip" else "bert",
                                   emb_trans_dec=variant == "class_token", context_len=C, pred_len=0, **over)
    model, diffusion = model_util.create_model_and_diffusion(args, _native_lib=native_lib, num_heads=D // 128, precision=prec,
                                                             ff_size=ff)
    model_util.load_model_wo_clip(model, sd)
    model.to(device)
    model.eval()
    return model, diffusion


def _pair(engine_options, route, device, native_lib, weights, D, ff, C, variant, guided, steps=50):
    """(callable model, diffusion, engine) of one route: ONE engine per (route, weights, width, C, variant, steps), whatever the
    shape and the guidance mode (mdm_amd/mdm.py keys the engine by the options in force, so they are set on every call)."""
    from mdm_amd.cfg_sampler import ClassifierFreeSampleModel
    prec, opts = ROUTES[route]
    engine_options(**opts)
    sd = _sd(weights, D, ff, variant)
    model, diffusion = memo(("dec_model", route, weights, D, ff, C, variant, steps, str(device), native_lib is not None),
                            lambda: _model(sd, D, ff, C, variant, steps, device, native_lib, prec))
    eng = model.engine()
    for k, v in opts.items():
        assert eng.get_option(k) == v, (k, v)
    assert eng.weights_in_range, "the model left the weight planes' range (mdm_weights_in_range)"
    return (ClassifierFreeSampleModel(model) if guided else model), diffusion, eng


def _launches(eng, call):
    """The engine's launch counters per profiler class over one call."""
    eng.profile(True)
    try:
        call()
        return {k: v["launches"] for k, v in eng.profile_read().items()}
    finally:
        eng.profile(False)


def _form_checked(eng, forward, route, D, S, ntok, nseq, guided, variant, want):
    """One profiled forward: the launch counters must be those of the form expected_form names; `want` (a part of the form a test
    states on its own, e.g. {"xattn": "seqhead"}) must agree with the rule too.  -> the form."""
    prec, opts = ROUTES[route]
    form = expected_form(D, S, ntok, nseq, prec, opts)
    named = dict(zip(("selfattn", "xattn", "tiling"), form))
    for k, v in (want or {}).items():
        assert named[k] == v, f"the case table expects {k} = {v} where the rule of include/mdm_hip.h names {named[k]}"
    expect = form_launches(form, guided, variant == "class_token")
    got = _launches(eng, forward)
    assert got == expect, f"route {route}: expected the form {form} ({expect}), the launch counters say {got}"
    return form


def _report(where, route, form, what, err, e_ref, floor, k):
    ratio = err / max(e_ref, floor)
    print(f"[decoder] {where} route={route} form={'/'.join(form)} {what} err={err:.3e} e_ref={e_ref:.3e} floor={floor:.3e} "
          f"ratio={ratio:.3f} k={k}")
    return ratio


def check_route(engine_options, route, device, native_lib, weights, D, ff, B, C, P, text_lengths, lengths=None, holes=False,
                guided=False, variant="bert", want=None):
    """One forward of a one-layer decoder on one route: the form by the launch counters, then parity against the fp64 oracle under
    `err <= k * max(e_ref, floor)`.  -> (ratio, form)."""
    from helpers import to_dev
    sd, x, t, y, ref, e_ref = case(weights, D, ff, B, C, P, text_lengths, lengths, holes, guided, variant)
    model, _, eng = _pair(engine_options, route, device, native_lib, weights, D, ff, C, variant, guided)
    xd, td, yd = x.to(device), t.to(device), to_dev(dict(y), device)
    S = P + (1 if variant == "class_token" else C)
    ntok = 1 if variant == "clip" else int(max(text_lengths))
    form = _form_checked(eng, lambda: model(xd, td, y=dict(yd)), route, D, S, ntok, B * (2 if guided else 1), guided, variant, want)
    out = model(xd, td, y=dict(yd))
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    k = K_BOUND["route_f32" if ROUTES[route][0] == "f32" else "route_x3"]
    ratio = _report("emu" if native_lib is not None else "gpu", route, form,
                    f"weights={weights} variant={variant} D={D} ff={ff} B={B} C={C} P={P} ntok={list(text_lengths)} lengths={lengths} "
                    f"holes={int(holes)} guided={int(guided)}", maxabs(out.cpu(), ref), e_ref, floor_of(D, ff, guided), k)
    assert ratio <= k, (route, form, ratio)
    return ratio, form


def check_loop(engine_options, route, device, native_lib, weights, D, ff, B, C, P, text_lengths, lengths=None, guided=False,
               variant="bert", steps=2, inpaint=False, skip=0, want=None):
    """One window loop (mdm_sample_loop_dec through diffusion.p_sample_loop with an injected noise sequence) on one route against the
    fp64 oracle's loop, under the same bound.  The form is proved twice: by the counters of a stand-alone forward of the same shapes
    on the same engine, and by the counters of one profiled call of the loop itself against loop_launches -- the hoisted path has a
    launch pattern and route conditions of its own.  The parity loop then runs with profiling off."""
    from helpers import to_dev
    sd, y, seq, ref, e_ref = loop_case(weights, D, ff, B, C, P, text_lengths, lengths, guided, variant, steps, inpaint, skip)
    model, diffusion, eng = _pair(engine_options, route, device, native_lib, weights, D, ff, C, variant, guided, steps=steps)
    yd = to_dev(dict(y), device)
    S = P + (1 if variant == "class_token" else C)
    ntok = 1 if variant == "clip" else int(max(text_lengths))
    x0, t0 = seq[0].to(device), torch.zeros(B, dtype=torch.long, device=device)
    form = _form_checked(eng, lambda: model(x0, t0, y=dict(yd)), route, D, S, ntok, B * (2 if guided else 1), guided, variant, want)
    assert variant != "class_token"

    def loop():
        return diffusion.p_sample_loop(model, (B, 263, 1, P), clip_denoised=bool(inpaint), model_kwargs={"y": dict(yd)},
                                       skip_timesteps=skip, noise_sequence=[s.to(device) for s in seq])
    got, expect = _launches(eng, loop), loop_launches(form, guided, steps - skip)
    assert got == expect, f"route {route}: a {steps - skip}-step loop on the form {form} makes {expect}, the launch counters say {got}"
    out = loop()
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    k = K_BOUND["route_f32" if ROUTES[route][0] == "f32" else "route_x3"]
    ratio = _report("emu" if native_lib is not None else "gpu", route, form,
                    f"loop steps={steps - skip} of {steps} inpaint={int(inpaint)} weights={weights} variant={variant} D={D} ff={ff} B={B} C={C} P={P} "
                    f"ntok={list(text_lengths)} lengths={lengths} guided={int(guided)}", maxabs(out.cpu(), ref), e_ref,
                    floor_of(D, ff, guided), k)
    assert ratio <= k, (route, form, ratio)
    return ratio, form


def ragged_text(B, ntok):
    """B prompt lengths that include a full one and a one-token one."""
    return [ntok, 1, max(1, ntok // 2)][:B] if B <= 3 else [ntok, 1] + [1 + (7 * b) % ntok for b in range(2, B)]
