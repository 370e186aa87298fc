"""The trans_dec (DiP) decoder's routes on the MI355X through ONE-layer models against the fp64 oracle: the (sequence, head) kernel of
csrc/selfattn_block.h in its three modes, the one-kernel cross-attention block of csrc/xattn_block.h, the fall-back order between them
and the three-launch form, the by-size default, the row-tile and sequence-tile GEMM kinds the decoder uses, share0 / skip_uncond under
guidance, the fp32 skeleton, the f32 precision, the class-token and one-token-memory variants, and the hoisted window loop with its
fused sampler tail.  One layer deep the fp32 oracle's own error against fp64 (e_ref) is about 1.5e-6, so under

    err <= k * max(e_ref, floor)                  (tests/decoder_helpers.py; k: profiles/r11a_gemm_parity.md)

a wrong folded-LayerNorm term, a wrong kadd / vadd row or an off-by-one in a mask cannot hide the way it can behind the 2e-5 ... 2e-4
of the eight-layer tests.  Every case first proves, by the engine's launch counters, that the form it means to cover is the form that
ran (decoder_helpers.expected_form / form_launches), and prints `[decoder] gpu route=... form=... ratio=...` before it asserts.
latent_dim 512 / ff 1024 and B = 3 with ragged prompts (a full one, a one-token one) unless said otherwise."""
import pytest
import torch

import decoder_helpers as dh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, FF, B = 512, 1024, 3
TEN = [r for r in dh.ROUTES if r != "bysize"]
TEXT = dh.ragged_text(B, 24)


def _fwd(engine_options, route, weights, C, P, text=None, width=(D, FF), batch=B, **kw):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    text = dh.ragged_text(batch, 24) if text is None else text
    return dh.check_route(engine_options, route, DEV, None, weights, width[0], width[1], batch, C, P, text, **kw)


def _loop(engine_options, route, weights, C, P, **kw):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return dh.check_loop(engine_options, route, DEV, None, weights, D, FF, B, C, P, TEXT, **kw)


def _ragged(P):
    return [P, (P + 1) // 2, max(1, P - 5)]


@pytest.mark.parametrize("C,S", [(0, S) for S in dh.WINDOW_S] + [(20, S) for S in dh.WINDOW_S if S >= 33])
@pytest.mark.parametrize("route", TEN)
def test_every_window_edge_on_every_route(engine_options, route, C, S):
    """S = C + P across the 32- and 64-row tile edges, the last length of both (sequence, head) kernels (64) and their first refusal
    (65), the first and last length on sequence tiles (129, 224) and the first on the streaming attention (225); ragged frame counts.
    `seqtiles` must be on sequence tiles at 129 .. 224 and on row tiles outside; the block / two-launch self-attention must switch at 65."""
    want = {"selfattn": "block" if S <= 64 and route in ("planes32", "planes64", "x2", "x1", "x0") else "two"}
    if route == "seqtiles":
        want = {"tiling": "seq" if 129 <= S <= 224 else "row"}
    _fwd(engine_options, route, "plain", C, S - C, lengths=_ragged(S - C), want=want)


@pytest.mark.parametrize("ntok", dh.MEMORY_NTOK)
@pytest.mark.parametrize("route", ["x2", "x1", "x0", "skeleton", "f32"])
def test_every_memory_edge(engine_options, route, ntok):
    """Window 20 + 40.  64 / 65 memory tokens: the (sequence, head) kernel's limit; 96 / 97: the one-kernel block's; 230: the streaming
    fp32 attention.  The fall-back: dec_fused_xattn = 2 falls to 1 from 65 tokens and to the three launches from 97; 1 falls straight
    to the three launches from 97 (a 65-token memory does not fit the (sequence, head) kernel either)."""
    xa = {"x2": "seqhead" if ntok <= 64 else ("one" if ntok <= 96 else "three"), "x1": "one" if ntok <= 96 else "three"}.get(route, "three")
    _fwd(engine_options, route, "plain", 20, 40, text=dh.ragged_text(B, ntok), want={"xattn": xa})


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("C,P", [(20, 40), (0, 64)])
@pytest.mark.parametrize("route", TEN)
def test_both_guidance_modes_on_every_route(engine_options, route, C, P, guided):
    _fwd(engine_options, route, "plain", C, P, guided=guided)


@pytest.mark.parametrize("S", [129, 224])
def test_sequence_tiles_under_guidance(engine_options, S):
    """share0 (layer 0's self-attention block computed on the conditional half and copied) and skip_uncond (the unconditional half's
    cross-attention as row constants: gather_value_rows_kernel / uncond_xblock_rows_kernel): four launches the counters must show."""
    _fwd(engine_options, "seqtiles", "plain", 0, S, lengths=_ragged(S), guided=True, want={"tiling": "seq"})


@pytest.mark.parametrize("C,P,lengths,holes", [
    (20, 40, [40, 5, 20], False),           # S = 60: counts that end in key tile 2, 1, 2
    (20, 76, [76, 5, 30], False),           # S = 96: tiles 3, 1, 2
    (0, 160, [160, 100, 40], False),        # S = 160 (sequence tiles on `seqtiles`): tiles 5, 4, 2
    (0, 160, [130, 70, 20], False),         #                                          tiles 5, 3, 1
    (0, 40, [40, 1, 17], False),            # a sample with ONE valid frame
    (20, 40, [40, 33, 40], True),           # the bitmap form of `lengths`: interior frames and frame 0 of one sample cleared
    (0, 160, [160, 100, 150], True)])
@pytest.mark.parametrize("route", ["planes32", "sa0", "seqtiles", "skeleton"])
def test_frame_masks(engine_options, route, C, P, lengths, holes):
    _fwd(engine_options, route, "plain", C, P, lengths=lengths, holes=holes, guided=(P == 160 and holes))


@pytest.mark.parametrize("C,P", [(20, 40), (0, 65)])
@pytest.mark.parametrize("route", TEN)
def test_narrow_model_batch_of_one(engine_options, route, C, P):
    """latent_dim 256 with ff 256 (two heads, one 256-column statistics partial), B = 1; guided at 20 + 40, unguided at 0 + 65."""
    _fwd(engine_options, route, "plain", C, P, width=(256, 256), batch=1, guided=(C == 20))


@pytest.mark.parametrize("route,xa", [("x1", "seqhead"), ("planes32", "seqhead"), ("skeleton", "three"), ("f32", "three")])
def test_latent_dim_768(engine_options, route, xa):
    """Six heads and six 128-column partials per row.  The one-kernel cross-attention block exists for latent_dim 256 / 512 only: an
    explicit dec_fused_xattn = 1 must fall to the (sequence, head) form, not to the three launches."""
    _fwd(engine_options, route, "plain", 20, 40, width=(768, 1024), guided=True, want={"xattn": xa})


@pytest.mark.parametrize("b,xa", [(35, "seqhead"), (36, "one")])
def test_by_size_default_switches_at_144_row_tiles(engine_options, b, xa):
    """dec_fused_xattn = 3 (the default): 20 + 40 under guidance is 2 B sequences of two 32-row tiles -- 140 tiles at B = 35, 144 at 36."""
    _fwd(engine_options, "bysize", "plain", 20, 40, batch=b, guided=True, want={"xattn": xa})


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("route,variant,P", [(r, v, p) for r in ("planes32", "skeleton", "f32") for v in ("clip", "class_token")
                                             for p in (40, 64)] + [("seqtiles", "class_token", 159), ("seqtiles", "clip", 160)])
def test_class_token_and_one_token_memory(engine_options, route, variant, P, guided):
    """`clip`: ONE memory token per sample and no pad mask (a one-key softmax in the cross-attention).  `class_token` (emb_trans_dec):
    the timestep embedding leads the sequence as a never-masked row, so P = 64 is 65 tokens -- past the (sequence, head) kernels --
    and P = 159 is 160 tokens on sequence tiles."""
    _fwd(engine_options, route, "plain", 0, P, lengths=_ragged(P), variant=variant, guided=guided)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("C,P", [(20, 40), (0, 33)])
@pytest.mark.parametrize("route", TEN)
def test_hostile_weights(engine_options, route, C, P, guided):
    """oracle/synth.py synth_dip_state_dict_hostile / synth_dip_y_hostile: outlier channels and large row means through the three folded
    LayerNorms, ten-fold weight rows, a 20x text memory."""
    _fwd(engine_options, route, "hostile", C, P, lengths=[P, P // 2, 5], guided=guided)


LOOP_ROUTES = ["planes32", "x1", "x0sa0", "skeleton", "f32"]


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("route", LOOP_ROUTES)
def test_window_loop(engine_options, route, guided):
    """mdm_sample_loop_dec, two steps at 20 + 40: kv_text / kv_time hoisted, the step's kadd / vadd rows, the sampler update in the
    tail of OutputProcess on the plane routes."""
    _loop(engine_options, route, "plain", 20, 40, lengths=[40, 13, 33], guided=guided, steps=2)


@pytest.mark.parametrize("guided", [False, True])
def test_window_loop_on_sequence_tiles(engine_options, guided):
    """S = 129 on sequence tiles; under guidance the row constants of the unconditional half are hoisted too (o_text / o_time)."""
    _loop(engine_options, "seqtiles", "plain", 0, 129, lengths=[129, 40, 100], guided=guided, steps=2, want={"tiling": "seq"})


def test_window_loop_with_inpainting_and_clamp(engine_options):
    """The fused tail's inpainting blend and clip_denoised clamp."""
    _loop(engine_options, "planes32", "plain", 20, 40, guided=True, steps=2, inpaint=True)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("route", LOOP_ROUTES + ["seqtiles"])
def test_window_loop_on_hostile_weights_one_step(engine_options, route, guided):
    """ONE step: a second step feeds a hostile model's rounding error back through the model, and e_ref of one trajectory stops being a
    scale for another (profiles/r14a_decoder_parity.md).  A one-step schedule cannot be built -- the posterior tables of
    gaussian_diffusion.py:190-195 index step 1 -- so this is the last step of a two-step schedule (skip_timesteps = 1).
    What that step is NOT: a test of the sampler update on hostile weights.  At t = 0 posterior_mean_coef2 is 0 and the noise is
    masked out, so the tail reduces to out = x0 (a one-step schedule would have had the same property): these cases are hostile
    forwards through the loop's hoisted key / value path (kv_text / kv_time, kadd / vadd, o_text / o_time) and through the tail's
    guidance combine.  DecTail's blend of x_t, x0 and noise is covered on plain weights only, by the two-step loops above."""
    C, P = (0, 129) if route == "seqtiles" else (20, 40)
    _loop(engine_options, route, "hostile", C, P, lengths=[P, P // 2, 5], guided=guided, steps=2, skip=1)
