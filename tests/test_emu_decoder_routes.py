"""A subset of tests/test_gpu_decoder_routes.py on the CPU wave emulator of tests/emu, through the same checker and under the same
bound (tests/decoder_helpers.py): one-layer trans_dec models of width 256 (ff 256), B <= 2, against the fp64 oracle on every decoder
route -- every route at S = 64 and 65 (the (sequence, head) kernels' last length and first refusal), a sample of the routes at
S = 1, 32, 33 (a 32-row tile edge; the full cross is the MI355X file's) and, on sequence tiles, 129; memories of 1, 33, 65 and 97
tokens (the fall-back from the (sequence, head) form to the one-kernel block to the three launches); one hostile forward per route;
a two-step window loop on the plane route and on the fp32 skeleton.  The emulator's build of the profiler counts launches per class (csrc/api_runtime.h), so every case proves the form it ran exactly as on the MI355X."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import decoder_helpers as dh  # noqa: E402
from emu_lib import emu  # noqa: E402


def _fwd(engine_options, route, weights, B, C, P, text, **kw):
    return dh.check_route(engine_options, route, "cpu", emu(), weights, 256, 256, B, C, P, text, **kw)


_AT_64 = {"planes32": {"selfattn": "block", "xattn": "seqhead"}, "planes64": {"selfattn": "block", "xattn": "seqhead"},
          "x2": {"selfattn": "block", "xattn": "seqhead"}, "x1": {"selfattn": "block", "xattn": "one"},
          "x0": {"selfattn": "block", "xattn": "three"}, "sa0": {"selfattn": "two", "xattn": "seqhead"},
          "x0sa0": {"selfattn": "two", "xattn": "three"}, "seqtiles": {"selfattn": "block", "xattn": "seqhead", "tiling": "row"},
          "skeleton": {"tiling": "skeleton"}, "f32": {"tiling": "skeleton"}}
_AT_65 = {"planes32": {"selfattn": "two", "xattn": "one"}, "planes64": {"selfattn": "two", "xattn": "one"},
          "x2": {"selfattn": "two", "xattn": "one"}, "x1": {"selfattn": "two", "xattn": "one"},
          "x0": {"selfattn": "two", "xattn": "three"}, "sa0": {"selfattn": "two", "xattn": "one"},
          "x0sa0": {"selfattn": "two", "xattn": "three"}, "seqtiles": {"selfattn": "two", "xattn": "one", "tiling": "row"},
          "skeleton": {"tiling": "skeleton"}, "f32": {"tiling": "skeleton"}}
_GUIDED_AT_64 = ("f32",)


@pytest.mark.parametrize("route,B,S,guided,want",
                         # every route at its own switching edge: 64, the last length of both (sequence, head) kernels, and 65
                         [(r, 1, 64, r in _GUIDED_AT_64, _AT_64[r]) for r in _AT_64] + [(r, 1, 65, False, _AT_65[r]) for r in _AT_65] + [
    # ... and 1, 32, 33 spread over the routes
    ("planes32", 2, 1, False, {"selfattn": "block", "xattn": "seqhead"}),
    ("x1", 2, 32, False, {"xattn": "one"}),
    ("seqtiles", 2, 32, False, {"tiling": "row"}),
    ("seqtiles", 1, 129, True, {"tiling": "seq"}),
    ("f32", 2, 33, False, {"tiling": "skeleton"}),
])
def test_emulated_decoder_routes(engine_options, route, B, S, guided, want):
    """A SAMPLE of the (route, S) cross, not the cross: every route at 64 and 65, the lengths 1, 32 and 33 on one or two routes each
    (every route meets 33 again on hostile weights below).  No prefix (one engine per route whatever the window), ragged frame
    counts and prompts."""
    _fwd(engine_options, route, "plain", B, 0, S, [9, 1][:B], lengths=[S, (S + 1) // 2][:B], guided=guided, want=want)


@pytest.mark.parametrize("route,ntok,xa", [("x2", 33, "seqhead"), ("x2", 65, "one"), ("x1", 1, "one"), ("x1", 97, "three")])
def test_emulated_decoder_memory_edges(engine_options, route, ntok, xa):
    _fwd(engine_options, route, "plain", 1, 0, 33, [ntok], want={"xattn": xa})


@pytest.mark.parametrize("route", [r for r in dh.ROUTES if r != "bysize"])
def test_emulated_decoder_routes_on_hostile_weights(engine_options, route):
    _fwd(engine_options, route, "hostile", 2, 0, 33, [9, 1], lengths=[33, 11], guided=route == "x0")


@pytest.mark.parametrize("route,guided,B,C,P,text,lengths", [("planes32", True, 2, 5, 12, [6, 3], [12, 7]),
                                                            ("skeleton", False, 2, 5, 12, [6, 3], [12, 7])])
def test_emulated_decoder_window_loop(engine_options, route, guided, B, C, P, text, lengths):
    """Two steps, with the loop's own launch counts (decoder_helpers.loop_launches).  The loop on sequence tiles (o_text / o_time
    hoisted) costs 50 s on the emulator and runs on the MI355X only (test_window_loop_on_sequence_tiles)."""
    dh.check_loop(engine_options, route, "cpu", emu(), "plain", 256, 256, B, C, P, text, lengths=lengths, guided=guided, steps=2)
