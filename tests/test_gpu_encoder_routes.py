"""The encoder's GEMM routes on the MI355X through ONE-layer models against the fp64 oracle: the folded-LayerNorm kinds of
csrc/gemm_x3.h (sequence tiles) and csrc/gemm_x3s.h (32- and 64-row tiles), the paired layer-0 in_proj, and the exact-fp32 mode, which
no building block of the C ABI reaches alone.  One layer deep, the fp32 oracle's own error against fp64 (e_ref) is a few 1e-7, so under

    err <= k * max(e_ref, floor)                  (tests/gemm_helpers.py check_route; k: profiles/r11a_gemm_parity.md)

a wrong epilogue term cannot hide the way it can behind the 3e-5 ... 1.2e-4 of the eight-layer forwards.  Sequence lengths S = T + 1
cross the 32- and 64-row tile edges, the paired launch's limit (S = 207) and first refusal (S = 208), the last length on sequence tiles
(S = 224) and the first on row tiles; the hostile weights (oracle/synth.py synth_state_dict_hostile) put large row means through the
folded statistics' Chan merge.  Every test prints `[gemm] gpu kernel=route:... ratio=...` before it asserts."""
import pytest
import torch

import gemm_helpers as gh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(engine_options, route, weights, D, ff, B, T, lengths=None, guided=None):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return gh.check_route(engine_options, route, DEV, None, weights, D, ff, B, T, lengths, guided)


@pytest.mark.parametrize("T", gh.ROUTE_TS)
@pytest.mark.parametrize("route", list(gh.ROUTES))
def test_every_length_on_every_route(engine_options, route, T):
    """B = 3, latent_dim 512, ff 1024; unguided except on the two routes that exist under guidance only."""
    _check(engine_options, route, "plain", 512, 1024, 3, T)


@pytest.mark.parametrize("T", [31, 64, 207])
@pytest.mark.parametrize("route", list(gh.ROUTES))
def test_narrow_model_batch_of_one_and_the_other_guidance_mode(engine_options, route, T):
    """latent_dim 256 with ff 256 (two heads; one partial statistic per row where 512 has two), B = 1, and the guidance mode
    test_every_length_on_every_route does not run: guided on small / small64 / seq / f32, unguided on the seq_shared option sets (where
    the option must be inert)."""
    _check(engine_options, route, "plain", 256, 256, 1, T, guided=not gh.route_guided(route))


@pytest.mark.parametrize("route", list(gh.ROUTES))
def test_ragged_lengths(engine_options, route):
    """S = 66: frame counts ending in the first, second and third key tile, on a 64-row tile edge."""
    _check(engine_options, route, "plain", 512, 1024, 3, 65, lengths=[65, 17, 40])


@pytest.mark.parametrize("T", [32, 207])
@pytest.mark.parametrize("route", list(gh.ROUTES))
def test_hostile_weights(engine_options, route, T):
    _check(engine_options, route, "hostile", 512, 1024, 3, T, lengths=[T, T // 2, 5])
