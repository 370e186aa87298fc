"""Round 8: layer 0's in_proj of a guided trans_enc forward computes every sample's frame rows ONCE and writes them to both branches'
Q / K / V^T planes (csrc/gemm_x3.h PAIR; include/mdm_hip.h MDM_OPT_ENC_SHARED_LAYER0).  The two sequences of a sample differ only in
token 0, which rides in tile row S of the sample's 208-row tile.  Every output element keeps its products and their order, so the
option is held to BIT equality against the one-tile-per-sequence launch (`enc_shared_layer0=0`) -- forwards, a 10-step loop -- and,
once, to the oracle at the forward tolerance of tests/test_gpu_parity.py.  small_gemm_max_seqs = 0 forces the sequence-tile kernel at
these small batches."""
import pytest
import torch

from helpers import make_pair, maxabs, memo, orc, synth_state_dict, synth_y

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_FWD = 3e-5            # tests/test_gpu_parity.py TOL_FWD['f16x3']; guided output: 4 x (the 2 s - 1 amplification)


@pytest.fixture(scope="module")
def sd():
    return synth_state_dict(seed=0)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mdm_amd import _native
    assert _native.load_native().path.endswith("libmdm_hip.so")


def _inputs(B, T, lengths=None, mixed_t=False):
    y = synth_y(B, T, seed=B * 1000 + T, lengths=lengths)
    g = torch.Generator().manual_seed(T)
    x = torch.randn(B, 263, 1, T, generator=g)
    t = torch.randint(0, 50, (B,), generator=g) if mixed_t else torch.full((B,), 17)
    return x, t, y


def _forward(engine_options, sd, shared, x, t, y, guided=True):
    engine_options(small_gemm_max_seqs=0, enc_shared_layer0=shared)
    model, _ = make_pair(sd, 50, DEV, guided=guided)
    inner = model.model if guided else model
    out = model(x.to(DEV), t.to(DEV), y=dict(y)).cpu()
    assert inner.engine().get_option("enc_shared_layer0") == shared and inner.engine().get_option("small_gemm_max_seqs") == 0
    return out


# T = 196: the headline's S = 197; T = 20: a short sequence, tile row S far from 197 (one key tile); T = 206: S = 207, the last S that
# fits -- the shared row is tile row 207; T = 207: S = 208 does not fit and must take the unshared launch; B = 3, T = 60: per-sample
# timesteps, mixed lengths (a prefix mask per sample), the unconditional branch built through uncond_from_branch (forward_both)
@pytest.mark.parametrize("B,T,lengths,mixed_t", [(2, 196, None, False), (3, 20, None, False), (2, 206, None, False),
                                                 (2, 207, None, False), (3, 60, [60, 7, 33], True)])
def test_guided_forward_is_bit_identical_with_the_shared_layer0_in_proj(engine_options, sd, B, T, lengths, mixed_t):
    x, t, y = _inputs(B, T, lengths, mixed_t)
    on = _forward(engine_options, sd, 1, x, t, y)
    off = _forward(engine_options, sd, 0, x, t, y)
    assert torch.isfinite(on).all()
    assert torch.equal(on, off), maxabs(on, off)


def test_guided_forward_with_the_shared_layer0_in_proj_matches_the_oracle(engine_options, sd):
    B, T, lengths = 3, 60, [60, 7, 33]
    x, t, y = _inputs(B, T, lengths, True)
    got = _forward(engine_options, sd, 1, x, t, y)
    want = memo(("shared_l0", B, T), lambda: orc.cfg_forward(sd, x, t, y))
    err = maxabs(got, want)
    print(f"[parity] guided forward B={B} T={T}, enc_shared_layer0=1: max-abs vs oracle = {err:.3e}")
    assert err < 4 * TOL_FWD


def test_guided_loop_is_bit_identical_with_the_shared_layer0_in_proj(engine_options, sd):
    steps, B, T = 10, 2, 196
    shape = (B, 263, 1, T)
    y = synth_y(B, T, seed=5, lengths=[T, 150])
    x_T, noises = orc.make_noise(shape, steps, 11)
    seq = [x_T] + [n.contiguous() for n in noises]
    outs = {}
    for shared in (1, 0):
        engine_options(small_gemm_max_seqs=0, enc_shared_layer0=shared)
        model, diffusion = make_pair(sd, steps, DEV, guided=True)
        outs[shared] = diffusion.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": dict(y)}, noise_sequence=seq).cpu()
    assert torch.isfinite(outs[1]).all()
    assert torch.equal(outs[1], outs[0]), maxabs(outs[1], outs[0])


def test_single_branch_forward_does_not_take_the_shared_route(engine_options, sd):
    """One branch per forward (no guidance): nothing to share -- the option must not change what runs.  B = 4 is even on purpose: a
    route test on the sequence count alone would pair samples 0 / 2 and 1 / 3."""
    x, t, y = _inputs(4, 40, [40, 9, 40, 22], True)
    on = _forward(engine_options, sd, 1, x, t, y, guided=False)
    off = _forward(engine_options, sd, 0, x, t, y, guided=False)
    assert torch.equal(on, off), maxabs(on, off)
    want = memo(("shared_l0_single", 4, 40), lambda: orc.mdm_forward(sd, x, t, y))
    assert maxabs(on, want) < TOL_FWD
