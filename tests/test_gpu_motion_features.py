"""joints -> features on the MI355X (csrc/motion_features.h behind mdm_amd.motion_process): every fixture of
tests/golden/motion_features_*.npz through the Python interface, the ragged batch's NaN poison, batch invariance, and the round
trip through recover_from_ric.  Only tests/golden/ is read.  Bounds: tests/motion_features_helpers.py."""
import numpy as np
import pytest
import torch

import motion_features_helpers as mh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def report():
    return mh.pin_report()


@pytest.mark.parametrize("name", list(mh.case_names()))
def test_case_matches_oracle_and_reference(report, name):
    d = mh.load_case(name)
    mh.check_case(name, d, mh.run_case(name, d, DEV), report)


def test_ragged_batch_ignores_the_poison_and_is_batch_invariant():
    """NaN beyond each clip's length reaches no valid frame; a clip alone gives bit-identical results to the same clip inside the
    batch, with process_file's transform (a reduction over the clip) switched on."""
    from mdm_amd.motion_process import joints_to_features
    d = mh.load_case("humanml_ragged")
    x = torch.from_numpy(mh.to_bj3t(d["joints"])).to(DEV)
    assert x.isnan().any()
    for canon in (False, True):
        both = joints_to_features(x, lengths=d["lengths"], canonicalise=canon)
        assert both.shape == (3, 263, 1, 196) and both.isfinite().all()
        for b, L in enumerate(d["lengths"]):
            alone = joints_to_features(x[b:b + 1, :, :, :L].contiguous(), canonicalise=canon)
            assert torch.equal(alone[0], both[b, :, :, :L - 1]) and not both[b, :, :, L - 1:].any()
    # ... and across the 64-clip launches
    many = joints_to_features(x[:1].repeat(65, 1, 1, 1))
    assert torch.equal(many[64], many[0]) and torch.equal(many[63], many[0])


@pytest.mark.parametrize("name", ["humanml_process", "humanml_retarget", "kit_process", "kit_retarget"])
def test_round_trip_through_recover_from_ric(report, name):
    """recover_from_ric(joints_to_features(x, canonicalise=True)) against the canonicalised joints process_file returns as
    global_positions, frames 0 .. L - 2.  The features do not determine the joints exactly (qnormalize's 1e-4 tilts the root
    rotation out of the xz plane, and the heading is integrated from asin of one quaternion component): the bound is twice what the
    same round trip costs with the reference's own two functions (PIN report, round_trip_ref)."""
    from mdm_amd.motion_process import joints_to_features, recover_from_ric
    c = mh.case_names()[name]
    d = mh.load_case(name)
    F = d["ref_data"].shape[1]
    x = torch.from_numpy(mh.to_bj3t(d["joints"])).to(DEV)
    feats = joints_to_features(x, dataset=c["dataset"], canonicalise=True, tgt_offsets=d.get("tgt_offsets"))
    back = recover_from_ric(feats, torch.zeros(F), torch.ones(F))                # [1, J, 3, T - 1]
    want = torch.from_numpy(mh.to_bj3t(d["ref_global"]))[..., :-1]
    err, bound = (back.cpu() - want).abs().max().item(), 2.0 * report["cases"][name]["round_trip_ref"]
    print(f"[motion_features] {name}: round trip {err:.3e} (reference's own {report['cases'][name]['round_trip_ref']:.3e})", flush=True)
    assert err <= bound, (err, bound)
    # with the dataset's statistics the normalised features invert the same way
    rng = np.random.default_rng(9)
    mean, std = torch.from_numpy(rng.normal(size=F).astype(np.float32)), torch.from_numpy(rng.uniform(0.5, 2.0, F).astype(np.float32))
    back_n = recover_from_ric(joints_to_features(x, dataset=c["dataset"], mean=mean, std=std, tgt_offsets=d.get("tgt_offsets")), mean, std)
    assert (back_n.cpu() - want).abs().max().item() <= bound


def run_integration_recipes(device, lib=None):
    """INTEGRATION.md's two recipes as written, on synthetic weights: a previous generation's joints as DiP's prefix, and joints as
    the fixed region of an in-between edit."""
    from types import SimpleNamespace
    from helpers import dip_small_state_dict, make_pair, small_state_dict, synth_dip_y, synth_y, to_dev
    from mdm_amd.motion_process import joints_to_features
    from mdm_amd.sampler_util import AutoRegressiveSampler
    B, context_len, pred_len, steps = 2, 20, 40, 4
    rng = np.random.default_rng(4)
    mean = torch.from_numpy(rng.normal(size=263).astype(np.float32)).to(device)
    std = torch.from_numpy(rng.uniform(0.5, 2.0, 263).astype(np.float32)).to(device)
    xyz = torch.from_numpy(mh.to_bj3t(mh.load_case("humanml_T82")["joints"])).repeat(B, 1, 1, 1).to(device)    # [B, 22, 3, 82]

    # 1. a previous generation's joints as DiP prefix
    prefix = joints_to_features(xyz, mean=mean, std=std, _native_lib=lib)[..., -context_len:]
    model, diffusion = make_pair(dip_small_state_dict(), steps, device, guided=True, native_lib=lib, context_len=context_len, pred_len=pred_len)
    y = to_dev(synth_dip_y(B, pred_len, context_len, seed=1, text_lengths=[7, 12]), device)
    y['prefix'] = prefix
    args = SimpleNamespace(pred_len=pred_len, context_len=context_len, autoregressive_include_prefix=True)
    sampler = AutoRegressiveSampler(args, diffusion.p_sample_loop, required_frames=context_len + pred_len)
    motion = sampler.sample(model, (B, 263, 1, pred_len), clip_denoised=False, model_kwargs={'y': y})
    assert motion.shape == (B, 263, 1, context_len + pred_len) and motion.isfinite().all() and torch.equal(motion[..., :context_len], prefix)

    # 2. joints as the fixed region of an in-between edit (sample/edit.py --edit_mode in_between)
    feats = joints_to_features(xyz, mean=mean, std=std, _native_lib=lib)                   # [B, 263, 1, 81]
    n = feats.shape[-1]
    model, diffusion = make_pair(small_state_dict(), steps, device, guided=True, native_lib=lib)
    y = to_dev(synth_y(B, n, seed=2), device)
    y['inpainted_motion'] = feats
    y['inpainting_mask'] = torch.ones_like(feats, dtype=torch.bool)
    y['inpainting_mask'][..., n // 4: 3 * n // 4] = False                                  # the model fills the middle half
    sample = diffusion.p_sample_loop(model, feats.shape, clip_denoised=False, model_kwargs={'y': y})
    keep = y['inpainting_mask']
    assert sample.isfinite().all() and torch.allclose(sample[keep], feats[keep], atol=1e-5)
    assert not torch.allclose(sample[~keep], feats[~keep], atol=1e-2)


def test_integration_recipes_run_on_synthetic_weights():
    run_integration_recipes(DEV)
