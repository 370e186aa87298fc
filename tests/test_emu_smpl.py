"""csrc/smpl_joints.h (mdm_rot6d_to_smpl_joints behind mdm_amd/rotation2xyz.py) on the CPU emulator of tests/emu: the reference's
own outputs (tests/golden/smpl_joints_*.npz), an fp64 restatement at odd shapes, and an action-to-motion model's sample through
sample/generate.py:167-171's exact call, bare and through the guidance wrapper."""
import numpy as np
import pytest
import torch

from emu.emu_lib import emu
from helpers import make_pair, maxabs
from oracle.synth import synth_a2m_state_dict
from smpl_helpers import CALLER_KW, fixture_names, load_fixture, rest_tables, smpl_joints_fp64, synthetic_model, write_smpl_model

TOL = 1e-5
A2M = dict(dataset="humanact12", num_actions=12)


@pytest.fixture(scope="module")
def lib():
    return emu()


def _r2x(lib, path):
    from mdm_amd.rotation2xyz import Rotation2xyz
    return Rotation2xyz(model_path=path, _native_lib=lib)


@pytest.mark.parametrize("name", fixture_names())
def test_emulated_smpl_joints_match_reference_fixture(lib, tmp_path, name):
    g, mask = load_fixture(name)
    path = write_smpl_model(tmp_path, dict(v_template=g["v_template"], J_regressor=g["J_regressor"],
                                           kintree_table=g["kintree_table"]))
    x = torch.from_numpy(g["x"])
    m = torch.from_numpy(mask) if mask is not None else None
    got = _r2x(lib, path)(x=x, mask=m, **CALLER_KW)
    assert got.shape == g["out"].shape and got.dtype == torch.float32
    assert torch.isfinite(got).all()
    err = maxabs(got, torch.from_numpy(g["out"]))
    print(f"[smpl] {name}: max-abs vs reference = {err:.3e}")
    assert err <= TOL


def test_fixtures_cover_the_issue_cases():
    names = fixture_names()
    assert len(names) >= 4
    Ts, full, frame0_masked, tiny = set(), False, False, False
    for n in names:
        g, mask = load_fixture(n)
        Ts.add(g["x"].shape[-1])
        if mask is not None:
            full |= bool(mask.all())
            frame0_masked |= bool((~mask[:, 0]).any() and mask[:, 0].any())
        halves = np.linalg.norm(g["x"][:, :24].reshape(g["x"].shape[0], 24, 2, 3, -1), axis=3)
        valid = np.ones((g["x"].shape[0], g["x"].shape[-1]), bool) if mask is None else mask
        tiny |= bool(((halves == 0) & valid[:, None, None]).any() and ((halves > 0) & (halves < 1e-12) & valid[:, None, None]).any())
    assert {60, 196} <= Ts and full and frame0_masked and tiny


@pytest.mark.parametrize("B,T,seed", [(3, 37, 0), (5, 1, 1), (2, 129, 2)])
def test_emulated_smpl_joints_match_fp64_oracle(lib, tmp_path, B, T, seed):
    fields = synthetic_model(seed)
    path = write_smpl_model(tmp_path, fields)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 25, 6, T, generator=g)
    lengths = torch.randint(1, T + 1, (B,), generator=g)
    mask = torch.arange(T)[None] < lengths[:, None]
    mask[-1, 0] = False                                        # frame 0 masked: its translation is still the origin
    got = _r2x(lib, path)(x=x, mask=mask, **CALLER_KW)
    want = smpl_joints_fp64(x.numpy(), mask.numpy(), *rest_tables(fields))
    assert maxabs(got, torch.from_numpy(want)) <= TOL
    # masked frames: the translation offset alone, on every joint
    tr = x[:, 24, :3]
    off = (tr - tr[:, :, :1])[:, None].expand(B, 24, 3, T)
    assert torch.equal(got.permute(0, 3, 1, 2)[~mask], off.permute(0, 3, 1, 2)[~mask])
    # mask=None: every frame valid
    got = _r2x(lib, path)(x=x, mask=None, **CALLER_KW)
    assert maxabs(got, torch.from_numpy(smpl_joints_fp64(x.numpy(), None, *rest_tables(fields)))) <= TOL


def test_emulated_action_model_through_generate_call(lib, tmp_path, monkeypatch):
    """sample/generate.py:167-171 verbatim on a humanact12 model: the SMPL file is read from ./body_models/smpl/ (the reference's
    location, relative to the working directory), both through the bare model and through ClassifierFreeSampleModel."""
    fields = synthetic_model(3)
    write_smpl_model(tmp_path, fields)
    monkeypatch.chdir(tmp_path)
    B, T, steps = 2, 13, 2
    sd = synth_a2m_state_dict(seed=0, latent_dim=256, num_layers=1)
    model, diffusion = make_pair(sd, steps, "cpu", guided=True, native_lib=lib, **A2M)
    assert model.data_rep == "rot6d" and model.rot2xyz is model.model.rot2xyz
    lengths = torch.tensor([13, 6])
    model_kwargs = {"y": {"mask": (torch.arange(T)[None] < lengths[:, None]).view(B, 1, 1, T), "lengths": lengths,
                          "action": torch.tensor([[3], [7]]), "scale": torch.ones(B) * 2.5}}
    sample = diffusion.p_sample_loop(model, (B, model.njoints, model.nfeats, T), clip_denoised=False,
                                     model_kwargs=model_kwargs, noise=torch.randn(B, 25, 6, T, generator=torch.Generator().manual_seed(5)))
    n_frames, batch_size = T, B
    # ---- sample/generate.py:167-171 ----
    rot2xyz_pose_rep = 'xyz' if model.data_rep in ['xyz', 'hml_vec'] else model.data_rep
    rot2xyz_mask = None if rot2xyz_pose_rep == 'xyz' else model_kwargs['y']['mask'].reshape(batch_size, n_frames).bool()
    out = model.rot2xyz(x=sample, mask=rot2xyz_mask, pose_rep=rot2xyz_pose_rep, glob=True, translation=True,
                        jointstype='smpl', vertstrans=True, betas=None, beta=0, glob_rot=None,
                        get_rotations_back=False)
    assert out.shape == (B, 24, 3, T)
    want = torch.from_numpy(smpl_joints_fp64(sample.numpy(), rot2xyz_mask.numpy(), *rest_tables(fields)))
    assert maxabs(out, want) <= TOL
    bare = model.model.rot2xyz(x=sample, mask=rot2xyz_mask, **CALLER_KW)
    assert torch.equal(bare, out)
    model.rot2xyz.smpl_model.eval()                               # train/train_mdm.py:47
