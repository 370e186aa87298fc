"""GPU tests (`-m gpu`) of the SMPL joints of rot6d samples (csrc/smpl_joints.h behind mdm_rot6d_to_smpl_joints and
mdm_amd/rotation2xyz.py) on the MI355X: the reference's own outputs (tests/golden/smpl_joints_*.npz), the fp64 restatement at the
shapes of the action evaluation (eval/a2m/stgcn_eval.py:55: B 64 / 128, T 60 / 196, ragged masks), a full-size action model's
guided sample through sample/generate.py:167-171's call, and run-to-run bit identity."""
import numpy as np
import pytest
import torch

from helpers import make_pair, maxabs, memo
from oracle.synth import synth_a2m_state_dict
from smpl_helpers import CALLER_KW, fixture_names, load_fixture, rest_tables, smpl_joints_fp64, synthetic_model, write_smpl_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-5
A2M = dict(dataset="humanact12", num_actions=12)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mdm_amd import _native
    assert _native.load_native().path.endswith("libmdm_hip.so")


def _r2x(path):
    from mdm_amd.rotation2xyz import Rotation2xyz
    return Rotation2xyz(model_path=path)


def _ragged(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(1, T + 1, (B,), generator=g)
    lengths[0] = T
    mask = torch.arange(T)[None] < lengths[:, None]
    mask[1, 0] = False
    return mask


@pytest.mark.parametrize("name", fixture_names())
def test_smpl_joints_match_reference_fixture(tmp_path, name):
    g, mask = load_fixture(name)
    path = write_smpl_model(tmp_path, dict(v_template=g["v_template"], J_regressor=g["J_regressor"],
                                           kintree_table=g["kintree_table"]))
    m = torch.from_numpy(mask).to(DEV) if mask is not None else None
    got = _r2x(path)(x=torch.from_numpy(g["x"]).to(DEV), mask=m, **CALLER_KW)
    assert got.device.type == "cuda" and got.shape == g["out"].shape
    err = maxabs(got.cpu(), g["out"])
    print(f"[smpl] {name}: max-abs vs reference = {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("B,T", [(64, 60), (64, 196), (128, 60), (128, 196)])
def test_smpl_joints_match_fp64_oracle_at_eval_shapes(tmp_path, B, T):
    fields = synthetic_model(B + T)
    path = write_smpl_model(tmp_path, fields)
    x = torch.randn(B, 25, 6, T, generator=torch.Generator().manual_seed(B * T))
    mask = _ragged(B, T, T)
    r2x = _r2x(path)
    got = r2x(x=x.to(DEV), mask=mask.to(DEV), **CALLER_KW)
    err = maxabs(got.cpu(), smpl_joints_fp64(x.numpy(), mask.numpy(), *rest_tables(fields)))
    print(f"[smpl] B={B} T={T}: max-abs vs fp64 = {err:.3e}")
    assert err <= TOL
    again = r2x(x=x.to(DEV), mask=mask.to(DEV), **CALLER_KW)
    assert torch.equal(got, again)                                  # bit-identical run to run


def test_full_size_action_model_through_generate_call(tmp_path, monkeypatch):
    """p_sample_loop of a full-size humanact12 model (8 layers, d = 512) under guidance, then sample/generate.py:167-171 verbatim;
    the SMPL file is found at ./body_models/smpl/ as the reference's scripts expect."""
    fields = synthetic_model(7)
    write_smpl_model(tmp_path, fields)
    monkeypatch.chdir(tmp_path)
    B, T, steps = 8, 60, 10
    sd = memo("sd_a2m", lambda: synth_a2m_state_dict(seed=0))
    model, diffusion = make_pair(sd, steps, DEV, guided=True, **A2M)
    g = torch.Generator().manual_seed(11)
    lengths = torch.randint(20, T + 1, (B,), generator=g)
    lengths[0] = T
    model_kwargs = {"y": {"mask": (torch.arange(T)[None] < lengths[:, None]).view(B, 1, 1, T).to(DEV), "lengths": lengths.to(DEV),
                          "action": torch.randint(0, 12, (B, 1), generator=g).to(DEV), "scale": (torch.ones(B) * 2.5).to(DEV)}}
    sample = diffusion.p_sample_loop(model, (B, model.njoints, model.nfeats, T), clip_denoised=False, model_kwargs=model_kwargs,
                                     noise=torch.randn(B, 25, 6, T, generator=g).to(DEV))
    n_frames, batch_size = T, B
    # ---- sample/generate.py:167-171 ----
    rot2xyz_pose_rep = 'xyz' if model.data_rep in ['xyz', 'hml_vec'] else model.data_rep
    rot2xyz_mask = None if rot2xyz_pose_rep == 'xyz' else model_kwargs['y']['mask'].reshape(batch_size, n_frames).bool()
    out = model.rot2xyz(x=sample, mask=rot2xyz_mask, pose_rep=rot2xyz_pose_rep, glob=True, translation=True,
                        jointstype='smpl', vertstrans=True, betas=None, beta=0, glob_rot=None,
                        get_rotations_back=False)
    assert out.device == sample.device and out.shape == (B, 24, 3, T)
    want = smpl_joints_fp64(sample.cpu().numpy(), rot2xyz_mask.cpu().numpy(), *rest_tables(fields))
    err = maxabs(out.cpu(), want)
    print(f"[smpl] action model B={B} T={T}: max-abs vs fp64 of the same sample = {err:.3e}")
    assert err <= TOL
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0.1
