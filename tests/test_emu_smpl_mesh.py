"""csrc/smpl_mesh.h (mdm_smpl_forward behind mdm_amd/smpl_mesh.py's Rotation2xyzFull) on the CPU emulator of tests/emu: the
reference's own outputs for every jointstype, pose_rep and argument (tests/golden/smpl_mesh_*.npz), the fp64 restatement at odd
shapes, and the delegation of the case the old class supports."""
import numpy as np
import pytest
import torch

from emu.emu_lib import emu
from helpers import maxabs
from smpl_helpers import CALLER_KW
from smpl_mesh_helpers import (TOL, fixture_inputs, fixture_model, fixture_names, load_fixture, make_x, smpl_full_fp64,
                               synthetic_full_model, with_small_angles, write_model_files)


@pytest.fixture(scope="module")
def lib():
    return emu()


def _full(lib, paths, ids):
    from mdm_amd.smpl_mesh import Rotation2xyzFull
    return Rotation2xyzFull(model_path=paths[0], extra_regressor_path=paths[1], vertex_joint_ids=ids, _native_lib=lib)


def _t(a):
    return None if a is None else torch.from_numpy(np.asarray(a))


@pytest.mark.parametrize("name", fixture_names())
def test_emulated_full_pass_matches_reference_fixture(lib, tmp_path, name):
    fields, extra, ids, _ = fixture_model()
    g, call = load_fixture(name)
    x, mask, betas = fixture_inputs(g)
    got = _full(lib, write_model_files(tmp_path, fields, extra), ids)(x=_t(x), mask=_t(mask), betas=_t(betas), **call)
    if call["get_rotations_back"]:
        got, rotations, global_orient = got
        assert rotations.shape == g["rotations"].shape and global_orient.shape == g["global_orient"].shape
        rerr = max(maxabs(rotations, _t(g["rotations"])), maxabs(global_orient, _t(g["global_orient"])))
        print(f"[smpl-mesh] {name}: rotations max-abs vs reference = {rerr:.3e}")
        assert rerr <= TOL
    assert got.shape == g["out"].shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    err = maxabs(got, _t(g["out"]))
    print(f"[smpl-mesh] {name}: max-abs vs reference = {err:.3e}")
    assert err <= TOL


def test_fixtures_cover_the_issue_cases():
    seen = dict(jointstype=set(), pose_rep=set(), T=set())
    flags = dict(glob_false=False, no_translation=False, no_vertstrans=False, beta=False, betas_frames=False, betas_one=False,
                 ragged_first_masked=False, back=False, small_angle=False, glob_rot_zero=False)
    for n in fixture_names():
        g, call = load_fixture(n)
        x, mask, betas = fixture_inputs(g)
        seen["jointstype"].add(call["jointstype"])
        seen["pose_rep"].add(call["pose_rep"])
        seen["T"].add(x.shape[-1])
        flags["glob_false"] |= not call["glob"]
        flags["no_translation"] |= not call["translation"]
        flags["no_vertstrans"] |= not call["vertstrans"]
        flags["beta"] |= call["beta"] != 0
        flags["back"] |= bool(call["get_rotations_back"])
        flags["glob_rot_zero"] |= call["glob_rot"] is not None and not any(call["glob_rot"])
        if call["pose_rep"] == "rotvec":                        # both sides of the small-angle branch, on valid frames
            ang = np.linalg.norm(x[:, :(-1 if call["translation"] else None), :3].astype(np.float64), axis=2)      # [B, rows, T]
            ok = np.ones((x.shape[0], x.shape[-1]), bool) if mask is None else mask
            a = ang[np.broadcast_to(ok[:, None], ang.shape)]
            flags["small_angle"] |= bool((a == 0).any() and ((a > 0) & (a < 1e-6)).any() and ((a > 1e-6) & (a < 1e-5)).any())
        if betas is not None:
            flags["betas_one" if betas.shape[0] == 1 else "betas_frames"] = True
        if mask is not None:
            flags["ragged_first_masked"] |= bool((~mask[:, 0]).any() and not mask.all(1).all() and mask[:, 0].any() or
                                                 (mask.shape[0] == 1 and not mask[0, 0] and mask.any()))
        assert "restated" in str(g["meta"])                     # smplx is restated, not run: every file says so
    assert seen["jointstype"] == {"vertices", "smpl", "a2m", "a2mpl", "vibe"}
    assert seen["pose_rep"] == {"rot6d", "rotvec", "rotmat", "rotquat"}
    assert {60, 196} <= seen["T"]
    assert all(flags.values()), flags


# V = 75 is not a multiple of the 32-vertex tile (and spans three of them); T = 1, 37, 129: below, beside and over the 32-frame tile
@pytest.mark.parametrize("B,T,V,jointstype,pose_rep", [(3, 37, 75, "vertices", "rot6d"), (2, 1, 75, "vibe", "rotvec"),
                                                        (2, 129, 40, "a2m", "rotquat"), (1, 37, 300, "a2mpl", "rotmat")])
def test_emulated_full_pass_matches_fp64_at_odd_shapes(lib, tmp_path, B, T, V, jointstype, pose_rep):
    fields, extra, ids = synthetic_full_model(seed=B + T, V=V)
    r2x = _full(lib, write_model_files(tmp_path, fields, extra), ids)
    x = make_x(B, T, pose_rep, True, True, seed=T)
    g = torch.Generator().manual_seed(T)
    lengths = torch.randint(1, T + 1, (B,), generator=g)
    mask = torch.arange(T)[None] < lengths[:, None]
    if T > 1:
        mask[-1, 0] = False
    call = dict(pose_rep=pose_rep, translation=True, glob=True, jointstype=jointstype, vertstrans=True, beta=0.7)
    got = r2x(x=_t(x), mask=mask, **call)
    want = smpl_full_fp64(x, mask.numpy(), fields, ids, extra, **call)
    err = maxabs(got, _t(want))
    print(f"[smpl-mesh] B={B} T={T} V={V} {jointstype} {pose_rep}: max-abs vs fp64 = {err:.3e}")
    assert got.shape == want.shape and err <= TOL
    # masked frames: the translation offset alone on every point
    tr = torch.from_numpy(x[:, -1, :3])
    off = (tr - tr[:, :, :1])[:, None].expand(B, got.shape[1], 3, T)
    assert torch.equal(got.permute(0, 3, 1, 2)[~mask], off.permute(0, 3, 1, 2)[~mask])
    got = r2x(x=_t(x), mask=None, **call)
    assert maxabs(got, _t(smpl_full_fp64(x, None, fields, ids, extra, **call))) <= TOL


def test_emulated_small_angles_and_zero_glob_rot_match_fp64(lib, tmp_path):
    """axis_angle_to_quaternion's small-angle branch (exact zeros, angles on both sides of 1e-6) in the kernel's front end, and in the
    host's glob_rot conversion (a glob_rot of zeros is the identity; one of 1e-7 takes the same branch)."""
    fields, extra, ids = synthetic_full_model(seed=3, V=40)
    r2x = _full(lib, write_model_files(tmp_path, fields, extra), ids)
    x = with_small_angles(make_x(2, 9, "rotvec", False, True, seed=1))
    for glob_rot in ([0.0, 0.0, 0.0], [1e-7, 0.0, -2e-7], [0.4, 0.1, -0.3]):
        call = dict(pose_rep="rotvec", translation=True, glob=False, jointstype="vertices", vertstrans=True, glob_rot=glob_rot,
                    get_rotations_back=True)
        got, rot, go = r2x(x=_t(x), mask=None, **call)
        want, w_rot, w_go = smpl_full_fp64(x, None, fields, ids, extra, **call)
        assert torch.isfinite(got).all() and torch.isfinite(rot).all()
        assert maxabs(got, _t(want)) <= TOL and maxabs(rot, _t(w_rot)) <= TOL and maxabs(go, _t(w_go)) <= TOL
        if not any(glob_rot):
            assert torch.equal(go[0, 0], torch.eye(3))
    zero = rot.view(2, 9, 23, 3, 3)[0, 1, 2]                        # with_small_angles: an exact-zero rotvec is the identity
    assert torch.equal(zero, torch.eye(3))


def test_supported_case_is_delegated_bit_identically(lib, tmp_path):
    from mdm_amd.rotation2xyz import Rotation2xyz
    fields, extra, ids = synthetic_full_model(seed=5, V=64)
    paths = write_model_files(tmp_path, fields, extra)
    x = _t(make_x(3, 45, "rot6d", True, True, seed=9))
    mask = torch.arange(45)[None] < torch.tensor([45, 20, 7])[:, None]
    old = Rotation2xyz(model_path=paths[0], _native_lib=lib)(x=x, mask=mask, **CALLER_KW)
    new = _full(lib, paths, ids)(x=x, mask=mask, **CALLER_KW)
    assert torch.equal(old, new)
    # ... while the same call through the general path (a beta that is not 0 by a hair) is a different computation, close to it
    near = _full(lib, paths, ids)(x=x, mask=mask, **dict(CALLER_KW, beta=1e-30))
    assert maxabs(near, old) <= TOL
