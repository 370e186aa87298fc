"""GPU tests (`-m gpu`) of the full SMPL pass (csrc/smpl_mesh.h behind mdm_smpl_forward and mdm_amd/smpl_mesh.py) on the MI355X:
the reference's own outputs (tests/golden/smpl_mesh_*.npz), the fp64 restatement on a synthetic model of the real size (6,890
vertices) at the shapes of the mesh renderer (B 1 / T 196) and of the action evaluation (B 128 / T 60, a2m B 64 / T 60), run-to-run
bit identity, the two reference callers' literal calls, and a graph captured on a side stream after a warm-up.

Measured on the MI355X (max-abs): fixtures 2.9e-6 at most; fp64 at V = 6890: 5.7e-7 (vertices B 1 / T 196), 5.9e-6 (vertices
B 128 / T 60), 3.5e-6 (a2m B 64 / T 60) -- DESIGN.md section 4, profiles/r07a_smpl_mesh.md."""
import numpy as np
import pytest
import torch

from helpers import maxabs
from smpl_mesh_helpers import (TOL, fixture_inputs, fixture_model, fixture_names, load_fixture, make_x, smpl_full_fp64,
                               synthetic_full_model, write_model_files)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mdm_amd import _native
    assert _native.load_native().path.endswith("libmdm_hip.so")


@pytest.fixture(scope="module")
def real_size(tmp_path_factory):
    """(Rotation2xyzFull, fields, extra, ids) on the seeded 6,890-vertex model: dense weights, posedirs ~ N(0, 0.01)."""
    from mdm_amd.smpl_mesh import Rotation2xyzFull
    fields, extra, ids = synthetic_full_model(seed=0, V=6890)
    paths = write_model_files(tmp_path_factory.mktemp("smpl6890"), fields, extra)
    return Rotation2xyzFull(model_path=paths[0], extra_regressor_path=paths[1], vertex_joint_ids=ids), fields, extra, ids


def _t(a, dev=DEV):
    return None if a is None else torch.from_numpy(np.asarray(a)).to(dev)


def _ragged(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(1, T + 1, (B,), generator=g)
    lengths[0] = T
    mask = torch.arange(T)[None] < lengths[:, None]
    if B > 1:
        mask[1, 0] = False
    return mask


@pytest.mark.parametrize("name", fixture_names())
def test_full_pass_matches_reference_fixture(tmp_path, name):
    from mdm_amd.smpl_mesh import Rotation2xyzFull
    fields, extra, ids, _ = fixture_model()
    paths = write_model_files(tmp_path, fields, extra)
    g, call = load_fixture(name)
    x, mask, betas = fixture_inputs(g)
    r2x = Rotation2xyzFull(model_path=paths[0], extra_regressor_path=paths[1], vertex_joint_ids=ids)
    got = r2x(x=_t(x), mask=_t(mask), betas=_t(betas), **call)
    if call["get_rotations_back"]:
        got, rotations, global_orient = got
        assert rotations.shape == g["rotations"].shape and global_orient.shape == g["global_orient"].shape
        rerr = max(maxabs(rotations.cpu(), g["rotations"]), maxabs(global_orient.cpu(), g["global_orient"]))
        print(f"[smpl-mesh] {name}: rotations max-abs vs reference = {rerr:.3e}")
        assert rerr <= TOL
    assert got.device.type == "cuda" and got.shape == g["out"].shape and got.dtype == torch.float32
    err = maxabs(got.cpu(), g["out"])
    print(f"[smpl-mesh] {name}: max-abs vs reference = {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("B,T,jointstype", [(1, 196, "vertices"), (128, 60, "vertices"), (64, 60, "a2m")])
def test_full_pass_matches_fp64_at_real_size(real_size, B, T, jointstype):
    r2x, fields, extra, ids = real_size
    x = make_x(B, T, "rot6d", True, True, seed=B + T)
    mask = _ragged(B, T, T)
    call = dict(pose_rep="rot6d", translation=True, glob=True, jointstype=jointstype, vertstrans=True)
    got = r2x(x=_t(x), mask=mask.to(DEV), **call)
    again = r2x(x=_t(x), mask=mask.to(DEV), **call)
    assert torch.equal(got, again)                                  # bit-identical run to run (no floating-point atomics)
    want = smpl_full_fp64(x, mask.numpy(), fields, ids, extra, **call)
    assert got.shape == want.shape
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"[smpl-mesh] V=6890 B={B} T={T} {jointstype}: max-abs vs fp64 = {err:.3e}, absmax {float(np.abs(want).max()):.2f}")
    assert err <= TOL


def test_npy2obj_call_sequence(real_size):
    """visualize/vis_utils.py:33-40: one rot6d motion [1, 25, 6, T] as a CPU array, mask=None, jointstype='vertices'; the faces
    are read from smpl_model before the first call (vis_utils.py:16)."""
    r2x, fields, extra, ids = real_size
    motion = make_x(1, 120, "rot6d", True, True, seed=3)
    with pytest.raises(ValueError, match="'f' field"):
        r2x.smpl_model.faces                                        # (the synthetic model file has no triangles)
    vertices = r2x(torch.tensor(motion).to(DEV), mask=None,
                   pose_rep='rot6d', translation=True, glob=True,
                   jointstype='vertices',
                   vertstrans=True)
    assert vertices.shape == (1, 6890, 3, 120)
    want = smpl_full_fp64(motion, None, fields, ids, extra, pose_rep="rot6d", translation=True, glob=True, jointstype="vertices",
                          vertstrans=True)
    assert float(np.abs(vertices.cpu().numpy() - want).max()) <= TOL


def test_action2motion_recognition_call(real_size):
    """eval/a2m/action2motion/models.py:85-113: params carries the dataset's keys too; x [1, 25, 6, 60], an all-ones bool mask."""
    r2x, fields, extra, ids = real_size
    params = {"pose_rep": "rot6d",
              "translation": True,
              "glob": True,
              "jointstype": "a2m",
              "vertstrans": True,
              "num_frames": 60,
              "sampling": "conseq",
              "sampling_step": 1}
    xn = make_x(1, 60, "rot6d", True, True, seed=4)
    x = torch.from_numpy(xn).to("cuda")
    mask = torch.ones(1, x.shape[-1], dtype=bool, device="cuda")
    xyz_t = r2x(x, mask, **params)
    assert xyz_t.shape == (1, 18, 3, 60)
    want = smpl_full_fp64(xn, None, fields, ids, extra, pose_rep="rot6d", translation=True, glob=True, jointstype="a2m",
                          vertstrans=True)
    assert float(np.abs(xyz_t.cpu().numpy() - want).max()) <= TOL


@pytest.mark.parametrize("jointstype", ["vertices", "a2m"])
def test_side_stream_and_graph_replay(real_size, jointstype):
    r2x, fields, extra, ids = real_size
    B, T = 4, 60
    x = _t(make_x(B, T, "rot6d", True, True, seed=8))
    mask = _ragged(B, T, 5).to(DEV)
    call = dict(pose_rep="rot6d", translation=True, glob=True, jointstype=jointstype, vertstrans=True)
    ref = r2x(x=x, mask=mask, **call)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = r2x(x=x, mask=mask, **call)                          # a call on a non-default stream, the capture's warm-up
    side.synchronize()
    assert torch.equal(warm, ref)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = r2x(x=x, mask=mask, **call)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
