"""Host-side behaviour of mdm_amd/smpl_mesh.py (Rotation2xyzFull) and of the ABI's argument validation (mdm_smpl_forward,
mdm_smpl_workspace_bytes; on the emulator library, where a refused call launches nothing): the loader's fields and messages, which
files a call opens, the reference's errors, the selector ids, the index maps, and the old class left as it was."""
import builtins
import ctypes as C
import pickle
import sys
import types

import numpy as np
import pytest
import torch

from emu.emu_lib import emu
from smpl_mesh_helpers import fixture_model, make_x, synthetic_full_model, write_model_files

CALL = dict(pose_rep="rot6d", translation=True, glob=True, jointstype="vertices", vertstrans=True)


@pytest.fixture(scope="module")
def lib():
    return emu()


@pytest.fixture()
def small(tmp_path):
    fields, extra, ids = synthetic_full_model(seed=1, V=40)
    return fields, extra, ids, write_model_files(tmp_path, fields, extra)


def _full(lib, paths, ids=None):
    from mdm_amd.smpl_mesh import Rotation2xyzFull
    return Rotation2xyzFull(model_path=paths[0], extra_regressor_path=paths[1], vertex_joint_ids=ids, _native_lib=lib)


def test_loader_reads_the_fields_of_the_full_pass(small):
    from mdm_amd.smpl_mesh import load_smpl_model
    fields, _, _, paths = small
    m = load_smpl_model(paths[0])
    assert m["shapedirs"].shape == (40, 3, 10) and m["posedirs"].shape == (40, 3, 207) and m["weights"].shape == (40, 24)
    assert m["parents"][0] == -1 and m["parents"].dtype == np.int32 and m["faces"] is None
    np.testing.assert_array_equal(m["posedirs"], fields["posedirs"])
    wide = dict(fields, shapedirs=np.concatenate([fields["shapedirs"], np.ones((40, 3, 290))], axis=2))      # the official 300
    with open(paths[0], "wb") as f:
        pickle.dump(wide, f, protocol=2)
    np.testing.assert_array_equal(load_smpl_model(paths[0])["shapedirs"], fields["shapedirs"])


@pytest.mark.parametrize("field", ["shapedirs", "posedirs", "weights", "v_template", "J_regressor", "kintree_table"])
def test_loader_names_a_missing_field(small, field):
    from mdm_amd.smpl_mesh import load_smpl_model
    fields, _, _, paths = small
    with open(paths[0], "wb") as f:
        pickle.dump({k: v for k, v in fields.items() if k != field}, f, protocol=2)
    with pytest.raises(ValueError, match=f"no '{field}' field"):
        load_smpl_model(paths[0])


def test_loader_errors_follow_the_joints_loader(small, tmp_path, monkeypatch):
    from mdm_amd.smpl_mesh import load_smpl_model
    fields, _, _, paths = small
    with pytest.raises(FileNotFoundError, match="SMPL_NEUTRAL.pkl"):
        load_smpl_model(str(tmp_path / "nowhere" / "SMPL_NEUTRAL.pkl"))
    # a stand-in chumpy (module chumpy.ch, class Ch), importable while pickling only: the official file holds posedirs as one
    mod, pkg = types.ModuleType("chumpy.ch"), types.ModuleType("chumpy")

    class Ch:
        def __init__(self, x):
            self.x = x

        def __getstate__(self):
            return {"x": self.x}

    Ch.__module__, Ch.__qualname__ = "chumpy.ch", "Ch"
    mod.Ch, pkg.ch = Ch, mod
    with monkeypatch.context() as mp:
        mp.setitem(sys.modules, "chumpy", pkg)
        mp.setitem(sys.modules, "chumpy.ch", mod)
        with open(paths[0], "wb") as f:
            pickle.dump(dict(fields, posedirs=Ch(fields["posedirs"])), f, protocol=2)
    assert "chumpy" not in sys.modules
    with pytest.raises(ValueError, match="'posedirs' is a chumpy object"):
        load_smpl_model(paths[0])
    with open(paths[0], "wb") as f:
        pickle.dump(dict(fields, weights=fields["weights"][:, :23]), f, protocol=2)
    with pytest.raises(ValueError, match="weights"):
        load_smpl_model(paths[0])


def test_xyz_is_a_passthrough_that_opens_no_file(lib, tmp_path):
    r2x = _full(lib, (str(tmp_path / "missing.pkl"), str(tmp_path / "missing.npy")))
    x = torch.randn(2, 22, 3, 9)
    assert r2x(x, None, "xyz", True, True, "vertices", True) is x
    assert r2x(x=x, mask=None, pose_rep="xyz", translation=False, glob=False, jointstype="nothing", vertstrans=False) is x


def test_extra_regressor_is_opened_only_for_the_joints_families_that_need_it(lib, small, monkeypatch):
    _, _, ids, paths = small
    opened = []
    real_open = builtins.open

    def spy(file, *a, **k):
        opened.append(str(file))
        return real_open(file, *a, **k)
    monkeypatch.setattr(builtins, "open", spy)
    x = torch.from_numpy(make_x(1, 3, "rot6d", True, True, seed=0))
    r2x = _full(lib, paths, ids)
    r2x(x=x, mask=None, **CALL)
    r2x(x=x, mask=None, **dict(CALL, jointstype="smpl", beta=0.5))
    assert not any(p.endswith("J_regressor_extra.npy") for p in opened) and any(p.endswith("SMPL_NEUTRAL.pkl") for p in opened)
    for jt in ("a2m", "a2mpl", "vibe"):
        fresh = _full(lib, paths, ids)
        del opened[:]
        fresh(x=x, mask=None, **dict(CALL, jointstype=jt))
        assert any(p.endswith("J_regressor_extra.npy") for p in opened), jt
    gone = _full(lib, (paths[0], paths[1] + ".gone"), ids)
    gone(x=x, mask=None, **CALL)                                    # 'vertices' does not need it
    with pytest.raises(FileNotFoundError, match="J_regressor_extra.npy"):
        gone(x=x, mask=None, **dict(CALL, jointstype="a2m"))


def test_errors_of_the_reference(lib, small):
    _, _, ids, paths = small
    r2x = _full(lib, paths, ids)
    x = torch.from_numpy(make_x(1, 3, "rot6d", True, True, seed=0))
    with pytest.raises(TypeError, match="You must specify global rotation if glob is False"):       # rotation2xyz.py:26-27
        r2x(x=x, mask=None, **dict(CALL, glob=False))
    with pytest.raises(NotImplementedError, match="This jointstype is not implemented."):            # :29-30
        r2x(x=x, mask=None, **dict(CALL, jointstype="openpose"))
    with pytest.raises(NotImplementedError, match="No geometry for this one."):                      # :50-51
        r2x(x=x, mask=None, **dict(CALL, pose_rep="euler"))
    with pytest.raises(ValueError, match=r"x must be \[B, 25, 3, T\]"):
        r2x(x=x, mask=None, **dict(CALL, pose_rep="rotvec"))
    with pytest.raises(ValueError, match="valid frames"):
        r2x(x=x, mask=None, betas=torch.zeros(2, 10), **CALL)


def test_selector_ids_must_fit_the_model(lib, small):
    from mdm_amd import smpl_mesh
    _, _, ids, paths = small
    assert len(smpl_mesh.SMPLH_VERTEX_JOINT_IDS) == 21 and len(set(smpl_mesh.SMPLH_VERTEX_JOINT_IDS)) == 21
    assert max(smpl_mesh.SMPLH_VERTEX_JOINT_IDS) < 6890
    x = torch.from_numpy(make_x(1, 3, "rot6d", True, True, seed=0))
    with pytest.raises(ValueError, match="the model has 40 vertices, but vertex_joint_ids reaches vertex 6787"):
        _full(lib, paths, None)(x=x, mask=None, **CALL)             # the default table on a 40-vertex model
    with pytest.raises(ValueError, match="21 vertices"):
        _full(lib, paths, ids[:20])(x=x, mask=None, **CALL)


def test_index_maps_equal_the_reference_arithmetic():
    from mdm_amd import smpl_mesh
    maps = smpl_mesh.joint_maps()
    _, _, _, ref_maps = fixture_model()                             # the maps model/smpl.py itself built (tools/make_golden_smpl_mesh.py)
    assert set(maps) == set(ref_maps) == {"vibe", "a2m", "smpl", "a2mpl"}
    for k in maps:
        np.testing.assert_array_equal(maps[k], ref_maps[k])
    assert len(maps["vibe"]) == 49 and len(maps["a2m"]) == 18 and maps["a2m"][0] == 0 and maps["vibe"][8] == 0
    assert smpl_mesh.JOINTSTYPE_ROOT == {"a2m": 0, "smpl": 0, "a2mpl": 0, "vibe": 8}
    assert max(maps["vibe"]) == 53 == 24 + 21 + 9 - 1


def test_abi_argument_validation(lib):
    from mdm_amd import _native as nat
    parents = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21], np.int32)
    i32p = C.POINTER(C.c_int32)
    buf = np.zeros(1 << 16, np.float32)
    p = buf.ctypes.data

    def model(**over):
        kw = dict(j0=p, jdirs=p, blend=p, weights_t=p, sel_blend=p, sel_weights_t=p, extra_t=p, parents=parents.ctypes.data_as(i32p),
                  J=24, V=40, n_sel=21, n_extra=9)
        kw.update(over)
        return nat.MdmSmplModel(**kw)

    pmap = np.arange(24, dtype=np.int32)

    def call(**over):
        kw = dict(pose_rep=0, glob=1, translation=1, vertstrans=1, n_points=0, root_point=0, point_map=None, glob_rot_mat=None, beta1=0.0)
        kw.update(over)
        return nat.MdmSmplCall(**kw)

    def err():
        return lib.lib.mdm_last_error().decode()

    def ws(m, c, B=1, T=2):
        return lib.mdm_smpl_workspace_bytes(C.byref(m), C.byref(c), B, T)

    def fwd(m, c, rows=25, feats=6, B=1, T=2, nbytes=1 << 18, x=p, out=p):
        return lib.mdm_smpl_forward(C.byref(m), C.byref(c), x, None, None, out, None, B, T, rows, feats, p, nbytes, None)

    n = ws(model(), call())
    assert n >= 2 * (220 + 288 + 3 + 3 * 54) * 4                    # the header's bound, without the mesh chunk
    with_mesh = ws(model(), call(n_points=1, point_map=np.array([53], np.int32).ctypes.data_as(i32p)))
    assert with_mesh - n == 16 * 32 * 3 * 40 * 4                    # 16 frame tiles of the mesh, whatever B and T are
    assert ws(model(), call(n_points=1, point_map=np.array([53], np.int32).ctypes.data_as(i32p)), B=64, T=60) - ws(model(), call(), B=64, T=60) \
        == 16 * 32 * 3 * 40 * 4
    assert ws(model(J=25), call()) == 0 and "at most 24 joints" in err()
    assert ws(model(V=0), call()) == 0 and "vertex count" in err()
    assert ws(model(n_extra=17), call()) == 0 and "n_extra" in err()
    bad = parents.copy()
    bad[5] = 7
    assert ws(model(parents=bad.ctypes.data_as(i32p)), call()) == 0 and "parents[5] must lie in [0, 5)" in err()
    bad = parents.copy()
    bad[0] = 0
    assert ws(model(parents=bad.ctypes.data_as(i32p)), call()) == 0 and "parents[0] must be -1" in err()
    assert ws(model(), call(pose_rep=4)) == 0 and "pose_rep" in err()
    assert ws(model(), call(glob=0)) == 0 and "glob_rot_mat" in err()
    assert ws(model(), call(n_points=65)) == 0 and "n_points" in err()
    assert ws(model(), call(n_points=24)) == 0 and "point_map" in err()
    assert ws(model(), call(n_points=24, point_map=pmap.ctypes.data_as(i32p), root_point=24)) == 0 and "root_point" in err()
    far = pmap.copy()
    far[3] = 54
    assert ws(model(), call(n_points=24, point_map=far.ctypes.data_as(i32p))) == 0 and "point_map[3] = 54" in err()
    assert ws(model(n_extra=0), call(n_points=1, point_map=np.array([45], np.int32).ctypes.data_as(i32p))) == 0    # no such joint
    assert ws(model(), call(), B=0) == 0 and ws(model(), call(), T=4097) == 0 and "4096 frames" in err()
    # the forward call: the same refusals, then the shapes of x, the tables a map needs and the workspace
    assert fwd(model(J=25), call()) == -5 and "at most 24 joints" in err()
    assert fwd(model(), call(), rows=24) == -1 and "x has 24 rows; need 24 rotation rows and the translation row" in err()
    assert fwd(model(), call(translation=0), rows=25) == -1 and "need 24 rotation rows" in err()
    assert fwd(model(), call(pose_rep=1), feats=6) == -1 and "this pose_rep has 3" in err()
    assert fwd(model(), call(), nbytes=64) == -3 and "workspace too small" in err()
    assert fwd(model(), call(), x=None) == -1 and "null x" in err()
    assert fwd(model(blend=None), call()) == -1 and "blend" in err()
    a2m_like = np.array([0, 30, 50], np.int32).ctypes.data_as(i32p)
    assert fwd(model(extra_t=None), call(n_points=3, point_map=a2m_like)) == -1 and "extra_t" in err()
    assert fwd(model(sel_blend=None), call(n_points=3, point_map=a2m_like)) == -1 and "sel_blend" in err()
    assert fwd(model(blend=None, weights_t=None, sel_blend=None, sel_weights_t=None, extra_t=None),
               call(n_points=24, point_map=pmap.ctypes.data_as(i32p))) == 0       # 'smpl': only the pose tables are needed


def test_old_class_still_refuses():
    """Rotation2xyz -- what model.rot2xyz is -- is unchanged by the full pass living beside it."""
    from mdm_amd.rotation2xyz import Rotation2xyz
    r2x = Rotation2xyz()
    x = torch.zeros(1, 25, 6, 2)
    for kw in (dict(jointstype="vertices"), dict(jointstype="a2m"), dict(pose_rep="rotvec"), dict(glob=False), dict(beta=1),
               dict(translation=False), dict(vertstrans=False), dict(betas=torch.zeros(1, 10)), dict(get_rotations_back=True)):
        args = dict(pose_rep="rot6d", jointstype="smpl", glob=True, translation=True, vertstrans=True)
        args.update(kw)
        with pytest.raises(NotImplementedError, match=r"^rot2xyz: " + list(kw)[0] + "="):
            r2x(x=x, mask=None, **args)
    assert not hasattr(r2x, "maps") and len(list(r2x.smpl_model.state_dict())) == 0
