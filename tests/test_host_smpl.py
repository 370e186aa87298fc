"""Host logic of mdm_amd/rotation2xyz.py (no GPU): the SMPL model loader (plain, scipy-sparse and chumpy-holding pickles), the
missing-file error, the refusals, the 'xyz' passthrough, the state-dict contract, and the argument validation of
mdm_rot6d_to_smpl_joints in the gfx950 library loaded without a device."""
import ctypes as C
import os
import pickle
import sys
import types

import numpy as np
import pytest
import scipy.sparse
import torch

from helpers import make_pair
from oracle.synth import synth_a2m_state_dict, synth_state_dict
from smpl_helpers import CALLER_KW, SMPL_PARENTS, rest_tables, synthetic_model, write_smpl_model


def _load(path):
    from mdm_amd.rotation2xyz import load_smpl_tables
    return load_smpl_tables(path)


def _check_tables(fields, rest, parents):
    want_rest, want_parents = rest_tables(fields)
    assert rest.dtype == np.float32 and rest.shape == (24, 3) and parents.dtype == np.int32
    assert np.array_equal(parents, SMPL_PARENTS) and np.array_equal(parents, want_parents)
    assert np.array_equal(rest, want_rest.astype(np.float32))      # computed in float64, stored as fp32


def test_loader_plain_pickle(tmp_path):
    fields = synthetic_model(0)
    _check_tables(fields, *_load(write_smpl_model(tmp_path, fields)))


def test_loader_scipy_sparse_regressor(tmp_path):
    fields = synthetic_model(1)
    fields["J_regressor"] = scipy.sparse.csc_matrix(np.where(fields["J_regressor"] > 0.03, fields["J_regressor"], 0.0))
    _check_tables(fields, *_load(write_smpl_model(tmp_path, fields)))


def _fake_chumpy():
    """A stand-in chumpy (module chumpy.ch, class Ch) importable while pickling only."""
    mod = types.ModuleType("chumpy.ch")

    class Ch:
        def __init__(self, x):
            self.x = x

        def __getstate__(self):
            return {"x": self.x, "_dirty_vars": set()}

    Ch.__module__, Ch.__qualname__ = "chumpy.ch", "Ch"
    mod.Ch = Ch
    pkg = types.ModuleType("chumpy")
    pkg.ch = mod
    return pkg, mod, Ch


def _pickle_with_chumpy(tmp_path, fields, chumpy_keys, monkeypatch):
    pkg, mod, Ch = _fake_chumpy()
    with monkeypatch.context() as m:
        m.setitem(sys.modules, "chumpy", pkg)
        m.setitem(sys.modules, "chumpy.ch", mod)
        fields = {k: (Ch(v) if k in chumpy_keys else v) for k, v in fields.items()}
        path = write_smpl_model(tmp_path, fields)
    assert "chumpy" not in sys.modules and "chumpy.ch" not in sys.modules
    return path


def test_loader_chumpy_fields_without_chumpy(tmp_path, monkeypatch):
    """The official file holds chumpy objects in fields this path never reads (shapedirs, ...): they load as inert placeholders."""
    fields = synthetic_model(2)
    path = _pickle_with_chumpy(tmp_path, fields, {"shapedirs", "weights"}, monkeypatch)
    _check_tables(fields, *_load(path))
    assert "chumpy" not in sys.modules


def test_loader_refuses_a_required_chumpy_field(tmp_path, monkeypatch):
    path = _pickle_with_chumpy(tmp_path, synthetic_model(3), {"v_template"}, monkeypatch)
    with pytest.raises(ValueError, match=r"v_template.*chumpy.*clean_ch"):
        _load(path)


def test_loader_refuses_foreign_classes(tmp_path):
    path = write_smpl_model(tmp_path, {**synthetic_model(4), "extra": types.SimpleNamespace(a=1)})
    with pytest.raises(pickle.UnpicklingError, match="types.SimpleNamespace"):
        _load(path)


def test_missing_smpl_file_names_path_and_download_script(tmp_path, monkeypatch):
    from mdm_amd.rotation2xyz import Rotation2xyz
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match=r"body_models/smpl/SMPL_NEUTRAL\.pkl.*prepare/download_smpl_files\.sh"):
        Rotation2xyz()(x=torch.zeros(1, 25, 6, 4), mask=None, **CALLER_KW)


@pytest.mark.parametrize("arg,value", [("pose_rep", "rotvec"), ("pose_rep", "rotmat"), ("pose_rep", "rotquat"),
                                       ("jointstype", "vertices"), ("jointstype", "a2m"), ("jointstype", "a2mpl"),
                                       ("jointstype", "vibe"), ("glob", False), ("translation", False), ("vertstrans", False),
                                       ("beta", 1), ("betas", torch.zeros(4, 10)), ("get_rotations_back", True)])
def test_every_refusal_names_its_argument(tmp_path, monkeypatch, arg, value):
    from mdm_amd.rotation2xyz import Rotation2xyz
    monkeypatch.chdir(tmp_path)                                   # (no SMPL file: refusals come first)
    with pytest.raises(NotImplementedError, match=rf"^rot2xyz: {arg}="):
        Rotation2xyz()(x=torch.zeros(1, 25, 6, 4), mask=None, **{**CALLER_KW, arg: value})


def test_xyz_passthrough_never_opens_a_file(monkeypatch):
    import builtins
    from mdm_amd.rotation2xyz import Rotation2xyz

    def no_open(*a, **k):
        raise AssertionError("pose_rep='xyz' opened a file")
    r2x = Rotation2xyz(model_path="/nonexistent/SMPL_NEUTRAL.pkl")
    monkeypatch.setattr(builtins, "open", no_open)
    x = torch.randn(2, 22, 3, 5)
    assert r2x(x, mask=None, pose_rep="xyz", glob=True, translation=True, jointstype="smpl", vertstrans=True) is x
    assert r2x(x, pose_rep="xyz") is x
    assert r2x._tables is None


def test_rot2xyz_adds_no_state_dict_keys():
    from mdm_amd.rotation2xyz import Rotation2xyz
    sd = synth_state_dict(0, num_layers=1)
    model, _ = make_pair(sd, 50, "cpu", guided=True)
    assert isinstance(model.rot2xyz, Rotation2xyz) and model.rot2xyz is model.model.rot2xyz
    assert not any(k.startswith("rot2xyz") for k in model.model.state_dict())
    assert "rot2xyz" not in dict(model.model.named_modules())
    sm = model.rot2xyz.smpl_model
    assert isinstance(sm, torch.nn.Module) and not list(sm.parameters()) and not list(sm.buffers())
    assert sm.eval() is sm                                        # train/train_mdm.py:47
    a2m, _ = make_pair(synth_a2m_state_dict(seed=0, latent_dim=256, num_layers=1), 50, "cpu", guided=False,
                       dataset="humanact12", num_actions=12)
    want = set(synth_a2m_state_dict(seed=0, latent_dim=256, num_layers=1))
    assert want <= set(a2m.state_dict())
    assert {k for k in set(a2m.state_dict()) - want if not k.endswith("sequence_pos_encoder.pe")} == set()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mdm_amd import _native
    return _native.MdmLib(_native.LIB_PATH)


def test_smpl_joints_entry_point_validates_before_touching_the_device(lib):
    """mdm_rot6d_to_smpl_joints: every refusal comes before any launch (no device here), with a message."""
    rest = (C.c_float * 72)(*([0.1] * 72))
    par = (C.c_int32 * 24)(*SMPL_PARENTS)
    buf = (C.c_float * 16)()
    p = C.addressof(buf)

    def call(x=p, mask=None, rest_=rest, par_=par, out=p, B=2, T=60, nin=25, J=24):
        return lib.mdm_rot6d_to_smpl_joints(x, mask, rest_, par_, out, B, T, nin, J, None)

    for kw, rc in ((dict(x=None), -1), (dict(out=None), -1), (dict(rest_=None), -1), (dict(par_=None), -1),
                   (dict(B=0), -1), (dict(T=0), -1), (dict(J=0, nin=1), -1), (dict(nin=24), -1), (dict(nin=26), -1),
                   (dict(J=25, nin=26), -5), (dict(T=4097), -5), (dict(B=1 << 20, T=4096), -5)):
        assert call(**kw) == rc, kw
        assert lib.mdm_last_error()
    bad_root = (C.c_int32 * 24)(*([0] + SMPL_PARENTS[1:]))
    assert call(par_=bad_root) == -1 and b"parents[0]" in lib.mdm_last_error()
    for i, v in ((1, -1), (5, 5), (7, 9)):
        bad = list(SMPL_PARENTS)
        bad[i] = v
        assert call(par_=(C.c_int32 * 24)(*bad)) == -1 and f"parents[{i}]".encode() in lib.mdm_last_error()
