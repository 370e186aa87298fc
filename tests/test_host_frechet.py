"""mdm_frechet_workspace_bytes / mdm_frechet_distance and their Python seams without a device (the emulator library): every refusal
of the two native calls with its message in mdm_last_error, the ABI version and the header's declarations, the module's ValueErrors by
argument name, the product path's refusal of host data, and the device option of humanml_eval.evaluate_fid (the module switch
FID_ON_DEVICE: the function keeps the reference's parameter list) -- off: the lines and values of an untouched module; on: the device
function's value, within the rule of tests/frechet_helpers.py; unconstrained_eval has the keyword `fid_on_device`."""
import io
import os
import re

import numpy as np
import pytest
import torch

import frechet_helpers as fh
from emu.emu_lib import emu
from mdm_amd import _native as nat
from mdm_amd import metrics as M


@pytest.fixture()
def lib():
    M.NATIVE_LIB = emu()
    yield M.NATIVE_LIB
    M.NATIVE_LIB = None


def test_native_calls_refuse_bad_arguments_with_a_message(lib):
    err = lambda: lib.mdm_last_error().decode()      # noqa: E731
    EINVAL, ENOSPC = -1, -3
    D = 4
    need = lib.mdm_frechet_workspace_bytes(D)
    assert need == 64 + 1024 + 2 * 1024 * 8 + 7 * 16 * 8
    assert lib.mdm_frechet_workspace_bytes(3) == need                      # an odd D has a pad row / column
    assert lib.mdm_frechet_workspace_bytes(1024) == 64 + 1024 + 2 * 1024 * 8 + 7 * 1024 * 1024 * 8
    for bad in (0, -1, 1025):
        assert lib.mdm_frechet_workspace_bytes(bad) == 0 and "between 1 and 1024" in err()
    mu, sigma = np.zeros(8), np.eye(D)
    res, sw, ws = np.zeros(8), np.zeros(2, dtype=np.int32), np.zeros(need, dtype=np.uint8)
    base = dict(mu1=mu.ctypes.data, sigma1=sigma.ctypes.data, mu2=mu.ctypes.data, sigma2=sigma.ctypes.data, D=D, res=res.ctypes.data,
                sw=sw.ctypes.data, ws=ws.ctypes.data, n=need, stream=None)
    call = lambda **o: lib.mdm_frechet_distance(*[{**base, **o}[k] for k in base])      # noqa: E731
    for key, name in (("mu1", "mu1_dev"), ("sigma1", "sigma1_dev"), ("mu2", "mu2_dev"), ("sigma2", "sigma2_dev"), ("res", "result4_dev")):
        assert call(**{key: None}) == EINVAL and f"null {name}" in err()
        assert call(**{key: base[key] + 4}) == EINVAL and f"{name} must be 8-byte aligned" in err()
    assert call(sw=None) == EINVAL and "null sweeps2_dev" in err()
    assert call(sw=base["sw"] + 2) == EINVAL and "sweeps2_dev must be 4-byte aligned" in err()
    for bad in (0, -3, 1025):
        assert call(D=bad) == EINVAL and "D must be between 1 and 1024" in err()
    assert call(ws=None) == EINVAL and "null workspace_dev" in err()
    assert call(n=need - 1) == ENOSPC and "workspace_bytes too small (mdm_frechet_workspace_bytes)" in err()
    assert call(n=0) == ENOSPC
    assert np.array_equal(res, np.zeros(8)) and np.array_equal(sw, np.zeros(2, dtype=np.int32))      # nothing was launched
    assert call() == 0 and res[0] == 0.0 and res[1] == D and sw.tolist() == [0, 0]                 # (the same arguments, unharmed, run)
    assert lib.mdm_abi_version() == 10


def test_both_names_are_declared_and_exported(lib):
    src = open(os.path.join(fh.ROOT, "include", "mdm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("mdm_frechet_workspace_bytes", "mdm_frechet_distance"):
        assert re.search(r"\b" + name + r"\s*\(", src) and name in nat.EXPORTED_SYMBOLS and hasattr(lib.lib, name)
    assert "#define MDM_ABI_VERSION 10" in src and nat.ABI_VERSION == 10
    assert "mdm_frechet" not in open(os.path.join(fh.ROOT, "include", "mdm_hip_probe.h")).read()
    assert lib.mdm_metrics_workspace_bytes(9, 8, 1) == 0                   # no metrics kind was added for it


def test_the_module_refuses_bad_arguments_by_name(lib):
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)      # noqa: E731
    with pytest.raises(ValueError, match="mean vectors have different lengths"):
        M.frechet_distance_device(f64(3), f64(3, 3), f64(4), f64(3, 3))
    with pytest.raises(ValueError, match="covariances have different dimensions"):
        M.frechet_distance_device(f64(3), f64(3, 3), f64(3), f64(4, 4))
    with pytest.raises(ValueError, match="mu1 must be .D. and sigma1 .D, D."):
        M.frechet_distance_device(f64(3), f64(4, 4), f64(3), f64(4, 4))
    with pytest.raises(ValueError, match="sigma2 must be float64"):
        M.frechet_distance_device(f64(3), f64(3, 3), f64(3), torch.zeros(3, 3))
    with pytest.raises(ValueError, match="mu2 must be a tensor"):
        M.frechet_distance_device(f64(3), f64(3, 3), np.zeros(3), f64(3, 3))
    with pytest.raises(nat.MdmError, match="between 1 and 1024"):
        M.frechet_distance_device(f64(1025), f64(1025, 1025), f64(1025), f64(1025, 1025))
    eye = torch.eye(3, dtype=torch.float64)
    assert M.calculate_fid_device((f64(3), eye), (f64(3), eye)).item() == 0.0
    assert M.frechet_distance_device(f64(3), eye, f64(3) + 1.0, eye, check=False).item() == 3.0
    from mdm_amd import humanml_metrics as hm
    assert hm.frechet_distance_device is M.frechet_distance_device and hm.calculate_fid_device is M.calculate_fid_device


def test_product_path_refuses_host_data(monkeypatch):
    class Product:
        path = "/somewhere/" + nat.LIB_NAME
    monkeypatch.setattr(M, "NATIVE_LIB", Product())
    eye = torch.eye(3, dtype=torch.float64)
    with pytest.raises(nat.MdmError, match="cuda"):
        M.frechet_distance_device(torch.zeros(3, dtype=torch.float64), eye, torch.zeros(3, dtype=torch.float64), eye)
    with pytest.raises(nat.MdmError, match="sigma1 on a cuda"):
        M.frechet_distance_device(torch.zeros(3, dtype=torch.float64), np.eye(3), torch.zeros(3, dtype=torch.float64), eye)


class _Wrapper:
    """eval_wrapper stand-in: the "embedding" of a motion batch is the batch."""
    def get_motion_embeddings(self, motions, m_lens):
        return motions


def test_evaluate_fid_keeps_its_lines_and_values_with_the_option_off(lib, capsys, monkeypatch):
    """32 rows of 16 features per set.  Off (set, and as the module is imported): the same printed and logged lines, the same
    floats.  On: the device function's .item(), within max(100 d, 1e-11 S) of the default path's."""
    from mdm_amd import humanml_eval as he
    x_gt, x_gen = fh.make_sets(16, 32, 7501)
    gt_loader = [(None, None, None, None, torch.from_numpy(x_gt[i:i + 16]), None, None) for i in (0, 16)]
    acts = {"ground truth": torch.from_numpy(x_gt), "vald": torch.from_numpy(x_gen)}
    runs = {}
    assert he.FID_ON_DEVICE is False
    for key, switch in (("plain", None), ("off", False), ("on", True)):
        if switch is not None:
            monkeypatch.setattr(he, "FID_ON_DEVICE", switch)
        log = io.StringIO()
        values = he.evaluate_fid(_Wrapper(), gt_loader, acts, log)
        runs[key] = (values, capsys.readouterr().out, log.getvalue())
    assert runs["off"] == runs["plain"] and list(runs["plain"][0]) == ["ground truth", "vald"]
    assert "========== Evaluating FID ==========" in runs["plain"][1] and "---> [vald] FID: " in runs["plain"][2]
    s_gt, s_gen = fh.stats_fp64(x_gt), fh.stats_fp64(x_gen)
    d = abs(runs["plain"][0]["vald"] - fh.frechet_eigh(*s_gt, *s_gen)[0])
    S = fh.scale_of(*s_gt, *s_gen)
    for name in acts:
        on, off = runs["on"][0][name], runs["plain"][0][name]
        print(f"[frechet] evaluate_fid {name}: |on - off| / S {abs(on - off) / S:.3e}  d / S {d / S:.3e}")
        assert isinstance(on, float) and abs(on - off) <= fh.bound(d, S)
    assert abs(runs["on"][0]["ground truth"]) <= 1e-11 * S
    assert [ln[:12] for ln in runs["on"][1].splitlines()] == [ln[:12] for ln in runs["plain"][1].splitlines()]
    import inspect
    assert "fid_on_device" not in inspect.signature(he.evaluation).parameters      # (the reference's parameter lists stay)
    from mdm_amd import unconstrained_eval as ue
    assert inspect.signature(ue.evaluate_unconstrained_metrics).parameters["fid_on_device"].default is False
