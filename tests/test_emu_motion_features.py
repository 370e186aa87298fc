"""csrc/motion_features.h compiled for the CPU lock-step emulator (tests/emu) and driven through the C ABI (mdm_joints_to_features)
by mdm_amd.motion_process, on a subset of the fixtures of tests/golden/motion_features_*.npz: T in {2, 4, 82, 258} for both
skeletons, the ragged batch with NaN beyond each length, the adversarial foot case and the process_file cases.  Bounds: see
tests/motion_features_helpers.py (device against oracle: fp32 rounding of the store; against the reference: 2 * d_ref; foot flags:
no mismatch)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

from emu_lib import emu, ptr  # noqa: E402
import motion_features_helpers as mh  # noqa: E402

SUBSET = [f"{ds}_T{T}" for ds in ("humanml", "kit") for T in mh.EMU_T] + \
         ["humanml_ragged", "humanml_foot", "kit_foot", "humanml_process", "humanml_retarget", "kit_process", "kit_retarget"]


@pytest.fixture(scope="module")
def lib():
    return emu()


@pytest.fixture(scope="module")
def report():
    return mh.pin_report()


@pytest.mark.parametrize("name", SUBSET)
def test_emulated_case(lib, report, name):
    d = mh.load_case(name)
    mh.check_case(name, d, mh.run_case(name, d, "cpu", lib), report)


def test_emulated_interface_forms_agree_and_leave_their_input_alone(lib):
    """extract_features / process_file with numpy and tensor arguments, both layouts, normalisation, a subset of the canonicalising
    steps, a clip alone against the same clip inside a batch of 65 (two launches)."""
    from mdm_amd import motion_process as mp
    tab, sk = mp.SKELETONS["kit"], mh.SKELETONS["kit"]
    d = mh.load_case("kit_T41")
    P = d["joints"]
    keep = P.copy()
    args = (tab["feet_thre"], torch.tensor(tab["raw_offsets"]), tab["kinematic_chain"], tab["face_joint_indx"], tab["fid_r"], tab["fid_l"])
    a = mp.extract_features(P, *args, _native_lib=lib)
    pt = torch.from_numpy(P)
    b = mp.extract_features(pt, *args, _native_lib=lib)
    assert isinstance(a, np.ndarray) and torch.is_tensor(b) and a.shape == (40, 251) and np.array_equal(a, b.numpy())
    assert np.array_equal(P, keep) and np.array_equal(pt.numpy(), keep)              # the reference subtracts the root's xz in place
    x = torch.from_numpy(mh.to_bj3t(P))
    base = mp.joints_to_features(x, dataset="kit", canonicalise=False, _native_lib=lib)
    assert base.shape == (1, 251, 1, 40) and np.array_equal(base[0, :, 0].t().numpy(), a)
    assert torch.equal(mp.joints_to_features(pt[None], dataset="kit", canonicalise=False, layout="btj3", _native_lib=lib), base)
    # (x - mean) / std, in fp64 before the one rounding
    rng = np.random.default_rng(3)
    mean, std = rng.normal(size=251).astype(np.float32), rng.uniform(0.5, 2.0, 251).astype(np.float32)
    got = mp.joints_to_features(x, dataset="kit", mean=mean, std=std, canonicalise=False, _native_lib=lib)[0, :, 0].t().numpy()
    want = (d["fp64_data"] - mean.astype(np.float64)) / std.astype(np.float64)
    for g, s in mh.groups(21).items():
        assert np.abs(got[:, s] - want[:, s]).max() <= mh.oracle_tol(want[:, s]), g
    # process_file, numpy in -> numpy out, argument untouched; then two of its three steps against the oracle
    res = mp.process_file(P, tab["feet_thre"], dataset="kit", _native_lib=lib)
    assert all(isinstance(r, np.ndarray) for r in res) and [r.shape for r in res] == [(40, 251), (41, 21, 3), (41, 21, 3), (40, 2)]
    assert np.array_equal(P, keep)
    full = mp.joints_to_features(x, dataset="kit", _native_lib=lib)
    assert np.array_equal(full[0, :, 0].t().numpy(), res[0])
    part = mp.joints_to_features(x, dataset="kit", canonicalise=("floor", "face_z"), _native_lib=lib)[0, :, 0].t().numpy()
    G = mh.canonicalise(sk, P, origin_xz=False)
    want = mh.extract(sk, G, sk["feet_thre"])[0]
    for g, s in mh.groups(21).items():
        assert np.abs(part[:, s] - want[:, s]).max() <= mh.oracle_tol(want[:, s]), g
    # batch invariance across the 64-clip launches
    d2 = mh.load_case("humanml_T4")
    x2 = torch.from_numpy(mh.to_bj3t(d2["joints"]))
    alone = mp.joints_to_features(x2, _native_lib=lib)
    many = mp.joints_to_features(x2.repeat(65, 1, 1, 1), lengths=[4] * 64 + [3], _native_lib=lib)
    assert torch.equal(many[0], alone[0]) and torch.equal(many[63], alone[0])
    assert torch.equal(many[64, :, :, :2].isfinite(), torch.ones_like(many[64, :, :, :2], dtype=torch.bool)) and not many[64, :, :, 2].any()


def test_emulated_ragged_batch_is_batch_invariant_and_ignores_the_poison(lib):
    from mdm_amd import motion_process as mp
    d = mh.load_case("humanml_ragged")
    x = torch.from_numpy(mh.to_bj3t(d["joints"]))
    assert x.isnan().any()
    both = mp.joints_to_features(x, lengths=d["lengths"], canonicalise=True, _native_lib=lib)
    assert both.isfinite().all()
    for b, L in enumerate(d["lengths"]):
        clip = x[b:b + 1, :, :, :L].contiguous()
        alone = mp.joints_to_features(clip, canonicalise=True, _native_lib=lib)
        assert torch.equal(alone[0], both[b, :, :, :L - 1]) and not both[b, :, :, L - 1:].any()


def test_c_abi_refusals(lib):
    from mdm_amd import _native as nat
    from mdm_amd import motion_process as mp
    tab = mp.SKELETONS["humanml"]
    sk = mp._skeleton_struct(tab["raw_offsets"], tab["kinematic_chain"], tab["face_joint_indx"], tab["fid_r"], tab["fid_l"], 5, 8)
    call = nat.MdmJointsToFeaturesCall(layout=0, feet_thre=0.002)
    B, T = 2, 6
    x = np.zeros((B, 22, 3, T), dtype=np.float32)
    out = np.zeros((B, 263, 1, T - 1), dtype=np.float32)

    def run(sk_=sk, call_=call, x_=ptr(x), lengths=None, out_=ptr(out), B_=B, T_=T, F=263, ws=None, ws_bytes=0):
        arr = None if lengths is None else (C.c_int32 * len(lengths))(*lengths)
        return lib.mdm_joints_to_features(C.byref(sk_) if sk_ is not None else None, C.byref(call_), x_, arr, out_, B_, T_, F, ws, ws_bytes, None)
    assert lib.mdm_abi_version() == 10
    assert run(lengths=[6, 1]) == -1 and b"lengths[1]" in lib.mdm_last_error()
    assert run(lengths=[7, 6]) == -1 and b"lengths[0]" in lib.mdm_last_error()
    assert run(F=251) == -1 and b"F must be" in lib.mdm_last_error()
    assert run(x_=None) == -1 and run(out_=None) == -1 and run(sk_=None) == -1
    assert run(T_=1) == -1
    assert run(T_=1025) == -5 and b"1024 frames" in lib.mdm_last_error()
    canon = nat.MdmJointsToFeaturesCall(layout=0, feet_thre=0.002, floor=1)
    assert run(call_=canon) == -1 and b"workspace" in lib.mdm_last_error()
    need = lib.mdm_joints_to_features_workspace_bytes(B, T, 22)
    assert need >= B * 22 * 3 * T * 8 and lib.mdm_joints_to_features_workspace_bytes(0, T, 22) == 0
    ws = np.zeros(need, dtype=np.uint8)
    assert run(call_=canon, ws=ptr(ws), ws_bytes=need - 1) == -3
    bad = mp._skeleton_struct(tab["raw_offsets"], tab["kinematic_chain"][:4], tab["face_joint_indx"], tab["fid_r"], tab["fid_l"], 5, 8)
    assert run(sk_=bad) == -1 and b"is on no chain" in lib.mdm_last_error()
    half = nat.MdmJointsToFeaturesCall(layout=0, feet_thre=0.002, mean_dev=ptr(out))
    assert run(call_=half) == -1 and b"mean_dev and std_dev" in lib.mdm_last_error()
