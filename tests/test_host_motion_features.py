"""joints -> features, the host side (no GPU, no kernel): the fp64 oracle of tests/motion_features_helpers.py against the fixtures the
reference wrote (tests/make_golden_motion_features.py), the skeleton tables, the refusals of the Python interface, and that
nothing modifies its argument."""
import os

import numpy as np
import pytest
import torch

import motion_features_helpers as mh

CASES = list(mh.case_names())


@pytest.fixture(scope="module")
def report():
    return mh.pin_report()


@pytest.mark.parametrize("name", CASES)
def test_oracle_against_the_fixture(name, report):
    """The oracle recomputed from the stored joints: equal to the stored oracle output, within d_ref of the stored reference output
    (d_ref is what the generator measured, so this pins both), foot flags equal; T = 3: as far from the reference as recorded."""
    c = mh.case_names()[name]
    sk = mh.SKELETONS[c["dataset"]]
    with np.load(os.path.join(mh.GOLDEN, f"motion_features_{name}.npz")) as z:
        d = {k: z[k] for k in z.files}
    assert d["joints"].dtype == np.float32
    before = d["joints"].copy()
    orc = mh.oracle_case(name, d["joints"], d.get("tgt_offsets"))
    assert np.array_equal(before, d["joints"], equal_nan=True)                  # the oracle leaves its input alone
    assert orc["fp64_data"].shape[-1] == mh.feat_dim(sk["joints"]) == {22: 263, 21: 251}[sk["joints"]]
    assert ("fp64_data" in d) == (c["T"] <= mh.STORE_ORACLE_MAX_T)
    for k in orc:
        if k in d:
            assert np.abs(orc[k] - d[k]).max() <= 1e-12, (name, k)
    entry = report["cases"][name]
    if c["T"] == 3:
        assert "ref_data" not in d and "d_ref" not in entry
        assert min(entry["reference_differs"].values()) > 1e-2             # the reference's frame-axis cross: not an fp32 difference
        return
    err = mh.group_errors(d["ref_data"], orc["fp64_data"], sk["joints"])
    assert err["feet"] == 0.0
    for g, v in entry["d_ref"].items():
        assert err[g] <= v * (1 + 1e-9) + 1e-18, (name, g, err[g], v)
        assert v <= report["bounds"]["scale"] * max(1.0, entry["magnitude"][g]) / min(1.0, entry.get("conditions", {}).get("w_min", mh.W_MIN))
    if c["kind"] == "process":
        rt = float(np.abs(mh.recover_from_ric(orc["fp64_data"], sk["joints"]) - orc["fp64_global"][:-1]).max())
        assert abs(rt - entry["round_trip_fp64"]) <= 1e-12 and entry["round_trip_ref"] > 0


@pytest.mark.parametrize("name", [n for n, c in mh.case_names().items() if c["kind"] in ("extract", "process")])
def test_fixture_inputs_meet_the_yardstick_conditions(name):
    c = mh.case_names()[name]
    d = mh.load_case(name)
    got = mh.check_conditions(c["dataset"], d["joints"], mh.SKELETONS[c["dataset"]]["feet_thre"], d.get("tgt_offsets"), canon=c["kind"] == "process")
    assert got["w_min"] >= mh.W_MIN and got["foot_margin"] >= mh.FOOT_MARGIN and got["bone_min"] > 0


@pytest.mark.parametrize("dataset", ["humanml", "kit"])
def test_adversarial_foot_fixture_sits_on_the_threshold(dataset, report):
    sk = mh.SKELETONS[dataset]
    d = mh.load_case(f"{dataset}_foot")
    flags, sums = mh.foot_flags(sk, d["joints"], sk["feet_thre"])
    centre = np.float32(sk["feet_thre"])
    for target in (centre, np.nextafter(centre, np.float32(0)), np.nextafter(centre, np.float32(1))):
        assert (sums == target).sum() >= 30
    assert np.array_equal(flags, d["ref_data"][:, -4:])                          # the expected flags are the reference's
    # the fp32 number nearest the threshold is not below it as a double: only the lower neighbour counts as planted
    assert flags.sum() == (sums.astype(np.float64) < sk["feet_thre"]).sum() == report["cases"][f"{dataset}_foot"]["foot_sums"]["flags_set"]


def test_skeleton_tables():
    from mdm_amd import motion_process as mp
    assert sorted(mp.SKELETONS) == sorted(mh.SKELETONS)
    for ds, want in mh.SKELETONS.items():
        tab = mp.SKELETONS[ds]
        assert tab["joints"] == want["joints"] and tab["feet_thre"] == want["feet_thre"]
        assert tab["kinematic_chain"] == want["chains"] and tab["raw_offsets"] == want["raw"]
        assert tab["face_joint_indx"] == want["face"] and tab["fid_r"] == want["fid_r"] and tab["fid_l"] == want["fid_l"]
        assert (tab["l_idx1"], tab["l_idx2"]) == (want["l_idx1"], want["l_idx2"])
        J = tab["joints"]
        assert mp.feature_dim(J) == mh.feat_dim(J)
        reached = [j for ch in tab["kinematic_chain"] for j in ch[1:]]
        assert sorted(reached) == list(range(1, J)) and tab["kinematic_chain"][0][0] == 0          # every joint once, root first
        raw = np.asarray(tab["raw_offsets"])
        assert raw.shape == (J, 3) and not raw[0].any() and (np.abs(raw[1:]).sum(axis=1) == 1).all()   # unit axes
        sk = mp._skeleton_struct(tab["raw_offsets"], tab["kinematic_chain"], tab["face_joint_indx"], tab["fid_r"], tab["fid_l"],
                                 tab["l_idx1"], tab["l_idx2"])
        assert sk.joints == J and sk.n_chains == 5 and list(sk.chains[3])[:sk.chain_len[3]] == tab["kinematic_chain"][3]


def test_refusals_name_the_argument():
    """Every refusal comes before the library is touched (`_native_lib` is a stand-in that has nothing)."""
    from mdm_amd import motion_process as mp
    lib = object()
    x = torch.zeros(2, 22, 3, 8)
    for kwargs, match in ((dict(dataset="h36m"), "dataset"), (dict(layout="tbj3"), "layout"), (dict(lengths=[8]), "lengths"),
                          (dict(lengths=[8, 1]), "lengths"), (dict(lengths=[9, 8]), "lengths"), (dict(dataset="kit"), "joints"),
                          (dict(mean=np.zeros(263)), "mean and std"), (dict(mean=np.zeros(251), std=np.ones(251)), "mean / std"),
                          (dict(tgt_offsets=np.zeros((21, 3))), "tgt_offsets"), (dict(feet_thre=0.0), "feet_thre"),
                          (dict(canonicalise=("floor", "spin")), "canonicalise"), (dict(layout="btj3"), "joints")):
        with pytest.raises(ValueError, match=match):
            mp.joints_to_features(x, _native_lib=lib, **kwargs)
    with pytest.raises(ValueError, match="joints"):
        mp.joints_to_features(torch.zeros(2, 22, 3, 1), _native_lib=lib)
    with pytest.raises(ValueError, match="at most 1024 frames"):
        mp.joints_to_features(torch.zeros(1, 22, 3, 1025), _native_lib=lib)
    with pytest.raises(ValueError, match="joints must be a tensor"):
        mp.joints_to_features(np.zeros((2, 22, 3, 8), dtype=np.float32), _native_lib=lib)
    tab = mp.SKELETONS["humanml"]
    args = (tab["raw_offsets"], tab["kinematic_chain"], tab["face_joint_indx"], tab["fid_r"], tab["fid_l"])
    with pytest.raises(ValueError, match="positions"):
        mp.extract_features(np.zeros((8, 21, 3)), 0.002, *args, _native_lib=lib)
    with pytest.raises(ValueError, match="n_raw_offsets"):
        mp.extract_features(np.zeros((8, 22, 3)), 0.002, np.zeros((30, 3)), *args[1:], _native_lib=lib)
    with pytest.raises(ValueError, match="kinematic_chain"):
        mp.extract_features(np.zeros((8, 22, 3)), 0.002, args[0], [[0]], *args[2:], _native_lib=lib)
    with pytest.raises(ValueError, match="positions"):
        mp.process_file(np.zeros((8, 22, 3)), 0.05, dataset="kit", _native_lib=lib)
