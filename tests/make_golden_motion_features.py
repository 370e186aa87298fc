"""Writes tests/golden/motion_features_<case>.npz and tests/golden/PIN_REPORT_motion_features.json.

Run on the CPU, with the reference checkout's path:   python tests/make_golden_motion_features.py /path/to/motion-diffusion-model

The reference's own data_loaders/humanml/scripts/motion_process.py (extract_features, process_file, recover_from_ric) is IMPORTED
here, at generation time only, and run on COPIES of the inputs tests/motion_features_helpers.py builds (the reference mutates its
argument); the files hold data only: the fp32 joints, the reference's outputs and (up to 82 frames) the fp64 oracle's.  numpy 2 dropped the
`np.float` alias the reference uses, so this process sets it first; process_file reads its skeleton tables from module globals,
which are injected here; for the cases without a target skeleton its uniform_skeleton step is replaced by the identity.

The report records, per case and feature group (root, ric, rot6d, local_velocity), d_ref = max|reference - oracle|, the foot-flag
mismatches (asserted zero), the measured yardstick conditions, and for the process cases the reference's own round trip
max|recover_from_ric(process_file(x).data) - global_positions[:-1]|.  For T = 3 the reference crosses along the frame axis inside
qbetween (torch.cross without dim): its output is not stored, only how far it is from the oracle.  The generator fails if the
oracle is not within the reference's fp32 error scale of the reference: SCALE * max(1, max|group|) / w_min."""
import json
import os
import sys
import warnings

import numpy as np

np.float = float                                        # noqa: the alias numpy 2 removed (motion_process.py:55)

import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import motion_features_helpers as mh  # noqa: E402

SCALE = 2e-5        # ~ 300 fp32 epsilons: a chain of five fp32 quaternion products and a rotation of metre-sized vectors


def inject(mp, sk, tgt):
    mp.n_raw_offsets = torch.from_numpy(np.asarray(sk["raw"], dtype=np.int64))
    mp.kinematic_chain = sk["chains"]
    mp.face_joint_indx = sk["face"]
    mp.fid_r, mp.fid_l = sk["fid_r"], sk["fid_l"]
    mp.l_idx1, mp.l_idx2 = sk["l_idx1"], sk["l_idx2"]
    mp.tgt_offsets = None if tgt is None else torch.from_numpy(np.asarray(tgt, dtype=np.float32))


def ref_extract(mp, sk, P32):
    inject(mp, sk, None)
    return mp.extract_features(P32.copy(), sk["feet_thre"], mp.n_raw_offsets, sk["chains"], sk["face"], sk["fid_r"], sk["fid_l"])


def main(ref_root):
    sys.path.insert(0, ref_root)
    warnings.filterwarnings("ignore")
    from data_loaders.humanml.scripts import motion_process as mp
    real_uniform = mp.uniform_skeleton
    torch.set_num_threads(2)
    report = {"cases": {}, "bounds": {"oracle_tol": "4 * 2^-24 * max|group|", "reference": "2 * d_ref", "w_min": mh.W_MIN,
                                      "foot_margin": mh.FOOT_MARGIN, "scale": SCALE}}
    os.makedirs(mh.GOLDEN, exist_ok=True)
    for name, c in mh.case_names().items():
        sk = mh.SKELETONS[c["dataset"]]
        J = sk["joints"]
        joints, tgt = mh.case_input(name)
        orc = mh.oracle_case(name, joints, tgt)
        entry = {"kind": c["kind"], "dataset": c["dataset"], "T": c["T"]}
        save = {"joints": joints}
        if c["kind"] == "process":
            inject(mp, sk, tgt)
            mp.uniform_skeleton = real_uniform if tgt is not None else (lambda positions, target_offset: positions)
            data, G, ric, lv = mp.process_file(joints.copy(), sk["feet_thre"])
            mp.uniform_skeleton = real_uniform
            rec = mp.recover_from_ric(torch.from_numpy(np.asarray(data)).unsqueeze(0).float(), J)[0].numpy()
            entry["round_trip_ref"] = float(np.abs(rec.astype(np.float64) - np.asarray(G, dtype=np.float64)[:-1]).max())
            entry["round_trip_fp64"] = float(np.abs(mh.recover_from_ric(orc["fp64_data"], J) - orc["fp64_global"][:-1]).max())
            entry["d_ref_global"] = float(np.abs(np.asarray(G, dtype=np.float64) - orc["fp64_global"]).max())
            entry["d_ref_ric_positions"] = float(np.abs(np.asarray(ric, dtype=np.float64) - orc["fp64_ric"]).max())
            entry["conditions"] = mh.check_conditions(c["dataset"], joints, sk["feet_thre"], tgt, canon=True)
            save.update(ref_data=np.asarray(data, dtype=np.float64), ref_global=np.asarray(G, dtype=np.float32),
                        ref_ric=np.asarray(ric, dtype=np.float32), ref_l_velocity=np.asarray(lv, dtype=np.float64))
            if tgt is not None:
                save["tgt_offsets"] = tgt
            ref = np.asarray(data, dtype=np.float64)
        elif c["kind"] == "ragged":
            ref = np.zeros_like(orc["fp64_data"])
            for b, L in enumerate(mh.RAGGED_LENGTHS):
                ref[b, :L - 1] = ref_extract(mp, sk, joints[b, :L])
            entry["lengths"] = list(mh.RAGGED_LENGTHS)
            save.update(ref_data=ref, lengths=np.asarray(mh.RAGGED_LENGTHS, dtype=np.int32))
        else:
            ref = np.asarray(ref_extract(mp, sk, joints), dtype=np.float64)
            entry["conditions"] = mh.check_conditions(c["dataset"], joints, sk["feet_thre"], foot=c["kind"] != "foot")
            if c["T"] != 3:
                save["ref_data"] = ref
        err = mh.group_errors(ref, orc["fp64_data"], J)
        g = mh.groups(J)
        entry["feet_mismatches"] = int((ref[..., g["feet"]] != orc["fp64_data"][..., g["feet"]]).sum())
        assert entry["feet_mismatches"] == 0, (name, entry)
        entry["magnitude"] = {k: float(np.abs(orc["fp64_data"][..., s]).max()) for k, s in g.items() if k != "feet"}
        if c["T"] == 3:
            entry["reference_differs"] = {k: v for k, v in err.items() if k != "feet"}
            entry["note"] = "qbetween crosses along the frame axis in the reference for a clip of 3 frames: compared with the oracle only"
        else:
            entry["d_ref"] = {k: v for k, v in err.items() if k != "feet"}
            w_min = entry.get("conditions", {}).get("w_min", mh.W_MIN)
            for k, v in entry["d_ref"].items():
                assert v <= SCALE * max(1.0, entry["magnitude"][k]) / min(1.0, w_min), (name, k, v, entry)
        if c["kind"] == "foot":
            _, sums = mh.foot_flags(sk, joints, sk["feet_thre"])
            centre = np.float32(sk["feet_thre"])
            entry["foot_sums"] = {"on": int((sums == centre).sum()), "below": int((sums == np.nextafter(centre, np.float32(0))).sum()),
                                  "above": int((sums == np.nextafter(centre, np.float32(1))).sum()),
                                  "flags_set": int(ref[..., g["feet"]].sum())}
        if c["T"] <= mh.STORE_ORACLE_MAX_T:          # the long clips' oracle outputs are recomputed by mh.load_case: the files stay small
            save.update(orc)
        np.savez_compressed(os.path.join(mh.GOLDEN, f"motion_features_{name}.npz"), **save)
        report["cases"][name] = entry
        print(name, {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in entry.items() if k not in ("note",)}, flush=True)
    with open(mh.PIN_REPORT, "w") as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
    print("wrote", mh.PIN_REPORT)


if __name__ == "__main__":
    main(sys.argv[1])
