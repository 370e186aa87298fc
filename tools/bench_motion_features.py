"""One joints_to_features call at B = 32, T = 197 on the GPU (profiles/r23a_motion_features.md): the span between device events around
the call, 200 calls after 30 warm ones, with and without process_file's transform.  Prints one JSON line.

    python tools/bench_motion_features.py [--reference /path/to/motion-diffusion-model]

With --reference (CPU only, no GPU needed) it times the reference's own process_file loop over the same 32 clips on the host cores
instead: five passes, uniform_skeleton replaced by the identity as in the device call without tgt_offsets."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

B = 32


def device():
    import torch
    import motion_features_helpers as mh
    from mdm_amd.motion_process import joints_to_features
    x = torch.from_numpy(mh.to_bj3t(mh.load_case("humanml_T197")["joints"])).repeat(B, 1, 1, 1).cuda()
    res = {"B": B, "T": 197, "device": torch.cuda.get_device_name(0)}
    for canon in (True, False):
        for _ in range(30):
            joints_to_features(x, canonicalise=canon)
        torch.cuda.synchronize()
        ts = []
        for _ in range(200):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            joints_to_features(x, canonicalise=canon)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        ts = np.sort(np.array(ts))
        res["canonicalise" if canon else "extract_only"] = {"median_us": float(np.median(ts)), "min_us": float(ts[0]), "p90_us": float(ts[180])}
    print(json.dumps(res))


def reference(root):
    np.float = float                                    # the alias numpy 2 removed, which the reference uses
    import warnings
    import torch
    warnings.filterwarnings("ignore")
    sys.path.insert(0, root)
    import motion_features_helpers as mh
    import make_golden_motion_features as mg
    from data_loaders.humanml.scripts import motion_process as mp
    mg.inject(mp, mh.SKELETONS["humanml"], None)
    mp.uniform_skeleton = lambda positions, target_offset: positions
    P = mh.load_case("humanml_T197")["joints"]
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _b in range(B):
            mp.process_file(P.copy(), 0.002)
        ts.append(time.perf_counter() - t0)
    print(json.dumps({"B": B, "T": 197, "reference_process_file_loop_s": sorted(ts), "torch_threads": torch.get_num_threads(),
                      "cores": len(os.sched_getaffinity(0))}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--reference":
        reference(sys.argv[2])
    else:
        device()
