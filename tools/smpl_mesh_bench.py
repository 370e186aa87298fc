"""Wall time of the full SMPL pass (mdm_amd/smpl_mesh.py Rotation2xyzFull, csrc/smpl_mesh.h) on a synthetic model of the real
size, against a torch restatement of the same pass on the same device (smplx's lbs as batched float32 matmuls that materialise
the per-vertex 4x4 transforms, which is what the reference runs), at the shapes of tests/test_gpu_smpl_mesh.py.

    python tools/smpl_mesh_bench.py [--runs 5] [--no-torch]          (under rocprofv3 --kernel-trace --stats for the kernel split)
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mdm_amd  # noqa: E402,F401
import smpl_mesh_helpers as H  # noqa: E402
from mdm_amd.smpl_mesh import Rotation2xyzFull, joint_maps  # noqa: E402

SHAPES = [(1, 196, "vertices"), (128, 60, "vertices"), (64, 60, "a2m")]


def torch_pass(x, mask, t, jointstype, ids, chunk=1024):
    """rot6d -> lbs -> points, float32 on x's device, frames in chunks of `chunk` (the 4x4 transforms of 7,680 frames are 3.4 GB)."""
    B, _, _, T = x.shape
    xr = x[:, :-1].permute(0, 3, 1, 2)[mask]
    a1, a2 = xr[..., :3], xr[..., 3:]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    rot = torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)
    outs = []
    eye = torch.eye(3, device=x.device)
    for s in range(0, rot.shape[0], chunk):
        R = rot[s:s + chunk]
        n = R.shape[0]
        v_shaped = t["v_template"][None].expand(n, -1, -1)
        J = torch.einsum("jv,nvc->njc", t["J_regressor"], v_shaped)
        v_posed = v_shaped + torch.matmul((R[:, 1:] - eye).reshape(n, -1), t["posedirs"]).view(n, -1, 3)
        rel = J.clone()
        rel[:, 1:] -= J[:, t["parents"][1:]]
        tm = torch.cat([torch.nn.functional.pad(R, [0, 0, 0, 1]), torch.nn.functional.pad(rel[..., None], [0, 0, 0, 1], value=1.0)], dim=-1)
        chain = [tm[:, 0]]
        for i in range(1, 24):
            chain.append(torch.matmul(chain[int(t["parents"][i])], tm[:, i]))
        G = torch.stack(chain, dim=1)
        A = G - torch.nn.functional.pad(torch.matmul(G, torch.nn.functional.pad(J[..., None], [0, 0, 0, 1])), [3, 0])
        Tm = torch.matmul(t["weights"], A.view(n, 24, 16)).view(n, -1, 4, 4)
        vh = torch.cat([v_posed, torch.ones(n, v_posed.shape[1], 1, device=x.device)], dim=2)
        verts = torch.matmul(Tm, vh[..., None])[:, :, :3, 0]
        if jointstype == "vertices":
            outs.append(verts)
        else:
            allj = torch.cat([G[:, :, :3, 3], verts[:, ids], torch.einsum("ev,nvc->nec", t["extra"], verts)], dim=1)
            outs.append(allj[:, t["map"]])
    pts = torch.cat(outs)
    out = torch.zeros(B, T, pts.shape[1], 3, device=x.device)
    out[mask] = pts
    out = out.permute(0, 2, 3, 1).contiguous()
    if jointstype != "vertices":
        out = out - out[:, [0]]
    tr = x[:, -1, :3]
    return out + (tr - tr[:, :, [0]])[:, None]


def timed(fn, runs):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    fields, extra, ids = H.synthetic_full_model(seed=0, V=6890)
    with tempfile.TemporaryDirectory() as tmp:
        paths = H.write_model_files(tmp, fields, extra)
        r2x = Rotation2xyzFull(model_path=paths[0], extra_regressor_path=paths[1], vertex_joint_ids=ids)
        parents = np.asarray(fields["kintree_table"][0]).astype(np.int64)
        parents[0] = -1
        f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)   # noqa: E731
        t = dict(v_template=f32(fields["v_template"]), J_regressor=f32(fields["J_regressor"]), weights=f32(fields["weights"]),
                 posedirs=f32(fields["posedirs"].reshape(-1, 207).T), extra=f32(extra), parents=torch.from_numpy(parents).to(dev))
        for B, T, jt in SHAPES:
            x = torch.from_numpy(H.make_x(B, T, "rot6d", True, True, seed=B + T)).to(dev)
            mask = torch.ones(B, T, dtype=torch.bool, device=dev)
            call = dict(pose_rep="rot6d", translation=True, glob=True, jointstype=jt, vertstrans=True)
            if jt != "vertices":
                t["map"] = torch.from_numpy(joint_maps()[jt]).to(dev)
            row = dict(B=B, T=T, jointstype=jt)
            row["hip_ms_median"], row["hip_ms_min"] = timed(lambda: r2x(x=x, mask=mask, **call), args.runs)
            if not args.no_torch:
                row["torch_ms_median"], row["torch_ms_min"] = timed(lambda: torch_pass(x, mask, t, jt, ids), args.runs)
                row["max_abs_hip_vs_torch"] = float((r2x(x=x, mask=mask, **call) - torch_pass(x, mask, t, jt, ids)).abs().max())
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
