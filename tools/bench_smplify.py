"""Wall time of one SMPLify fit (mdm_amd/simplify_loc2rot.py joints2smpl, csrc/smplify.h) at T = 196 frames and 150 iterations on the
synthetic model and mixture of tests/smplify_helpers.py, with its function evaluations; what one evaluation costs and how much of it is
the host's read of the reduced scalars; and, for context, a float32 torch restatement of the reference's loop (torch.optim.LBFGS with
strong_wolfe over the helper's losses under autograd) on the same device, at fewer step() calls (`--torch-calls`), per evaluation.

    python tools/bench_smplify.py [--frames 196] [--iters 150] [--runs 2] [--torch-calls 10] [--no-torch]
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
import smpl_mesh_helpers as smh  # noqa: E402
import smplify_helpers as H  # noqa: E402
from mdm_amd import _native as nat  # noqa: E402
from mdm_amd import simplify_loc2rot as s2r  # noqa: E402


def torch_loop(j3d, dev, num_iters, calls1, calls2):
    """SMPLify3D.__call__'s two optimisers over the helper's float32 losses; returns (ms, closure evaluations, final loss)."""
    T = j3d.shape[0]
    tab = H.tables64(H.model_fields())
    tab = dict(j0=torch.tensor(tab["j0"], dtype=torch.float32, device=dev), jdirs=torch.tensor(tab["jdirs"], dtype=torch.float32, device=dev),
               parents=tab["parents"])
    g = s2r.prepare_gmm(H.synthetic_gmm())
    pr = dict(means=torch.tensor(g["means"], device=dev), prec=torch.tensor(g["precisions"], device=dev),
              nlw=torch.tensor(g["neg_log_nll_weights"], device=dev))
    pose0, shape0 = H.mean_params()
    go = torch.tensor(np.tile(pose0[:3], (T, 1)), device=dev)
    body = torch.tensor(np.tile(pose0[3:], (T, 1)), device=dev)
    betas = torch.tensor(np.tile(shape0, (T, 1)), device=dev)
    preserve = body.clone()
    tj = torch.tensor(j3d, device=dev)
    conf = torch.ones(22, device=dev)
    evals = [0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        mj = H.model_joints(torch.cat([go, body], 1), betas, tab)
        cam_est = (tj[:, [2, 1, 17, 16]] - mj[:, [2, 1, 17, 16]]).sum(1) / 4.0
    cam = cam_est.clone()
    go.requires_grad_(True)
    cam.requires_grad_(True)
    opt = torch.optim.LBFGS([go, cam], max_iter=num_iters, lr=1e-2, line_search_fn="strong_wolfe")

    def closure1():
        opt.zero_grad()
        loss = H.stage1_frames(go, cam, body, betas, cam_est, tj, tab).sum()
        loss.backward()
        evals[0] += 1
        return loss
    for _ in range(calls1):
        opt.step(closure1)
    body.requires_grad_(True)
    betas.requires_grad_(True)
    opt2 = torch.optim.LBFGS([body, betas, go, cam], max_iter=num_iters, lr=1e-2, line_search_fn="strong_wolfe")
    last = [None]

    def closure2():
        opt2.zero_grad()
        loss = H.stage2_frames(body, betas, go, cam, preserve, tj, conf, tab, pr).sum()
        loss.backward()
        evals[0] += 1
        last[0] = loss
        return loss
    for _ in range(calls2):
        opt2.step(closure2)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, evals[0], float(last[0].detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=196)
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--torch-calls", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev, T = "cuda:0", args.frames
    fields, extra, _ids, _maps = smh.fixture_model()
    j3d = H.fit_targets(T, seed=4000 + T)
    row = dict(T=T, num_iters=args.iters)
    with tempfile.TemporaryDirectory() as tmp:
        model_path, _ = smh.write_model_files(tmp, fields, extra)
        fit = s2r.joints2smpl(T, 0, smpl_model_path=model_path, gmm_path=H.write_gmm(os.path.join(tmp, "prior")), mean_params=H.mean_params(),
                              num_smplify_iters=args.iters)
        fit.joint2smpl(j3d[:T])                                   # warm-up: tables, workspace, the pinned read-back buffer
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            _thetas, opt = fit.joint2smpl(j3d)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        st = fit.last_stats
        evals = st["stage1"]["func_evals"] + st["stage2"]["func_evals"]
        iters = st["stage1"]["n_iter"] + st["stage2"]["n_iter"]
        dist = float(torch.linalg.norm(fit.last_fit["joints"][:, :22] + opt["cam"] - torch.from_numpy(j3d).to(dev), dim=-1).max())
        row.update(fit_ms_median=float(np.median(ts)), fit_ms_min=float(min(ts)), func_evals=evals, iterations=iters,
                   final_loss=st["stage2"]["loss"], worst_joint_distance_mm=dist * 1e3, us_per_eval_wall=float(min(ts)) * 1e3 / evals)
    # one evaluation on its own, for scale only: mdm_smplify_value_grad is two launches and two reads (the finiteness pass, then the
    # evaluation), and this harness uploads the inputs and downloads the outputs around it
    bench = H.Bench(nat.load_native(), dev)
    inp = {k: np.resize(v, (T,) + v.shape[1:]) for k, v in H.value_grad_inputs().items()}
    for stage in (1, 2):
        bench.value_grad(stage, inp, H.conf_of("ones"), T)
        t0 = time.perf_counter()
        for _ in range(20):
            bench.value_grad(stage, inp, H.conf_of("ones"), T)
        row["value_grad_stage%d_us_per_call_with_copies" % stage] = (time.perf_counter() - t0) * 1e6 / 20
    # the floor of "a launch and a read": a trivial kernel, 28 floats to pinned memory, one synchronisation
    small, pinned = torch.zeros(28, device=dev), torch.zeros(28).pin_memory()
    stream = torch.cuda.current_stream()
    for n in (10, 200):
        t0 = time.perf_counter()
        for _ in range(n):
            small.add_(1.0)
            pinned.copy_(small, non_blocking=True)
            stream.synchronize()
        row["trivial_launch_and_read_us"] = (time.perf_counter() - t0) * 1e6 / n
    print(json.dumps(row), flush=True)
    if not args.no_torch:
        ms, ev, loss = torch_loop(j3d, dev, args.iters, 1, args.torch_calls)
        row.update(torch_calls=(1, args.torch_calls), torch_ms=ms, torch_func_evals=ev, torch_us_per_eval=ms * 1e3 / ev, torch_loss_there=loss)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
