"""Measures mdm_amd/stgcn.py on one MI355X and writes profiles/r15a_stgcn.md:
  * per case of tests/stgcn_helpers.py at full width: max-abs error of features / yhat against fp64 next to e_ref and the 4 x e_ref bound;
  * `STGCN.forward` of the a2m net (ten blocks, V = 24, trained-like weights) at (N, T) = (1, 60), (32, 60), (128, 60): HIP events
    around groups of 10 warm calls, >= 20 groups, median / min / max per call (host-side checks included);
  * torch's own operators on the same weights, in fp32, on the same device in the same session: conv2d, batch_norm and einsum in the
    order of the network's definition -- what a user runs today;
  * per-kernel-class times of one profiled run per shape, when its kernel-trace table is handed over.

    python tools/bench_stgcn.py [--calls 30] [--kernel-stats N T table.md]... [--out profiles/r15a_stgcn.md]

A per-kernel table comes from a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/bench_stgcn.py --profile-pass N T
    python tools/rocpd_summary.py DIR/.../trace_results.db > table.md
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import stgcn_helpers as sh  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 60), (32, 60), (128, 60)]
GROUP = 10
CLASSES = (("GraphMixLoader", "graph convolution GEMM (neighbour-mix loader, BN + ReLU epilogue)"),
           ("Tap9GatherLoader", "temporal convolution GEMM (9-tap gather loader, BN + residual + ReLU epilogue)"),
           ("StrideRowLoader", "residual convolution GEMM (strided row loader, BN epilogue)"),
           ("stgcn_input_kernel", "input permute + data_bn"), ("stgcn_tail_kernel", "pooling + fcn"))


def timed(fn, groups, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(groups):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(GROUP):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / GROUP)
    return statistics.median(ms), min(ms), max(ms)


def torch_forward(sd, blocks, x):
    """The network's definition on torch's own fp32 operators (eval mode): x [N, V, C, T] -> (features, yhat)."""
    def bn(h, p):
        return F.batch_norm(h, sd[p + "running_mean"], sd[p + "running_var"], sd[p + "weight"], sd[p + "bias"], False, 0.0, 1e-5)
    N, V, C, T = x.shape
    h = bn(x.reshape(N, V * C, T), "data_bn.").reshape(N, V, C, T).permute(0, 2, 3, 1).contiguous()
    for b, (_, co, s, residual) in enumerate(blocks):
        p = f"st_gcn_networks.{b}."
        ci = h.shape[1]
        A_b = sd["A"] * sd[f"edge_importance.{b}"]
        y = F.conv2d(h, sd[p + "gcn.conv.weight"], sd[p + "gcn.conv.bias"])
        n, kc, t, v = y.shape
        g = torch.einsum("nkctv,kvw->nctw", y.view(n, A_b.shape[0], co, t, v), A_b).contiguous()
        g = F.relu(bn(g, p + "tcn.0."))
        z = bn(F.conv2d(g, sd[p + "tcn.2.weight"], sd[p + "tcn.2.bias"], stride=(s, 1), padding=(4, 0)), p + "tcn.3.")
        if not residual:
            r = 0
        elif ci == co and s == 1:
            r = h
        else:
            r = bn(F.conv2d(h, sd[p + "residual.0.weight"], sd[p + "residual.0.bias"], stride=(s, 1)), p + "residual.1.")
        h = F.relu(z + r)
    feat = F.avg_pool2d(h, h.shape[2:])
    return feat.flatten(1), F.conv2d(feat, sd["fcn.weight"], sd["fcn.bias"]).flatten(1)


def class_table(path):
    """Sum a tools/rocpd_summary.py table by kernel class."""
    acc = {label: [0, 0.0] for _, label in CLASSES}
    other = [0, 0.0]
    with open(path) as fh:
        for ln in fh:
            cells = [c.strip() for c in ln.strip().strip("|").split("|")]
            if len(cells) < 4 or not cells[0].startswith("`"):
                continue
            slot = next((acc[label] for key, label in CLASSES if key in cells[0]), other)
            slot[0] += int(cells[1])
            slot[1] += float(cells[2])
    rows = [(label, n, ms) for label, (n, ms) in acc.items()] + [("everything else in the trace (weight preparation, copies)", *other)]
    total = sum(ms for _, _, ms in rows) or 1.0
    return ["| kernel class | launches | total ms | % |", "|---|---|---|---|"] + \
           [f"| {label} | {n} | {ms:.3f} | {100 * ms / total:.1f} |" for label, n, ms in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30, help="timed groups of 10 calls per shape")
    ap.add_argument("--kernel-stats", nargs=3, action="append", default=[], metavar=("N", "T", "TABLE"),
                    help="tools/rocpd_summary.py table of a --profile-pass run at that shape")
    ap.add_argument("--profile-pass", nargs=2, type=int, default=None, metavar=("N", "T"), help="four calls at that shape, nothing written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15a_stgcn.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available() and a.calls >= 20
    weights = sh.build_weights("a2m", 102, "trained")
    model = sh.loaded_model("a2m", weights, DEV)
    if a.profile_pass:
        x = torch.from_numpy(sh.make_input("a2m", 500, *a.profile_pass)).to(DEV)
        for _ in range(4):
            model({"output": x})
        torch.cuda.synchronize()
        return
    lines = ["# r15a — the ST-GCN action recogniser (csrc/stgcn.h) on the MI355X", "",
             f"Device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Written by `tools/bench_stgcn.py`.", "",
             "## Accuracy: max-abs error against the fp64 restatement", "",
             "| case | N x T | features error | yhat error | e_ref (reference fp32 vs fp64) | bound 4 x e_ref | worst error / e_ref | ok |",
             "|---|---|---|---|---|---|---|---|"]
    rep = sh.pin_report()
    models = {("a2m", "trained"): (model, weights)}
    for name, c in sh.CASES.items():
        if c["net"].startswith("red_"):
            continue
        key = (c["net"], c["regime"])
        if key not in models:
            w = sh.build_weights(c["net"], c["wseed"], c["regime"])
            models[key] = (sh.loaded_model(c["net"], w, DEV), w)
        m, w = models[key]
        x = sh.case_input(name)
        if c["fixture"]:
            g = sh.load_fixture(name)
            want = (g["fp64_features"], g["fp64_yhat"])
        else:
            want = sh.forward_fp64(c["net"], w, x)
        ef, ey = sh.errors(sh.run_case(m, name, x), want)
        e = rep[name]["e_ref"]
        lines.append(f"| {name} | {c['N']} x {c['T']} | {ef:.3e} | {ey:.3e} | {e:.3e} | {4 * e:.3e} | {max(ef, ey) / e:.2f} | "
                     f"{'yes' if max(ef, ey) <= 4 * e else 'NO'} |")

    sd = {k: v.to(DEV) for k, v in weights.items()}
    blocks = sh.net_blocks("a2m")
    lines += ["", f"## Timings: one call of the a2m net (ten blocks, V = 24, 6 channels, 40 classes), trained-like weights "
              f"(HIP events around {a.calls} groups of {GROUP} warm calls)", "",
              "| N x T | `STGCN.forward` median ms | min | max | samples / s | torch fp32 operators, same device and weights: median ms | min | max | "
              "outputs differ by |", "|---|---|---|---|---|---|---|---|---|"]
    for N, T in SHAPES:
        x = torch.from_numpy(sh.make_input("a2m", 500, N, T)).to(DEV)
        med, lo, hi = timed(lambda: model({"output": x}), a.calls)
        with torch.no_grad():
            tf, ty = torch_forward(sd, blocks, x)
            mine = model({"output": x})
            diff = max(float((tf - mine["features"].reshape(N, -1)).abs().max()), float((ty - mine["yhat"]).abs().max()))
            t = timed(lambda: torch_forward(sd, blocks, x), a.calls)
        lines.append(f"| {N} x {T} | {med:.3f} | {lo:.3f} | {hi:.3f} | {N / med * 1e3:.0f} | {t[0]:.3f} | {t[1]:.3f} | {t[2]:.3f} | {diff:.1e} |")
    for N, T, path in a.kernel_stats:
        lines += ["", f"## Kernel classes of one profiled run at {N} x {T} (rocprofv3 --kernel-trace; 4 calls of 24 launches)", ""] + class_table(path)
        with open(path) as fh:
            lines += ["", "The kernels of that run:", ""] + [ln.rstrip() for ln in fh if ln.startswith("|")]
    lines.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
