"""Measures mdm_amd/gru_recogniser.py on one MI355X and writes profiles/r17a_gru_recogniser.md:
  * per full-width case of tests/gru_recogniser_helpers.py: max-abs error of features / yhat against fp64 next to the pooled e_ref and
    the 4 x e_ref bound;
  * `MotionDiscriminator.forward` of the published shape (I = 72, H = 128, two layers, 12 classes; trained-like weights) at
    (B, T) = (1, 60), (32, 60), (128, 60): HIP events around groups of 10 warm calls, >= 20 groups, median / min / max per call;
  * INTERLEAVED with it, group by group in the same session: torch.nn.GRU + Linear (the reference's forward) on the same weights and
    device -- what a user runs today -- and the speed condition at (32, 60): the HIP median must not lie above torch's median by
    more than torch's own max - min spread;
  * the per-kernel times of one traced run per shape, when its table is handed over, and the recurrence's time per step from it.

    python tools/bench_gru_recogniser.py [--calls 30] [--kernel-stats B T table.md]... [--out profiles/r17a_gru_recogniser.md]

A per-kernel table comes from a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/bench_gru_recogniser.py --profile-pass B T
    python tools/rocpd_summary.py DIR/.../trace_results.db > table.md
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gru_recogniser_helpers as gh  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 60), (32, 60), (128, 60)]
GROUP = 10
PROFILE_CALLS = 4


class TorchRecogniser(torch.nn.Module):
    """The reference's forward on torch's own operators (nn.GRU is MIOpen's RNN path on this device)."""

    def __init__(self, net, weights):
        super().__init__()
        f = gh.NETS[net]
        self.recurrent = torch.nn.GRU(gh.input_size(net), f["H"], f["L"])
        self.linear1 = torch.nn.Linear(f["H"], gh.MID)
        self.linear2 = torch.nn.Linear(gh.MID, f["classes"])
        self.load_state_dict(weights)

    def forward(self, x, lengths, h0):
        bs, nj, nf, T = x.shape
        seq = x.reshape(bs, nj * nf, T).permute(2, 0, 1)
        gru_o, _ = self.recurrent(seq.float(), h0)
        out = gru_o[tuple(torch.stack((lengths - 1, torch.arange(bs, device=x.device))))]
        lin1 = torch.tanh(self.linear1(out))
        return lin1, self.linear2(lin1)


def group_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(GROUP):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / GROUP


def timed_interleaved(fa, fb, groups, warm=5):
    """Per-call milliseconds of fa and of fb, their groups alternating: (median, min, max) each."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ma, mb = [], []
    for _ in range(groups):
        ma.append(group_ms(fa))
        mb.append(group_ms(fb))
    return [(statistics.median(m), min(m), max(m)) for m in (ma, mb)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30, help="timed groups of 10 calls per shape and side")
    ap.add_argument("--kernel-stats", nargs=3, action="append", default=[], metavar=("B", "T", "TABLE"),
                    help="tools/rocpd_summary.py table of a --profile-pass run at that shape")
    ap.add_argument("--profile-pass", nargs=2, type=int, default=None, metavar=("B", "T"), help="four calls at that shape, nothing written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17a_gru_recogniser.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available() and a.calls >= 20
    weights = gh.build_weights("full", "trained")
    model = gh.loaded_model("full", weights, DEV)
    if a.profile_pass:
        B, T = a.profile_pass
        xn, h0n = gh.make_input("full", 600, B, T)
        x, h0, lens = torch.from_numpy(xn).to(DEV), torch.from_numpy(h0n).to(DEV), torch.full((B,), T, device=DEV)
        for _ in range(PROFILE_CALLS):
            model(x, lens, h0)
        torch.cuda.synchronize()
        return

    lines = ["# r17a — the HumanAct12 GRU action recogniser (csrc/gru_recogniser.h) on the MI355X", "",
             f"Device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Written by `tools/bench_gru_recogniser.py`.", "",
             "## Accuracy: max-abs error against the fp64 restatement", "",
             "e_ref is the reference's own fp32 error against fp64, pooled per (net, regime, output) "
             "(`tests/golden/PIN_REPORT_gru_recogniser.json`); the bound is 4 x e_ref.", "",
             "| case | B x T | features error | bound | yhat error | bound | worst error / e_ref | ok |", "|---|---|---|---|---|---|---|---|"]
    models = {("full", "trained"): (model, weights)}
    for name, c in gh.CASES.items():
        if c["net"].startswith("red"):
            continue
        key = (c["net"], c["regime"])
        if key not in models:
            w = gh.build_weights(*key)
            models[key] = (gh.loaded_model(c["net"], w, DEV), w)
        m, w = models[key]
        x, lens, h0 = gh.case_input(name)
        ef, ey = gh.errors(gh.run_model(m, x, lens, h0), gh.forward_fp64(c["net"], w, x, lens, h0))
        bf, by = gh.bound(*key)
        lines.append(f"| {name} | {c['B']} x {c['T']} | {ef:.3e} | {bf:.3e} | {ey:.3e} | {by:.3e} | {max(4 * ef / bf, 4 * ey / by):.2f} | "
                     f"{'yes' if ef <= bf and ey <= by else 'NO'} |")

    ref = TorchRecogniser("full", weights).to(DEV).eval()
    lines += ["", f"## Timings: one forward of the published shape (I = 72, H = 128, two layers), trained-like weights, full lengths "
              f"(HIP events around {a.calls} groups of {GROUP} warm calls per side, the two sides' groups alternating)", "",
              "| B x T | `MotionDiscriminator.forward` median ms | min | max | sequences / s | torch.nn.GRU + Linear, same device and weights: "
              "median ms | min | max | torch / HIP | outputs differ by |", "|---|---|---|---|---|---|---|---|---|---|"]
    gate = None
    for B, T in SHAPES:
        xn, h0n = gh.make_input("full", 600, B, T)
        x, h0, lens = torch.from_numpy(xn).to(DEV), torch.from_numpy(h0n).to(DEV), torch.full((B,), T, device=DEV)
        with torch.no_grad():
            mine, theirs = model.run(x, lens, h0), ref(x, lens, h0)
            diff = max(float((mine[0] - theirs[0]).abs().max()), float((mine[1] - theirs[1]).abs().max()))
            (med, lo, hi), (tm, tl, th) = timed_interleaved(lambda: model(x, lens, h0), lambda: ref(x, lens, h0), a.calls)
        lines.append(f"| {B} x {T} | {med:.3f} | {lo:.3f} | {hi:.3f} | {B / med * 1e3:.0f} | {tm:.3f} | {tl:.3f} | {th:.3f} | {tm / med:.2f} | "
                     f"{diff:.1e} |")
        if (B, T) == (32, 60):
            gate = (med, tm, th - tl)
    med, tm, spread = gate
    ok = med <= tm + spread
    lines += ["", f"Speed condition at 32 x 60: HIP median {med:.3f} ms against torch's median {tm:.3f} ms + its max - min spread {spread:.3f} ms "
              f"= {tm + spread:.3f} ms: {'MET' if ok else 'NOT MET'}."]
    for B, T, path in a.kernel_stats:
        with open(path) as fh:
            rows = [ln.rstrip() for ln in fh if ln.startswith("|")]
        lines += ["", f"## Kernels of one traced run at {B} x {T} (rocprofv3 --kernel-trace; {PROFILE_CALLS} calls)", ""] + rows
        for ln in rows:
            cells = [c.strip() for c in ln.strip("|").split("|")]
            if "gru_seq_kernel" in cells[0]:
                lines += ["", f"`gru_seq_kernel`: {float(cells[3]):.1f} us per launch of {T} steps = {float(cells[3]) / int(T):.2f} us per step."]
    lines.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    main()
