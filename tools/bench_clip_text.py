"""Measures mdm_amd/clip_text.py on one MI355X and writes profiles/r18a_clip_text.md:
  * per fixture of tests/golden/clip_text_*.npz and per sweep case of tests/clip_text_helpers.py: max-abs error against the fp64
    restatement next to the pooled e_ref and the 4 x e_ref bound;
  * `ClipText.encode_text` over B = 1, 32, 128 context-22 prompts (ragged lengths, full width, trained-like weights) against
    `transformers.CLIPTextModelWithProjection` on the same weights and device in fp32 and in fp16 over all 77 positions -- what a
    caller computes today: the tokens zero-padded to 77 as model/mdm.py:163-178 does.  HIP events around groups of 10 warm calls,
    the three encoders interleaved group by group in this one process; median / min / max per call, the copy of the ids included.
    Condition (B = 1 and 32): this encoder's median <= HF fp32's median + HF fp32's (max - min) over the groups;
  * per-kernel times of one profiled run per shape, when its kernel-trace table is handed over.

    python tools/bench_clip_text.py [--calls 30] [--kernel-stats B table.md]... [--out profiles/r18a_clip_text.md]

A per-kernel table comes from a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/bench_clip_text.py --profile-pass B
    python tools/rocpd_summary.py DIR/.../trace_results.db > table.md
"""
import argparse
import copy
import os
import socket
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import clip_text_helpers as ch  # noqa: E402

DEV = "cuda:0"
BATCHES = [1, 32, 128]
GATED = (1, 32)
GROUP = 10


def timed_interleaved(fns, groups, warm=5):
    """{name: (median, min, max) ms per call}: per group, GROUP calls of each fn in turn between two events."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(groups):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(GROUP):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / GROUP)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def prompts(B):
    """B context-22 prompts of ragged lengths -> (tokens [B, 22], the same zero-padded to [B, 77]), int64 on the host."""
    t22 = ch.make_tokens(400 + B, B, 22, [22] + [3 + (7 * b) % 20 for b in range(1, B)])
    t77 = torch.zeros(B, 77, dtype=torch.int64)
    t77[:, :22] = torch.from_numpy(t22)
    return torch.from_numpy(t22), t77


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30, help="timed groups of 10 calls per shape and encoder")
    ap.add_argument("--kernel-stats", nargs=2, action="append", default=[], metavar=("B", "TABLE"),
                    help="tools/rocpd_summary.py table of a --profile-pass run at that batch")
    ap.add_argument("--profile-pass", type=int, default=None, metavar="B", help="four calls at that batch, nothing written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18a_clip_text.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available() and a.calls >= 20
    clip = ch.make_clip("full", True, DEV)
    if a.profile_pass:
        t22, _ = prompts(a.profile_pass)
        for _ in range(4):
            clip.encode_text(t22)
        torch.cuda.synchronize()
        return
    lines = ["# r18a — the CLIP text encoder (csrc/clip_text.h) on the MI355X", "",
             f"Box: `{socket.gethostname()}`, {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Written by `tools/bench_clip_text.py`.", "",
             "## Accuracy: max-abs error against the fp64 restatement", "",
             "| case | B x L | GPU error | pooled e_ref (HF fp32 vs fp64) | bound 4 x e_ref | error / e_ref | ok |", "|---|---|---|---|---|---|---|"]
    clips = {("full", True): clip}

    def row(name, cfg, trained, tokens, want):
        if (cfg, trained) not in clips:
            clips[cfg, trained] = ch.make_clip(cfg, trained, DEV)
        err, e = ch.maxabs(clips[cfg, trained].encode_text(torch.from_numpy(tokens)), want), ch.pooled_e_ref(cfg, trained)
        lines.append(f"| {name} | {tokens.shape[0]} x {tokens.shape[1]} | {err:.3e} | {e:.3e} | {4 * e:.3e} | {err / e:.2f} | {'yes' if err <= 4 * e else 'NO'} |")

    for name, f in ch.FIXTURES.items():
        g = ch.load_fixture(name)
        row(name, f["cfg"], f["trained"], g["tokens"], g["fp64"])
    for name, c in ch.SWEEP.items():
        tokens = ch.sweep_inputs(name)
        row(name, c["cfg"], c["trained"], tokens, ch.encode_text_fp64(ch.weights(c["cfg"], c["trained"]), tokens, ch.CFGS[c["cfg"]]["heads"]))

    hf32 = ch.hf_model("full", True).to(DEV)
    hf16 = copy.deepcopy(hf32).half()
    lines += ["", f"## Timings: one call, ViT-B/32's text tower (12 layers, width 512), trained-like weights, context-22 prompts of ragged "
              f"lengths (HIP events around {a.calls} groups of {GROUP} warm calls, the three encoders interleaved)", "",
              "`ClipText.encode_text` takes the [B, 22] tokens; HF takes them zero-padded to [B, 77], as upstream's model does.", "",
              "| B | `ClipText.encode_text` median ms | min | max | prompts / s | HF fp32 median ms | min | max | HF fp16 median ms | min | max "
              "| condition: median <= HF fp32 median + (max - min) |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for B in BATCHES:
        t22, t77 = prompts(B)
        with torch.no_grad():
            want = hf32(input_ids=t77.to(DEV)).text_embeds
            d32 = float((want - clip.encode_text(t22)).abs().max())
            d16 = float((want - hf16(input_ids=t77.to(DEV)).text_embeds.float()).abs().max())
            t = timed_interleaved({"ours": lambda: clip.encode_text(t22),
                                   "hf32": lambda: hf32(input_ids=t77.to(DEV)).text_embeds,
                                   "hf16": lambda: hf16(input_ids=t77.to(DEV)).text_embeds}, a.calls)
        o, h, q = t["ours"], t["hf32"], t["hf16"]
        limit = h[0] + (h[2] - h[1])
        verdict = f"{'met' if o[0] <= limit else 'MISSED'} ({o[0]:.3f} vs {limit:.3f})" if B in GATED else f"not gated ({o[0]:.3f} vs {limit:.3f})"
        lines.append(f"| {B} | {o[0]:.3f} | {o[1]:.3f} | {o[2]:.3f} | {B / o[0] * 1e3:.0f} | {h[0]:.3f} | {h[1]:.3f} | {h[2]:.3f} (output differs "
                     f"from ours by {d32:.1e}) | {q[0]:.3f} | {q[1]:.3f} | {q[2]:.3f} (differs from HF fp32 by {d16:.1e}) | {verdict} |")
    for B, path in a.kernel_stats:
        with open(path) as fh:
            table = [ln.rstrip() for ln in fh if ln.startswith("|")]
        lines += ["", f"## Kernels of one profiled run at B = {B} (rocprofv3 --kernel-trace; 4 calls of 87 launches, and the copies of the "
                  f"weight preparation)", ""] + table
    lines.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
