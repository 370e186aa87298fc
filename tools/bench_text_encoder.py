"""Measures mdm_amd/text_encoder.py on one MI355X and writes profiles/r14a_text_encoder.md:
  * per fixture of tests/golden/text_encoder_*.npz and per sweep case of tests/text_encoder_helpers.py: max-abs error against the fp64
    restatement over valid rows next to e_ref and the 4 x e_ref bound;
  * `BERT.encode_ids` at (B, L) = (1, 12), (32, 24), (128, 24), full width, trained-like weights, ragged lengths: HIP events around
    groups of 10 warm calls, >= 20 groups, median / min / max per call (host-side checks and the copy of the ids included);
  * the same prompts through `transformers.DistilBertModel` in fp32 on the same device and weights -- what a user runs today --
    when that package is importable there; otherwise the column says so;
  * per-kernel times of one profiled run per shape, when its kernel-trace table is handed over.

    python tools/bench_text_encoder.py [--calls 30] [--kernel-stats B L table.md]... [--out profiles/r14a_text_encoder.md]

A per-kernel table comes from a run of its own (tracing slows the host):
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/bench_text_encoder.py --profile-pass B L
    python tools/rocpd_summary.py DIR/.../trace_results.db > table.md
"""
import argparse
import os
import socket
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import text_encoder_helpers as th  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 12), (32, 24), (128, 24)]
GROUP = 10


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


def prompts(B, L):
    lens = [L] + [3 + (7 * b) % (L - 2) for b in range(1, B)]
    ids, mask = th.make_ids(400 + B, B, L, lens)
    return torch.from_numpy(ids), torch.from_numpy(mask), lens


def hf_model():
    try:
        from transformers import DistilBertConfig, DistilBertModel
    except ImportError:
        return None
    c = th.FULL
    m = DistilBertModel(DistilBertConfig(vocab_size=len(th.VOCAB), max_position_embeddings=c["max_pos"], n_layers=c["n_layers"],
                                         n_heads=c["n_heads"], dim=c["dim"], hidden_dim=c["hidden"], pad_token_id=th.PAD))
    m.load_state_dict(th.weights("full", True))
    return m.to(DEV).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30, help="timed groups of 10 calls per shape")
    ap.add_argument("--kernel-stats", nargs=3, action="append", default=[], metavar=("B", "L", "TABLE"),
                    help="tools/rocpd_summary.py table of a --profile-pass run at that shape")
    ap.add_argument("--profile-pass", nargs=2, type=int, default=None, metavar=("B", "L"), help="four calls at that shape, nothing written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14a_text_encoder.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available() and a.calls >= 20
    bert = th.make_bert("full", True, DEV)
    if a.profile_pass:
        ids, mask, _ = prompts(*a.profile_pass)
        for _ in range(4):
            bert.encode_ids(ids, mask)
        torch.cuda.synchronize()
        return
    lines = ["# r14a — the DistilBERT text encoder (csrc/text_encoder.h) on the MI355X", "",
             f"Box: `{socket.gethostname()}`, {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Written by `tools/bench_text_encoder.py`.", "",
             "## Accuracy: max-abs error against the fp64 restatement over valid rows", "",
             "| case | B x L | GPU error | e_ref (reference fp32 vs fp64) | bound 4 x e_ref | error / e_ref | ok |", "|---|---|---|---|---|---|---|"]
    rep = th.pin_report()
    berts = {("full", True): bert}

    def row(name, cfg, trained, ids, mask, lens, want):
        if (cfg, trained) not in berts:
            berts[cfg, trained] = th.make_bert(cfg, trained, DEV)
        err, e = th.valid_maxabs(th.encode(berts[cfg, trained], ids, mask), want, lens), rep[name]["e_ref"]
        lines.append(f"| {name} | {ids.shape[0]} x {ids.shape[1]} | {err:.3e} | {e:.3e} | {4 * e:.3e} | {err / e:.2f} | {'yes' if err <= 4 * e else 'NO'} |")

    for name, f in th.FIXTURES.items():
        g = th.load_fixture(name)
        row(name, f["cfg"], f["trained"], g["ids"], g["mask"], th.FIXTURE_LENS, g["fp64"])
    for name, c in th.SWEEP.items():
        ids, mask, lens = th.sweep_inputs(name)
        row(name, c["cfg"], c["trained"], ids, mask, lens, th.encoder_fp64(th.weights(c["cfg"], c["trained"]), ids, lens, th.CFGS[c["cfg"]]["n_heads"]))

    hf = hf_model()
    lines += ["", f"## Timings: one call, full width (6 layers, dim 768), trained-like weights, ragged lengths "
              f"(HIP events around {a.calls} groups of {GROUP} warm calls)", "",
              "| B x L | `BERT.encode_ids` median ms | min | max | prompts / s | `transformers.DistilBertModel` fp32, same device: median ms | min | max |",
              "|---|---|---|---|---|---|---|---|"]
    for B, L in SHAPES:
        ids, mask, _ = prompts(B, L)
        med, lo, hi = timed(lambda: bert.encode_ids(ids, mask), a.calls)
        if hf is not None:
            am = mask.to(torch.int64)
            with torch.no_grad():
                want = hf(input_ids=ids.to(DEV), attention_mask=am.to(DEV)).last_hidden_state
                diff = float((want - bert.encode_ids(ids, mask))[mask.to(DEV)].abs().max())
                t = timed(lambda: hf(input_ids=ids.to(DEV), attention_mask=am.to(DEV)).last_hidden_state, a.calls)
            other = f"{t[0]:.3f} | {t[1]:.3f} | {t[2]:.3f} (outputs differ by {diff:.1e})"
        else:
            other = "transformers not importable here | | "
        lines.append(f"| {B} x {L} | {med:.3f} | {lo:.3f} | {hi:.3f} | {B / med * 1e3:.0f} | {other} |")
    for B, L, path in a.kernel_stats:
        with open(path) as fh:
            table = [ln.rstrip() for ln in fh if ln.startswith("|")]
        lines += ["", f"## Kernels of one profiled run at {B} x {L} (rocprofv3 --kernel-trace; 4 calls of 43 launches, and the copies and "
                  f"concatenations of the weight preparation)", ""] + table
    lines.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
