"""Measures mdm_amd/evaluator.py on one MI355X and writes profiles/r09a_evaluator.md:
  * per fixture of tests/golden/evaluator_*.npz: max-abs error against the fp64 restatement next to e_ref and the 4 x e_ref bound;
  * embeddings per second at B = 32, T = 196 (motion) and L = 22 (text): HIP events around each of >= 20 warm calls, median and spread;
  * the marginal time of one recurrent step (gru_step_kernel launch + kernel): (49-step call - 1-step call) / 48 at B = 32;
  * for context only, a torch-ROCm restatement of the same three modules (nn.Conv1d / nn.GRU on packed sequences) on the same box.

    python tools/bench_evaluator.py [--calls 30] [--out profiles/r09a_evaluator.md]
"""
import argparse
import os
import socket
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import evaluator_helpers as eh  # noqa: E402

DEV = "cuda:0"


def timed(fn, calls, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


class TorchRestatement(nn.Module):
    """The same three networks in stock torch modules (context for the timings; not a parity target)."""

    def __init__(self, weights, d):
        super().__init__()
        mv, tx, mo = weights
        self.c1, self.c2 = nn.Conv1d(d["dim_pose"] - 4, d["dim_movement_enc_hidden"], 4, 2, 1), nn.Conv1d(d["dim_movement_enc_hidden"], d["dim_movement_latent"], 4, 2, 1)
        self.out = nn.Linear(d["dim_movement_latent"], d["dim_movement_latent"])
        for m, k in ((self.c1, "main.0"), (self.c2, "main.3"), (self.out, "out_net")):
            m.weight.data.copy_(mv[k + ".weight"]); m.bias.data.copy_(mv[k + ".bias"])
        self.enc = nn.ModuleDict()
        for name, sd, din in (("motion", mo, d["dim_movement_latent"]), ("text", tx, d["dim_word"])):
            H = sd["hidden"].shape[-1]
            e = nn.ModuleDict(dict(inp=nn.Linear(din, H), gru=nn.GRU(H, H, batch_first=True, bidirectional=True), o1=nn.Linear(2 * H, H),
                                   ln=nn.LayerNorm(H), o2=nn.Linear(H, sd["output_net.3.weight"].shape[0])))
            e["inp"].load_state_dict({"weight": sd["input_emb.weight"], "bias": sd["input_emb.bias"]})
            e["gru"].load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("gru.")})
            for m, k in ((e["o1"], "output_net.0"), (e["ln"], "output_net.1"), (e["o2"], "output_net.3")):
                m.load_state_dict({"weight": sd[k + ".weight"], "bias": sd[k + ".bias"]})
            self.enc[name] = e
            self.register_buffer(name + "_h0", sd["hidden"].clone())
        self.pos = nn.Linear(d["dim_pos_ohot"], d["dim_word"])
        self.pos.load_state_dict({"weight": tx["pos_emb.weight"], "bias": tx["pos_emb.bias"]})

    def _tail(self, name, x, lens):
        e = self.enc[name]
        h0 = getattr(self, name + "_h0").repeat(1, x.shape[0], 1)
        _, last = e["gru"](pack_padded_sequence(e["inp"](x), lens, batch_first=True), h0)
        return e["o2"](nn.functional.leaky_relu(e["ln"](e["o1"](torch.cat([last[0], last[1]], -1))), 0.2))

    def motion(self, motions, lens):
        x = motions[..., :-4].permute(0, 2, 1)
        x = nn.functional.leaky_relu(self.c2(nn.functional.leaky_relu(self.c1(x), 0.2)), 0.2).permute(0, 2, 1)
        return self._tail("motion", self.out(x), [l // 4 for l in lens])

    def text(self, word, pos, lens):
        return self._tail("text", word + self.pos(pos), lens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09a_evaluator.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available() and a.calls >= 20
    lines = ["# r09a — the evaluator (csrc/evaluator.h) on the MI355X", "",
             f"Box: `{socket.gethostname()}`, {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Written by `tools/bench_evaluator.py`.", "",
             "## Accuracy: max-abs error against the fp64 restatement, per fixture", "",
             "| fixture | output | GPU error | e_ref (reference fp32 vs fp64) | bound 4 x e_ref | ok |", "|---|---|---|---|---|---|"]
    rep = eh.pin_report()
    for name, f in eh.FIXTURES.items():
        inp, g = eh.fixture_inputs(name), eh.load_fixture(name)
        w = eh.make_wrapper(name, eh.fixture_weights(name), DEV)
        t = {k: torch.from_numpy(v) for k, v in inp.items()}
        got = {}
        if f["kind"] == "motion":
            got["motion"] = w.get_motion_embeddings(t["motions"], t["m_lens"])
        elif f["kind"] == "text":
            got["text"] = w._text_rows(t["word_embs"].to(DEV), t["pos_ohot"].to(DEV), inp["cap_lens"].tolist())
        else:
            got["text"], got["motion"] = w.get_co_embeddings(t["word_embs"], t["pos_ohot"], t["cap_lens"], t["motions"], t["m_lens"])
        for k, v in got.items():
            err = float(np.abs(v.cpu().numpy().astype(np.float64) - g[f"fp64_{k}"]).max())
            e = rep[name]["e_ref"]
            lines.append(f"| {name} | {k} | {err:.3e} | {e:.3e} | {4 * e:.3e} | {'yes' if err <= 4 * e else 'NO'} |")
        del w
    # timings, full width, default weights
    weights = eh.build_weights(1, eh.FULL)
    w = eh.make_wrapper(eh.FULL, weights, DEV)
    B, T, L = 32, 196, 22
    m_lens = sorted([40 + (i * 61) % 157 for i in range(31)] + [196], reverse=True)
    cap_lens = sorted([3 + (i * 7) % 20 for i in range(B)], reverse=True)
    motions = torch.from_numpy(eh.make_motion_inputs(1, B, T, 263, m_lens)).to(DEV)
    word, pos = (torch.from_numpy(x).to(DEV) for x in eh.make_text_inputs(1, B, L, 300, 15, cap_lens))
    rows = []
    rows.append(("motion, B = 32, T = 196, lengths 40..196 (49 steps)", timed(lambda: w._motion_rows(motions, m_lens), a.calls), B))
    rows.append(("text, B = 32, L = 22, lengths 3..22", timed(lambda: w._text_rows(word, pos, cap_lens), a.calls), B))
    t49 = timed(lambda: w._motion_rows(motions, [196] * B), a.calls)
    t1 = timed(lambda: w._motion_rows(motions, [4] * B), a.calls)
    ref = TorchRestatement(weights, eh.FULL).to(DEV).eval()
    with torch.no_grad():
        rows.append(("torch-ROCm restatement, motion (context)", timed(lambda: ref.motion(motions, m_lens), a.calls), B))
        rows.append(("torch-ROCm restatement, text (context)", timed(lambda: ref.text(word, pos, cap_lens), a.calls), B))
    lines += ["", f"## Timings (HIP events around each of {a.calls} warm calls, host-side length checks and allocations included)", "",
              "| call | median ms | min | max | embeddings / s (median) |", "|---|---|---|---|---|"]
    for what, (med, lo, hi), n in rows:
        lines.append(f"| {what} | {med:.3f} | {lo:.3f} | {hi:.3f} | {n / med * 1e3:.0f} |")
    lines += ["", f"One recurrent step at B = 32, H = 1024 (launch + `gru_step_kernel`, both directions): (49-step call {t49[0]:.3f} ms - 1-step call "
              f"{t1[0]:.3f} ms) / 48 = **{(t49[0] - t1[0]) / 48 * 1e3:.1f} us**.", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
