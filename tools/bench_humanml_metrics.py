"""Measures mdm_amd/humanml_metrics.py and mdm_amd/a2m_metrics.py on one MI355X and writes profiles/r22a_humanml_metrics.md:
  * the metric part of evaluate_matching_score for ONE loader at the HumanML3D test-set size (145 batches of 32 embeddings, D = 512):
    the device path -- concatenate the batches' embeddings on the device, one `retrieval` call, the four numbers to the host -- per
    call, as the device span (HIP events) and the host wall time ending in the host reads: median / min / max of --calls calls after
    two warm calls; next to it the host loop on the same device tensors (tests/humanml_metrics_helpers.py host_retrieval_loop: two
    .cpu().numpy() copies, a Gram-form matrix, a trace, an argsort and the top-k hits per batch), the same number of calls;
  * calculate_diversity_multimodality at N = 1190 activations of D = 256 with 12 labels: the device path (labels to the host once, the
    draws on the host, two native calls) against this tool's restatement of the host path on the same device tensors (a device label
    read per draw, one torch.dist per pair, accumulated on the device), under the same seed;
  * calculate_accuracy's arithmetic at the same size: one mdm_confusion call against one Python iteration per sample on device tensors;
  * the accuracy figures of the same session for the two timed shapes.
There is no speed gate: the note is the record.

    python tools/bench_humanml_metrics.py [--calls 10] [--out profiles/r22a_humanml_metrics.md]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import humanml_metrics_helpers as hh  # noqa: E402

DEV = "cuda:0"
GROUPS, GROUP_ROWS, D = 145, 32, 512
A2M_N, A2M_D, A2M_LABELS = 1190, 256, 12


def host_diversity_multimodality(activations, labels, num_labels):
    """The host path on device tensors: every label read and every pair distance is a device operation of its own."""
    n = len(activations)
    first, second = np.random.randint(0, n, 200), np.random.randint(0, n, 200)
    diversity = 0
    for i, j in zip(first, second):
        diversity += torch.dist(activations[i, :], activations[j, :])
    diversity /= 200
    quotas = np.zeros(num_labels)
    quotas[labels.unique().cpu().numpy()] = 20
    multimodality = 0
    while np.any(quotas > 0):
        i = np.random.randint(0, n)
        li = labels[i]
        if not quotas[li]:
            continue
        j = np.random.randint(0, n)
        while li != labels[j]:
            j = np.random.randint(0, n)
        quotas[li] -= 1
        multimodality += torch.dist(activations[i, :], activations[j, :])
    multimodality /= 20 * num_labels
    return diversity.item(), multimodality.item()


def host_confusion(yhat, labels, num_labels):
    confusion = torch.zeros(num_labels, num_labels, dtype=torch.long)
    pred = yhat.max(dim=1).indices
    for label, p in zip(labels, pred):
        confusion[label][p] += 1
    return confusion


def timed(fn, calls, warm=2):
    """(device span ms, wall ms) as (median, min, max) each; the wall clock stops when fn has returned (fn ends in its host reads)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return [(statistics.median(v), min(v), max(v)) for v in (dev, wall)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22a_humanml_metrics.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available()
    from mdm_amd import a2m_metrics as A
    from mdm_amd import humanml_metrics as H

    rows = []
    # ---- matching score / R-precision of one loader
    sizes = [GROUP_ROWS] * GROUPS
    text_n, motion_n = hh.make_pair(GROUPS * GROUP_ROWS, D, 6, 1.0, 9101)
    batches = [(torch.from_numpy(text_n[b:e]).to(DEV), torch.from_numpy(motion_n[b:e]).to(DEV)) for b, e in hh.groups(sizes)]

    def device_path():
        text, motion = torch.cat([t for t, _ in batches]), torch.cat([m for _, m in batches])
        _, _, topk, diag_sum = H.retrieval(text, motion, sizes, hh.TOP_K)
        return topk.cpu().numpy(), float(diag_sum.item())

    def call_only():
        return H.retrieval(text_all, motion_all, sizes, hh.TOP_K)

    text_all, motion_all = torch.cat([t for t, _ in batches]), torch.cat([m for _, m in batches])
    d_dev, d_wall = timed(device_path, a.calls)
    c_dev, c_wall = timed(call_only, a.calls)
    h_dev, h_wall = timed(lambda: hh.host_retrieval_loop(batches), a.calls)
    topk, diag_sum = device_path()
    h_topk, h_trace, _ = hh.host_retrieval_loop(batches)
    want_rank, want_diag, want_topk = hh.retrieval_fp64(text_n, motion_n, sizes)
    fragile = hh.fragile_rows(text_n, motion_n, sizes)[0]
    rank, diag, _, _ = call_only()
    rows.append(("matching score + R-precision, one loader: cat + `retrieval` + host reads", d_dev, d_wall))
    rows.append(("... the `retrieval` call alone (two launches, results left on the device)", c_dev, c_wall))
    rows.append(("... the host loop on the same device tensors (145 batches)", h_dev, h_wall))
    note1 = (f"top-k counts: device {topk.tolist()}, host loop {h_topk.tolist()}, fp64 {want_topk.tolist()} of {len(text_n)} rows "
             f"({fragile} fragile rows in this input; ranks equal to fp64 in {int((rank.cpu().numpy() == want_rank).sum())} rows); "
             f"matching-score sum: device {diag_sum:.6f}, host loop {h_trace:.6f}, fp64 {want_diag.sum():.6f}; diag relative error "
             f"{hh.rel_err(diag.cpu().numpy(), want_diag):.3e} (bound {hh.rel_bound(D):.3e})")

    # ---- a2m diversity / multimodality
    rs = np.random.RandomState(9102)
    labels_n = rs.randint(0, A2M_LABELS, A2M_N).astype(np.int64)
    x_n = (rs.standard_normal((A2M_LABELS, A2M_D))[labels_n] + 0.5 * rs.standard_normal((A2M_N, A2M_D))).astype(np.float32)
    x, labels = torch.from_numpy(x_n).to(DEV), torch.from_numpy(labels_n).to(DEV)
    np.random.seed(5)
    m_dev, m_wall = timed(lambda: A.calculate_diversity_multimodality(x, labels, A2M_LABELS), a.calls)
    np.random.seed(6)
    hm_dev, hm_wall = timed(lambda: host_diversity_multimodality(x, labels, A2M_LABELS), a.calls)
    np.random.seed(7)
    got = A.calculate_diversity_multimodality(x, labels, A2M_LABELS)
    np.random.seed(7)
    host = host_diversity_multimodality(x, labels, A2M_LABELS)
    want = hh.a2m_fp64(x_n, labels_n, A2M_LABELS, seed=7)
    rows.append((f"`calculate_diversity_multimodality`, N = {A2M_N}, {A2M_LABELS} labels, D = {A2M_D}", m_dev, m_wall))
    rows.append(("... the host path on the same device tensors", hm_dev, hm_wall))
    note2 = (f"same seed: device {got[0]:.7f} / {got[1]:.7f}, host path {host[0]:.7f} / {host[1]:.7f}, fp64 {want[0]:.7f} / {want[1]:.7f}")

    # ---- accuracy
    yhat = torch.from_numpy(rs.standard_normal((A2M_N, A2M_LABELS)).astype(np.float32)).to(DEV)
    k_dev, k_wall = timed(lambda: A.confusion(yhat, labels, A2M_LABELS)[1].cpu(), a.calls)
    hk_dev, hk_wall = timed(lambda: host_confusion(yhat, labels, A2M_LABELS), a.calls)
    same = torch.equal(A.confusion(yhat, labels, A2M_LABELS)[1].cpu(), host_confusion(yhat, labels, A2M_LABELS))
    rows.append((f"argmax + confusion matrix, N = {A2M_N}, {A2M_LABELS} labels: one `mdm_confusion` call + the matrix to the host", k_dev, k_wall))
    rows.append(("... one Python iteration per sample on the same device tensors", hk_dev, hk_wall))
    note3 = f"the two confusion matrices are {'equal' if same else 'DIFFERENT'}"

    lines = ["# r22a — the HumanML3D and a2m evaluation metrics (csrc/humanml_metrics.h) on the MI355X", "",
             f"Device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Written by `tools/bench_humanml_metrics.py`.", "",
             "## Timings", "",
             f"Every row: {a.calls} calls after two warm calls in one process; `device` is the span between HIP events around the call, `wall` "
             "a host clock from before the call until its results are on the host (for the `retrieval` call alone: until a synchronise).  "
             f"The loader is {GROUPS} batches of {GROUP_ROWS} text and motion embeddings of D = {D}, already on the device, as "
             "`get_co_embeddings` returns them.  The host rows are restatements of the reference's host code on the library calls it makes "
             "(the reference tree is not part of this repository), run on the same device tensors in the same session.", "",
             "| what | device ms median | min | max | wall ms median | min | max |", "|---|---|---|---|---|---|---|"]
    for name, (dm, dl, dh), (wm, wl, wh) in rows:
        lines.append(f"| {name} | {dm:.3f} | {dl:.3f} | {dh:.3f} | {wm:.3f} | {wl:.3f} | {wh:.3f} |")
    lines += ["", "Not measured: per-kernel times (no traced run), the share of any peak, the reference's own functions (the host rows are "
              "restatements), the networks that produce the embeddings, and a full evaluation run.  No speed gate applies.", "",
              "## Values in the same session", "", f"* {note1}.", f"* {note2}.", f"* {note3}.", ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
