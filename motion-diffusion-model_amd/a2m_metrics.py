"""The metrics of the action-to-motion evaluations (eval/a2m/action2motion and eval/a2m/stgcn: diversity.py, accuracy.py) on the HIP
path: `calculate_diversity_multimodality` and `calculate_accuracy` under the reference's names, on device activations.

`calculate_diversity_multimodality` covers both upstream variants (`seed` is the ST-GCN one's).  Upstream indexes a device `labels`
tensor inside its rejection loop (one synchronisation per draw); here `labels` goes to the host ONCE, the index sequence is drawn on
the host exactly as upstream draws it -- two randint vectors, then the quota loop with its rejection draws, so numpy's global
generator ends in upstream's state -- and the pair distances are two mdm_gather_dist calls (csrc/metrics.h).

`calculate_accuracy` replaces the Python iteration per sample by one mdm_confusion call per batch (csrc/humanml_metrics.h) into one
device matrix.  A label outside [0, num_labels) is an error (upstream: an IndexError, or a silent wrap for a negative one).

The library is mdm_amd.metrics' (`metrics.NATIVE_LIB`: None for the product library; the emulator tests bind theirs there)."""
import numpy as np
import torch

from . import metrics as _m
from ._native_model import native_stream

DIVERSITY_TIMES = 200
MULTIMODALITY_TIMES = 20
STYLES = ("action2motion", "stgcn")


def draw_pairs(labels, num_motions, num_labels, seed=None, unconstrained=False):
    """Upstream's index sequence on numpy's global generator: (first, second) of diversity, then (first, second) of multimodality
    (empty if `unconstrained`).  `labels` is a host integer array."""
    if seed is not None:
        np.random.seed(seed)
    first_indices = np.random.randint(0, num_motions, DIVERSITY_TIMES)
    second_indices = np.random.randint(0, num_motions, DIVERSITY_TIMES)
    mm_first, mm_second = [], []
    if not unconstrained:
        label_quotas = np.zeros(num_labels)
        label_quotas[np.unique(labels)] = MULTIMODALITY_TIMES      # a label that does not appear keeps a zero quota
        while np.any(label_quotas > 0):
            first_idx = np.random.randint(0, num_motions)
            first_label = labels[first_idx]
            if not label_quotas[first_label]:
                continue
            second_idx = np.random.randint(0, num_motions)
            while labels[second_idx] != first_label:
                second_idx = np.random.randint(0, num_motions)
            label_quotas[first_label] -= 1
            mm_first.append(first_idx)
            mm_second.append(second_idx)
    return (first_indices, second_indices), (np.asarray(mm_first, dtype=np.int64), np.asarray(mm_second, dtype=np.int64))


def calculate_diversity_multimodality(activations, labels, num_labels, seed=None, unconstrained=False):
    """(diversity, multimodality) as Python floats: the mean distance of 200 random pairs, and the sum of the distances of 20 pairs of
    equal label per label that appears, divided by 20 * num_labels as upstream divides it (nan if `unconstrained`)."""
    x = _m._features(activations, "activations")
    num_motions = x.shape[0]
    host_labels = None
    if not unconstrained:
        host_labels = (labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)).astype(np.int64).reshape(-1)
        if len(host_labels) != num_motions:
            raise ValueError(f"labels holds {len(host_labels)} entries, activations {num_motions} rows")
        if host_labels.min() < 0 or host_labels.max() >= num_labels:
            raise ValueError(f"labels must lie in [0, {num_labels}), got {int(host_labels.min())} .. {int(host_labels.max())}")
    (first, second), (mm_first, mm_second) = draw_pairs(host_labels, num_motions, num_labels, seed, unconstrained)
    diversity = float(_m.gather_dist(x, first, second)[1].item())
    if unconstrained:
        return diversity, float("nan")
    mean = float(_m.gather_dist(x, mm_first, mm_second)[1].item())
    return diversity, mean * len(mm_first) / (MULTIMODALITY_TIMES * num_labels)


def confusion(yhat, labels, num_labels, confusion_matrix=None, bad=None):
    """One mdm_confusion call: (pred [N] int32, confusion [C, C] int64, bad 0-dim int32) on yhat's device.  Given `confusion_matrix`
    and `bad` (from an earlier call), the call adds to them."""
    lib = _m._lib()
    y = _m._features(yhat, "yhat")
    N, C = y.shape
    if C != num_labels:
        raise ValueError(f"yhat has {C} classes, num_labels is {num_labels}")
    lab = (labels if torch.is_tensor(labels) else torch.as_tensor(np.asarray(labels))).detach().reshape(-1)
    if lab.numel() != N:
        raise ValueError(f"labels holds {lab.numel()} entries, yhat {N} rows")
    lab = lab.to(device=y.device, dtype=torch.int32).contiguous()
    stream = native_stream(lib, y, "yhat")
    if confusion_matrix is None:
        confusion_matrix = torch.zeros(C, C, dtype=torch.int64, device=y.device)
        bad = torch.zeros((), dtype=torch.int32, device=y.device)
    elif (tuple(confusion_matrix.shape) != (C, C) or confusion_matrix.dtype != torch.int64 or not confusion_matrix.is_contiguous()
          or confusion_matrix.device != y.device or bad is None or bad.dtype != torch.int32 or bad.device != y.device):
        raise ValueError(f"confusion_matrix must be a contiguous int64 [{C}, {C}] tensor and bad an int32 scalar, both on {y.device}")
    ws, nbytes = _m._workspace(lib, "confusion", N, 1, y.device)
    pred = torch.empty(N, dtype=torch.int32, device=y.device)
    lib.check(lib.mdm_confusion(y.data_ptr(), lab.data_ptr(), N, C, pred.data_ptr(), confusion_matrix.data_ptr(), bad.data_ptr(),
                                ws.data_ptr(), nbytes, stream), "mdm_confusion")
    return pred, confusion_matrix, bad


def calculate_accuracy(model, motion_loader, num_labels, classifier, device, style="action2motion"):
    """(accuracy float, confusion LongTensor [num_labels, num_labels] on the host).  `style` is the upstream calling convention of
    `classifier`: "action2motion" -- classifier(batch["output_xyz"], lengths=batch["lengths"]) returns the scores; "stgcn" --
    classifier(batch)["yhat"].  `model` and `device` are upstream's unused arguments."""
    if style not in STYLES:
        raise ValueError(f"style must be one of {STYLES}, got {style!r}")
    matrix = bad = None
    with torch.no_grad():
        for batch in motion_loader:
            batch_prob = classifier(batch["output_xyz"], lengths=batch["lengths"]) if style == "action2motion" else classifier(batch)["yhat"]
            _, matrix, bad = confusion(batch_prob, batch["y"], num_labels, matrix, bad)
    if matrix is None:
        raise ValueError("motion_loader yields no batch")
    if int(bad.item()) != 0:
        raise ValueError(f"{int(bad.item())} labels lie outside [0, {num_labels})")
    matrix = matrix.cpu()
    accuracy = torch.trace(matrix) / torch.sum(matrix)
    return accuracy.item(), matrix


def calculate_accuracy_stgcn(model, motion_loader, num_labels, classifier, device):
    return calculate_accuracy(model, motion_loader, num_labels, classifier, device, style="stgcn")
