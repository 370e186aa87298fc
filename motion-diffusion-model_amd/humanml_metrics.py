"""The metrics of the HumanML3D / KIT evaluation on the HIP path, under the names and signatures of the reference's
data_loaders/humanml/utils/metrics.py: `euclidean_distance_matrix`, `calculate_top_k`, `calculate_R_precision`,
`calculate_matching_score`, `calculate_activation_statistics`, `calculate_frechet_distance`, `calculate_diversity` and
`calculate_multimodality`, and `retrieval`, the one fused call the evaluation loop (mdm_amd/humanml_eval.py) makes per loader.
Features are device tensors and stay there: the arithmetic is csrc/humanml_metrics.h (mdm_retrieval_ranks, mdm_dist_matrix) and
csrc/metrics.h (mdm_gather_dist, mdm_feature_stats), with no torch / numpy distance and no fall-back when the library is missing.
On the host: the random draws (numpy's global generator, the reference's calls in the reference's order) and the matrix square root
of `calculate_frechet_distance`, the default; `frechet_distance_device` is the same distance on the device (csrc/frechet.h).

Differences from upstream: distances are direct differences in fp32 (upstream: the Gram form, which cancels and returns nan for
equal rows); ranks are positions in a STABLE ascending sort (upstream's np.argsort is quicksort: the same wherever a row has no tie);
a group smaller than top_k is fine in `calculate_R_precision` (every row is a hit from the group's size on); sums and means are
fp64.  The library is mdm_amd.metrics' (`metrics.NATIVE_LIB`: None for the product library; the emulator tests bind theirs there)."""
import numpy as np
import torch

from . import _native as nat
from . import metrics as _m
from ._native_model import native_stream
from .metrics import calculate_activation_statistics, calculate_frechet_distance, gather_dist      # noqa: F401  (upstream's names)
from .metrics import calculate_fid_device, frechet_distance_device      # noqa: F401  (the device option of the distance)

MATCHING_GROUP_ROWS = 64      # calculate_matching_score's groups: one row tile each (a row's distance does not depend on its group)


def _tensor(x):
    return x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))


def _group_sizes(batch_sizes, n):
    """The reference's batches as a list of positive Python ints that add up to n."""
    try:
        sizes = [int(b) for b in batch_sizes]
        ok = all(s == b for s, b in zip(sizes, batch_sizes))
    except (TypeError, ValueError):
        sizes, ok = [], False
    if not ok or not sizes:
        raise ValueError(f"batch_sizes must be a non-empty sequence of integers, got {batch_sizes!r}")
    if min(sizes) < 1:
        raise ValueError(f"batch_sizes must be positive, got {min(sizes)}")
    if sum(sizes) != n:
        raise ValueError(f"batch_sizes add up to {sum(sizes)}, the embeddings hold {n} rows")
    return sizes


def retrieval(text, motion, batch_sizes, top_k=3):
    """(rank [N] int32, diag [N] fp32, topk_count [top_k] int64, diag_sum 0-dim fp64) on the embeddings' device, for text and motion
    embeddings [N, D] whose rows the host integers `batch_sizes` cut into the reference's batches: rank[i] is the position of motion
    i among its batch's motions by distance from text i (stable), diag[i] that distance, topk_count[k] the rows with rank <= k over
    all batches (upstream's summed top_k_mat) and diag_sum the sum of diag (upstream's summed dist_mat.trace())."""
    lib = _m._lib()
    q, c = _m._features(text, "text"), _m._features(motion, "motion")
    _m._same_width(q, c, "text", "motion")
    if q.shape[0] != c.shape[0]:
        raise ValueError(f"text holds {q.shape[0]} rows, motion {c.shape[0]}")
    if top_k != int(top_k) or not 1 <= int(top_k) <= nat.RETRIEVAL_TOPK_MAX:
        raise ValueError(f"top_k must be an integer between 1 and {nat.RETRIEVAL_TOPK_MAX}, got {top_k}")
    N, D = q.shape
    sizes = _group_sizes(batch_sizes, N)
    stream = native_stream(lib, q, "text")
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(q.device)
    ws, nbytes = _m._workspace(lib, "retrieval_ranks", N, 1, q.device)
    rank = torch.empty(N, dtype=torch.int32, device=q.device)
    diag = torch.empty(N, dtype=torch.float32, device=q.device)
    topk_count = torch.empty(int(top_k), dtype=torch.int64, device=q.device)
    diag_sum = torch.empty((), dtype=torch.float64, device=q.device)
    lib.check(lib.mdm_retrieval_ranks(q.data_ptr(), c.data_ptr(), N, D, offsets.data_ptr(), len(sizes), max(sizes), int(top_k),
                                      rank.data_ptr(), diag.data_ptr(), topk_count.data_ptr(), diag_sum.data_ptr(), ws.data_ptr(),
                                      nbytes, stream), "mdm_retrieval_ranks")
    return rank, diag, topk_count, diag_sum


def euclidean_distance_matrix(matrix1, matrix2):
    """dist [N1, N2] fp32: dist[i, j] = ||matrix1[i] - matrix2[j]||."""
    lib = _m._lib()
    a, b = _m._features(matrix1, "matrix1"), _m._features(matrix2, "matrix2")
    _m._same_width(a, b, "matrix1", "matrix2")
    stream = native_stream(lib, a, "matrix1")
    ws, nbytes = _m._workspace(lib, "dist_matrix", a.shape[0], 1, a.device)
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    lib.check(lib.mdm_dist_matrix(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1], out.data_ptr(), ws.data_ptr(), nbytes,
                                  stream), "mdm_dist_matrix")
    return out


def calculate_top_k(mat, top_k):
    """top_k_mat [size, top_k] bool for an index matrix (an argsort, row i's candidates in ascending distance): column k says whether
    i is among row i's first k + 1 entries.  Plain torch; like upstream's, an IndexError when the matrix has fewer than top_k columns."""
    mat = mat if torch.is_tensor(mat) else torch.as_tensor(np.asarray(mat))
    if top_k > mat.shape[1]:
        raise IndexError(f"index {mat.shape[1]} is out of bounds for axis 1 with size {mat.shape[1]}")
    own = torch.arange(mat.shape[0], device=mat.device).unsqueeze(1)
    return (mat[:, :top_k] == own).cumsum(dim=1) > 0


def calculate_R_precision(embedding1, embedding2, top_k, sum_all=False):
    """top_k_mat [N, top_k] bool (or its column sums, int64 [top_k]) with all rows as ONE group: whether embedding2[i] is among the
    k + 1 rows of embedding2 nearest to embedding1[i]."""
    n = len(embedding1)
    native_k = min(int(top_k), nat.RETRIEVAL_TOPK_MAX)
    rank, _, topk_count, _ = retrieval(embedding1, embedding2, [n], native_k)
    if sum_all and native_k == top_k:
        return topk_count
    top_k_mat = rank.unsqueeze(1) <= torch.arange(int(top_k), device=rank.device, dtype=rank.dtype).unsqueeze(0)
    return top_k_mat.sum(dim=0) if sum_all else top_k_mat


def calculate_matching_score(embedding1, embedding2, sum_all=False):
    """dist [N] fp32, ||embedding1[i] - embedding2[i]|| (or their sum, 0-dim fp64)."""
    n = len(embedding1)
    sizes = [MATCHING_GROUP_ROWS] * (n // MATCHING_GROUP_ROWS) + ([n % MATCHING_GROUP_ROWS] if n % MATCHING_GROUP_ROWS else [])
    _, diag, _, diag_sum = retrieval(embedding1, embedding2, sizes, 1)
    return diag_sum if sum_all else diag


def calculate_diversity(activation, diversity_times):
    """Upstream's two np.random.choice(replace=False) draws in upstream's order, one native call: the fp64 mean (0-dim, on the device)."""
    activation = _tensor(activation)
    if activation.dim() != 2:
        raise ValueError(f"activation must be [num_samples, dim_feat], got {tuple(activation.shape)}")
    num_samples = activation.shape[0]
    if not num_samples > diversity_times:
        raise ValueError(f"activation must hold more than diversity_times = {diversity_times} rows, got {num_samples}")
    first_indices = np.random.choice(num_samples, diversity_times, replace=False)
    second_indices = np.random.choice(num_samples, diversity_times, replace=False)
    return gather_dist(activation, first_indices, second_indices)[1]


def calculate_multimodality(activation, multimodality_times):
    """activation [N, R, D]: upstream's two draws of `multimodality_times` of the R repetitions, then the N x times pair distances
    ||activation[n, first[t]] - activation[n, second[t]]|| in one native call on the flattened rows: their fp64 mean (0-dim)."""
    activation = _tensor(activation)
    if activation.dim() != 3:
        raise ValueError(f"activation must be [num_sentences, num_per_sent, dim_feat], got {tuple(activation.shape)}")
    n, num_per_sent = activation.shape[0], activation.shape[1]
    if not num_per_sent > multimodality_times:
        raise ValueError(f"activation must hold more than multimodality_times = {multimodality_times} repetitions, got {num_per_sent}")
    first_dices = np.random.choice(num_per_sent, multimodality_times, replace=False)
    second_dices = np.random.choice(num_per_sent, multimodality_times, replace=False)
    base = np.arange(n, dtype=np.int64)[:, None] * num_per_sent
    return gather_dist(activation.reshape(n * num_per_sent, activation.shape[2]), (base + first_dices[None, :]).reshape(-1),
                       (base + second_dices[None, :]).reshape(-1))[1]
