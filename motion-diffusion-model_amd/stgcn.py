"""The ST-GCN action recogniser on the HIP path: `STGCN` of eval/a2m/recognition/models/stgcn.py (UESTC: ten blocks, layout `smpl`,
reads batch["output"]) and its six-block copy of eval/unconstrained/models/stgcn.py (`STGCNUnconstrained`: the 15-node `openpose`,
reads batch["x"]), eval mode, one person per sample.

The modules carry the reference's parameter and buffer names, so `load_state_dict(torch.load('uestc_rot6d_stgcn.tar'))` works as it
does upstream; the arithmetic is csrc/stgcn.h behind include/mdm_hip.h's mdm_stgcn_forward (exact fp32; no Conv2d / BatchNorm / einsum
call, and no fall-back when the library is missing).  The metrics of the unconstrained evaluation (FID statistics, KID, diversity,
precision / recall: eval/unconstrained/metrics/*.py) have their device path in mdm_amd/metrics.py; multimodality and accuracy of the
a2m family (eval/a2m/stgcn/*.py) run on the returned `features` / `yhat` as they are."""
import pickle

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from ._native_model import NativeModelMixin

ROW_CHUNK = 128            # samples per native call: bounds the workspace (a sample's result does not depend on the batch it is in)
TEMPORAL_KERNEL = 9
BN_EPS = 1e-5
DEFAULT_KINTREE_PATH = "./body_models/smpl/kintree_table.pkl"      # utils/config.py SMPL_KINTREE_PATH

# (c_in, c_out, stride, residual) per block; c_in None = the network's in_channels
A2M_BLOCKS = ((None, 64, 1, False), (64, 64, 1, True), (64, 64, 1, True), (64, 64, 1, True), (64, 128, 2, True), (128, 128, 1, True),
              (128, 128, 1, True), (128, 256, 2, True), (256, 256, 1, True), (256, 256, 1, True))
UNCONSTRAINED_BLOCKS = ((None, 64, 1, False), (64, 64, 1, True), (64, 64, 1, True), (64, 128, 2, True), (128, 128, 1, True),
                        (128, 256, 2, True))

# Skeletons as the neighbour of every node but one (-1): the undirected edges are {i, LINK[i]}.  Node counts and centres as in the
# two stgcnutils/graph.py copies; `openpose` is the 18-joint OpenPose skeleton of eval/a2m, `openpose15` the 15-node skeleton the
# copy under eval/unconstrained builds under the same name.
_LINKS = {
    "openpose": ([1, -1, 1, 2, 3, 1, 5, 6, 2, 8, 9, 5, 11, 12, 0, 0, 14, 15], 1),
    "openpose15": ([-1, 0, 1, 2, 3, 1, 5, 6, 1, 8, 9, 10, 8, 12, 13], 1),
    "ntu-rgb+d": ([1, 20, 20, 2, 20, 4, 5, 6, 20, 8, 9, 10, 0, 12, 13, 14, 0, 16, 17, 18, -1, 22, 7, 24, 11], 20),
    "ntu_edge": ([1, -1, 1, 2, 1, 4, 5, 6, 1, 8, 9, 10, 0, 12, 13, 14, 0, 16, 17, 18, 21, 7, 23, 11], 2),
}
LAYOUTS = tuple(_LINKS) + ("smpl", "smpl_noglobal")
STRATEGIES = ("uniform", "distance", "spatial")


def _kintree_edges(path):
    """(parent, child) pairs of kintree_table.pkl: row 0 the parents, row 1 the joint ids; the root's entry is skipped."""
    with open(path, "rb") as fh:
        try:
            kt = pickle.load(fh)
        except UnicodeDecodeError:
            fh.seek(0)
            kt = pickle.load(fh, encoding="latin1")
    kt = np.asarray(kt)
    return [(int(kt[0][i]), int(kt[1][i])) for i in range(1, kt.shape[1])]


class Graph:
    """The skeleton graph and its partitioned, column-normalised adjacency `A` [K, V, V] (ST-GCN, arXiv:1801.07455, section 3.4):
    `uniform` one partition, `distance` one per hop, `spatial` per hop the nodes as far from the centre as the target or farther
    (root + centripetal) and, from hop 1 on, the nearer ones (centrifugal).  Hop distances beyond max_hop are infinite -- also those
    to the centre, as in the reference: with max_hop = 1 most pairs compare inf with inf and land in the first partition."""

    def __init__(self, layout="openpose", strategy="uniform", kintree_path=DEFAULT_KINTREE_PATH, max_hop=1, dilation=1):
        self.max_hop, self.dilation, self.kintree_path = max_hop, dilation, kintree_path
        self.layout, self.strategy = layout, strategy
        if layout in _LINKS:
            link, self.center = _LINKS[layout]
            self.num_node = len(link)
            pairs = [(i, j) for i, j in enumerate(link) if j >= 0]
        elif layout == "smpl":
            self.num_node, self.center = 24, 0
            pairs = _kintree_edges(kintree_path)
        elif layout == "smpl_noglobal":
            self.num_node, self.center = 23, 0
            pairs = [(i - 1, j - 1) for i, j in _kintree_edges(kintree_path) if i != 0 and j != 0]
        else:
            raise NotImplementedError(f"layout {layout!r} is not supported (one of {', '.join(LAYOUTS)})")
        self.edge = [(i, i) for i in range(self.num_node)] + pairs
        self.hop_dis = self._hops()
        self.A = self._partition(strategy)

    def _hops(self):
        """Breadth-first hop counts up to max_hop; inf beyond."""
        V = self.num_node
        near = [set() for _ in range(V)]
        for i, j in self.edge:
            near[i].add(j)
            near[j].add(i)
        hop = np.full((V, V), np.inf)
        for s in range(V):
            seen, frontier = {s}, {s}
            hop[s, s] = 0
            for d in range(1, self.max_hop + 1):
                frontier = {j for i in frontier for j in near[i]} - seen
                for j in frontier:
                    hop[s, j] = d
                seen |= frontier
        return hop

    def _partition(self, strategy):
        V, hop = self.num_node, self.hop_dis
        hops = list(range(0, self.max_hop + 1, self.dilation))
        reach = np.zeros((V, V))
        for h in hops:
            reach[hop == h] = 1
        degree = reach.sum(0)
        norm = np.zeros((V, V))
        for i in range(V):
            if degree[i] > 0:
                norm[:, i] = reach[:, i] * degree[i] ** (-1)
        if strategy == "uniform":
            return norm[None].copy()
        if strategy == "distance":
            return np.stack([np.where(hop == h, norm, 0.0) for h in hops])
        if strategy == "spatial":
            to_centre = hop[:, self.center]
            same = to_centre[:, None] == to_centre[None, :]          # [j, i]: source j as far from the centre as target i
            farther = to_centre[:, None] > to_centre[None, :]
            parts = []
            for h in hops:
                at = hop == h
                root = np.where(at & same, norm, 0.0)
                close = np.where(at & ~same & farther, norm, 0.0)
                further = np.where(at & ~same & ~farther, norm, 0.0)
                if h == 0:
                    parts.append(root)
                else:
                    parts.append(root + close)
                    parts.append(further)
            return np.stack(parts)
        raise NotImplementedError(f"strategy {strategy!r} is not supported (one of {', '.join(STRATEGIES)})")


def t_out(t_in, stride):
    """Frames behind Conv2d(., ., (9, 1), (stride, 1), (4, 0))."""
    return (t_in - 1) // stride + 1


class _GraphConv(nn.Module):          # `gcn`: ConvTemporalGraphical's parameters (gcn.conv.weight [K c_out, c_in, 1, 1], gcn.conv.bias)
    def __init__(self, c_in, c_out, K):
        super().__init__()
        self.kernel_size = K
        self.conv = nn.Conv2d(c_in, c_out * K, kernel_size=(1, 1))


class _Block(nn.Module):
    """One st_gcn block as a parameter container: gcn.conv, tcn.0 (BN), tcn.2 (9 x 1 convolution), tcn.3 (BN) and, for a block
    that changes width or stride, residual.0 (1 x 1 convolution) and residual.1 (BN)."""

    def __init__(self, c_in, c_out, K, stride, residual, dropout=0):
        super().__init__()
        self.c_in, self.c_out, self.stride = c_in, c_out, stride
        self.gcn = _GraphConv(c_in, c_out, K)
        self.tcn = nn.Sequential(nn.BatchNorm2d(c_out), nn.ReLU(inplace=True),
                                 nn.Conv2d(c_out, c_out, (TEMPORAL_KERNEL, 1), (stride, 1), ((TEMPORAL_KERNEL - 1) // 2, 0)),
                                 nn.BatchNorm2d(c_out), nn.Dropout(dropout, inplace=True))
        if not residual:
            self.residual_kind = "none"
        elif c_in == c_out and stride == 1:
            self.residual_kind = "identity"
        else:
            self.residual_kind = "conv"
            self.residual = nn.Sequential(nn.Conv2d(c_in, c_out, kernel_size=1, stride=(stride, 1)), nn.BatchNorm2d(c_out))

    def forward(self, *a, **k):
        raise nat.MdmError("st_gcn blocks are parameter containers: call STGCN.forward (the HIP path); there is no eager PyTorch forward")


def _bn_fold(bn, bias=None):
    """BatchNorm in eval mode (with the bias of the layer in front of it) as y = x scale + shift, in fp64."""
    g, b = bn.weight.detach().double().cpu().numpy(), bn.bias.detach().double().cpu().numpy()
    mean, var = bn.running_mean.detach().double().cpu().numpy(), bn.running_var.detach().double().cpu().numpy()
    scale = g / np.sqrt(var + bn.eps)
    shift = b - mean * scale
    if bias is not None:
        shift = shift + bias * scale
    return scale, shift


class STGCN(NativeModelMixin, nn.Module):
    """eval/a2m/recognition/models/stgcn.py STGCN: same constructor, parameter / buffer names and batch contract.
    forward(batch) reads batch["output"] [N, V, in_channels, T] and sets batch["features"] (`squeeze()`d: [256] for N = 1) and
    batch["yhat"] [N, num_class]."""

    BLOCKS = A2M_BLOCKS
    INPUT_KEY = "output"
    LAYOUT_ALIASES = {}

    def __init__(self, in_channels, num_class, graph_args, edge_importance_weighting, device, **kwargs):
        super().__init__()
        self._native_lib = kwargs.pop("_native_lib", None)
        blocks = kwargs.pop("_blocks", None) or self.BLOCKS          # (reduced nets of the emulator tests)
        dropout = kwargs.pop("dropout", 0)
        if kwargs:
            raise TypeError(f"unexpected st_gcn arguments {sorted(kwargs)}: only `dropout` is taken")
        self.device = device
        self.num_class = num_class
        self.in_channels = in_channels
        self.losses = ["accuracy", "cross_entropy", "mixed"]
        self.criterion = torch.nn.CrossEntropyLoss(reduction='mean')

        graph_args = dict(graph_args)
        graph_args["layout"] = self.LAYOUT_ALIASES.get(graph_args.get("layout", "openpose"), graph_args.get("layout", "openpose"))
        self.graph = Graph(**graph_args)
        A = torch.tensor(self.graph.A, dtype=torch.float32, requires_grad=False)
        self.register_buffer('A', A)
        K, V = A.size(0), A.size(1)
        if len(blocks) > nat.STGCN_MAX_BLOCKS:
            raise ValueError(f"{len(blocks)} blocks: the native layer takes at most {nat.STGCN_MAX_BLOCKS}")

        self.data_bn = nn.BatchNorm1d(in_channels * V)
        self.st_gcn_networks = nn.ModuleList(
            _Block(in_channels if c_in is None else c_in, c_out, K, stride, residual, dropout=0 if i == 0 else dropout)
            for i, (c_in, c_out, stride, residual) in enumerate(blocks))
        if edge_importance_weighting:
            self.edge_importance = nn.ParameterList([nn.Parameter(torch.ones(self.A.size())) for _ in self.st_gcn_networks])
        else:
            self.edge_importance = [1] * len(self.st_gcn_networks)
        self.fcn = nn.Conv2d(blocks[-1][1], num_class, kernel_size=1)

    # ---- native model ----------------------------------------------------------------------------------------------------------
    def _native_version(self):
        return tuple((t._version, t.data_ptr()) for t in list(self.parameters()) + list(self.buffers()))

    def _neighbour_lists(self, A_b):
        """The non-zero A_b[k, v, w] per (k, w), v ascending -> (idx [K, V, 8] int32, weights [K, V, 8] fp32, counts [K, V] int32)."""
        K, V, _ = A_b.shape
        nb = nat.STGCN_MAX_NEIGHBOURS
        idx, wgt, cnt = np.zeros((K, V, nb), np.int32), np.zeros((K, V, nb), np.float32), np.zeros((K, V), np.int32)
        for k in range(K):
            for w in range(V):
                vs = np.nonzero(A_b[k, :, w])[0]
                if len(vs) > nb:
                    raise nat.MdmError(f"A * edge_importance has {len(vs)} non-zero entries in column {w} of partition {k}: the graph "
                                       f"convolution's neighbour lists hold at most {nb} (MDM_STGCN_MAX_NEIGHBOURS)")
                idx[k, w, :len(vs)], wgt[k, w, :len(vs)], cnt[k, w] = vs, A_b[k, vs, w], len(vs)
        return idx, wgt, cnt

    def _build_native(self, keep):
        """The prepared tables -- A * importance as neighbour lists, the BatchNorm scale / shift pairs (fp64, rounded once), the
        k-behind-c_out graph weights and the tap-major temporal weights -- and the C structs over them."""
        dev = self.fcn.weight.device

        def put(a, dtype=np.float32):
            t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
            keep.append(t)
            return t.data_ptr()

        A = self.A.detach().float().cpu()
        K, V = A.shape[0], A.shape[1]
        C = self.in_channels
        Cp = (C + 3) // 4 * 4
        blocks = (nat.MdmStgcnBlock * len(self.st_gcn_networks))()
        c_prev_p = Cp
        for b, (blk, imp) in enumerate(zip(self.st_gcn_networks, self.edge_importance)):
            imp = imp.detach().float().cpu() if torch.is_tensor(imp) else imp
            A_b = (A * imp).numpy()                                          # fp32, as the reference forms it
            idx, wgt, cnt = self._neighbour_lists(A_b)
            ci, co = blk.c_in, blk.c_out
            w = blk.gcn.conv.weight.detach().double().cpu().numpy().reshape(K, co, ci)
            gw = np.zeros((co, K, c_prev_p))
            gw[:, :, :ci] = w.transpose(1, 0, 2)
            gb = blk.gcn.conv.bias.detach().double().cpu().numpy().reshape(K, co)
            node_bias = np.einsum("kc,kw->wc", gb, A_b.astype(np.float64).sum(1))      # [V, c_out]
            s1, h1 = _bn_fold(blk.tcn[0])
            tw = blk.tcn[2].weight.detach().float().cpu().numpy()[:, :, :, 0].transpose(0, 2, 1)      # [c_out][9][c_out]
            s2, h2 = _bn_fold(blk.tcn[3], blk.tcn[2].bias.detach().double().cpu().numpy())
            d = blocks[b]
            d.c_in, d.c_out, d.stride, d.residual = ci, co, blk.stride, nat.STGCN_RES[blk.residual_kind]
            d.gcn_w, d.gcn_scale, d.gcn_shift = put(gw), put(s1), put(node_bias * s1[None, :] + h1[None, :])
            d.nbr_idx, d.nbr_w, d.nbr_cnt = put(idx, np.int32), put(wgt), put(cnt, np.int32)
            d.tcn_w, d.tcn_scale, d.tcn_shift = put(tw), put(s2), put(h2)
            if blk.residual_kind == "conv":
                rw = np.zeros((co, c_prev_p))
                rw[:, :ci] = blk.residual[0].weight.detach().double().cpu().numpy().reshape(co, ci)
                sr, hr = _bn_fold(blk.residual[1], blk.residual[0].bias.detach().double().cpu().numpy())
                d.res_w, d.res_scale, d.res_shift = put(rw), put(sr), put(hr)
            c_prev_p = co
        s0, h0 = _bn_fold(self.data_bn)
        keep.append(blocks)
        return nat.MdmStgcnModel(blocks=blocks, in_scale=put(s0), in_shift=put(h0),
                                 fcn_w=put(self.fcn.weight.detach().float().cpu().numpy().reshape(self.num_class, -1)),
                                 fcn_b=put(self.fcn.bias.detach().float().cpu().numpy()),
                                 n_blocks=len(blocks), V=V, K=K, num_class=self.num_class)

    def _check(self, x):
        if self.training:
            raise nat.MdmError("training mode is not implemented (BatchNorm batch statistics, dropout, gradients): call .eval() first")
        V = self.A.size(1)
        if x.dim() == 5:
            raise nat.MdmError(f"M > 1 is not implemented: the input must be [N, V, C, T] with one person per sample, got {tuple(x.shape)}")
        if x.dim() != 4 or x.shape[1] != V or x.shape[2] != self.in_channels:
            raise ValueError(f"batch[{self.INPUT_KEY!r}] must be [N, {V}, {self.in_channels}, T], got {tuple(x.shape)}")
        if x.shape[0] < 1 or x.shape[3] < 1:
            raise ValueError(f"batch[{self.INPUT_KEY!r}] must hold at least one sample and one frame, got {tuple(x.shape)}")

    def run(self, x):
        """x [N, V, C, T] -> (features [N, C_last], yhat [N, num_class]) on the parameters' device."""
        self._check(x)
        lib, model = self._lib(), self._model()
        dev = self.fcn.weight.device
        x = x.detach().to(device=dev, dtype=torch.float32).contiguous()
        stream = self._stream(lib, x, "the model")
        N, T = x.shape[0], x.shape[3]
        features = torch.empty(N, self.fcn.weight.shape[1], dtype=torch.float32, device=dev)
        yhat = torch.empty(N, self.num_class, dtype=torch.float32, device=dev)
        ws, nbytes = self._workspace("mdm_stgcn_workspace_bytes", model, min(N, ROW_CHUNK), T, dev=dev)
        for n0 in range(0, N, ROW_CHUNK):
            n = min(ROW_CHUNK, N - n0)
            lib.check(lib.mdm_stgcn_forward(nat.C.byref(model), x[n0:n0 + n].data_ptr(), features[n0:n0 + n].data_ptr(),
                                            yhat[n0:n0 + n].data_ptr(), n, T, ws.data_ptr(), nbytes, stream), "mdm_stgcn_forward")
        return features, yhat

    def forward(self, batch):
        with torch.no_grad():
            features, yhat = self.run(batch[self.INPUT_KEY])
        batch["features"] = features.squeeze()
        batch["yhat"] = yhat
        return batch

    def compute_accuracy(self, batch):
        confusion = torch.zeros(self.num_class, self.num_class, dtype=int)
        for label, pred in zip(batch["y"], batch["yhat"].max(dim=1).indices):
            confusion[label][pred] += 1
        return torch.trace(confusion) / torch.sum(confusion)

    def compute_loss(self, batch):
        raise nat.MdmError("training mode is not implemented: compute_loss belongs to the reference's training loop")


class STGCNUnconstrained(STGCN):
    """eval/unconstrained/models/stgcn.py STGCN: six blocks, reads batch["x"]; that tree's `openpose` layout is its 15-node skeleton."""

    BLOCKS = UNCONSTRAINED_BLOCKS
    INPUT_KEY = "x"
    LAYOUT_ALIASES = {"openpose": "openpose15"}
