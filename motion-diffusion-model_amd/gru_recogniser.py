"""The HumanAct12 GRU action recogniser on the HIP path: `MotionDiscriminator` / `MotionDiscriminatorForFID` of
eval/a2m/action2motion/models.py, the network behind A2MEvaluation (eval/a2m/gru_eval.py: accuracy, FID, diversity, multimodality).

The modules carry the reference's constructor, parameter names (`recurrent.weight_ih_l0` ..., `linear1.*`, `linear2.*`) and
`forward(motion_sequence, lengths, hidden_unit)`, so `load_classifier` / `load_classifier_for_fid` read
`./assets/actionrecognition/humanact12_gru.tar` as they do upstream; the arithmetic is csrc/gru_recogniser.h behind
include/mdm_hip.h's mdm_gru_cls_forward (exact fp32; no torch.nn.GRU call, and no fall-back when the library is missing).  Both classes
are views of the same native call: one returns `yhat`, the other `features`.

Differences from upstream, both on inputs upstream mishandles: `lengths=None` raises a ValueError (upstream fails on `None - 1`); a
CPU `lengths` outside [1, T] is refused, a device `lengths` is clamped to [1, T] by the kernel without a host synchronisation
(upstream wraps a zero length to the last frame and raises an index error beyond T)."""
import torch
import torch.nn as nn

from . import _native as nat
from ._native_model import NativeModelMixin

ROW_CHUNK = 256            # sequences per native call: bounds the workspace (a row's result does not depend on the batch it is in)
MID = 30                   # linear1's width


class MotionDiscriminator(NativeModelMixin, nn.Module):
    """eval/a2m/action2motion/models.py MotionDiscriminator: forward returns the logits [bs, output_size]."""

    def __init__(self, input_size, hidden_size, hidden_layer, device, output_size=12, use_noise=None, _native_lib=None):
        super().__init__()
        self.device = device
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.hidden_layer = hidden_layer
        self.use_noise = use_noise
        self._native_lib = _native_lib
        if not 1 <= hidden_layer <= nat.GRU_CLS_MAX_LAYERS:
            raise ValueError(f"hidden_layer = {hidden_layer}: the native layer takes 1 to {nat.GRU_CLS_MAX_LAYERS} GRU layers")
        self.recurrent = nn.GRU(input_size, hidden_size, hidden_layer)      # a parameter container: its forward is never called
        self.linear1 = nn.Linear(hidden_size, MID)
        self.linear2 = nn.Linear(MID, output_size)

    # ---- native model --------------------------------------------------------------------------------------------------------------
    def _native_version(self):
        return tuple((t._version, t.data_ptr()) for t in self.parameters())

    def _build_native(self, keep):
        """The C struct over fp32, contiguous, 16-byte aligned copies of the parameters on their device (the parameters themselves
        where they already are that)."""
        dev = self.linear1.weight.device

        def put(t):
            t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
            if t.data_ptr() % 16 != 0:
                pad = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
                off = (-pad.data_ptr() % 16) // 4
                pad[off:off + t.numel()] = t.reshape(-1)
                t = pad[off:off + t.numel()]
            keep.append(t)
            return t.data_ptr()

        model = nat.MdmGruClsModel(lin1_w=put(self.linear1.weight), lin1_b=put(self.linear1.bias), lin2_w=put(self.linear2.weight),
                                   lin2_b=put(self.linear2.bias), input_size=self.input_size, hidden_size=self.hidden_size,
                                   num_layers=self.hidden_layer, mid=self.linear1.out_features, num_class=self.linear2.out_features)
        for l in range(self.hidden_layer):
            y = model.layers[l]
            y.w_ih, y.w_hh = put(getattr(self.recurrent, f"weight_ih_l{l}")), put(getattr(self.recurrent, f"weight_hh_l{l}"))
            y.b_ih, y.b_hh = put(getattr(self.recurrent, f"bias_ih_l{l}")), put(getattr(self.recurrent, f"bias_hh_l{l}"))
        return model

    def run(self, motion_sequence, lengths=None, hidden_unit=None):
        """motion_sequence [bs, njoints, nfeats, T] -> (features [bs, 30], yhat [bs, output_size]) on the parameters' device."""
        if lengths is None:
            raise ValueError("`lengths` is required: the classifier reads the GRU's output at frame lengths - 1 of every sequence")
        if motion_sequence.dim() != 4:
            raise ValueError(f"motion_sequence must be [bs, njoints, nfeats, num_frames], got {tuple(motion_sequence.shape)}")
        bs, njoints, nfeats, T = motion_sequence.shape
        if njoints * nfeats != self.input_size:
            raise ValueError(f"motion_sequence has njoints * nfeats = {njoints * nfeats} features, the classifier takes {self.input_size}")
        if bs < 1 or T < 1:
            raise ValueError(f"motion_sequence must hold at least one sequence and one frame, got {tuple(motion_sequence.shape)}")
        if hidden_unit is None:
            hidden_unit = self.initHidden(bs, self.hidden_layer)
        if tuple(hidden_unit.shape) != (self.hidden_layer, bs, self.hidden_size):
            raise ValueError(f"hidden_unit must be [{self.hidden_layer}, {bs}, {self.hidden_size}], got {tuple(hidden_unit.shape)}")
        lengths = torch.as_tensor(lengths)
        if lengths.dtype.is_floating_point or lengths.dtype == torch.bool or tuple(lengths.shape) != (bs,):
            raise ValueError(f"`lengths` must be an integer tensor of shape [{bs}], got {lengths.dtype} {tuple(lengths.shape)}")
        if not lengths.is_cuda and (int(lengths.min()) < 1 or int(lengths.max()) > T):
            raise ValueError(f"`lengths` must lie in [1, {T}] (the frames of motion_sequence), got {int(lengths.min())} .. {int(lengths.max())}")

        lib, model = self._lib(), self._model()
        dev = self.linear1.weight.device
        stream = self._stream(lib, dev, "the model")
        x = motion_sequence.detach().reshape(bs, njoints * nfeats, T).to(device=dev).float().contiguous()
        h0 = hidden_unit.detach().to(device=dev, dtype=torch.float32).contiguous()
        lens = lengths.to(device=dev, dtype=torch.int32).contiguous()
        features = torch.empty(bs, model.mid, dtype=torch.float32, device=dev)
        yhat = torch.empty(bs, model.num_class, dtype=torch.float32, device=dev)
        chunk = min(bs, ROW_CHUNK)
        ws, nbytes = self._workspace("mdm_gru_cls_workspace_bytes", model, chunk, T, dev=dev)
        for n0 in range(0, bs, chunk):
            n = min(chunk, bs - n0)
            h0c = h0 if n == bs else h0[:, n0:n0 + n].contiguous()
            lib.check(lib.mdm_gru_cls_forward(nat.C.byref(model), x[n0:n0 + n].data_ptr(), lens[n0:n0 + n].data_ptr(), h0c.data_ptr(),
                                              features[n0:n0 + n].data_ptr(), yhat[n0:n0 + n].data_ptr(), n, T, ws.data_ptr(), nbytes,
                                              stream), "mdm_gru_cls_forward")
        return features, yhat

    def forward(self, motion_sequence, lengths=None, hidden_unit=None):
        with torch.no_grad():
            return self.run(motion_sequence, lengths, hidden_unit)[1]

    def initHidden(self, num_samples, layer):
        return torch.randn(layer, num_samples, self.hidden_size, device=self.device, requires_grad=False)


class MotionDiscriminatorForFID(MotionDiscriminator):
    """eval/a2m/action2motion/models.py MotionDiscriminatorForFID: forward returns tanh(linear1(.)) [bs, 30]."""

    def forward(self, motion_sequence, lengths=None, hidden_unit=None):
        with torch.no_grad():
            return self.run(motion_sequence, lengths, hidden_unit)[0]


model_path = "./assets/actionrecognition/humanact12_gru.tar"


def _load(cls, input_size_raw, num_classes, device):
    model = torch.load(model_path, map_location=device)
    classifier = cls(input_size_raw, 128, 2, device=device, output_size=num_classes).to(device)
    classifier.load_state_dict(model["model"])
    classifier.eval()
    return classifier


def load_classifier(input_size_raw, num_classes, device):
    return _load(MotionDiscriminator, input_size_raw, num_classes, device)


def load_classifier_for_fid(input_size_raw, num_classes, device):
    return _load(MotionDiscriminatorForFID, input_size_raw, num_classes, device)
