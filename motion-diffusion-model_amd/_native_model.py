"""What the modules with a native model behind them share (text_encoder, clip_text, stgcn, gru_recogniser, evaluator, smpl_mesh,
rotation2xyz; motion_process takes the stream check): the library handle, the device / stream check in front of a call, the
prepared-model cache and the workspace of include/mdm_hip.h's `*_workspace_bytes` entry points.  Each class keeps what is its own: the layout of its tables
(`_build_native`), what its parameters' version is (`_native_version`) and its chunking loop."""
import torch
import torch.nn as nn

from . import _native as nat


class _ParamContainer(nn.Module):
    """Parameters under the reference module's state-dict keys and nothing else: `load_state_dict`, `.to()`, `.eval()` and
    `state_dict()` behave as on the reference's module; there is no forward (the wrapper runs the HIP path)."""

    def __init__(self, shapes):
        super().__init__()
        self.shapes = list(shapes)
        for key, shape in self.shapes:
            mod = self
            *path, leaf = key.split(".")
            for name in path:
                if name not in mod._modules:
                    mod.add_module(name, nn.Module())
                mod = mod._modules[name]
            mod.register_parameter(leaf, nn.Parameter(torch.zeros(*shape), requires_grad=False))

    def forward(self, *a, **k):
        raise nat.MdmError("the evaluator's encoders are parameter containers: call EvaluatorMDMWrapper.get_co_embeddings / "
                           "get_motion_embeddings (the HIP path); there is no eager PyTorch forward")

    def version(self):
        return tuple((p._version, p.data_ptr()) for p in self.parameters())


def native_stream(lib, where, what):
    """The raw current-stream handle of `where` (a device or a tensor), None on the host.  The product library refuses a host
    device; `what` says in the message what should have been on the GPU."""
    dev = where.device if torch.is_tensor(where) else where
    if lib.path.endswith(nat.LIB_NAME) and dev.type != "cuda":      # (any other library is the CPU emulation)
        raise nat.MdmError(f"the MI355X HIP path needs {what} on a cuda (ROCm) device; got " + str(dev))
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None


class NativeModelMixin:
    """No nn.Module base: it combines with the classes that are modules and with those that are not.  A class sets `_native_lib`
    in its constructor (None: the product library); one that caches workspaces starts with `_ws = {}`."""

    _native_lib = None
    _prepared = None

    def _lib(self):
        return self._native_lib if self._native_lib is not None else nat.load_native()

    _stream = staticmethod(native_stream)

    def _model(self):
        """The C struct over the prepared tables; rebuilt (and the cached workspaces dropped) when `_native_version()` has changed:
        a parameter or buffer was replaced (load_state_dict, .to()) or written since.  `_build_native(keep)` returns the struct and
        appends to `keep` whatever the struct points into (the tensors that own its tables, its arrays of layer structs)."""
        ver = self._native_version()
        if self._prepared is None or self._prepared[0] != ver:
            keep = []
            model = self._build_native(keep)
            self._prepared = (ver, model, keep)
            self._ws = {}
        return self._prepared[1]

    def _workspace(self, symbol, model, *dims, dev, stream=None, cache=False):
        """(uint8 tensor, its size) for `symbol` = one of the `mdm_*_workspace_bytes` entry points at (model, *dims).  With `cache`
        the tensor is kept on the object per shape, device and stream (two streams may be inside a model at once)."""
        key = (*dims, str(dev), stream)
        if not cache or key not in self._ws:
            lib = self._lib()
            nbytes = getattr(lib, symbol)(*(nat.C.byref(a) if isinstance(a, nat.C.Structure) else a for a in (model,) + dims))
            if nbytes == 0:
                lib.check(-1, symbol)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes
            if not cache:
                return ws
            if len(self._ws) >= 8:           # (batches come in few shapes; an odd caller must not pile workspaces up)
                self._ws = {}
            self._ws[key] = ws
        return self._ws[key]
