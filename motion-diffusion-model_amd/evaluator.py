"""The HumanML3D / KIT evaluator on the HIP path: `EvaluatorMDMWrapper` of data_loaders/humanml/networks/evaluator_wrapper.py:121-187
over the MovementConvEncoder, MotionEncoderBiGRUCo and TextEncoderBiGRUCo of networks/modules.py:79-98, :311-386.

The three encoders are plain parameter containers with the reference's state-dict keys; the arithmetic is csrc/evaluator.h behind
include/mdm_hip.h's mdm_eval_* entry points (exact fp32; no nn.GRU / Conv1d call, and no fall-back when the library is missing).
R-precision, FID, matching score, diversity and multimodality (data_loaders/humanml/utils/metrics.py) run on the returned
embeddings as they are."""
import os
from os.path import join as pjoin

import numpy as np
import torch

from . import _native as nat
from ._native_model import NativeModelMixin, _ParamContainer      # (_ParamContainer: text_encoder / clip_text took it from here)

DIM_POS_OHOT = 15          # len(POS_enumerator), data_loaders/humanml/utils/word_vectorizer.py
ROW_CHUNK = 128            # rows per native call: bounds the workspace (a row's result does not depend on the batch it is in)

_GRU_KEYS = [f"gru.{n}_l0{sfx}" for sfx in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def default_opt(dataset_name, device):
    """evaluator_wrapper.py:124-139, entry for entry."""
    return {
        'dataset_name': dataset_name,
        'device': device,
        'dim_word': 300,
        'max_motion_length': 196,
        'dim_pos_ohot': DIM_POS_OHOT,
        'dim_motion_hidden': 1024,
        'max_text_len': 20,
        'dim_text_hidden': 512,
        'dim_coemb_hidden': 512,
        'dim_pose': 263 if dataset_name == 'humanml' else 251,
        'dim_movement_enc_hidden': 512,
        'dim_movement_latent': 512,
        'checkpoints_dir': '.',
        'unit_length': 4,
    }


def _gru_shapes(hidden):
    shapes = {}
    for sfx in ("", "_reverse"):
        shapes[f"gru.weight_ih_l0{sfx}"] = (3 * hidden, hidden)
        shapes[f"gru.weight_hh_l0{sfx}"] = (3 * hidden, hidden)
        shapes[f"gru.bias_ih_l0{sfx}"] = (3 * hidden,)
        shapes[f"gru.bias_hh_l0{sfx}"] = (3 * hidden,)
    return [(k, shapes[k]) for k in _GRU_KEYS]


def _output_net_shapes(hidden, out):
    return [("output_net.0.weight", (hidden, 2 * hidden)), ("output_net.0.bias", (hidden,)),
            ("output_net.1.weight", (hidden,)), ("output_net.1.bias", (hidden,)),
            ("output_net.3.weight", (out, hidden)), ("output_net.3.bias", (out,))]


def movement_encoder_shapes(input_size, hidden_size, output_size):
    return [("main.0.weight", (hidden_size, input_size, 4)), ("main.0.bias", (hidden_size,)),
            ("main.3.weight", (output_size, hidden_size, 4)), ("main.3.bias", (output_size,)),
            ("out_net.weight", (output_size, output_size)), ("out_net.bias", (output_size,))]


def text_encoder_shapes(word_size, pos_size, hidden_size, output_size):
    return [("hidden", (2, 1, hidden_size)), ("pos_emb.weight", (word_size, pos_size)), ("pos_emb.bias", (word_size,)),
            ("input_emb.weight", (hidden_size, word_size)), ("input_emb.bias", (hidden_size,))] + \
        _gru_shapes(hidden_size) + _output_net_shapes(hidden_size, output_size)


def motion_encoder_shapes(input_size, hidden_size, output_size):
    return [("hidden", (2, 1, hidden_size)), ("input_emb.weight", (hidden_size, input_size)), ("input_emb.bias", (hidden_size,))] + \
        _gru_shapes(hidden_size) + _output_net_shapes(hidden_size, output_size)


def _check_widths(opt):
    """What the kernels' tiles take (include/mdm_hip.h mdm_eval_model_t), refused here, at create time."""
    for k in ("dim_motion_hidden", "dim_text_hidden"):
        if opt[k] not in (256, 512, 768, 1024):
            raise ValueError(f"{k} = {opt[k]}: the GRU step kernel and the LayerNorm take a hidden size of 256, 512, 768 or 1024")
    for k in ("dim_movement_enc_hidden", "dim_movement_latent", "dim_coemb_hidden", "dim_word"):
        if opt[k] <= 0 or opt[k] % 4:
            raise ValueError(f"{k} = {opt[k]}: must be a positive multiple of 4")
    if opt["dim_pose"] < 5 or opt["dim_pos_ohot"] < 1:
        raise ValueError(f"dim_pose = {opt['dim_pose']} (at least 5) / dim_pos_ohot = {opt['dim_pos_ohot']} (at least 1)")
    if opt["unit_length"] != 4:
        raise ValueError(f"unit_length = {opt['unit_length']}: the two stride-2 convolutions reduce time by 4")


def build_containers(opt):
    _check_widths(opt)
    movement = _ParamContainer(movement_encoder_shapes(opt['dim_pose'] - 4, opt['dim_movement_enc_hidden'], opt['dim_movement_latent']))
    text = _ParamContainer(text_encoder_shapes(opt['dim_word'], opt['dim_pos_ohot'], opt['dim_text_hidden'], opt['dim_coemb_hidden']))
    motion = _ParamContainer(motion_encoder_shapes(opt['dim_movement_latent'], opt['dim_motion_hidden'], opt['dim_coemb_hidden']))
    return text, motion, movement


def build_evaluators(opt):
    """evaluator_wrapper.py:95-118."""
    text_enc, motion_enc, movement_enc = build_containers(opt)
    ckpt_dir = opt['dataset_name']
    if opt['dataset_name'] == 'humanml':
        ckpt_dir = 't2m'
    checkpoint = torch.load(pjoin(opt['checkpoints_dir'], ckpt_dir, 'text_mot_match', 'model', 'finest.tar'),
                            map_location=opt['device'])
    movement_enc.load_state_dict(checkpoint['movement_encoder'])
    text_enc.load_state_dict(checkpoint['text_encoder'])
    motion_enc.load_state_dict(checkpoint['motion_encoder'])
    print('Loading Evaluation Model Wrapper (Epoch %d) Completed!!' % (checkpoint['epoch']))
    return text_enc, motion_enc, movement_enc


def _lens_list(lens):
    return lens.data.tolist() if torch.is_tensor(lens) else [int(v) for v in lens]


def _check_packed_lengths(lens, limit, what):
    """What pack_padded_sequence(..., enforce_sorted=True) refuses (modules.py:344, :380), plus its bound on the padded length."""
    if len(lens) == 0:
        raise RuntimeError(f"{what}: empty batch")
    if any(a < b for a, b in zip(lens, lens[1:])):
        raise RuntimeError(f"{what}: `lengths` array must be sorted in decreasing order (pack_padded_sequence with enforce_sorted)")
    if lens[-1] <= 0:
        raise RuntimeError(f"{what}: length of all samples has to be greater than 0, but found an element in 'lengths' that is <= 0")
    if lens[0] > limit:
        raise RuntimeError(f"{what}: a length of {lens[0]} is beyond the {limit} steps of the padded input")


class EvaluatorMDMWrapper(NativeModelMixin):
    """evaluator_wrapper.py:121-187: same constructor, attributes and methods; results in the reference's (sorted) order."""

    def __init__(self, dataset_name, device, _native_lib=None):
        opt = default_opt(dataset_name, device)
        self._native_lib = _native_lib
        self.text_encoder, self.motion_encoder, self.movement_encoder = build_evaluators(opt)
        self._finish(opt)

    @classmethod
    def from_state_dicts(cls, movement, text, motion, dataset_name, device, dims=None, _native_lib=None):
        """The wrapper over three state dicts (`checkpoint['movement_encoder' | 'text_encoder' | 'motion_encoder']`) instead of
        ./{t2m|kit}/text_mot_match/model/finest.tar.  `dims` overrides entries of `opt` (reduced widths: dim_pose, dim_word,
        dim_pos_ohot, dim_movement_enc_hidden, dim_movement_latent, dim_motion_hidden, dim_text_hidden, dim_coemb_hidden)."""
        self = cls.__new__(cls)
        opt = default_opt(dataset_name, device)
        for k, v in (dims or {}).items():
            if k not in opt or k in ("dataset_name", "device", "checkpoints_dir"):
                raise ValueError(f"dims: unknown entry {k!r}")
            opt[k] = int(v)
        self._native_lib = _native_lib
        self.text_encoder, self.motion_encoder, self.movement_encoder = build_containers(opt)
        self.movement_encoder.load_state_dict(movement)
        self.text_encoder.load_state_dict(text)
        self.motion_encoder.load_state_dict(motion)
        self._finish(opt)
        return self

    def _finish(self, opt):
        self.opt = opt
        self.device = opt['device']
        for enc in (self.text_encoder, self.motion_encoder, self.movement_encoder):
            enc.to(opt['device'])
            enc.eval()

    # ---- native model ----------------------------------------------------------------------------------------------------------
    def _gru_tables(self, enc, in_dim):
        sd = {k: v.detach().float() for k, v in enc.state_dict().items()}
        H = sd["hidden"].shape[-1]
        t = dict(in_w=sd["input_emb.weight"], in_b=sd["input_emb.bias"],
                 w_ih=torch.cat([sd["gru.weight_ih_l0"], sd["gru.weight_ih_l0_reverse"]], 0),
                 b_ih=torch.cat([sd["gru.bias_ih_l0"], sd["gru.bias_ih_l0_reverse"]], 0),
                 w_hh=torch.stack([sd["gru.weight_hh_l0"], sd["gru.weight_hh_l0_reverse"]], 0),
                 b_hh=torch.stack([sd["gru.bias_hh_l0"], sd["gru.bias_hh_l0_reverse"]], 0),
                 h0=sd["hidden"].reshape(2, H),
                 o1_w=sd["output_net.0.weight"], o1_b=sd["output_net.0.bias"], ln_g=sd["output_net.1.weight"],
                 ln_b=sd["output_net.1.bias"], o2_w=sd["output_net.3.weight"], o2_b=sd["output_net.3.bias"])
        t = {k: v.contiguous().clone() for k, v in t.items()}          # own storage: 16-byte aligned, unaffected by later loads
        return t, nat.MdmEvalGru(in_dim=in_dim, hidden=H, out=sd["output_net.3.weight"].shape[0],
                                 **{k: v.data_ptr() for k, v in t.items()})

    def _native_version(self):
        return (self.movement_encoder.version(), self.text_encoder.version(), self.motion_encoder.version())

    def _build_native(self, keep):
        """The prepared weight tables (concatenated GRU directions, tap-major convolution weights) and the C struct over them."""
        mv = {k: v.detach().float() for k, v in self.movement_encoder.state_dict().items()}
        tx = self.text_encoder.state_dict()
        top = dict(conv1_w=mv["main.0.weight"].permute(0, 2, 1), conv1_b=mv["main.0.bias"],     # [out][tap][in]
                   conv2_w=mv["main.3.weight"].permute(0, 2, 1), conv2_b=mv["main.3.bias"],
                   out_w=mv["out_net.weight"], out_b=mv["out_net.bias"],
                   pos_w=tx["pos_emb.weight"].detach().float(), pos_b=tx["pos_emb.bias"].detach().float())
        top = {k: v.contiguous().clone() for k, v in top.items()}
        o = self.opt
        mt, mg = self._gru_tables(self.motion_encoder, o['dim_movement_latent'])
        tt, tg = self._gru_tables(self.text_encoder, o['dim_word'])
        keep += [top, mt, tt]
        return nat.MdmEvalModel(motion=mg, text=tg, dim_pose=o['dim_pose'], conv_hidden=o['dim_movement_enc_hidden'],
                                latent=o['dim_movement_latent'], word=o['dim_word'], pos=o['dim_pos_ohot'],
                                unit_length=o['unit_length'], **{k: v.data_ptr() for k, v in top.items()})

    def _check_motion(self, motions, m_lens):
        o = self.opt
        if motions.dim() != 3 or motions.shape[-1] != o['dim_pose']:
            raise ValueError(f"motions must be [B, T, {o['dim_pose']}], got {tuple(motions.shape)}")
        B, T = motions.shape[0], motions.shape[1]
        if len(m_lens) != B:
            raise ValueError(f"m_lens has {len(m_lens)} entries for {B} motions")
        if T < 4:
            raise ValueError(f"motions of {T} frames: the movement encoder needs at least 4")
        _check_packed_lengths([l // o['unit_length'] for l in m_lens], (T // 2) // 2, "m_lens // unit_length")

    def _motion_rows(self, motions, m_lens):
        """motions [B, T, dim_pose] and frame counts, both already in descending-length order -> [B, dim_coemb_hidden]."""
        self._check_motion(motions, m_lens)
        o = self.opt
        B, T = motions.shape[0], motions.shape[1]
        lib, model = self._lib(), self._model()
        motions = motions.contiguous()
        stream = self._stream(lib, motions, "tensors")
        dev = motions.device
        out = torch.empty(B, o['dim_coemb_hidden'], dtype=torch.float32, device=dev)
        lens_dev = torch.tensor(m_lens, dtype=torch.int32).to(dev)
        ws, nbytes = self._workspace("mdm_eval_workspace_bytes", model, min(B, ROW_CHUNK), T, 0, dev=dev)
        for b0 in range(0, B, ROW_CHUNK):
            n = min(ROW_CHUNK, B - b0)
            lib.check(lib.mdm_eval_motion_embeddings(nat.C.byref(model), motions[b0:b0 + n].data_ptr(), lens_dev[b0:b0 + n].data_ptr(),
                                                     out[b0:b0 + n].data_ptr(), n, T, int(m_lens[b0]), ws.data_ptr(), nbytes, stream),
                      "mdm_eval_motion_embeddings")
        return out

    def _check_text(self, word_embs, pos_ohot, cap_lens):
        o = self.opt
        if word_embs.dim() != 3 or word_embs.shape[-1] != o['dim_word']:
            raise ValueError(f"word_embs must be [B, L, {o['dim_word']}], got {tuple(word_embs.shape)}")
        B, L = word_embs.shape[0], word_embs.shape[1]
        if tuple(pos_ohot.shape) != (B, L, o['dim_pos_ohot']):
            raise ValueError(f"pos_ohot must be [B, L, {o['dim_pos_ohot']}] = {(B, L, o['dim_pos_ohot'])}, got {tuple(pos_ohot.shape)}")
        if len(cap_lens) != B:
            raise ValueError(f"cap_lens has {len(cap_lens)} entries for {B} captions")
        _check_packed_lengths(cap_lens, L, "cap_lens")

    def _text_rows(self, word_embs, pos_ohot, cap_lens):
        self._check_text(word_embs, pos_ohot, cap_lens)
        o = self.opt
        B, L = word_embs.shape[0], word_embs.shape[1]
        lib, model = self._lib(), self._model()
        word_embs, pos_ohot = word_embs.contiguous(), pos_ohot.contiguous()
        stream = self._stream(lib, word_embs, "tensors")
        dev = word_embs.device
        out = torch.empty(B, o['dim_coemb_hidden'], dtype=torch.float32, device=dev)
        lens_dev = torch.tensor(cap_lens, dtype=torch.int32).to(dev)
        ws, nbytes = self._workspace("mdm_eval_workspace_bytes", model, min(B, ROW_CHUNK), 0, L, dev=dev)
        for b0 in range(0, B, ROW_CHUNK):
            n = min(ROW_CHUNK, B - b0)
            lib.check(lib.mdm_eval_text_embeddings(nat.C.byref(model), word_embs[b0:b0 + n].data_ptr(), pos_ohot[b0:b0 + n].data_ptr(),
                                                   lens_dev[b0:b0 + n].data_ptr(), out[b0:b0 + n].data_ptr(), n, L, int(cap_lens[b0]),
                                                   ws.data_ptr(), nbytes, stream), "mdm_eval_text_embeddings")
        return out

    def _sort_motions(self, motions, m_lens):
        """evaluator_wrapper.py:160-162, after the checks the reference leaves to the first failing torch call."""
        if motions.dim() < 1 or len(m_lens) != motions.shape[0]:
            raise ValueError(f"m_lens has {len(m_lens)} entries for {motions.shape[0] if motions.dim() else 0} motions")
        align_idx = np.argsort(m_lens.data.tolist())[::-1].copy()
        motions = motions[align_idx]
        m_lens = [int(v) for v in _lens_list(m_lens[align_idx])]
        self._check_motion(motions, m_lens)
        return motions, m_lens, align_idx

    # Please note that the results does not following the order of inputs
    def get_co_embeddings(self, word_embs, pos_ohot, cap_lens, motions, m_lens):
        with torch.no_grad():
            word_embs = word_embs.detach().to(self.device).float()
            pos_ohot = pos_ohot.detach().to(self.device).float()
            motions = motions.detach().to(self.device).float()

            motions, m_lens, align_idx = self._sort_motions(motions, m_lens)
            cap_lens = [int(v) for v in _lens_list(cap_lens)]
            self._check_text(word_embs, pos_ohot, cap_lens)          # every refusal comes before the first launch

            '''Movement Encoding'''
            motion_embedding = self._motion_rows(motions, m_lens)

            '''Text Encoding'''
            text_embedding = self._text_rows(word_embs, pos_ohot, cap_lens)
            text_embedding = text_embedding[align_idx]
        return text_embedding, motion_embedding

    # Please note that the results does not following the order of inputs
    def get_motion_embeddings(self, motions, m_lens):
        with torch.no_grad():
            motions = motions.detach().to(self.device).float()
            motions, m_lens, _ = self._sort_motions(motions, m_lens)
            motion_embedding = self._motion_rows(motions, m_lens)
        return motion_embedding
