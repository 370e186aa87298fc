"""Shared by tests/test_emu_model_setup.py and tests/test_gpu_model_setup.py: the constant workspace of a model handle (csrc/model_setup.h
carve_const behind mdm_const_bytes and mdm_prepare) through poisoned blocks.  Two-layer models at latent_dim 256, ff_size 1024 and a
512-row positional table reach every region: layer 1 has a gamma-folded in_proj, layer 0 has none."""
import numpy as np
import torch

from helpers import make_pair, memo, synth_dip_state_dict, synth_state_dict

MDM_OK, MDM_ENOSPC = 0, -3
POISON, SLACK = 0xA5, 4096
SHAPE = dict(latent_dim=256, ff_size=1024, num_layers=2)

# name -> (state dict, make_pair arguments)
CONFIGS = {
    "enc_263": (lambda: synth_state_dict(seed=0, **SHAPE), {}),                                             # jf_k 288
    "enc_kit_251": (lambda: synth_state_dict(seed=0, input_feats=251, **SHAPE), dict(dataset="kit")),       # jf_k 256
    "dec_context_20": (lambda: synth_dip_state_dict(seed=0, **SHAPE), dict(context_len=20, pred_len=40)),   # DiP
    "dec_time_token": (lambda: synth_dip_state_dict(seed=0, bert_dim=512, **SHAPE),                         # context_len 1
                       dict(text_encoder_type="clip", emb_trans_dec=True, mask_frames=True)),
}
PURE_CONFIGS = ["enc_263", "dec_context_20"]


def bound_engine(name, device, native_lib=None):
    """The engine of configuration `name`, bound and prepared (one per configuration and device; its model is kept alive with it)."""
    def build():
        sd, over = CONFIGS[name]
        model, _ = make_pair(sd(), 2, device, guided=False, native_lib=native_lib, pos_embed_max_len=512, **over)
        return model, model.engine()
    return memo(("model_setup", name, str(device)), build)[1]


def poisoned_block(nbytes, device):
    """nbytes of POISON at a 256-byte boundary -> (pointer, read); read() gives the block's bytes as numpy after a synchronise."""
    if torch.device(device).type == "cpu":
        raw = np.full(nbytes + 256, POISON, dtype=np.uint8)
        view = raw[-raw.ctypes.data % 256:][:nbytes]
        return view.ctypes.data, lambda: view
    raw = torch.full((nbytes + 256,), POISON, dtype=torch.uint8, device=device)
    view = raw[-raw.data_ptr() % 256:][:nbytes]

    def read():
        torch.cuda.synchronize(device)
        return view.cpu().numpy()
    return view.data_ptr(), read


def _prepare_back_into_the_engines_block(eng):
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)
    ws = eng._const_ws
    eng.lib.check(eng.lib.mdm_prepare(eng.handle, ws.data_ptr(), ws.numel(), eng.stream()), "mdm_prepare")


def check_block_is_exactly_as_large_as_reported(eng):
    lib, h = eng.lib, eng.handle
    with eng._on_device():
        n = lib.mdm_const_bytes(h)
        try:
            ptr, read = poisoned_block(n + SLACK, eng.device)
            assert lib.mdm_prepare(h, ptr, n, eng.stream()) == MDM_OK, lib.mdm_last_error()
            got = read()
            print(f"mdm_const_bytes = {n}; last byte written at offset {int(np.flatnonzero(got != POISON).max())}")
            assert (got[n:] == POISON).all(), "mdm_prepare wrote behind mdm_const_bytes"
            assert not (got[n - 256:n] == POISON).all(), "the last region does not reach mdm_const_bytes"
            ptr, read = poisoned_block(n + SLACK, eng.device)
            assert lib.mdm_prepare(h, ptr, n - 1, eng.stream()) == MDM_ENOSPC
            assert lib.mdm_last_error() == b"mdm_prepare: const workspace too small"
            assert (read() == POISON).all(), "a refused mdm_prepare wrote to the block"
            assert lib.mdm_const_bytes(h) == n
        finally:
            _prepare_back_into_the_engines_block(eng)


def check_prepare_is_a_pure_function_of_the_weights(eng):
    lib, h = eng.lib, eng.handle
    with eng._on_device():
        n = lib.mdm_const_bytes(h)
        try:
            blocks = []
            for _ in range(2):
                ptr, read = poisoned_block(n + SLACK, eng.device)
                assert lib.mdm_prepare(h, ptr, n, eng.stream()) == MDM_OK, lib.mdm_last_error()
                blocks.append(read()[:n].copy())
            assert np.array_equal(blocks[0], blocks[1]), f"{int((blocks[0] != blocks[1]).sum())} of {n} bytes differ"
        finally:
            _prepare_back_into_the_engines_block(eng)
