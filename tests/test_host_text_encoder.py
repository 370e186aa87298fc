"""Host side of mdm_amd/text_encoder.py: the container's state-dict keys, the refusals of encode_ids, MDM's wiring, and -- where the
transformers package and the reference checkout are at hand -- the whole tokenizer path against the reference's load_bert."""
import os
import sys

import numpy as np
import pytest
import torch

import text_encoder_helpers as th


def test_container_keys_are_hf_distilbert_s():
    from mdm_amd.text_encoder import BERT
    want = th.state_dict_keys()
    bert = BERT.from_state_dict(th.build_weights(1, dict(th.FULL, n_layers=6, hidden=3072, dim=768, max_pos=512)))
    got = {k: list(v.shape) for k, v in bert.text_model.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert [k for k in bert.state_dict()] == ["text_model." + k for k in want]
    assert bert.cfg["n_heads"] == 12 and not any(p.requires_grad for p in bert.parameters())


def test_encode_ids_refuses_what_the_kernels_do_not_take():
    bert = th.make_bert("reduced", False, "cpu")
    ids, mask = th.make_ids(1, 2, 8, [8, 5])
    holes = mask.copy()
    holes[1, 2] = False
    with pytest.raises(ValueError, match="suffix mask"):
        th.encode(bert, ids, holes)
    left = mask[:, ::-1].copy()
    with pytest.raises(ValueError, match="suffix mask"):
        th.encode(bert, ids, left)
    with pytest.raises(ValueError, match="suffix mask"):
        th.encode(bert, ids, np.zeros_like(mask))
    ids129, mask129 = th.make_ids(1, 1, 129, [129])
    with pytest.raises(ValueError, match="prompt longer than 128 word pieces"):
        th.encode(bert, ids129, mask129)
    bad = ids.copy()
    bad[0, 3] = len(th.VOCAB)
    with pytest.raises(ValueError, match="vocabulary"):
        th.encode(bert, bad, mask)
    with pytest.raises(RuntimeError, match="no tokenizer"):
        bert(["w1 w2"])


def test_mdm_without_a_bert_path_names_the_argument():
    from mdm_amd import model_util
    args = model_util.default_args(layers=1, latent_dim=256, arch="trans_dec", text_encoder_type="bert")
    model, _ = model_util.create_model_and_diffusion(args, num_heads=2, ff_size=256)
    assert model.clip_model is None
    with pytest.raises(RuntimeError, match="bert_model_path"):
        model.encode_text(["a person walks"])


def test_tokenizer_path_against_the_reference_on_the_emulator(tmp_path, monkeypatch):
    """load_bert(dir)(texts) -- tokenizer, encoder, mask -- against the reference's load_bert on the same synthesised directory."""
    monkeypatch.setenv("HF_HUB_OFFLINE", "1")          # (the reference's load_bert does not pass local_files_only)
    monkeypatch.setenv("TRANSFORMERS_OFFLINE", "1")
    pytest.importorskip("transformers")
    from oracle import ref_harness
    ref_root = ref_harness.REFERENCE_ROOT
    if not os.path.isfile(os.path.join(ref_root, "model", "BERT", "BERT_encoder.py")):
        pytest.skip("needs the upstream reference source tree (MDM_REFERENCE_ROOT), which the repository does not hold")
    from emu.emu_lib import emu
    from mdm_amd.text_encoder import load_bert
    sys.path.insert(0, ref_root)
    try:
        from model.BERT.BERT_encoder import load_bert as ref_load_bert
    finally:
        sys.path.remove(ref_root)
    path = th.synth_model_dir(str(tmp_path / "m"), "reduced", True)
    texts = th.fixture_texts()
    with torch.no_grad():
        want, want_mask = ref_load_bert(path)(texts)
    got, mask = load_bert(path, _native_lib=emu())(texts)
    assert torch.equal(mask, want_mask) and mask.sum(1).tolist() == th.FIXTURE_LENS
    g = th.load_fixture("reduced_trained")
    err, bound = th.valid_maxabs(got, g["fp64"], th.FIXTURE_LENS), 4 * th.pin_report()["reduced_trained"]["e_ref"]
    print(f"[text encoder] tokenizer path: max-abs vs fp64 = {err:.3e} (bound {bound:.3e}); vs the reference's fp32 = "
          f"{th.valid_maxabs(got, want.numpy(), th.FIXTURE_LENS):.3e}")
    assert err <= bound
