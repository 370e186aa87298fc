"""Writes tests/golden/evaluator_*.npz, evaluator_state_dict_keys.json and PIN_REPORT_evaluator.json.

Run on the CPU, with the reference checkout's path:   python tests/make_golden_evaluator.py /path/to/motion-diffusion-model

The reference's own data_loaders/humanml/networks/modules.py and evaluator_wrapper.py are IMPORTED here, at generation time only, and
run in fp32 on the weights tests/evaluator_helpers.py builds; the files hold data only (outputs, the fp64 restatement's outputs, the
state-dict key lists).  Per fixture the report records e_ref = max |reference fp32 - fp64 restatement|, which is both the pin of the
restatement against the reference and the unit of the accuracy condition of tests/test_gpu_evaluator.py."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import evaluator_helpers as eh  # noqa: E402


def reference_wrapper(ref_modules, ref_wrapper, weights, dims):
    """The reference's EvaluatorMDMWrapper over freshly built reference modules (its constructor only adds the tar loading)."""
    d = dims
    movement = ref_modules.MovementConvEncoder(d["dim_pose"] - 4, d["dim_movement_enc_hidden"], d["dim_movement_latent"])
    text = ref_modules.TextEncoderBiGRUCo(word_size=d["dim_word"], pos_size=d["dim_pos_ohot"], hidden_size=d["dim_text_hidden"],
                                          output_size=d["dim_coemb_hidden"], device="cpu")
    motion = ref_modules.MotionEncoderBiGRUCo(input_size=d["dim_movement_latent"], hidden_size=d["dim_motion_hidden"],
                                              output_size=d["dim_coemb_hidden"], device="cpu")
    movement.load_state_dict(weights[0])
    text.load_state_dict(weights[1])
    motion.load_state_dict(weights[2])
    w = ref_wrapper.EvaluatorMDMWrapper.__new__(ref_wrapper.EvaluatorMDMWrapper)
    w.opt = {"unit_length": 4}
    w.device = "cpu"
    w.text_encoder, w.motion_encoder, w.movement_encoder = text.eval(), motion.eval(), movement.eval()
    return w


def main(ref_root):
    sys.path.insert(0, ref_root)
    from data_loaders.humanml.networks import evaluator_wrapper as ref_wrapper
    from data_loaders.humanml.networks import modules as ref_modules
    from data_loaders.humanml.utils.word_vectorizer import POS_enumerator
    assert len(POS_enumerator) == eh.FULL["dim_pos_ohot"]
    torch.manual_seed(0)
    torch.set_num_threads(8)
    report = {}
    for name, f in eh.FIXTURES.items():
        dims = eh.DIMS[f["dims"]]
        weights, inp = eh.fixture_weights(name), eh.fixture_inputs(name)
        ref = reference_wrapper(ref_modules, ref_wrapper, weights, dims)
        t = {k: torch.from_numpy(v) for k, v in inp.items()}
        got = {}
        if f["kind"] == "motion":
            got["motion"] = ref.get_motion_embeddings(t["motions"], t["m_lens"]).numpy()
        elif f["kind"] == "text":
            with torch.no_grad():
                got["text"] = ref.text_encoder(t["word_embs"], t["pos_ohot"], t["cap_lens"]).numpy()
        else:
            te, me = ref.get_co_embeddings(t["word_embs"], t["pos_ohot"], t["cap_lens"], t["motions"], t["m_lens"])
            got["text"], got["motion"] = te.numpy(), me.numpy()
        f64 = eh.run_fp64(name)
        e_ref = max(float(np.abs(got[k].astype(np.float64) - f64[k]).max()) for k in got)
        entry = {"fp64_vs_reference_fp32": e_ref, "e_ref": e_ref, "shape": {k: list(v.shape) for k, v in got.items()},
                 "max_abs_output": max(float(np.abs(v).max()) for v in f64.values())}
        if f["kind"] == "co":
            # the R-precision check of the GPU test relies on a ranking that rounding cannot decide
            gap = eh.nearest_gap(f64["text"], f64["motion"])
            entry["nearest_distance_gap"] = gap
            assert gap > 100 * e_ref, (gap, e_ref)
            assert np.array_equal(eh.top_k_matrix(got["text"], got["motion"]), eh.top_k_matrix(f64["text"], f64["motion"]))
        report[name] = entry
        arrays = {f"ref_{k}": v for k, v in got.items()}
        arrays.update({f"fp64_{k}": v for k, v in f64.items()})
        np.savez_compressed(os.path.join(eh.GOLDEN, f"evaluator_{name}.npz"), seed=f["seed"], **arrays)
        print(f"{name}: e_ref = {e_ref:.3e}  max|out| = {entry['max_abs_output']:.3f}", flush=True)

    # the full-width state-dict keys, from the reference's own constructor path: a finest.tar written here, loaded by build_evaluators
    weights = eh.build_weights(1, eh.FULL)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "t2m", "text_mot_match", "model"))
        torch.save({"movement_encoder": weights[0], "text_encoder": weights[1], "motion_encoder": weights[2], "epoch": 0},
                   os.path.join(tmp, "t2m", "text_mot_match", "model", "finest.tar"))
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            w = ref_wrapper.EvaluatorMDMWrapper("humanml", "cpu")
        finally:
            os.chdir(cwd)
    keys = {n: {k: list(v.shape) for k, v in getattr(w, n).state_dict().items()}
            for n in ("movement_encoder", "text_encoder", "motion_encoder")}
    with open(eh.KEYS_FILE, "w") as fh:
        json.dump(keys, fh, indent=1)
    with open(eh.PIN_REPORT, "w") as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
    print("wrote", eh.PIN_REPORT)


if __name__ == "__main__":
    main(sys.argv[1])
