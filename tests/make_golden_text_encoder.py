"""Writes tests/golden/text_encoder_{reduced,full}_{default,trained}.npz, text_encoder_state_dict_keys.json and
PIN_REPORT_text_encoder.json.

Run on the CPU, with the reference checkout's path:   python tests/make_golden_text_encoder.py /path/to/motion-diffusion-model

The reference's own model/BERT/BERT_encoder.py is IMPORTED here, at generation time only: per (config, regime) a local HF model
directory is synthesised from the weights tests/text_encoder_helpers.py builds (no download), the reference's `load_bert(dir)(texts)`
runs whole -- tokenizer, model, mask -- for the fixtures, and the loaded module's `text_model(input_ids, attention_mask)` for every
sweep case.  The files hold data only: ids, mask, the reference's fp32 output and the fp64 restatement's (valid rows; the rest
zeros).  Per case the report records e_ref = max |reference fp32 - fp64 restatement| over valid rows: the pin of the restatement
against the reference and the unit of the accuracy condition of tests/test_gpu_text_encoder.py; `fp64_agrees` says the restatement
matches the reference module run in fp64 (`.double()`) to 1e-10."""
import json
import os
import sys
import tempfile

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import text_encoder_helpers as th  # noqa: E402


def _entry(ref32, ref64, f64, lens):
    e_ref = th.valid_maxabs(ref32, f64, lens)
    keep = np.arange(f64.shape[1])[None, :] < np.asarray(lens)[:, None]
    agree = th.valid_maxabs(ref64, f64, lens)
    return {"e_ref": e_ref, "max_abs_output": float(np.abs(f64[keep]).max()), "fp64_vs_reference_fp64": agree,
            "fp64_agrees": bool(agree <= 1e-10), "shape": list(f64.shape), "lens": [int(v) for v in lens]}


def main(ref_root):
    sys.path.insert(0, ref_root)
    from model.BERT.BERT_encoder import load_bert
    torch.manual_seed(0)
    torch.set_num_threads(8)
    report, keys = {}, None
    texts = th.fixture_texts()
    for name, f in th.FIXTURES.items():
        cfg = th.CFGS[f["cfg"]]
        sd = th.weights(f["cfg"], f["trained"])
        with tempfile.TemporaryDirectory() as tmp:
            bert = load_bert(th.synth_model_dir(os.path.join(tmp, "m"), f["cfg"], f["trained"]))
        with torch.no_grad():
            out, mask = bert(texts)
            enc = bert.tokenizer(texts, return_tensors="pt", padding=True)
            ids = enc["input_ids"]
            assert torch.equal(mask, enc["attention_mask"].bool())
            lens = mask.sum(1).tolist()
            assert lens == th.FIXTURE_LENS and tuple(ids.shape) == (4, 33), (lens, ids.shape)
            f64 = th.encoder_fp64(sd, ids.numpy(), lens, cfg["n_heads"])
            dbl = bert.text_model.double()
            ref64 = dbl(input_ids=ids, attention_mask=enc["attention_mask"]).last_hidden_state.numpy()
            report[name] = _entry(out.numpy(), ref64, f64, lens)
            # rows at or beyond a length are stored as zeros: nothing compares them (HF computes padded queries over the valid keys
            # there, this project writes zeros), and the full-width file would not fit a committed file's size otherwise
            keep = mask.numpy()[..., None]
            np.savez_compressed(os.path.join(th.GOLDEN, f"text_encoder_{name}.npz"), seed=th.SEED, ids=ids.numpy().astype(np.int64),
                                mask=mask.numpy(), ref=np.where(keep, out.numpy(), np.float32(0)), fp64=np.where(keep, f64, 0.0))
            print(f"{name}: e_ref = {report[name]['e_ref']:.3e}  max|out| = {report[name]['max_abs_output']:.3f}  "
                  f"fp64 agrees: {report[name]['fp64_agrees']} ({report[name]['fp64_vs_reference_fp64']:.1e})", flush=True)
            if name == "full_default":
                keys = {k: list(v.shape) for k, v in dbl.state_dict().items()}
            for case, c in th.SWEEP.items():
                if c["cfg"] != f["cfg"] or c["trained"] != f["trained"]:
                    continue
                cids, cmask, clens = th.sweep_inputs(case)
                am = torch.from_numpy(cmask.astype(np.int64))
                ref64 = dbl(input_ids=torch.from_numpy(cids), attention_mask=am).last_hidden_state.numpy()
                ref32 = dbl.float()(input_ids=torch.from_numpy(cids), attention_mask=am).last_hidden_state.numpy()
                dbl = dbl.double()
                report[case] = _entry(ref32, ref64, th.encoder_fp64(sd, cids, clens, cfg["n_heads"]), clens)
                print(f"  {case}: e_ref = {report[case]['e_ref']:.3e}  fp64 agrees: {report[case]['fp64_agrees']}", flush=True)
    assert all(r["fp64_agrees"] for r in report.values())
    with open(th.KEYS_FILE, "w") as fh:
        json.dump(keys, fh, indent=1)
    with open(th.PIN_REPORT, "w") as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
    print("wrote", th.PIN_REPORT)


if __name__ == "__main__":
    main(sys.argv[1])
