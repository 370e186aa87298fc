"""Writes tests/golden/clip_text_{reduced,full}_{default,trained}.npz, clip_text_state_dict_keys.json and PIN_REPORT_clip_text.json.

Run on the CPU:   python tests/make_golden_clip_text.py

The pin is HF transformers' CLIPTextModelWithProjection built from a bare CLIPTextConfig with hidden_act="quick_gelu" -- OpenAI
CLIP's text tower under other names; no file is read and no connection opened --, loaded with the weights
tests/clip_text_helpers.py builds, through its OpenAI -> HF key map.  Per case it runs in fp32 and as .double(), and the report
records e_ref = max |HF fp32 - fp64 restatement| (the unit of the accuracy condition of tests/test_gpu_clip_text.py),
`fp64_agrees` (the restatement matches HF's .double() run to 1e-10), max_abs_output and, where torch's CPU half path runs the
module, e_half = max |HF fp16 - fp64|: what upstream's fp16 arithmetic costs, as context and not as a bound.  The files hold data
only, and a second run writes the same bytes."""
import copy
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import clip_text_helpers as ch  # noqa: E402


def save_npz(path, **arrays):
    """np.savez_compressed with a fixed time stamp on every member, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w") as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(a), allow_pickle=False)


def run_case(model, sd, heads, tokens):
    """-> (HF fp32 output, fp64 restatement, report entry); `model` is left in fp32 with its weights unchanged."""
    ids = torch.from_numpy(tokens)
    with torch.no_grad():
        ref32 = model(input_ids=ids).text_embeds.numpy()
        ref64 = copy.deepcopy(model).double()(input_ids=ids).text_embeds.numpy()
        try:
            ref16 = copy.deepcopy(model).half()(input_ids=ids).text_embeds.float().numpy()
        except RuntimeError:                # (no CPU half kernels for some operator of this torch build)
            ref16 = None
    f64 = ch.encode_text_fp64(sd, tokens, heads)
    agree = ch.maxabs(ref64, f64)
    entry = {"e_ref": ch.maxabs(ref32, f64), "max_abs_output": float(np.abs(f64).max()), "fp64_vs_hf_fp64": agree,
             "fp64_agrees": bool(agree <= 1e-10), "shape": list(f64.shape), "lens": [int(v) + 1 for v in tokens.argmax(-1)]}
    if ref16 is not None:
        entry["e_half"] = ch.maxabs(ref16, f64)
    return ref32, f64, entry


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    report = {}
    tokens = ch.fixture_tokens()
    assert [int(v) + 1 for v in tokens.argmax(-1)] == ch.FIXTURE_LENS
    for name, f in ch.FIXTURES.items():
        cfg, sd = ch.CFGS[f["cfg"]], ch.weights(f["cfg"], f["trained"])
        model = ch.hf_model(f["cfg"], f["trained"])
        ref32, f64, report[name] = run_case(model, sd, cfg["heads"], tokens)
        save_npz(os.path.join(ch.GOLDEN, f"clip_text_{name}.npz"), seed=np.int64(ch.SEED), tokens=tokens, lens=np.asarray(ch.FIXTURE_LENS),
                 ref=ref32, fp64=f64)
        r = report[name]
        print(f"{name}: e_ref = {r['e_ref']:.3e}  max|out| = {r['max_abs_output']:.3f}  fp64 agrees: {r['fp64_agrees']} "
              f"({r['fp64_vs_hf_fp64']:.1e})  e_half = {r.get('e_half', float('nan')):.3e}", flush=True)
        for case, c in ch.SWEEP.items():
            if (c["cfg"], c["trained"]) != (f["cfg"], f["trained"]):
                continue
            _, _, report[case] = run_case(model, sd, cfg["heads"], ch.sweep_inputs(case))
            print(f"  {case}: e_ref = {report[case]['e_ref']:.3e}  fp64 agrees: {report[case]['fp64_agrees']}", flush=True)
    assert all(r["fp64_agrees"] for r in report.values())
    key_map = ch.hf_key_map(ch.FULL)
    keys = {k: {"shape": list(shape), "hf": key_map[k]} for k, shape in ch.state_dict_shapes(ch.FULL, vocab=49408)}
    with open(ch.KEYS_FILE, "w") as fh:
        json.dump(keys, fh, indent=1)
    with open(ch.PIN_REPORT, "w") as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
    print("wrote", ch.PIN_REPORT)


if __name__ == "__main__":
    main()
