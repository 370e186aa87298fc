"""Condense gpurun_out/<tag>/pmc*.txt (tools/gpu_prof.sh ... pmc) + kernel_stats.md into profiles/<name>.json:
per kernel the mean duration, FETCH_SIZE / WRITE_SIZE (KB as reported) and the derived HBM-side bytes per launch with the
gfx950 correction MI355X_MICROARCH.md prescribes (FETCH_SIZE counts 64 B per 128-B request on wide streaming reads:
x2; WRITE_SIZE as is -- both calibrated in round 1 on layernorm_kernel, whose traffic is known exactly), MFMA busy fraction
and the shader clock.  The file records the sha256 of the kernel sources it was taken on (bench.csrc_sha256): bench.py
quotes `roofline.traffic` from it only while the sources are the same.
Usage: python tools/pmc_to_json.py gpurun_out/p3 profiles/r02_pmc.json"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
src, dst = sys.argv[1], sys.argv[2]


def classify(name):
    """-> (section, key) for the kernels of the sampling loop; the GEMM is told apart by its template arguments
    <ACT, RES, FLAGS> (csrc/gemm_x3.h X3_* bits) read from the END (names arrive truncated on the left)."""
    name = name.strip().strip("`")
    m = re.search(r"(\d+), (\d+), (\d+)u>", name)
    if m:   # (no other kernel of the library has an unsigned template argument)
        act, res, flags = (int(g) for g in m.groups())
        f32, qkv, fold, ostat, embed = (bool(flags >> bit & 1) for bit in (0, 2, 3, 4, 5))
        if embed:
            return "gemm", "InputProcess"
        if qkv:
            return "gemm", "in_proj" if fold else "in_proj_layer0"
        if ostat:
            return "gemm", "out_proj|linear2" if res == 3 else "out_proj_layer0"
        if act == 1:
            return "gemm", "linear1"
        if f32 and fold:
            return "gemm", "OutputProcess"
        return "gemm", f"other<{act}, {res}, {flags}u>"
    for pat, k in (("fold_layernorm_kernel", "fold_layernorm (mdm_prepare)"), ("attention_x3_kernel", "attention"), ("pose_to_planes_kernel", "pose_to_planes"), ("layernorm_kernel", "layernorm"),
                   ("outproj_finish_kernel", "outproj_finish"), ("cond_token_kernel", "cond_token")):
        if pat in name:
            return "other", k
    return None, None


ker = {}
for i in range(1, 9):
    f = os.path.join(src, f"pmc{i}.txt")
    if not os.path.isfile(f):
        continue
    cur = None
    for line in open(f):
        if line.startswith("=="):
            cur = classify(line[2:].split(" grid=")[0])
        elif cur and cur[0] and "mean" in line:
            ker.setdefault(cur, {})[line.split()[0]] = float(line.split()[-1])
ks = os.path.join(src, "kernel_stats.md")
if os.path.isfile(ks):
    for line in open(ks):
        if not line.startswith("| `"):
            continue
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        k = classify(cells[0])
        if k[0]:
            ker.setdefault(k, {})["avg_us"] = float(cells[3])
            ker[k]["calls"] = int(cells[1])
out = {"gemm": {}, "other": {}}
for (sec, k), c in ker.items():
    e = dict(c)
    if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
        e["hbm_read_bytes"] = c["FETCH_SIZE"] * 1024 * 2
        e["hbm_write_bytes"] = c["WRITE_SIZE"] * 1024
        e["hbm_bytes"] = e["hbm_read_bytes"] + e["hbm_write_bytes"]
    if "GRBM_GUI_ACTIVE" in c and "SQ_VALU_MFMA_BUSY_CYCLES" in c:
        cyc = c["GRBM_GUI_ACTIVE"] / 8.0          # summed over the 8 XCDs
        e["mfma_busy_frac"] = c["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024 * cyc)   # 256 CUs x 4 SIMDs
        if "avg_us" in c:
            e["shader_clock_ghz_under_pmc"] = cyc / c["avg_us"] / 1e3
    out[sec][k] = e
import bench  # noqa: E402
out["csrc_sha256"] = bench.csrc_sha256()
try:
    out["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True).strip()
except Exception:
    out["commit"] = None
out["source"] = f"tools/gpu_prof.sh {os.path.basename(src.rstrip('/'))} pmc (rocprofv3 --kernel-trace --pmc, separate passes)"
json.dump(out, open(dst, "w"), indent=1, sort_keys=True)
print(json.dumps(out, indent=1, sort_keys=True))
