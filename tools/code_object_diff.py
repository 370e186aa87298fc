#!/usr/bin/env python3
"""Do two builds of a library carry the same device code?  usage: code_object_diff.py OLD.so NEW.so [--keep DIR]

Extracts the gfx950 code object of each library, disassembles it and compares, kernel by kernel (paired by symbol name), each
instruction's text in front of `//` (symbol annotations of branch targets dropped), plus the kernels' .group_segment_fixed_size /
.kernarg_segment_size / register / scratch metadata.  Exit status 0: same kernel symbols, no differing stream, same metadata.
(The recipe of profiles/r12a_gemm_x3_strip.md.  Object hashes are not compared: they differ between build directories.)"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
META = (".group_segment_fixed_size", ".kernarg_segment_size", ".private_segment_fixed_size", ".sgpr_count", ".vgpr_count", ".agpr_count")


def run(*cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def code_object(lib):
    d = tempfile.mkdtemp()
    so = os.path.join(d, "lib.so")
    os.symlink(os.path.abspath(lib), so)
    run(os.path.join(LLVM, "llvm-objdump"), "--offloading", so, cwd=d)
    co = [os.path.join(d, f) for f in os.listdir(d) if "gfx950" in f]
    assert len(co) == 1, co
    return co[0]


def kernels(co):
    out, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(re.sub(r"<[^>]*>", "", line.split("//")[0]).strip())
    return out


def metadata(co):
    blocks = []                                             # one per kernel: its keys sit at four columns, the first behind "  - "
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"^  (- |  )(\.[a-z_]+):\s*(\S*)", line)
        if m and m.group(1) == "- ":
            blocks.append({})
        if m and blocks:
            blocks[-1][m.group(2)] = m.group(3)
    return {b[".name"]: tuple(b.get(k) for k in META) for b in blocks if ".name" in b and ".kernarg_segment_size" in b}


if __name__ == "__main__":
    cos = [code_object(p) for p in sys.argv[1:3]]
    old, new = kernels(cos[0]), kernels(cos[1])
    differing = [n for n in old if n in new and old[n] != new[n]]
    only = sorted(set(old) ^ set(new))
    mo, mn = metadata(cos[0]), metadata(cos[1])
    meta_diff = sorted(k for k in set(mo) | set(mn) if mo.get(k) != mn.get(k))
    print(f"kernels {len(old)} / {len(new)}  instructions {sum(map(len, old.values()))} / {sum(map(len, new.values()))}  "
          f"in one only: {len(only)}  differing streams: {len(differing)}  metadata rows {len(mo)} / {len(mn)}, differing: {len(meta_diff)}")
    for n in only + differing + meta_diff:
        print("  ", run("c++filt", n).strip()[:200])
    sys.exit(1 if (only or differing or meta_diff or not mo) else 0)
