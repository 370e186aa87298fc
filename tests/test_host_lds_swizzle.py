"""The A-stage LDS swizzle of csrc/gemm_x3.h (x3_swz) under the MI355X bank model: 64 banks x 4 bytes; a ds_read_b128 is served in
four groups of 16 lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same two + 32 -- and is conflict-free when the 16 lanes
of a group touch 64 different banks.  Image: 64-byte rows, the 16-byte chunk c of a row stored at chunk c ^ f((row >> 2) & 3).  Three
read patterns use it: 16x16x32 (row lane & 15, chunk lane >> 4) and 32x32x16 (row lane & 31, chunk 2 ksub + (lane >> 5)), ksub 0 / 1."""
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
GROUPS += [[l + 32 for l in g] for g in GROUPS]
PATTERNS = {"m16": lambda l: (l & 15, l >> 4), "m32_k0": lambda l: (l & 31, l >> 5), "m32_k1": lambda l: (l & 31, 2 + (l >> 5))}


def ways(f, pattern):
    worst = 0
    for g in GROUPS:
        hits = {}
        for lane in g:
            row, chunk = pattern(lane)
            byte = row * 64 + ((chunk ^ f[(row >> 2) & 3]) * 16)
            for b in range(byte // 4, byte // 4 + 4):
                hits[b % 64] = hits.get(b % 64, 0) + 1
        worst = max(worst, max(hits.values()))
    return worst


def header_permutation():
    """x3_swz as the header states it: the bit formula, evaluated here, must be the permutation its static_assert pins."""
    text = open(os.path.join(ROOT, "motion-diffusion-model_amd", "csrc", "gemm_x3.h")).read()
    body = re.search(r"constexpr int x3_swz\(int q\) \{ return (.*?); \}", text).group(1)
    f = tuple(eval(body, {"q": q}) for q in range(4))
    pins = re.search(r"static_assert\(x3_swz\(0\) == (\d) && x3_swz\(1\) == (\d) && x3_swz\(2\) == (\d) && x3_swz\(3\) == (\d)", text)
    assert f == tuple(int(v) for v in pins.groups())
    return f


def test_the_a_stage_swizzle_is_conflict_free_on_every_read_pattern():
    f = header_permutation()
    assert f == (0, 2, 3, 1)
    assert {name: ways(f, p) for name, p in PATTERNS.items()} == {"m16": 1, "m32_k0": 1, "m32_k1": 1}
    # rounds 1-7 XORed with (row >> 2) & 3 itself: fine for the 32x32x16 reads it was made for, 2-way on the 16x16x32 reads of round 7
    ident = (0, 1, 2, 3)
    assert {name: ways(ident, p) for name, p in PATTERNS.items()} == {"m16": 2, "m32_k0": 1, "m32_k1": 1}
    good = [p for p in itertools.permutations(range(4)) if all(ways(p, pat) == 1 for pat in PATTERNS.values())]
    assert len(good) == 8 and f in good
