"""Python model of the three record dumps (reference main.c:13-30, asm.c:41-55): the yardstick of tests/test_text_core_cpu.py and tests/test_gpu_text.py.
Lines are made with Python's % formatting of the values C's %d sees: a uint32_t handed to %d prints as the int with the same bits."""
import numpy as np

import miniasm_amd as ma

TILE = 12288  # csrc/text_dev.hpp: MA_TEXT_TILE
FIXED = {"paf": 163, "sg": 86, "bed": 25}  # csrc/text_core.h: TC_FIXED_* -- the longest line of a kind without its names
SLAB = 4 << 20  # csrc/text_dev.hpp: MA_TEXT_SLAB_DEFAULT


def slab_records(kind, slab, max_name):
    """records per slab: what was asked for (None: the default), clamped so that records x longest possible line stays below 2^32"""
    return min(slab or SLAB, 0xffffffff // (FIXED[kind] + (1 if kind == "bed" else 2) * max_name))

E31 = sorted({0, 2**31 - 1} | {10**k - 1 for k in range(1, 10)} | {10**k for k in range(1, 10)})  # 0, 9, 10, 99, 100, ..., 999999999, 1000000000, 2147483647
E32 = E31 + [2**31, 2**32 - 1]                                                                      # fields printed from a uint32_t: negative text above 2^31 - 1
S_PLUS1 = [x for x in E31 if x <= 2**31 - 2] + [2**31 - 2]                                          # sub.s where s + 1 is printed


def i32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >= 1 << 31 else x


def _read(names, sub, i):
    if sub is None:
        return names[i]
    return names[i] + b":%d-%d" % ((int(sub["sdel"][i]) & 0x7fffffff) + 1, i32(int(sub["e"][i])))


def _span(sub, i):
    return i32(int(sub["e"][i]) - (int(sub["sdel"][i]) & 0x7fffffff))


def paf_line(h, names, sub):
    q, t = int(h["qns"]) >> 32, int(h["tn"])
    return b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\n" % (
        _read(names, sub, q), _span(sub, q), i32(int(h["qns"])), i32(int(h["qe"])), b"+-"[int(h["mlrev"]) >> 31:][:1], _read(names, sub, t), _span(sub, t),
        i32(int(h["ts"])), i32(int(h["te"])), int(h["mlrev"]) & 0x7fffffff, int(h["bldel"]) & 0x7fffffff)


def sg_line(a, names, sub):
    u, v = int(a["ul"]) >> 32, int(a["v"])
    return b"L\t%s\t%s\t%s\t%s\t%d:\tL1:i:%d\n" % (_read(names, sub, u >> 1), b"+-"[u & 1:][:1], _read(names, sub, v >> 1), b"+-"[v & 1:][:1],
                                                  int(a["oldel"]) & 0x7fffffff, i32(int(a["ul"])))


def bed_line(i, names, sub, dele):
    s, e = int(sub["sdel"][i]) & 0x7fffffff, int(sub["e"][i])
    if (dele is not None and dele[i]) or s == e:
        return b""
    return b"%s\t%d\t%d\n" % (names[i], s, i32(e))


def lines(kind, records, names, sub=None, dele=None):
    if kind == "paf":
        return [paf_line(h, names, sub) for h in records]
    if kind == "sg":
        return [sg_line(a, names, sub) for a in records]
    return [bed_line(i, names, sub, dele) for i in range(len(names))]


def slow_lines(lens, slab):
    """lines the write kernel takes the slow way: those of a wave (64 consecutive records of a slab) whose bytes do not fit the LDS tile.  The first bytes of a
    wave's stretch may stand up to 15 bytes into the tile (the stretch's misalignment), so a stretch within 15 bytes of the tile is not predictable: None then."""
    n, slow = len(lens), 0
    for r0 in range(0, n, slab):
        for w0 in range(r0, min(n, r0 + slab), 64):
            w = lens[w0:min(n, r0 + slab, w0 + 64)]
            span = sum(w)
            if TILE - 15 <= span <= TILE:
                return None
            if span > TILE:
                slow += sum(1 for x in w if x)
    return slow


def _cycle(vals, i, shift):
    return vals[(i + shift) % len(vals)]


def edge_case(kind, with_sub=True):
    """records that take every integer field of a line kind through every value edge, both strands: (records, names, sub, dele)"""
    n = 2 * len(E32)
    names = [b"r" * (1 + i % 5) + b"%d" % i for i in range(n)]
    sub = np.zeros(n, dtype=ma.SUB_DT)
    for i in range(n):
        sub["sdel"][i] = _cycle(S_PLUS1 if kind != "bed" else E31, i, 0)
        sub["e"][i] = _cycle(E32, i, 5)
    if kind == "bed":
        dele = np.zeros(n, dtype=np.uint8)
        dele[3::7] = 1
        sub["e"][5::11] = sub["sdel"][5::11]  # s == e: no line
        return None, names, sub, dele
    if kind == "paf":
        rec = np.zeros(n, dtype=ma.HIT_DT)
        for i in range(n):
            rec["qns"][i] = (i << 32) | _cycle(E32, i, 1)
            rec["qe"][i] = _cycle(E32, i, 2)
            rec["tn"][i] = (i * 7 + 3) % n
            rec["ts"][i] = _cycle(E32, i, 3)
            rec["te"][i] = _cycle(E32, i, 4)
            rec["mlrev"][i] = _cycle(E31, i, 6) | (i & 1) << 31
            rec["bldel"][i] = _cycle(E31, i, 7)
        return rec, names, sub, None
    rec = np.zeros(n, dtype=ma.ARC_DT)
    for i in range(n):
        rec["ul"][i] = ((i << 1 | (i >> 1 & 1)) << 32) | _cycle(E32, i, 1)
        rec["v"][i] = ((i * 7 + 3) % n) << 1 | (i & 1)
        rec["oldel"][i] = _cycle(E31, i, 2)
    return rec, names, (sub if with_sub else None), None
