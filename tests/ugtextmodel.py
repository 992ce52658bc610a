"""Python model of the unitig GFA (reference asm.c:77-116, ma_ug_print): the yardstick of tests/test_text_ug_core_cpu.py and tests/test_gpu_text_ug.py.
Lines are made with Python's % formatting of the values C's %d sees (tests/textmodel.py: a uint32_t handed to %d prints as the int with the same bits).
The model speaks the device writer's RECORD space (csrc/text_core.h: tc_ug_t), so that the wave arithmetic of the slow path can be redone from the records'
lengths: the text is the records joined.

A unitig is (len, start, end, members): start == end == 0xffffffff for a circular one, members = the member words (vertex << 32 | length to the next read)."""
import numpy as np

import miniasm_amd as ma
import textmodel as TM

NONE = 0xffffffff
FIXED = 120        # csrc/text_core.h: TC_FIXED_UG -- the longest record without its names (the linear x line)
FIXED_PARTS = {"S": 119, "a": 69, "L": 68, "x": 120}
E31, E32, S_PLUS1, i32 = TM.E31, TM.E32, TM.S_PLUS1, TM.i32
UTG_IDS = [1, 9, 10, 999999, 1000000, 2**31 - 1]


def utg(id1, circ):
    return b"utg%.6d%s" % (i32(id1), b"c" if circ else b"l")


def s_tail(nm, ln, circ):
    t = b"\tLN:i:%d\n" % i32(ln)
    if circ:
        t += b"L\t%s\t+\t%s\t+\t0M\nL\t%s\t-\t%s\t-\t0M\n" % (nm, nm, nm, nm)
    return t


def a_line(nm, l, m, names, sub):
    return b"a\t%s\t%d\t%s\t%s\t%d\n" % (nm, i32(l), TM._read(names, sub, m >> 33), b"+-"[m >> 32 & 1:][:1], i32(m))


def l_line(a, units):
    u, v = int(a["ul"]) >> 32, int(a["v"])
    return b"L\t%s\t%s\t%s\t%s\t%dM\tSD:i:%d\n" % (utg((u >> 1) + 1, units[u >> 1][1] == NONE), b"+-"[u & 1:][:1], utg((v >> 1) + 1, units[v >> 1][1] == NONE), b"+-"[v & 1:][:1],
                                                   int(a["oldel"]) & 0x7fffffff, i32(int(a["ul"])))


def x_line(i, unit, cnt, names, sub, n=None):
    """n: the member count to print (default: that of the unit)"""
    ln, st, en, mem = unit
    n = len(mem) if n is None else n
    if st == NONE:
        return b"x\t%s\t%d\t%d\n" % (utg(i + 1, True), i32(ln), i32(n))
    return b"x\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%s\t%s\n" % (utg(i + 1, False), i32(ln), i32(n), i32(cnt[1]), i32(cnt[0]), TM._read(names, sub, st >> 1), b"+-"[st & 1:][:1],
                                                         TM._read(names, sub, en >> 1), b"+-"[en & 1:][:1])


def records(units, links, counts, names, sub=None, seqs=None, chunk=None):
    """the records of the device writer's record space, in order: per unitig its S record (with sequences: head, chunks of `chunk` bases, tail) and its a records;
    the L records; the x records"""
    out = []
    for i, (ln, st, en, mem) in enumerate(units):
        circ = st == NONE
        nm = utg(i + 1, circ)
        if seqs is None:
            out.append(b"S\t%s\t*" % nm + s_tail(nm, ln, circ))
        else:
            assert len(seqs[i]) == ln
            out.append(b"S\t%s\t" % nm)
            out += [bytes(seqs[i][k:k + chunk]) for k in range(0, ln, chunk)]
            out.append(s_tail(nm, ln, circ))
        l = 0
        for m in mem:
            out.append(a_line(nm, l, int(m), names, sub))
            l = (l + (int(m) & 0xffffffff)) & 0xffffffff
    out += [l_line(a, units) for a in (links if links is not None else [])]
    out += [x_line(i, u, counts[i], names, sub) for i, u in enumerate(units)]
    return out


def text(units, links, counts, names, sub=None, seqs=None):
    return b"".join(records(units, links, counts, names, sub, seqs, 1 << 30))


def slab_records(slab, max_name, chunk=0):
    """records per slab: what was asked for (None: the default), clamped so that records x longest possible record stays below 2^32 (csrc/text_dev.hpp: text_plan)"""
    return min(slab or TM.SLAB, 0xffffffff // max(FIXED + 2 * max_name, chunk))


def make_links(n, U, rnd):
    rec = np.zeros(n, dtype=ma.ARC_DT)
    if n:
        rec["ul"] = rnd.randint(0, 2 * U, n).astype(np.uint64) << np.uint64(32) | rnd.randint(0, 10 ** rnd.randint(1, 6), n).astype(np.uint64)
        rec["v"] = rnd.randint(0, 2 * U, n)
        rec["oldel"] = rnd.randint(0, 30000, n)
    return rec


def make_units(U, n_reads, rnd, members=(1, 2, 63, 64, 65, 200), circ_every=3, lens=None):
    """U unitigs with member counts drawn from `members`, every circ_every-th circular; lens: their lengths (default: the sum of the members' low words)"""
    units = []
    for i in range(U):
        k = int(members[rnd.randint(0, len(members))])
        mem = [(int(rnd.randint(0, 2 * n_reads)) << 32) | int(rnd.randint(0, 10 ** rnd.randint(1, 6))) for _ in range(k)]
        ln = sum(m & 0xffffffff for m in mem) & 0xffffffff if lens is None else lens[i]
        if circ_every and i % circ_every == circ_every - 1:
            units.append((ln, NONE, NONE, mem))
        else:
            units.append((ln, mem[0] >> 32, (mem[-1] >> 32) ^ 1, mem))
    return units


def make_sub(n_reads, rnd):
    sub = np.zeros(n_reads, dtype=ma.SUB_DT)
    sub["sdel"] = rnd.randint(0, 3000, n_reads)
    sub["e"] = sub["sdel"] + rnd.randint(0, 40000, n_reads)
    return sub


def make_seq(n, rnd):
    return bytes(rnd.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), n).tobytes())
