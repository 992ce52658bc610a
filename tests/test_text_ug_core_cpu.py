"""CPU: the unitig-GFA routines of csrc/text_core.h -- tc_utg, the S / a / L / x lines, the record space of tc_line_ug -- compiled for the host
(tests/text_ug_host.c -> miniasm_amd/lib/libtext_ug_host.so).  Every line routine runs next to snprintf with the reference's own format strings (asm.c:77-116),
at the value edges 0, 10^k - 1, 10^k, 2^31 - 1, 2^31, 2^32 - 1 of every integer field; the Python model (tests/ugtextmodel.py) is held against the same bytes;
the whole record space -- bisection, chunks, the wrapping offset l -- is walked on hand-made unitigs."""
import ctypes as C
import os

import numpy as np
import pytest

import miniasm_amd as ma
import textmodel as TM
import ugtextmodel as UM

LIB = os.path.join(ma.PKG, "lib", "libtext_ug_host.so")
CAP = 70000
NONE = UM.NONE


class TcUg(C.Structure):  # csrc/text_core.h: tc_ug_t
    _fields_ = [("U", C.c_uint32), ("n_links", C.c_uint32), ("chunk", C.c_uint32), ("n_unit_rec", C.c_uint64)] + \
               [(k, C.c_void_p) for k in ("u_n", "u_len", "u_start", "u_end", "moff", "rbase", "mscan", "links", "cnt", "mem", "uoff", "arena")]


@pytest.fixture(scope="module")
def tu():
    if not os.path.exists(LIB):
        ma.build()
    L = C.CDLL(LIB)
    u32, i32, cp, sz = C.c_uint32, C.c_int, C.c_char_p, C.c_size_t
    for name, args in (("tu_utg", [u32, i32]), ("tu_s", [u32, i32, u32, cp]), ("tu_a", [u32, i32, u32, C.c_uint64, cp, i32, u32, u32]), ("tu_l", [u32, u32, u32, u32, i32, i32]),
                       ("tu_x", [u32, u32, u32, u32, u32, u32, u32, cp, cp, i32, C.c_void_p])):
        f = getattr(L, name)
        f.restype = C.c_long
        f.argtypes = args + [C.c_void_p, sz]
    L.tu_dump.restype = C.c_longlong
    L.tu_dump.argtypes = [C.POINTER(TcUg), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, sz, C.POINTER(C.c_uint64)]
    L.tu_sizeof_ug.restype = sz
    assert L.tu_sizeof_ug() == C.sizeof(TcUg)
    return L


def call(f, *args):
    """the routine's bytes; the C side has already compared them with snprintf's"""
    buf = C.create_string_buffer(CAP)
    n = f(*args, buf, CAP)
    assert n >= 0, "%s%r: %s" % (f.__name__, args, {-1: "the length pass and the write pass disagree", -2: "differs from snprintf: %r" % buf.value, -3: "buffer"}[n])
    return buf.raw[:n]


@pytest.mark.parametrize("id1", UM.UTG_IDS + [2**31, 2**32 - 1])
def test_utg_name(tu, id1):
    """utg%.6d%c: six digits at least, more from 1 000 000 on; a sign stands in front of the padded digits"""
    for circ in (0, 1):
        assert call(tu.tu_utg, id1, circ) == UM.utg(id1, circ) == b"utg%.6d%s" % (TM.i32(id1), b"lc"[circ:circ + 1])
    if id1 < 2**31:
        assert len(call(tu.tu_utg, id1, 0)) == 3 + max(6, len(str(id1))) + 1


def test_s_line_at_every_edge(tu):
    for ln in UM.E32:
        for circ in (0, 1):
            for id1 in (1, 1000000):
                nm = UM.utg(id1, circ)
                assert call(tu.tu_s, id1, circ, ln, None) == b"S\t%s\t*" % nm + UM.s_tail(nm, ln, circ)
    for seq in (b"", b"A", b"ACGTNacgtn" * 300):
        for circ in (0, 1):
            nm = UM.utg(7, circ)
            assert call(tu.tu_s, 7, circ, len(seq), seq) == b"S\t%s\t%s" % (nm, seq) + UM.s_tail(nm, len(seq), circ)


@pytest.mark.parametrize("have_sub", [0, 1])
def test_a_line_at_every_edge(tu, have_sub):
    names = [b"read/1"]
    for k, v in enumerate(UM.E32):
        for field in range(4):
            l, low, s, e = 5, 7, 3, 9
            if field == 0:
                l = v
            elif field == 1:
                low = v
            elif field == 2:
                s = UM.S_PLUS1[k % len(UM.S_PLUS1)]
            else:
                e = v
            strand = k & 1
            m = strand << 32 | low
            sub = np.array([(s, e)], dtype=ma.SUB_DT) if have_sub else None
            got = call(tu.tu_a, 12, k >> 1 & 1, l, m, names[0], have_sub, s, e)
            assert got == UM.a_line(UM.utg(12, k >> 1 & 1), l, m, names, sub)
    assert len(call(tu.tu_a, 2**31, 0, 2**31, 1 << 32 | 2**31, b"", 1, 2**31 - 2, 2**31)) <= tu.tu_fixed(1)


def test_l_line_at_every_edge(tu):
    units = [(0, 0, 1, []), (0, NONE, NONE, [])] * 2
    for k, v in enumerate(UM.E32):
        for field in range(2):
            ol, ln = (UM.E31[k % len(UM.E31)], 77) if field == 0 else (12, v)
            u, w = k % 8, (k * 3 + 1) % 8
            rec = np.array([((u << 32) | ln, w, ol)], dtype=ma.ARC_DT)
            assert call(tu.tu_l, u, w, ol, ln, units[u >> 1][1] == NONE, units[w >> 1][1] == NONE) == UM.l_line(rec[0], units)
    for id1 in UM.UTG_IDS:  # the unitig ids of both ends
        got = call(tu.tu_l, (id1 - 1) << 1 | 1, (id1 - 1) << 1, 5, 6, 1, 0)
        assert got == b"L\t%s\t-\t%s\t+\t5M\tSD:i:6\n" % (UM.utg(id1, 1), UM.utg(id1, 0))
    assert len(call(tu.tu_l, 0xffffffff, 0xffffffff, 2**31 - 1, 2**31, 1, 1)) <= tu.tu_fixed(2)


@pytest.mark.parametrize("have_sub", [0, 1])
def test_x_line_at_every_edge(tu, have_sub):
    names = [b"alpha", b"be"]
    for k, v in enumerate(UM.E32):
        for field in range(6):
            ln, n, c0, c1, s, e = 100, 3, 1, 2, 4, 50
            if field == 0:
                ln = v
            elif field == 1:
                n = v
            elif field == 2:
                c0 = v
            elif field == 3:
                c1 = v
            elif field == 4:
                s = UM.S_PLUS1[k % len(UM.S_PLUS1)]
            else:
                e = v
            sw = np.array([s, e, 11, 22], dtype=np.uint32)
            sub = sw.view(ma.SUB_DT) if have_sub else None
            for start, end in ((k & 3, (k >> 1) & 3), (NONE, NONE)):
                got = call(tu.tu_x, 1000000, ln, n, start, end, c0, c1, names[0], names[1], have_sub, sw.ctypes.data)
                want = UM.x_line(999999, (ln, start, end, []), (c0, c1), names, sub, n=n)
                assert got == want
    sw = np.array([2**31 - 2, 2**31, 2**31 - 2, 2**31], dtype=np.uint32)
    assert len(call(tu.tu_x, 2**31, 2**31, 2**31, 1, 3, 2**31, 2**31, b"", b"", 1, sw.ctypes.data)) == tu.tu_fixed(3) - 2  # (s + 1 never needs the eleventh byte the bound grants every %d)
    assert tu.tu_fixed(3) == UM.FIXED
    assert [tu.tu_fixed(k) for k in range(4)] == [UM.FIXED_PARTS[k] for k in "SaLx"] and tu.tu_fixed(4) == max(UM.FIXED_PARTS.values())
    assert len(call(tu.tu_s, 2**31, 1, 2**31, None)) == tu.tu_fixed(0)


def host_gfa(tu, units, links, counts, names, sub, seqs, chunk):
    """the record space built as the device builds it (csrc/text_dev.hpp: text_plan_ug), walked by tc_line_ug on the host"""
    U = len(units)
    u_len = np.array([u[0] for u in units], dtype=np.uint32)
    u_start = np.array([u[1] for u in units], dtype=np.uint32)
    u_end = np.array([u[2] for u in units], dtype=np.uint32)
    u_n = np.array([len(u[3]) for u in units], dtype=np.uint32)
    mem = np.array([m for u in units for m in u[3]] + [0], dtype=np.uint64)
    per = 1 + u_n.astype(np.uint64) + (0 if seqs is None else 1 + (u_len.astype(np.uint64) + chunk - 1) // chunk)
    rbase = np.concatenate(([0], np.cumsum(per))).astype(np.uint32)
    moff = np.concatenate(([0], np.cumsum(u_n.astype(np.uint64)))).astype(np.uint32)
    mscan = np.concatenate(([0], np.cumsum(mem & np.uint64(0xffffffff)))).astype(np.uint64) & np.uint64(0xffffffff)
    mscan = mscan.astype(np.uint32)
    lk = np.ascontiguousarray(links, dtype=ma.ARC_DT)
    cnt = np.ascontiguousarray(np.array(list(counts) + [(0, 0)], dtype=np.uint32).reshape(-1))
    g = TcUg(U=U, n_links=len(lk), chunk=chunk, n_unit_rec=int(per.sum()))
    keep = dict(u_n=u_n, u_len=u_len, u_start=u_start, u_end=u_end, moff=moff, rbase=rbase, mscan=mscan, links=lk, cnt=cnt, mem=mem)
    if seqs is not None:
        keep["arena"] = np.frombuffer(b"".join(bytes(x) + b"\0" for x in seqs) + b"\0", dtype=np.uint8)
        keep["uoff"] = np.concatenate(([0], np.cumsum(u_len.astype(np.uint64) + 1))).astype(np.uint64)
    for k, a in keep.items():
        setattr(g, k, a.ctypes.data)
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
    blob = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
    n_rec = g.n_unit_rec + len(lk) + U
    nl = C.c_uint64(0)
    subp = None if sub is None else sub.ctypes.data
    total = tu.tu_dump(C.byref(g), n_rec, blob.ctypes.data, off.ctypes.data, subp, None, 0, C.byref(nl))
    buf = C.create_string_buffer(total + 1)
    assert tu.tu_dump(C.byref(g), n_rec, blob.ctypes.data, off.ctypes.data, subp, buf, total, C.byref(nl)) == total
    return buf.raw[:total], nl.value, n_rec


@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("with_seq", [False, True])
def test_record_space_on_the_host(tu, with_sub, with_seq):
    """mixed linear and circular unitigs, links, counts: every record through tc_line_ug, joined, against the model; the reported '\\n' count is the text's"""
    rnd = np.random.RandomState(11)
    names = [b"r%d" % i + b"x" * (i % 9) for i in range(50)]
    chunk = 128
    lens = [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, 5 * chunk + 17] if with_seq else None
    units = UM.make_units(7, len(names), rnd, members=(1, 2, 5, 70), lens=lens)
    links = UM.make_links(40, len(units), rnd)
    counts = [(int(rnd.randint(0, 9)), int(rnd.randint(0, 9))) for _ in units]
    sub = UM.make_sub(len(names), rnd) if with_sub else None
    seqs = [UM.make_seq(u[0], rnd) for u in units] if with_seq else None
    got, nl, n_rec = host_gfa(tu, units, links, counts, names, sub, seqs, chunk)
    recs = UM.records(units, links, counts, names, sub, seqs, chunk)
    assert got == b"".join(recs) == UM.text(units, links, counts, names, sub, seqs)
    assert nl == got.count(b"\n") and n_rec == len(recs)


def test_offset_l_wraps_through_2_32(tu):
    """members of 2^31, 2^31 and 5 bases: the reference's uint32_t l is 0, 2^31 (printed -2147483648), 0, 5"""
    names = [b"a", b"b", b"c", b"d"]
    units = [(7, 0, 7, [(0 << 32) | 2**31, (2 << 32) | 2**31, (4 << 32) | 5, (6 << 32) | 9])]
    got, _, _ = host_gfa(tu, units, UM.make_links(0, 1, None), [(0, 0)], names, None, None, 128)
    offs = [ln.split(b"\t")[2] for ln in got.splitlines() if ln.startswith(b"a\t")]
    assert offs == [b"0", b"-2147483648", b"0", b"5"]
    assert got == UM.text(units, [], [(0, 0)], names)
