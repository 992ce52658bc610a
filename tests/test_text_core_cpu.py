"""CPU: csrc/text_core.h -- the lines of the -p paf / -p sg / -p bed dumps, as the device text writer (csrc/text_dev.hpp) makes them -- compiled for the host
(tests/text_core_host.c -> miniasm_amd/lib/libtext_core_host.so) and checked line by line against Python's % formatting of the same records (tests/textmodel.py)
and, where oracle/_ref is built, against the reference binary's own dumps.  The length pass and the write pass are the same routine; both are looked at."""
import ctypes as C
import os

import numpy as np
import pytest

import miniasm_amd as ma
import refapi as R
import textmodel as TM

LIB = os.path.join(ma.PKG, "lib", "libtext_core_host.so")
KINDS = {"paf": 1, "sg": 2, "bed": 3}


@pytest.fixture(scope="module")
def tc():
    if not os.path.exists(LIB):
        ma.build()
    L = C.CDLL(LIB)
    vp = C.c_void_p
    L.tc_host_line.restype = C.c_long
    L.tc_host_line.argtypes = [C.c_int, C.c_uint64, vp, vp, vp, vp, vp, vp, C.c_size_t]
    L.tc_host_dump.restype = C.c_longlong
    L.tc_host_dump.argtypes = [C.c_int, C.c_uint64, vp, vp, vp, vp, vp, vp, C.c_size_t]
    L.tc_host_digit_check.restype = C.c_long
    return L


def _pack(names):
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
    return np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8), off


def _ptr(a):
    return None if a is None else a.ctypes.data


def host_lines(L, kind, rec, names, sub, dele):
    """every line through tc_host_line: first the length alone, then the bytes into a buffer of exactly that length"""
    blob, off = _pack(names)
    n = len(names) if kind == "bed" else len(rec)
    out = []
    for r in range(n):
        ln = L.tc_host_line(KINDS[kind], r, _ptr(rec), _ptr(blob), _ptr(off), _ptr(sub), _ptr(dele), None, 0)
        assert ln >= 0
        buf = C.create_string_buffer(ln + 1)
        buf[ln] = b"#"
        assert L.tc_host_line(KINDS[kind], r, _ptr(rec), _ptr(blob), _ptr(off), _ptr(sub), _ptr(dele), buf, ln) == ln
        assert buf[ln] == b"#", "the write pass went past the length the length pass gave"
        out.append(buf.raw[:ln])
    return out


def host_dump(L, kind, rec, names, sub, dele=None):
    blob, off = _pack(names)
    n = len(names) if kind == "bed" else len(rec)
    total = L.tc_host_dump(KINDS[kind], n, _ptr(rec), _ptr(blob), _ptr(off), _ptr(sub), _ptr(dele), None, 0)
    buf = C.create_string_buffer(total + 1)
    assert L.tc_host_dump(KINDS[kind], n, _ptr(rec), _ptr(blob), _ptr(off), _ptr(sub), _ptr(dele), buf, total) == total
    return buf.raw[:total]


def test_digits_without_division(tc):
    """tc_dig5 on every value below 100000 against the quotients, tc_ndig around every power of ten"""
    assert tc.tc_host_digit_check() == 0


@pytest.mark.parametrize("kind,with_sub", [("paf", True), ("sg", True), ("sg", False), ("bed", True)])
def test_value_edges_in_every_field(tc, kind, with_sub):
    rec, names, sub, dele = TM.edge_case(kind, with_sub)
    want = TM.lines(kind, rec, names, sub, dele)
    got = host_lines(tc, kind, rec, names, sub, dele)
    assert got == want
    text = b"".join(want)
    assert host_dump(tc, kind, rec, names, sub, dele) == text
    if kind == "bed":
        assert want.count(b"") >= 4 and any(want), "rows that are del or have s == e print nothing, the others a line"
    else:
        assert b"-2147483648" in text and (b"\t-1\t" in text or b":-1\n" in text) and b"2147483647" in text, "the fields printed from a uint32_t wrap to negative text"
        assert b"\t+\t" in text and b"\t-\t" in text
    if kind == "sg" and not with_sub:
        assert b":1-" not in text and text.startswith(b"L\tr0\t")


def test_bed_rows_that_print_nothing(tc):
    names = [b"a", b"bb", b"ccc", b"dddd"]
    sub = np.zeros(4, dtype=ma.SUB_DT)
    sub["sdel"] = [5, 7, 0, 1 << 31 | 3]  # (bit 31 of word 0 is sub.del, not part of s)
    sub["e"] = [5, 9, 0, 8]
    for dele, want in ((None, [b"", b"bb\t7\t9\n", b"", b"dddd\t3\t8\n"]), (np.array([0, 1, 0, 0], np.uint8), [b"", b"", b"", b"dddd\t3\t8\n"]),
                       (np.array([1, 1, 1, 1], np.uint8), [b""] * 4)):
        assert host_lines(tc, "bed", None, names, sub, dele) == want == TM.lines("bed", None, names, sub, dele)


def _parse_read(tok, names, sub_of):
    name, _, iv = tok.rpartition(b":")
    s1, _, e = iv.partition(b"-")  # (s + 1 is never negative; e may be)
    i = names.setdefault(name, len(names))
    sub_of[i] = (int(s1) - 1, int(e) & 0xffffffff)
    return i


@pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not built")
def test_reference_dumps_round_trip(tc, tmpdir_s):
    """the reference binary's three dumps of one small input, read back into records and written again through text_core.h: the same bytes"""
    paf = R.pafgen(os.path.join(tmpdir_s, "tc_small.paf"), 300, 6000, 17, ["-L", "uniform", "-d", "0.3", "-x", "0.03"])
    # -p paf
    ref, _ = R.run_cli(R.REF_BIN, ["-p", "paf"], paf)
    assert ref.count(b"\n") > 100
    names, sub_of, rows = {}, {}, []
    for ln in ref.splitlines():
        f = ln.split(b"\t")
        q, t = _parse_read(f[0], names, sub_of), _parse_read(f[5], names, sub_of)
        rows.append(((q << 32) | (int(f[2]) & 0xffffffff), int(f[3]), t, int(f[7]), int(f[8]), int(f[9]) | (f[4] == b"-") << 31, int(f[10])))
    rec = np.array(rows, dtype=ma.HIT_DT)
    sub = np.array([sub_of[i] for i in range(len(names))], dtype=ma.SUB_DT)
    assert host_dump(tc, "paf", rec, list(names), sub) == ref
    # -p sg, with kept intervals and (-1 -2) without
    for args, with_sub in ((["-p", "sg", "-S5"], True), (["-1", "-2", "-p", "sg"], False)):
        ref, _ = R.run_cli(R.REF_BIN, args, paf)
        assert ref.count(b"\n") > 20
        names, sub_of, rows = {}, {}, []
        for ln in ref.splitlines():
            f = ln.split(b"\t")
            if with_sub:
                u, v = _parse_read(f[1], names, sub_of), _parse_read(f[3], names, sub_of)
            else:
                u, v = names.setdefault(f[1], len(names)), names.setdefault(f[3], len(names))
            rows.append((((u << 1 | (f[2] == b"-")) << 32) | int(f[6].split(b":")[2]), v << 1 | (f[4] == b"-"), int(f[5].rstrip(b":"))))
        rec = np.array(rows, dtype=ma.ARC_DT)
        sub = np.array([sub_of[i] for i in range(len(names))], dtype=ma.SUB_DT) if with_sub else None
        assert host_dump(tc, "sg", rec, list(names), sub) == ref
    # -p bed
    ref, _ = R.run_cli(R.REF_BIN, ["-p", "bed"], paf)
    assert ref.count(b"\n") > 50
    rows = [ln.split(b"\t") for ln in ref.splitlines()]
    sub = np.array([(int(f[1]), int(f[2])) for f in rows], dtype=ma.SUB_DT)
    assert host_dump(tc, "bed", None, [f[0] for f in rows], sub) == ref
