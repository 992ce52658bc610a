"""The streamed PAF ingest (csrc/paf.hip: mahip_paf_stream_*; host/ingest_gpu.c: ma_hit_ingest_stream / ma_cut_next) at the edges its feature tests
(tests/test_gpu_ingest_stream.py) do not reach: the overflow road of the fold (a probe sequence that runs out, the 4 x rebuild from the arena, the repeated
fold), two names with the same 32-bit tag in one probe chain, the probe that wraps behind the last slot, the table-size decision at half full, the growth of the
arena, of the three per-id arrays and of the record buffer at an exact fit and one over, k_stream_last_bl walking back more than one 64-line step and choosing
among several lines of one step, the per-piece buffers reused by a large, a tiny and a large piece, calls out of order, and the host layer's refusal in the
middle of a stream, a truncated gzip stream, empty input and input without a newline.

Every case goes through check() of tests/test_gpu_ingest_stream.py (the stream against the whole parse, the host reader and, where built, the reference
library: integers, equality everywhere) and asserts from mahip_paf_stream_last, piece by piece, that it met the edge it names.  The names that crowd one probe
chain, share a tag or sit on the last slot are chosen with tests/streammodel.py, a model of the table's hash, which one test anchors to the device by
downloading the table (mahip_paf_stream_tab_download); each case asserts with the model's simulator that its names do what it needs before it runs.

Capacities are exact only without the pool (MA_DEV_POOL=0: a buffer is then the request rounded up to 256 bytes; the pool may hand out more): the growth counts
of the arena and of the per-id arrays are asserted as equalities there and as upper bounds with the pool, and the cases run a second time in a child process
with the pool off (the switch is read once per process).

Not covered, and not faked: the loop inside stream_table (a rebuild that itself runs out of probes).  Whatever the arena holds has already fitted a table of
at most that size, so no input reaches it."""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import miniasm_amd as ma
import refapi as R
import streammodel as SM
import test_gpu_ingest_edges as E
import test_gpu_ingest_stream as S
from test_gpu_ingest_stream import paf_files, tmp  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ln, forced_env, check, gen, cut, cli, n_pieces = E.ln, E.forced_env, S.check, S.gen, S.cut, S.cli, S.n_pieces
SHORT, TEXT = S.SHORT, S.TEXT
IS_EMU = getattr(ma, "IS_EMU", False)
POOL_OFF = os.environ.get("MA_DEV_POOL", "") == "0"


def piece_of(named):
    """lines that bring the (name, length) pairs in this order: line i has pair 2i as its query and pair 2i + 1 as its target, so that local ids follow the list;
    a last odd one is query and target of its line"""
    out = []
    for i in range(0, len(named), 2):
        (q, ql), (t, tl) = named[i], named[i + 1] if i + 1 < len(named) else named[i]
        out.append(ln(q=q, ql=ql, t=t, tl=tl, bl=4000 + i) + b"\n")
    return b"".join(out)


def first_seen(pieces_named):
    """names and lengths in order of first appearance over the pieces"""
    seen = {}
    for named in pieces_named:
        for nm, l in named:
            seen.setdefault(nm, l)
    return list(seen), list(seen.values())


def grow_count(got, want):
    """a growth count: exact without the pool, an upper bound with it (the pool may hand out more than was asked for)"""
    assert got == want if POOL_OFF else got <= want, (got, want, POOL_OFF)


# ------------------------------------------------------------------------------------------------ the model against the device
def test_the_table_holds_what_the_model_says(gpu_ctx, tmp):
    """a few hundred random names into 1 024 slots, a piece at a time; behind every piece the table is downloaded: every occupied slot holds tag << 32 | id of
    a name whose probe sequence reaches it over occupied slots only, every id sits in one slot, no provisional word is left.  The fourth piece makes the host
    rebuild the table (2 x 520 > 1 024): the same holds for the rebuilt one"""
    rs = np.random.RandomState(11)
    names = [b"n%x_%d" % (int(rs.randint(1, 1 << 30)), i) for i in range(520)]
    named = [[(nm, 1000 + i) for i, nm in enumerate(names)][a:b] for a, b in ((0, 150), (150, 300), (300, 450), (450, 520))]
    named[2] = named[2] + named[0][:20]  # some old names among the new ones
    L = ma.lib()
    tabs = []

    def each(k, rep):
        slots = np.zeros(rep.tab_cap, dtype=np.uint64)
        ma._chk(L.mahip_paf_stream_tab_download(gpu_ctx.h, slots.ctypes.data), "paf_stream_tab_download")
        tabs.append((rep.tab_cap, rep.n_rebuilds, slots))

    with forced_env(MA_STREAM_DICT_CAP_LOG2=10):
        info, rep = gpu_ctx.paf_stream([piece_of(p) for p in named], 0, 0, 1, each=each)
    ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")
    assert [(t[0], t[1]) for t in tabs] == [(1024, 0), (1024, 0), (1024, 0), (4096, 1)] and info.n_seq == 520
    for k, n in enumerate((150, 300, 450, 520)):
        assert SM.check_device_table(tabs[k][2], names[:n]) == n
    slots = np.zeros(4096, dtype=np.uint64)
    assert L.mahip_paf_stream_tab_download(gpu_ctx.h, slots.ctypes.data) != 0, "the table is gone behind mahip_paf_stream_end"
    check(gpu_ctx, tmp, [piece_of(p) for p in named], MA_STREAM_DICT_CAP_LOG2=10)


def test_the_model_hashes_as_the_scalar_form():
    h = SM.pool()
    for i in (0, 4, 700378, 1443127, SM.POOL_N - 1):
        assert int(h[i]) == SM.stream_hash(SM.pool_name(i))
    assert SM.home(b"c0700378", 16) == SM.home(b"c1443127", 16) == 15 and SM.tag(b"c0700378") == SM.tag(b"c1443127")


# ------------------------------------------------------------------------------------------------ the fold's overflow road
@pytest.fixture(scope="module")
def crowd():
    """set A: pool names whose home lies in slots 0..63 of 8 192; set B: those of A whose home lies in 0..63 of 32 768 as well"""
    a, b = SM.clustered(8192), SM.clustered(32768)
    assert len(a) >= 2200 and len(b) >= 2200 and set(b) <= set(a)
    return a, b


def _crowd_pieces(names):
    """piece 0: 1 900 names; piece 1: 300 more, interleaved with 50 of the old ones, which state another length"""
    p0 = [(nm, 1000 + i) for i, nm in enumerate(names[:1900])]
    p1 = []
    for i, nm in enumerate(names[1900:2200]):
        p1.append((nm, 5000 + i))
        if i % 6 == 0:
            p1.append((names[37 * (i // 6)], 9))
    assert len(p1) == 350
    return p0, p1


def _assert_overflow_certain(old, new, cap):
    """`old` fits `cap` slots whatever the order; with `new` behind it a probe sequence runs out, in forward and in reversed order"""
    assert SM.overflows(old, cap) == (False, False)
    for rev in (False, True):
        t, out = SM.simulate(old, cap, reverse=rev)
        assert not out and any(t.insert(nm, 0) is None for nm in (reversed(new) if rev else new))


@pytest.mark.parametrize("which", ["A", "B"])
def test_a_probe_sequence_runs_out_and_the_fold_repeats(which, crowd, gpu_ctx, tmp):
    """1 900 names whose homes are slots 0..63 of the 8 192-slot table fill slots below 1 963: no probe is longer than 1 963 < 2 048, in any order.  With 300
    more, 2 200 names need 2 200 slots from slot 0 on: one of them lies at least 2 136 slots behind its home, whatever the schedule.  The table is far from
    half full (2 x 2 250 <= 8 192), so the host does not grow it beforehand: the fold raises the overflow, the table is rebuilt at 32 768 from the arena, the
    claims of the failed launch are gone and the fold repeats.  Set B crowds slots 0..63 of the 32 768-slot table as well: its repeat overflows again"""
    names = crowd[0] if which == "A" else crowd[1]
    p0, p1 = _crowd_pieces(names)
    _assert_overflow_certain([n for n, _ in p0], [n for n, _ in p1 if n not in set(names[:1900])], 8192)
    if which == "B":
        _assert_overflow_certain([n for n, _ in p0], names[1900:2200], 32768)
    assert not any(SM.simulate(names[:2200], 131072 if which == "B" else 32768, reverse=r)[1] for r in (False, True))
    s, w = check(gpu_ctx, tmp, [piece_of(p0), piece_of(p1)], MA_STREAM_DICT_CAP_LOG2=13)
    want_names, want_lens = first_seen([p0, p1])
    assert (s.per[0]["n_fold_repeats"], s.per[0]["n_rebuilds"], s.per[0]["tab_cap"]) == (0, 0, 8192)
    k = 2 if which == "B" else 1
    assert (s.rep["n_fold_repeats"], s.rep["n_rebuilds"], s.rep["tab_cap"]) == (k, k, 8192 << 2 * k), s.rep
    assert s.names[:1900] == names[:1900], "the ids of piece 0 are unchanged"
    assert s.names[1900:] == names[1900:2200], "the new ids follow 2 x line + column"
    assert s.names == want_names and s.lens == want_lens and s.lens[:1900] == [1000 + i for i in range(1900)], "lengths are first-seen"
    assert (s.per[1]["last_local"], s.per[1]["last_new"]) == (350, 300)


def test_the_first_piece_overflows_an_empty_arena(crowd, gpu_ctx, tmp):
    """the overflowing piece first: the rebuild finds no id to insert (it launches nothing), the repeated fold claims every name anew; a second piece looks
    the old names up in the rebuilt table"""
    names = crowd[0]
    p0 = [(nm, 1000 + i) for i, nm in enumerate(names[:2200])]
    p1 = [(nm, 7) for nm in names[100:2200:150]] + [(names[2200], 4242)]
    assert all(SM.overflows(names[:2200], 8192)) and not any(SM.overflows(names[:2201], 32768))
    s, w = check(gpu_ctx, tmp, [piece_of(p0), piece_of(p1)], MA_STREAM_DICT_CAP_LOG2=13)
    assert (s.per[0]["n_fold_repeats"], s.per[0]["n_rebuilds"], s.per[0]["tab_cap"]) == (1, 1, 32768), s.per[0]
    assert (s.rep["n_fold_repeats"], s.rep["n_rebuilds"], s.per[1]["last_new"]) == (1, 1, 1)
    assert s.names == names[:2201] and s.lens == [1000 + i for i in range(2200)] + [4242]


# ------------------------------------------------------------------------------------------------ tags and the wrap, in 16 slots
@pytest.fixture(scope="module")
def twins():
    """two names with the same tag and the same home in 16 slots"""
    pairs = SM.equal_tag_pairs(16)
    assert (b"c0700378", b"c1443127") in pairs
    a, b = b"c0700378", b"c1443127"
    assert SM.tag(a) == SM.tag(b) and SM.home(a, 16) == SM.home(b, 16) == 15 and a != b
    return a, b


@pytest.mark.parametrize("order", [0, 1])
def test_equal_tags_in_different_pieces(order, twins, gpu_ctx, tmp):
    """the second twin's probe meets the first one's slot: same tag, same length, other bytes -- it must go on and claim a slot of its own; then both are
    looked up as targets"""
    a, b = twins[order], twins[1 - order]
    pieces = [ln(q=a, ql=111, t="x", tl=1) + b"\n", ln(q=b, ql=222, t="x", tl=2) + b"\n", ln(q="y", ql=3, t=a, tl=4) + b"\n" + ln(q="z", ql=5, t=b, tl=6) + b"\n"]
    s, w = check(gpu_ctx, tmp, pieces, MA_STREAM_DICT_CAP_LOG2=4)
    assert s.names == [a, b"x", b, b"y", b"z"] and s.lens == [111, 1, 222, 3, 5] and s.rep["tab_cap"] == 16
    assert [(p["last_local"], p["last_new"]) for p in s.per] == [(2, 2), (2, 1), (4, 2)]
    assert [int(h["tn"]) for h in s.hits[::2]] == [1, 1, 0, 2], "each twin keeps its own id"


def test_equal_tags_in_one_piece(twins, gpu_ctx, tmp):
    """both twins in one fold: the claim of one is a provisional word with their common tag while the other probes"""
    a, b = twins
    p0 = ln(q=a, ql=111, t=b, tl=222) + b"\n" + ln(q=b, ql=9, t=a, tl=9) + b"\n"
    p1 = ln(q=b, ql=1, t=a, tl=2) + b"\n"
    s, w = check(gpu_ctx, tmp, [p0, p1], MA_STREAM_DICT_CAP_LOG2=4)
    assert s.names == [a, b] and s.lens == [111, 222] and [(p["last_local"], p["last_new"]) for p in s.per] == [(2, 2), (2, 0)]
    assert [(int(h["qns"] >> 32), int(h["tn"])) for h in s.hits[::2]] == [(0, 1), (1, 0), (1, 0)]


def test_a_name_and_its_prefix_with_equal_tags(gpu_ctx, tmp):
    """the stored name is 11 bytes, the name looked up its first 8 bytes, both with one tag and one home: the length decides before any byte is compared
    (without it the 8 bytes compare equal).  The pair was found by search; the model confirms it"""
    long, short = b"p5052265iiz", b"p5052265"
    assert long.startswith(short) and SM.tag(long) == SM.tag(short) and SM.home(long, 16) == SM.home(short, 16) == 12
    p0 = ln(q=long, ql=111, t="x", tl=1) + b"\n"
    p1 = ln(q=short, ql=222, t=long, tl=2) + b"\n"
    p2 = ln(q=long, ql=3, t=short, tl=4) + b"\n"
    s, w = check(gpu_ctx, tmp, [p0, p1, p2], MA_STREAM_DICT_CAP_LOG2=4)
    assert s.names == [long, b"x", short] and s.lens == [111, 1, 222] and [p["last_form"] for p in s.per] == [TEXT, TEXT, TEXT]
    assert [(int(h["qns"] >> 32), int(h["tn"])) for h in s.hits[::2]] == [(0, 1), (2, 0), (0, 2)]


def test_the_probe_wraps_behind_the_last_slot(gpu_ctx, tmp):
    """four names whose home is slot 15 of 16: the second takes slot 0, the third slot 1; the fourth, in a later piece, wraps on its way in and every lookup
    of a later piece wraps on its way to them"""
    n = SM.with_home(15, 16, 4)
    assert n == [b"c0000004", b"c0000006", b"c0000013", b"c0000015"] and all(SM.home(x, 16) == 15 for x in n)
    t, out = SM.simulate(n, 16)
    assert not out and sorted(t.where.values()) == [0, 1, 2, 15]
    p0 = piece_of([(n[0], 10), (n[1], 11), (n[2], 12)])
    p1 = piece_of([(n[3], 13), (n[2], 99)])
    p2 = piece_of([(n[1], 98), (n[3], 97), (n[0], 96), (n[2], 95)])
    s, w = check(gpu_ctx, tmp, [p0, p1, p2], MA_STREAM_DICT_CAP_LOG2=4)
    assert s.names == n and s.lens == [10, 11, 12, 13] and s.rep["tab_cap"] == 16 and s.rep["n_rebuilds"] == 0
    assert [(p["last_local"], p["last_new"]) for p in s.per] == [(3, 3), (2, 1), (4, 0)]


def test_the_rebuild_wraps_behind_the_last_slot(gpu_ctx, tmp):
    """three names whose home is slot 63 of 64, first in 16 slots; six more names make the host rebuild the table at 64 slots: k_stream_rebuild puts one of the
    three on slot 63 and the others, behind the wrap, on slots 0 and 1, where the lookups of the last piece must find them"""
    n = SM.with_home(63, 64, 3)
    assert len(n) == 3 and all(SM.home(x, 64) == 63 and SM.home(x, 16) == 15 for x in n)
    for rev in (False, True):
        t, out = SM.simulate(n, 64, reverse=rev)
        assert not out and sorted(t.where.values()) == [0, 1, 63]
    more = _fresh(1, 6)
    pieces = [piece_of([(n[0], 10), (n[1], 11), (n[2], 12)]), piece_of(more), piece_of([(n[2], 99), (n[1], 98), (n[0], 97), (more[0][0], 96)])]
    s, w = check(gpu_ctx, tmp, pieces, MA_STREAM_DICT_CAP_LOG2=4)
    assert [(p["tab_cap"], p["n_rebuilds"]) for p in s.per] == [(16, 0), (64, 1), (64, 1)] and s.rep["n_fold_repeats"] == 0
    assert s.names == n + [x for x, _ in more] and s.lens[:3] == [10, 11, 12] and (s.per[2]["last_local"], s.per[2]["last_new"]) == (4, 0)


def test_a_nine_byte_and_an_eight_byte_name_share_a_home(gpu_ctx, tmp):
    """piece 0 holds names of at most 8 bytes (its local table is keyed by the bytes), piece 1 a 9-byte name with the same home in the persistent table (its
    local table compares text), piece 2 is short again and looks both up"""
    short = b"c0000004"
    nine = next(b"d%08d" % i for i in range(10000) if SM.home(b"d%08d" % i, 16) == SM.home(short, 16))
    assert len(nine) == 9 and SM.home(nine, 16) == SM.home(short, 16) == 15
    p0 = ln(q=short, ql=10, t="x", tl=1) + b"\n"
    p1 = ln(q=nine, ql=20, t=short, tl=2) + b"\n"
    p2 = ln(q="x", ql=3, t=short, tl=4) + b"\n"
    p3 = ln(q=nine, ql=5, t="y", tl=30) + b"\n"
    s, w = check(gpu_ctx, tmp, [p0, p1, p2, p3], MA_STREAM_DICT_CAP_LOG2=4)
    assert [p["last_form"] for p in s.per] == [SHORT, TEXT, SHORT, TEXT] and s.names == [short, b"x", nine, b"y"] and s.lens == [10, 1, 20, 30]


# ------------------------------------------------------------------------------------------------ the table-size decision
def _fresh(k, n, first=0):
    return [(b"t%d_%d" % (k, i), 100 * k + i + first) for i in range(n)]


@pytest.mark.parametrize("r1,want_cap,rebuilds", [(4, 16, 0), (5, 64, 1), (12, 64, 1), (13, 128, 1)])
def test_the_table_grows_when_more_than_half_could_fill(r1, want_cap, rebuilds, gpu_ctx, tmp):
    """16 slots, 4 names in them, a piece of r1 local names: 2 x (4 + r1) = 16 leaves the table alone, 18 grows it.  The new size is the larger of 4 x the old one
    and the power of two at or above 4 x (names so far + local names); since growth means names > half the slots, the latter is never the smaller: 9 to 16 names
    give 64 by either, 17 give 128 by the latter alone"""
    p0, p1 = _fresh(0, 4), _fresh(1, r1)
    s, w = check(gpu_ctx, tmp, [piece_of(p0), piece_of(p1)], MA_STREAM_DICT_CAP_LOG2=4)
    assert (s.per[0]["tab_cap"], s.per[0]["n_rebuilds"]) == (16, 0)
    assert (s.rep["tab_cap"], s.rep["n_rebuilds"], s.rep["n_fold_repeats"]) == (want_cap, rebuilds, 0), s.rep
    assert s.info["n_seq"] == 4 + r1 and s.per[1]["last_new"] == r1


def test_a_first_piece_too_large_for_the_switch(gpu_ctx, tmp):
    s, w = check(gpu_ctx, tmp, [piece_of(_fresh(0, 8))], MA_STREAM_DICT_CAP_LOG2=4)
    assert (s.rep["tab_cap"], s.rep["n_rebuilds"]) == (16, 0)
    s, w = check(gpu_ctx, tmp, [piece_of(_fresh(0, 9)), piece_of(_fresh(1, 2))], MA_STREAM_DICT_CAP_LOG2=4)
    assert (s.per[0]["tab_cap"], s.per[0]["n_rebuilds"]) == (64, 0), "the first table is sized for the piece; it replaces none"
    assert (s.rep["tab_cap"], s.rep["n_rebuilds"]) == (64, 0)


def test_a_piece_without_a_new_name_at_half_full(gpu_ctx, tmp):
    """the decision counts the piece's local names, not its new ones (those are known only behind the fold): 4 names + 4 old ones leave 16 slots alone; 8 names
    in 16 slots + 2 old ones grow the table although nothing is added"""
    p0 = _fresh(0, 4)
    s, w = check(gpu_ctx, tmp, [piece_of(p0), piece_of([(n, 7) for n, _ in reversed(p0)])], MA_STREAM_DICT_CAP_LOG2=4)
    assert (s.rep["tab_cap"], s.rep["n_rebuilds"], s.per[1]["last_local"], s.per[1]["last_new"]) == (16, 0, 4, 0)
    p1 = _fresh(1, 4)
    s, w = check(gpu_ctx, tmp, [piece_of(p0), piece_of(p1), piece_of([(p1[3][0], 7), (p0[0][0], 8)])], MA_STREAM_DICT_CAP_LOG2=4)
    assert [(p["tab_cap"], p["n_rebuilds"]) for p in s.per] == [(16, 0), (16, 0), (64, 1)] and (s.per[2]["last_local"], s.per[2]["last_new"]) == (2, 0)
    assert s.info["n_seq"] == 8


# ------------------------------------------------------------------------------------------------ arena and per-id arrays
def sized_names(k, total, w=24):
    """distinct names (with lengths to state) that take exactly `total` bytes of the arena (every name + its NUL)"""
    assert total >= 2 * w
    n = total // w - 1
    names = [(b"a%d_%04d" % (k, i)).ljust(w - 1, b"x") for i in range(n)]
    names.append((b"a%d_last" % k).ljust(total - n * w - 1, b"y"))
    assert sum(len(x) + 1 for x in names) == total and len(set(names)) == len(names)
    return [(nm, 100 + i) for i, nm in enumerate(names)]


def round256(x):
    return (x + 255) & ~255


def arena_model(totals):
    """paf_stream_fold's rule for the arena, without the pool: -> the growth count behind every piece"""
    cap = used = grows = 0
    out = []
    for t in totals:
        need = used + t + 16
        if need > cap:
            grows += cap > 0
            cap = round256(max(need, 2 * cap))
        used += t
        out.append(grows)
    return out


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_arena_fit_pool_off_too(d, gpu_ctx, tmp):
    """piece 0 leaves 500 bytes of names in an arena of 768 (500 + 16 rounded up to 256 bytes); piece 1 brings names that need one byte less than, exactly, and
    one byte more than those 768"""
    totals = [500, 768 - 16 - 500 + d]
    assert arena_model(totals) == [0, int(d > 0)]
    named = [sized_names(k, t) for k, t in enumerate(totals)]
    s, w = check(gpu_ctx, tmp, [piece_of(p) for p in named])
    assert s.info["name_bytes"] == sum(totals) and (s.names, s.lens) == tuple(first_seen(named))
    grow_count(s.rep["n_arena_grow"], int(d > 0))
    assert s.per[0]["n_arena_grow"] == 0


@pytest.mark.parametrize("how,totals,want", [("more_than_doubles", [500, 4000, 4608 - 16 - 4500], [0, 1, 1]), ("more_than_doubles_then_one_over", [500, 4000, 4608 - 16 - 4500 + 1], [0, 1, 2]),
                                             ("less_than_doubles", [500, 600, 1536 - 16 - 1100], [0, 1, 1]), ("less_than_doubles_then_one_over", [500, 600, 1536 - 16 - 1100 + 1], [0, 1, 2])])
def test_arena_growth_pool_off_too(how, totals, want, gpu_ctx, tmp):
    """a piece whose names (about 200 bytes each) need more than twice the arena: the new one is what is needed (4 516 -> 4 608 bytes); one that needs less than
    twice: the new one is twice the old (2 x 768).  Which it was shows in the piece behind: names that end exactly on the new capacity leave it alone, one more
    byte grows it again"""
    assert arena_model(totals) == want
    named = [sized_names(k, t, 200 if t >= 4000 else 24) for k, t in enumerate(totals)]
    named[2] = named[2] + named[0][:3]  # old names: what the copy kept is looked up
    s, w = check(gpu_ctx, tmp, [piece_of(p) for p in named])
    assert s.info["name_bytes"] == sum(totals) and (s.names, s.lens) == tuple(first_seen(named))
    for k in range(3):
        grow_count(s.per[k]["n_arena_grow"], want[k])


def ids_model(counts):
    """the rule for the three per-id arrays ((ids + 4) x 4 bytes each), without the pool: -> the growth count behind every piece"""
    cap = n = grows = 0
    out = []
    for k in counts:
        need = (n + k + 4) * 4
        if need > cap:
            grows += cap > 0
            cap = round256(max(need, 2 * cap))
        n += k
        out.append(grows)
    return out


@pytest.mark.parametrize("n_ids", [59, 60, 61, 123, 124, 125])
def test_per_id_arrays_pool_off_too(n_ids, gpu_ctx, tmp):
    """(ids + 4) x 4 bytes reach 256 at 60 ids and 512 at 124: 2 ids take 256 bytes; up to 60 fit them, 61 do not; 100 ids take 512, up to 124 fit, 125 do not"""
    counts = [2, n_ids - 2] if n_ids < 100 else [2, 98, n_ids - 100]
    want = ids_model(counts)
    assert want == {59: [0, 0], 60: [0, 0], 61: [0, 1], 123: [0, 1, 1], 124: [0, 1, 1], 125: [0, 1, 2]}[n_ids]
    named = [_fresh(k, c) for k, c in enumerate(counts)]
    named[-1] = named[-1] + named[0]  # the ids of piece 0 are looked up behind the copies
    s, w = check(gpu_ctx, tmp, [piece_of(p) for p in named])
    assert s.info["n_seq"] == n_ids and (s.names, s.lens) == tuple(first_seen(named))
    for k in range(len(counts)):
        grow_count(s.per[k]["n_ids_grow"], want[k])


def test_growth_cases_with_the_pool_off():
    """the capacity of a buffer is the rounded request only without the pool, and the switch is read once per process: the *_pool_off_too cases again in a child
    process with MA_DEV_POOL=0, where their growth counts are equalities"""
    if POOL_OFF:
        return  # this process already runs them so
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"] + (["-p", "emu_plugin"] if IS_EMU else [])
    cmd += [os.path.abspath(__file__), "-k", "pool_off_too"]
    r = subprocess.run(cmd, cwd=ma.ROOT, env=dict(os.environ, MA_DEV_POOL="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    tail = r.stdout[-4000:]
    assert r.returncode == 0, tail
    assert "13 passed" in tail and " failed" not in tail and " skipped" not in tail, tail


# ------------------------------------------------------------------------------------------------ the record buffer
def rec_model(cap, bounds, stored):
    """the rule for the record buffer: bounds[k] = the most records piece k can store, stored[k] = what it stores -> the growth count behind every piece"""
    n = grows = 0
    out = []
    for b, s in zip(bounds, stored):
        if n + b > cap:
            cap = max(2 * cap, n + b)
            grows += 1
        n += s
        out.append(grows)
    return out


def _rec_pieces(bi_dir):
    """pieces of 6, 4, 45 and 1 lines; with bi_dir two lines of piece 0 and one of piece 2 have q == t: their mirror is not stored, the bound counts it"""
    lines = gen(56, 21)
    own = [0, 3, 20] if bi_dir else []
    for i in own:
        lines[i] = ln(q="self%d" % i, ql=9000, t="self%d" % i, tl=9000, bl=700 + i) + b"\n"
    pieces = cut(lines, [6, 4, 45])
    m = 2 if bi_dir else 1
    bounds = [6 * m, 4 * m, 45 * m, 1 * m]
    stored = [6 * m - 2, 4 * m, 45 * m - 1, 1 * m] if bi_dir else bounds
    return pieces, bounds, stored


@pytest.mark.parametrize("bi_dir", [0, 1])
@pytest.mark.parametrize("short_by", [0, 1])
def test_the_record_buffer_at_an_exact_fit_and_one_over(short_by, bi_dir, gpu_ctx, tmp):
    """MA_STREAM_REC_CAP = what pieces 0 and 1 can store at most, and one record less: no growth, and one (to twice the capacity).  Piece 2 can store more than
    twice what there is: the buffer becomes exactly records + bound, so that piece 3, one line, grows it again.  With bi_dir the bound (2 per line) exceeds what
    is stored (lines with q == t have no mirror): the decision takes the bound"""
    pieces, bounds, stored = _rec_pieces(bi_dir)
    cap = stored[0] + bounds[1] - short_by
    want = rec_model(cap, bounds, stored)
    assert want == ([0, 0, 1, 2] if not short_by else [0, 1, 2, 3]) and bounds[2] > 2 * 2 * cap
    s, w = check(gpu_ctx, tmp, pieces, 0, 0, bi_dir, MA_STREAM_REC_CAP=cap)
    assert s.info["n_hits"] == sum(stored) and [p["n_rec_grow"] for p in s.per] == want, (s.per, want)
    if bi_dir:
        assert s.info["n_hits"] == 2 * s.info["n_stored_lines"] - 3


@pytest.mark.parametrize("bi_dir", [0, 1])
def test_the_first_piece_is_measured_by_its_bound(bi_dir, gpu_ctx, tmp):
    """with bi_dir, MA_STREAM_REC_CAP = the records piece 0 stores is one short of its bound: the buffer grows although everything would have fitted"""
    pieces, bounds, stored = _rec_pieces(bi_dir)
    s, w = check(gpu_ctx, tmp, pieces[:1], 0, 0, bi_dir, MA_STREAM_REC_CAP=stored[0])
    assert s.rep["n_rec_grow"] == (1 if bi_dir else 0) and s.info["n_hits"] == stored[0]
    s, w = check(gpu_ctx, tmp, pieces[:1], 0, 0, bi_dir, MA_STREAM_REC_CAP=bounds[0])
    assert s.rep["n_rec_grow"] == 0


# ------------------------------------------------------------------------------------------------ k_stream_last_bl
def _bl_case(ctx, tmp, L, ks, first9=False, last9=False):
    """piece 0 ends with an 11-column line (bl 1111); piece 1 has L lines of which those in ks have an 11th column (bl 2000 + line), the others ten; piece 2 is
    five 10-column lines, which inherit what piece 1 leaves behind: the bl of its last 11-column line, or 1111 when it has none"""
    p0 = ln(q="a", t="b", bl=7) + b"\n" + ln(q="a", t="c", bl=1111) + b"\n"
    mid = [ln(q="m%d" % (i % 7), t="n%d" % (i % 5), bl=2000 + i, ncol=11 if i in ks else 10) + b"\n" for i in range(L)]
    if first9:
        mid[0] = ln(q="junk", ncol=9) + b"\n"
    if last9:
        mid[-1] = ln(q="junk", ncol=9) + b"\n"
    p2 = b"".join(ln(q="z", t="y%d" % i, ncol=10) + b"\n" for i in range(5))
    s, w = check(ctx, tmp, [p0, b"".join(mid), p2], bi_dir=0)
    live = [k for k in ks if not (first9 and k == 0) and not (last9 and k == L - 1)]
    left = 2000 + max(live) if live else 1111
    assert [int(h["bldel"]) for h in s.hits[-5:]] == [left] * 5, (L, ks, [int(h["bldel"]) for h in s.hits[-5:]], left)
    assert [p["last_before"] for p in s.per] == [0, 1111, left], (L, ks, s.per)
    first_is_ten = 0 not in ks and not first9
    assert [p["n_inherited"] for p in s.per] == [0, int(first_is_ten), int(first_is_ten) + 1], (L, ks, s.per)
    assert s.last.n_lines == 5


@pytest.mark.parametrize("L", [1, 64, 65, 128, 129, 193])
def test_the_last_bl_of_a_piece_wherever_it_stands(L, gpu_ctx, tmp):
    """one wave walks back from the last line, 64 lines a step: the only 11-column line of the piece on both sides of every step border, in the first and the
    last line, and nowhere (what an earlier piece left stays)"""
    ks = sorted({k for k in (0, 1, L - 129, L - 128, L - 65, L - 64, L - 63, L - 1) if 0 <= k < L})
    _bl_case(gpu_ctx, tmp, L, ())
    for k in ks:
        _bl_case(gpu_ctx, tmp, L, (k,))


@pytest.mark.parametrize("L,ks", [(64, (3, 40)), (64, (0, 31, 62)), (130, (70, 100, 128)), (130, (10, 60, 64)), (130, (1, 65)), (193, (0, 64, 128)), (193, (5, 6, 7))])
def test_several_candidates_for_the_last_bl(L, ks, gpu_ctx, tmp):
    """two and three 11-column lines with different bl inside one 64-line step and across two: the highest line wins"""
    _bl_case(gpu_ctx, tmp, L, ks)


@pytest.mark.parametrize("L,ks", [(65, (0, 30)), (65, (0,)), (130, (129, 3)), (130, (129,)), (64, ())])
def test_a_nine_column_line_first_and_last(L, ks, gpu_ctx, tmp):
    """a line with fewer than 10 columns has no bl to leave and inherits none: as line 0 (whose flags decide n_inherited) and as the last line (where the walk
    starts)"""
    _bl_case(gpu_ctx, tmp, L, ks, first9=True)
    _bl_case(gpu_ctx, tmp, L, ks, last9=True)


# ------------------------------------------------------------------------------------------------ per-piece buffers reused
@pytest.mark.parametrize("small_stores", [True, False])
def test_large_tiny_large_pieces(small_stores, gpu_ctx, tmp):
    """3 000 lines / 1 line / 500 lines / 1 line / 3 000 lines: text, columns and the local table of a tiny piece live in the buffers of a large one and hold its
    leftovers.  Long names (the local table compares text) in the large pieces, short ones in the tiny; the largest start coordinate stands in piece 0"""
    big0, mid, big1 = gen(3000, 31, 300, "a_name_longer_than_eight_bytes_"), gen(500, 32, 300, "a_name_longer_than_eight_bytes_"), gen(3000, 33, 500, "a_name_longer_than_eight_bytes_")
    big0[1234] = ln(q="a_name_longer_than_eight_bytes_7", ql=99000, qs=77777, qe=90000, t="a_name_longer_than_eight_bytes_8", tl=99000, ts=100, te=12000, bl=13000) + b"\n"
    if small_stores:
        tiny = [ln(q="r1", ql=5000, t="r2", tl=6000) + b"\n", ln(q="r2", ql=1, t="r3", tl=7000) + b"\n"]
    else:
        tiny = [ln(q="r1", qs=0, qe=100, ts=0, te=100) + b"\n"] * 2  # spans of 100 < 2000: nothing stored
    pieces = [b"".join(big0), tiny[0], b"".join(mid), tiny[1], b"".join(big1)]
    s, w = check(gpu_ctx, tmp, pieces, 2000, 100)
    t = SHORT if small_stores else 0
    assert [p["last_form"] for p in s.per] == [TEXT, t, TEXT, t, TEXT], s.per
    assert [p["last_local"] for p in s.per][1::2] == ([2, 2] if small_stores else [0, 0])
    assert s.info["max_qs"] == 77777 == w.info["max_qs"]
    assert s.info["n_lines"] == 6502 and s.last.n_lines == 3000


def test_max_qs_is_the_streams_not_the_last_pieces(gpu_ctx, tmp):
    L = ma.lib()
    L.mahip_paf_max_qs.restype = C.c_uint32
    L.mahip_paf_max_qs.argtypes = [C.c_void_p]
    a, b = gen(30, 41), gen(30, 42)
    a[7] = ln(q="r1", ql=99000, qs=300, qe=9000, t="r2", tl=99000, ts=55555, te=64000) + b"\n"
    s = S.streamed(gpu_ctx, [b"".join(a), b"".join(b)], 2000, 100, 1, release=False)
    assert s.info["max_qs"] == 55555 and L.mahip_paf_max_qs(gpu_ctx.h) == 55555
    ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")
    s = S.streamed(gpu_ctx, [b"".join(b), b"".join(a)], 2000, 100, 1, release=False)
    assert s.info["max_qs"] == 55555 and L.mahip_paf_max_qs(gpu_ctx.h) == 55555
    ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")
    check(gpu_ctx, tmp, [b"".join(a), b"".join(b)], 2000, 100)


# ------------------------------------------------------------------------------------------------ calls out of order
def _same(a, b):
    assert a.info == b.info and a.names == b.names and a.lens == b.lens and a.hits.tobytes() == b.hits.tobytes()


@pytest.fixture(scope="module")
def fresh(gpu_ctx):
    """what a context that has done nothing else makes of one text, whole and in three pieces"""
    lines = gen(90, 51)
    pieces = cut(lines, [30, 30])
    c = ma.Ctx(0)
    try:
        w = S.whole(c, b"".join(lines), 2000, 100, 1)
    finally:
        c.close()
    c = ma.Ctx(0)
    try:
        s = S.streamed(c, pieces, 2000, 100, 1)
    finally:
        c.close()
    _same(s, w)
    assert w.info["n_hits"] > 40
    return pieces, w


def test_end_without_a_last_piece(fresh, gpu_ctx):
    """no piece was flagged last: end takes what there is"""
    pieces, want = fresh
    L = ma.lib()
    ma._chk(L.mahip_paf_stream_begin(gpu_ctx.h, 2000, 100, 1), "begin")
    for p in pieces:
        ma._chk(L.mahip_paf_stream_piece_mem(gpu_ctx.h, C.create_string_buffer(p, len(p)), len(p), 0), "piece")
    info = ma.PafInfo()
    ma._chk(L.mahip_paf_stream_end(gpu_ctx.h, C.byref(info)), "end")
    _same(S._results(gpu_ctx, info), want)
    assert gpu_ctx.paf_stream_last().n_pieces == 3
    ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")


def test_begin_twice_and_begin_over_a_loaded_text(fresh, gpu_ctx):
    pieces, want = fresh
    L = ma.lib()
    other = b"".join(gen(40, 52, prefix="other"))
    ma._chk(L.mahip_paf_stream_begin(gpu_ctx.h, 0, 0, 0), "begin")
    ma._chk(L.mahip_paf_stream_piece_mem(gpu_ctx.h, C.create_string_buffer(other, len(other)), len(other), 0), "piece")
    _same(S.streamed(gpu_ctx, pieces, 2000, 100, 1), want)  # its begin drops the stream above: no name, record or setting of it is left
    ma._chk(L.mahip_paf_load_mem(gpu_ctx.h, C.create_string_buffer(other, len(other)), len(other)), "paf_load_mem")
    s = S.streamed(gpu_ctx, pieces, 2000, 100, 1, release=False)  # over a loaded text nobody parsed
    _same(s, want)
    info = ma.PafInfo()
    assert L.mahip_paf_parse_excl(gpu_ctx.h, 0, 0, 1, 0, 0, C.c_float(0), C.byref(info)) != 0, "the loaded text is gone: nothing to parse"
    ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")


def test_abort_then_a_whole_parse_then_a_stream(fresh, gpu_ctx):
    pieces, want = fresh
    L = ma.lib()
    other = gen(40, 53, prefix="other")
    ma._chk(L.mahip_paf_stream_begin(gpu_ctx.h, 0, 0, 0), "begin")
    for p in cut(other, [10, 20]):
        ma._chk(L.mahip_paf_stream_piece_mem(gpu_ctx.h, C.create_string_buffer(p, len(p)), len(p), 0), "piece")
    assert gpu_ctx.paf_stream_last().n_pieces == 3
    ma._chk(L.mahip_paf_stream_abort(gpu_ctx.h), "abort")
    assert L.mahip_paf_stream_last(gpu_ctx.h, None) != 0
    _same(S.whole(gpu_ctx, b"".join(pieces), 2000, 100, 1), want)
    _same(S.streamed(gpu_ctx, pieces, 2000, 100, 1), want)


def test_columns_behind_end_are_the_last_pieces(gpu_ctx):
    """mahip_paf_cols_download behind mahip_paf_stream_end: the columns of the last piece that had text, as a whole parse of that piece alone leaves them (all
    its lines have an 11th column: nothing is inherited)"""
    lines = gen(75, 54)
    pieces = cut(lines, [40]) + [b""]
    alone = E.device_parse(gpu_ctx, pieces[1], 2000, 100, 1)
    ma._chk(ma.lib().mahip_paf_release(gpu_ctx.h), "paf_release")
    S.streamed(gpu_ctx, pieces, 2000, 100, 1, release=False)
    L = ma.lib()
    n = 35
    flags, odd, nums = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros((8, n), dtype=np.uint32)
    tnoff, qlen, tlen = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    lstart, tfirst = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(int(alone.rep.n_tiles), 1), dtype=np.uint64)
    ma._chk(L.mahip_paf_cols_download(gpu_ctx.h, flags.ctypes.data, odd.ctypes.data, nums.ctypes.data, tnoff.ctypes.data, qlen.ctypes.data, tlen.ctypes.data, lstart.ctypes.data,
                                      tfirst.ctypes.data), "paf_cols_download")
    ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")
    assert alone.rep.n_lines == n and (flags == alone.flags).all() and (nums == alone.nums).all() and (lstart == alone.lstart).all()
    assert (tnoff == alone.tnoff).all() and (qlen == alone.qlen).all() and (tlen == alone.tlen).all() and (flags & 1).all()


# ------------------------------------------------------------------------------------------------ the host layer: the command line
PIECE = S.PIECE


def _gz(path, text, level=1):
    with gzip.open(path, "wb", compresslevel=level) as g:
        g.write(text)
    return path


def test_cli_a_piece_refused_in_the_middle(paf_files, tmp):
    """one line of 9 000 bytes halfway through, MA_PAF_MAX_BYTES=4096: the pieces in front are taken, the long line's piece is refused.  A file is read again by the
    host reader (a warning, the output of the unstreamed run); what came from stdin is gone: an error of the run"""
    def long_line(text):
        lines = text.splitlines(keepends=True)
        k = len(lines) // 2
        lines[k] = lines[k][:-1] + b"\tzz:Z:" + b"Q" * (9000 - len(lines[k]) - 6) + b"\n"
        assert len(lines[k]) == 9000
        return b"".join(lines)
    path, text = S._rewrite(paf_files, tmp, "stream_mid.paf", long_line)
    gz = _gz(path + ".gz", text)
    env = dict(PIECE, MA_PAF_MAX_BYTES="4096")
    out, log, _ = cli([], gz, env=env)
    m = re.search(r"text of (\d+) bytes exceeds MA_PAF_MAX_BYTES", log)
    assert m and int(m.group(1)) >= 9000, "it was the long line's piece that was refused, not the first: " + log[-1500:]
    assert out == paf_files[2] and "using the host reader" in log and n_pieces(log) == 0
    out, log, rc = cli([], stdin=gz, env=env, ok=False)
    m = re.search(r"text of (\d+) bytes exceeds MA_PAF_MAX_BYTES", log)
    assert rc != 0 and "[E::" in log and out == b"" and m and int(m.group(1)) >= 9000, log[-1500:]
    out, log, _ = cli([], stdin=gz, env=PIECE)  # without the cap the long line is a piece like any other
    assert out == paf_files[2] and n_pieces(log) > 100


@pytest.mark.parametrize("how", ["file", "stdin"])
def test_cli_a_truncated_gzip_stream(how, paf_files, tmp):
    """a .gz file that lacks its last 20 000 bytes: zlib hands out what it can inflate and then reports the damage; the lines so far count (the last of them cut
    anywhere), as in the unstreamed run and in the reference"""
    with open(paf_files[0], "rb") as f:
        text = f.read()
    whole_gz = _gz(os.path.join(tmp, "stream_whole6.gz"), text, 6)
    with open(whole_gz, "rb") as f:
        comp = f.read()
    assert len(comp) > 40000
    path = os.path.join(tmp, "stream_cut.paf.gz")
    with open(path, "wb") as f:
        f.write(comp[:-20000])
    src = dict(paf=path) if how == "file" else dict(stdin=path)
    out, log, _ = cli([], env=PIECE, **src)
    off, log0, _ = cli([], env=dict(PIECE, MA_INGEST_STREAM="0"), **src)
    assert n_pieces(log) > 50 and n_pieces(log0) == 0
    assert out == off and out != paf_files[2]
    assert R.counters(log) == R.counters(log0)
    if R.have_ref():
        assert R.norm_lines(out) == R.norm_lines(R.run_cli(R.REF_BIN, [], path)[0])


def test_cli_empty_input(tmp):
    out, log, rc = cli([], env=PIECE)  # stdin at its end from the start
    assert (out, rc) == (b"", 0) and n_pieces(log) == 1, log[-1500:]
    path = os.path.join(tmp, "stream_empty.paf")
    open(path, "wb").close()
    for env in (PIECE, dict(PIECE, MA_INGEST_STREAM="1"), dict(PIECE, MA_INGEST_STREAM="0")):
        out, log, rc = cli([], path, env=env)
        assert (out, rc) == (b"", 0), log[-1500:]
    out, log, rc = cli([], stdin=path, env=PIECE)
    assert (out, rc) == (b"", 0) and n_pieces(log) == 1


def test_cli_text_without_any_newline(paf_files, tmp):
    """3 000 bytes, one line, no newline: the buffer grows twice and the end of the input hands the line over as the only piece"""
    line = E.padded(ln(q="q1", t="t1"), 3000)
    path = os.path.join(tmp, "stream_nonl.paf")
    with open(path, "wb") as f:
        f.write(line)
    out, log, rc = cli(["-p", "paf"], stdin=path, env=PIECE)
    off, log0, _ = cli(["-p", "paf"], stdin=path, env=dict(PIECE, MA_INGEST_STREAM="0"))
    assert n_pieces(log) == 1 and n_pieces(log0) == 0 and out == off and R.counters(log) == R.counters(log0)
    assert "read 1 hits; stored 2 hits" in log, log[-1500:]


def test_cli_text_of_newlines_only(tmp):
    path = os.path.join(tmp, "stream_nl.paf")
    with open(path, "wb") as f:
        f.write(b"\n" * 5000)
    out, log, rc = cli([], stdin=path, env=PIECE)
    off, log0, _ = cli([], stdin=path, env=dict(PIECE, MA_INGEST_STREAM="0"))
    assert n_pieces(log) == 5 and (out, rc) == (b"", 0) and out == off and R.counters(log) == R.counters(log0)
