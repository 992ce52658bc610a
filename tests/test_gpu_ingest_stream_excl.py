"""-R in the streamed PAF ingest (csrc/paf.hip: mahip_paf_stream_begin_excl; host/ingest_gpu.c: ma_hit_ingest_stream_excl, MA_STREAM_NOCONT=1): one text
handed over in pieces of whole lines must leave exactly what mahip_paf_parse_excl leaves on the concatenated text -- every mahip_paf_info_t field (n_excl
included), names, first-seen lengths, the records bytewise.  All are integers and bytes: equality everywhere.  Every case is compared with the same text through
the whole device parse, through tests/pafmodel.py, through the host reader (ma_hit_no_cont + ma_hit_ingest) and, where oracle/_ref is built, through the
reference library.  Texts are 5 to about 350 lines, pieces 0 to 4 KiB; each case asserts from mahip_paf_stream_excl_last that it met the edge it names.

One arrangement cannot come out as its first description had it: with the two containment lines in the LAST piece, "no line dropped early" cannot hold, because
a line that carries a verdict touches the name it flags and is dropped in its own piece (the verdicts of a piece come before its drop).  The case asserts that
EXACTLY these two lines are dropped early and every other excluded line late.

The command-line cases drive the host layer with MA_STREAM_NOCONT=1 MA_INGEST_PIECE=1024 on a gzip'd pafgen file with a length spread and compare with the same
command without the switch (the whole text inflated first, mahip_paf_parse_excl), with the plain file and, where built, with the reference binary."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import miniasm_amd as ma
import pafmodel as PM
import refapi as R
import test_gpu_ingest_edges as E
import test_gpu_ingest_stream as S

pytestmark = pytest.mark.gpu

ln, forced_env, cut = E.ln, E.forced_env, S.cut
IS_EMU = getattr(ma, "IS_EMU", False)
POOL_OFF = os.environ.get("MA_DEV_POOL", "") == "0"
SPAN, MATCH, NC = 2000, 100, (1000, 0.8)  # what test_no_cont_prefilter uses
SHORT, TEXT = 1, 2  # MAHIP_PAF_DICT_*
XFIELDS = [f for f, _ in ma.PafStreamExclReport._fields_] if hasattr(ma, "PafStreamExclReport") else []


@pytest.fixture(scope="module")
def tmp(tmpdir_s):
    return tmpdir_s


def streamed(ctx, pieces, min_span, min_match, bi_dir, no_cont):
    per = []
    info, rep = ctx.paf_stream(pieces, min_span, min_match, bi_dir, each=lambda k, r: per.append(S._copy(r)), no_cont=no_cont)
    r = S._results(ctx, info)
    r.rep, r.per = S._copy(rep), per
    x = ctx.paf_stream_excl_last()
    r.x = {f: int(getattr(x, f)) for f in XFIELDS}
    ma._chk(ma.lib().mahip_paf_release(ctx.h), "paf_release")
    return r


def same_as(s, info, names, lens, hits, who):
    assert s.info == info, (who, s.info, info)
    assert s.names == names and s.lens == lens, "names / first-seen lengths differ from " + who
    assert s.hits.tobytes() == hits.tobytes(), "records differ from " + who


def check(ctx, tmp, pieces, min_span=SPAN, min_match=MATCH, bi_dir=1, no_cont=NC, **env):
    """the pieces through the stream with -R (under the switches in env); their concatenation through the whole parse, the model, the host reader, the reference"""
    text = b"".join(pieces)
    with forced_env(**env):
        s = streamed(ctx, pieces, min_span, min_match, bi_dir, no_cont)
    d = E.device_parse(ctx, text, min_span, min_match, bi_dir, no_cont)
    ma._chk(ma.lib().mahip_paf_release(ctx.h), "paf_release")
    same_as(s, {f: int(getattr(d.info, f)) for f in S.INFO_FIELDS}, d.names, [int(x) for x in d.lens], d.hits, "the whole parse")
    M = PM.model(text, min_span, min_match, bi_dir, None, no_cont)
    assert s.names == M.names and s.lens == M.lens and s.hits.tobytes() == M.hits.tobytes(), "stream and model disagree"
    assert (s.info["n_lines"], s.info["n_records"], s.info["n_stored_lines"], s.info["n_hits"], s.info["n_seq"], s.info["n_excl"]) == \
        (M.L, int(M.valid.sum()), int(M.stored.sum()), len(M.hits), len(M.names), len(M.excl))
    path = os.path.join(tmp, "stream_excl.paf")
    with open(path, "wb") as f:
        f.write(text)
    h_hits, h_names, h_lens, h_excl = E.host_reader(path, min_span, min_match, bi_dir, no_cont)
    assert h_names == s.names and h_lens == s.lens and h_hits.tobytes() == s.hits.tobytes() and h_excl == s.info["n_excl"], "stream and host reader disagree"
    if os.path.exists(R.REF_LIB):
        r_hits, r_names, r_lens, r_excl = E.host_reader(path, min_span, min_match, bi_dir, no_cont, R.ref())
        r_hits["bldel"] &= 0x7FFFFFFF
        assert r_names == s.names and r_lens == s.lens and r_excl == s.info["n_excl"], "stream and reference library disagree"
        assert R.canon(r_hits).tobytes() == R.canon(s.hits).tobytes(), "stream and reference library disagree"
    # ---- the report's own arithmetic
    x = s.x
    assert s.rep["n_pieces"] == len(pieces) and s.rep["n_empty"] == sum(1 for p in pieces if not p)
    assert x["n_early_lines"] + x["n_late_lines"] == int(M.passed.sum()) - int(M.stored.sum()), (x, int(M.passed.sum()), int(M.stored.sum()))
    assert x["n_flagged"] == len(M.excl) and x["n_renumbered"] == len(M.names)
    assert x["peak_records"] == len(M.hits) + x["n_late_records"], "what the stream held at the peak: the records it keeps and those it retired at the end"
    if not bi_dir:
        assert x["n_late_records"] == x["n_late_lines"]
    return s, M


CONT = [ln(q="big1", ql=30000, qs=5000, qe=14000, t="inner1", tl=9000, ts=10, te=8990),           # verdict 1: the target is inside the query
        ln(q="inner2", ql=9000, qs=10, qe=8990, t="big2", tl=30000, ts=5000, te=14000, st="-")]   # verdict 2: the query is inside the target


def base_lines():
    """the text of test_no_cont_prefilter, line by line (each with its newline)"""
    lines = [ln(q="first", t="second", ql=9000, tl=9000, qs=100, qe=5000, ts=100, te=5000)] + CONT
    lines.append(ln(q="inner3", ql=9000, qs=10, qe=8990, t="big3", tl=30000, ts=5000, te=14000, ml=10))  # a line the filter drops: excludes nobody
    lines.append(ln(q="inner3", t="first"))
    for k in range(300):
        q, t = ("inner1", "big2") if k % 17 == 0 else ("r%d" % (k % 40), "inner2" if k % 13 == 0 else "r%d" % ((k * 7) % 43))
        lines.append(ln(q=q, t=t, qs=k, qe=4000 + k, ts=k, te=4100))
    return [x + b"\n" for x in lines]


def the_base_results(s, M):
    assert M.excl == {b"inner1", b"inner2"} and s.info["n_excl"] == 2 and b"inner3" in s.names and b"inner1" not in s.names and b"inner2" not in s.names
    assert b"big3" not in s.names, "a line the filter drops gives no verdict and no name"


# ------------------------------------------------------------------------------------------------ 1. cuts
def test_one_piece(gpu_ctx, tmp):
    s, M = check(gpu_ctx, tmp, [b"".join(base_lines())])
    the_base_results(s, M)
    assert s.x["n_late_lines"] == 0 and s.x["n_early_lines"] > 20, "one piece: its own verdicts drop every line at once"


def test_every_line_its_own_piece(gpu_ctx, tmp):
    s, M = check(gpu_ctx, tmp, base_lines())
    the_base_results(s, M)
    assert s.rep["n_pieces"] == 305 and s.x["n_early_lines"] > 20 and s.x["n_late_lines"] == 0, "the containment lines lead every line that touches their reads"


def test_empty_pieces_first_in_the_middle_and_last(gpu_ctx, tmp):
    L = base_lines()
    s, M = check(gpu_ctx, tmp, [b"", b"".join(L[:2]), b"", b"", b"".join(L[2:100]), b"", b"".join(L[100:]), b""])
    the_base_results(s, M)
    assert s.rep["n_empty"] == 5 and s.x["n_early_lines"] > 0


# ------------------------------------------------------------------------------------------------ 2. early and late
def _arranged(where):
    L = base_lines()
    rest = [L[0]] + L[3:]
    if where == "first":
        return [b"".join(L[:3])] + cut(rest[1:], [50, 100])
    if where == "last":
        return cut(rest, [50, 100, 100]) + [b"".join(L[1:3])]
    return cut(rest, [50, 100])[:2] + [b"".join(L[1:3])] + [b"".join(rest[150:])]


@pytest.mark.parametrize("early", [None, 0])
@pytest.mark.parametrize("where", ["first", "last", "middle"])
def test_early_and_late(gpu_ctx, tmp, where, early):
    pieces = _arranged(where)
    s, M = check(gpu_ctx, tmp, pieces, MA_STREAM_NOCONT_EARLY=early)
    the_base_results(s, M)
    x, n_dropped = s.x, int(M.passed.sum()) - int(M.stored.sum())
    assert n_dropped > 20
    if early == 0:  # the test switch: nothing goes early, the same bytes (check() has compared them)
        assert x["n_early_lines"] == 0 and x["n_late_lines"] == n_dropped
    elif where == "first":
        assert x["n_early_lines"] == n_dropped and x["n_late_lines"] == 0 and x["n_late_records"] == 0
    elif where == "last":  # (the two lines that carry the verdicts go in their own piece: see the module's docstring)
        assert x["n_early_lines"] == 2 and x["n_late_lines"] == n_dropped - 2 > 0 and x["n_late_records"] == 2 * x["n_late_lines"]
    else:
        assert x["n_early_lines"] > 2 and x["n_late_lines"] > 0 and x["n_early_lines"] + x["n_late_lines"] == n_dropped


# ------------------------------------------------------------------------------------------------ 3. ids shift
def test_a_name_without_a_surviving_line_gets_no_id(gpu_ctx, tmp):
    """big1's only line touches an excluded read: no id for it, and every later id moves up -- inner3 at index 2, not 6 (what test_no_cont_prefilter asserts on the model)"""
    L = base_lines()
    s, M = check(gpu_ctx, tmp, cut(L, [1, 1, 1, 1, 1, 40]))
    plain = PM.model(b"".join(L), SPAN, MATCH, 1)
    assert b"big1" not in s.names and b"big2" not in s.names and plain.names.index(b"inner3") == 6 and s.names.index(b"inner3") == 2
    assert s.x["n_renumbered"] == len(plain.names) - 4


# ------------------------------------------------------------------------------------------------ 4. first-seen length
@pytest.mark.parametrize("bi_dir", [1, 0])
@pytest.mark.parametrize("one_piece", [False, True])
def test_first_seen_length_is_that_of_the_first_surviving_line(gpu_ctx, tmp, bi_dir, one_piece):
    L = [ln(q="x", ql=9000, t="inner1", tl=9000),    # x first states 9000, on a line whose partner is excluded
         ln(q="inner2", ql=9000, t="y", tl=8000),    # y first states 8000, as a target, on such a line
         CONT[0], CONT[1],
         ln(q="z", ql=9500, t="y", tl=8100),         # the first surviving appearance of y
         ln(q="x", ql=9100, t="w", tl=9000),         # ... of x
         ln(q="y", ql=8200, t="x", tl=9200)]         # later statements do not count
    L = [x + b"\n" for x in L]
    s, M = check(gpu_ctx, tmp, [b"".join(L)] if one_piece else L, bi_dir=bi_dir)
    assert s.names == [b"z", b"y", b"x", b"w"] and s.lens == [9500, 8100, 9100, 9000], (s.names, s.lens)
    plain = PM.model(b"".join(L), SPAN, MATCH, bi_dir)
    assert plain.lens[plain.names.index(b"x")] == 9000 and plain.lens[plain.names.index(b"y")] == 8000, "without -R the first appearance overall counts"
    if not one_piece:
        assert s.x["n_late_lines"] == 2 and s.x["n_early_lines"] == 2


# ------------------------------------------------------------------------------------------------ 5. a dropped line gives no verdict
def test_a_line_the_filter_drops_gives_no_verdict(gpu_ctx, tmp):
    L = [ln(q="a", t="b"), ln(q="inner3", ql=9000, qs=10, qe=8990, t="big3", tl=30000, ts=5000, te=14000, ml=10), ln(q="inner3", t="a"), ln(q="big3", ql=30000, t="b")]
    L = [x + b"\n" for x in L]
    s, M = check(gpu_ctx, tmp, L)
    assert s.info["n_excl"] == 0 and s.names == [b"a", b"b", b"inner3", b"big3"] and s.info["n_stored_lines"] == 3 and s.x["n_early_lines"] == s.x["n_late_lines"] == 0
    s, M = check(gpu_ctx, tmp, L, min_match=5)  # with a lower bar the same line is stored and does exclude
    assert s.info["n_excl"] == 1 and b"inner3" not in s.names


# ------------------------------------------------------------------------------------------------ 6. everything excluded
def test_everything_excluded(gpu_ctx, tmp):
    L = base_lines()[1:3]
    for pieces in ([b"".join(L)], L):
        s, M = check(gpu_ctx, tmp, pieces)
        assert s.info["n_seq"] == s.info["n_hits"] == s.info["n_stored_lines"] == s.info["name_bytes"] == 0 and s.info["n_excl"] == 2
        assert s.x["n_early_lines"] == 2 and s.x["n_renumbered"] == 0 and s.x["peak_records"] == 0
    s, M = check(gpu_ctx, tmp, [L[0], L[1]], MA_STREAM_NOCONT_EARLY=0)  # ... at the end, out of a record buffer that holds four
    assert s.info["n_seq"] == s.info["n_hits"] == 0 and s.info["n_excl"] == 2 and s.x["n_late_records"] == 4 and s.x["peak_records"] == 4


def test_begin_excl_and_end_alone_give_zeros(gpu_ctx, tmp):
    s, M = check(gpu_ctx, tmp, [])
    assert all(v == 0 for v in s.info.values()) and all(v == 0 for v in s.x.values())
    s, M = check(gpu_ctx, tmp, [b""])
    assert all(v == 0 for v in s.info.values()) and s.rep["n_empty"] == 1


# ------------------------------------------------------------------------------------------------ 7. self hits
@pytest.mark.parametrize("bi_dir", [1, 0])
def test_self_hits_among_surviving_and_dropped_lines(gpu_ctx, tmp, bi_dir):
    """a self hit gives one record under -b (hit.c:87-98): the lines behind the records are counted from records and self hits, alive or dead"""
    L = [ln(q="a", t="b"), ln(q="a", t="a"), ln(q="inner1", t="inner1"), ln(q="inner1", t="a"), ln(q="b", t="b"),
         CONT[0], ln(q="inner1", t="inner1", qs=77, qe=4000), ln(q="b", t="a"), ln(q="c", t="c")]
    L = [x + b"\n" for x in L]
    s, M = check(gpu_ctx, tmp, cut(L, [2, 2, 1, 2]), bi_dir=bi_dir)
    assert s.info["n_stored_lines"] == 5 and s.info["n_hits"] == (7 if bi_dir else 5) and s.names == [b"a", b"b", b"c"]
    assert s.x["n_late_lines"] == 2 and s.x["n_late_records"] == (3 if bi_dir else 2) and s.x["n_early_lines"] == 2
    s, M = check(gpu_ctx, tmp, cut(L, [2, 2, 1, 2]), bi_dir=bi_dir, MA_STREAM_NOCONT_EARLY=0)
    assert s.x["n_late_lines"] == 4 and s.x["n_late_records"] == (6 if bi_dir else 4)


# ------------------------------------------------------------------------------------------------ 8. both verdicts, both strands; a name flagged twice
def test_both_verdicts_on_both_strands_and_a_name_flagged_twice(gpu_ctx, tmp):
    def v1(q, t, st):
        return ln(q=q, ql=30000, qs=5000, qe=14000, t=t, tl=9000, ts=10, te=8990, st=st)

    def v2(q, t, st):
        return ln(q=q, ql=9000, qs=10, qe=8990, t=t, tl=30000, ts=5000, te=14000, st=st)
    L = [ln(q="a", t="b"), ln(q="a", t="i1"), ln(q="i2", t="b"), ln(q="i3", t="a"), ln(q="b", t="i4"),
         v1("B1", "i1", "+"), v1("B2", "i2", "-"),
         v2("i3", "B3", "+"), v2("i4", "B4", "-"), ln(q="a", t="c"),
         v2("i1", "B5", "-"), v1("B3", "i4", "+"), ln(q="c", t="b")]  # i1 and i4 are flagged again, by another piece and by the other verdict
    L = [x + b"\n" for x in L]
    assert [PM.no_cont_verdict(30000, 5000, 14000, 9000, 10, 8990, r, *NC) for r in (False, True)] == [1, 1]
    assert [PM.no_cont_verdict(9000, 10, 8990, 30000, 5000, 14000, r, *NC) for r in (False, True)] == [2, 2]
    s, M = check(gpu_ctx, tmp, cut(L, [5, 2, 3]))
    assert M.excl == {b"i1", b"i2", b"i3", b"i4"} and s.info["n_excl"] == 4 and s.x["n_flagged"] == 4 and s.names == [b"a", b"b", b"c"]
    assert s.x["n_late_lines"] == 4 and s.x["n_early_lines"] == 6
    check(gpu_ctx, tmp, L, bi_dir=0)


# ------------------------------------------------------------------------------------------------ 9. the stale bl
def test_a_ten_column_line_inherits_the_bl_of_a_dropped_line(gpu_ctx, tmp):
    """paf.c:54 leaves bl alone on a 10-column line whatever happens to the line in front: a dropped 11-column line at the end of piece k still hands its bl on"""
    p0 = ln(q="a", t="b", bl=1111) + b"\n" + ln(q="big1", ql=30000, qs=5000, qe=14000, t="inner1", tl=9000, ts=10, te=8990, bl=777) + b"\n"
    p1 = ln(q="a", t="c", ncol=10) + b"\n" + ln(q="inner1", t="a", bl=55) + b"\n" + ln(q="b", t="c", ncol=10) + b"\n"
    s, M = check(gpu_ctx, tmp, [p0, p1], bi_dir=0)
    assert [int(h["bldel"]) for h in s.hits] == [1111, 777, 55] and s.per[1]["last_before"] == 777 and s.rep["n_inherited"] == 1
    assert s.x["n_early_lines"] == 2 and s.names == [b"a", b"b", b"c"]


# ------------------------------------------------------------------------------------------------ 10. growth
def growth_pieces():
    """flags are raised in piece 0; then 12 pieces of 30 new names each (the table, the per-id arrays, the flags, the records and the lengths are all replaced while
    those flags stand), lines that touch the flagged reads all along, and a containment in the last piece that kills lines of piece 3"""
    pieces = [b"".join(x + b"\n" for x in [ln(q="a", t="inner1"), ln(q="inner2", t="a")] + CONT)]
    for k in range(12):
        out = []
        for i in range(30):
            t = "inner1" if i % 11 == 3 else "n%d_%d" % (max(k - 1, 0), (7 * i) % 30)
            out.append(ln(q="n%d_%d" % (k, i), ql=9000 + i, t=t, tl=9000 + (7 * i) % 30, qs=i, qe=4000 + i))
        pieces.append(b"".join(x + b"\n" for x in out))
    pieces.append(ln(q="late", ql=30000, qs=5000, qe=14000, t="n3_5", tl=9005, ts=10, te=8990) + b"\n" + ln(q="n0_1", t="inner2") + b"\n")
    return pieces


def _growth(ctx, tmp):
    pieces = growth_pieces()
    s, M = check(ctx, tmp, pieces, MA_STREAM_DICT_CAP_LOG2=4, MA_STREAM_REC_CAP=8)
    assert M.excl == {b"inner1", b"inner2", b"n3_5"} and s.info["n_seq"] > 300
    assert s.rep["n_rebuilds"] > 0 and s.rep["n_rec_grow"] > 0, s.rep
    assert s.x["n_early_lines"] > 12 and s.x["n_late_lines"] == 2, s.x  # (n3_5 is a query in piece 4 and a target in piece 5)
    if POOL_OFF:  # whether a buffer must be REPLACED depends on what the pool handed out (it may give more than was asked for): without it, every one is
        assert s.rep["n_ids_grow"] > 0 and s.x["n_flag_grow"] > 0 and s.x["n_lens_grow"] > 0, (s.rep, s.x)
    t, _ = check(ctx, tmp, pieces)
    assert t.rep["n_rebuilds"] == 0 and t.rep["n_rec_grow"] == 0 and t.x["n_lens_grow"] == 0, "the same result without a single growth"
    assert (t.names, t.lens, t.hits.tobytes()) == (s.names, s.lens, s.hits.tobytes())
    return s


def test_flags_survive_every_growth(gpu_ctx, tmp):
    _growth(gpu_ctx, tmp)


def test_flags_survive_every_growth_pool_off_too(gpu_ctx, tmp):
    """(run by the case below in a process of its own with MA_DEV_POOL=0: a replaced buffer is then really another one, of exactly the rounded request)"""
    s = _growth(gpu_ctx, tmp)
    if POOL_OFF:  # 256 bytes of flags hold 240 ids + the 16 spare; 364 ids come in steps of 30: one replacement (256 -> 512)
        assert s.x["n_flag_grow"] == 1, s.x


def test_growth_with_the_pool_off():
    if POOL_OFF:
        return  # this process already runs it so
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"] + (["-p", "emu_plugin"] if IS_EMU else [])
    cmd += [os.path.abspath(__file__), "-k", "pool_off_too"]
    r = subprocess.run(cmd, cwd=ma.ROOT, env=dict(os.environ, MA_DEV_POOL="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    tail = r.stdout[-4000:]
    assert r.returncode == 0, tail
    assert "1 passed" in tail and " failed" not in tail and " skipped" not in tail, tail


# ------------------------------------------------------------------------------------------------ 11. long names
def test_an_excluded_long_name_then_short_names(gpu_ctx, tmp):
    long_in, long_big = "inner_read_with_a_long_name/1", "a_big_read_with_a_long_name/22"
    p0 = [ln(q="long_name_a", t=long_in), ln(q=long_big, ql=30000, qs=5000, qe=14000, t=long_in, tl=9000, ts=10, te=8990), ln(q="long_name_a", t="long_name_bb")]
    p1 = [ln(q="s1", t="s2"), ln(q="s2", t="s3")]
    p2 = [ln(q="s3", t=long_in), ln(q="s1", t="long_name_a")]
    s, M = check(gpu_ctx, tmp, [b"".join(x + b"\n" for x in p) for p in (p0, p1, p2)])
    assert [p["last_form"] for p in s.per] == [TEXT, SHORT, TEXT] and M.excl == {long_in.encode()}
    assert s.names == [b"long_name_a", b"long_name_bb", b"s1", b"s2", b"s3"] and s.x["n_early_lines"] == 3 and s.x["n_late_lines"] == 0
    s, M = check(gpu_ctx, tmp, [b"".join(x + b"\n" for x in p) for p in (p1, p2, p0)])  # the long name is excluded by the last piece
    assert s.names == [b"s1", b"s2", b"s3", b"long_name_a", b"long_name_bb"] and s.x["n_late_lines"] == 1 and s.x["n_early_lines"] == 2


# ------------------------------------------------------------------------------------------------ 12. random texts, cut at random line borders
def gen_spread(n, seed, n_names=40):
    """n lines over a pool of names of which a tenth are reads of 30 000 and the rest reads of 9 000; where a short read meets a long one, three lines in ten put
    it clearly inside; the other lines are ordinary overlaps with their own numbers"""
    rs = np.random.RandomState(seed)
    length = [30000 if i % 10 == 0 else 9000 for i in range(n_names)]
    out = []
    for i in range(n):
        q, t = (int(v) for v in rs.randint(0, n_names, 2))
        ql, tl = length[q], length[t]
        inside = ql != tl and rs.randint(0, 10) < 3
        if inside and ql < tl:
            qs, qe, ts, te = 10, 8990, 5000, 14000
        elif inside:
            qs, qe, ts, te = 5000, 14000, 10, 8990
        else:
            qs, ts = int(rs.randint(0, 3000)), int(rs.randint(0, 3000))
            span = int(rs.randint(500, 6000))
            qe, te = qs + span, ts + span
        out.append(ln(q="r%d" % q, ql=ql, qs=qs, qe=qe, st="+-"[i & 1], t="r%d" % t, tl=tl, ts=ts, te=te, ml=int(rs.randint(50, 900)), bl=1000 + i, ncol=10 if i % 7 == 3 else None) + b"\n")  # (the first line has 11 columns: what a 10-column first line holds is left open by paf.c:54)
    return out


SEEDS = list(range(100, 120))  # chosen on the CPU: each meets the condition below on the model alone


@pytest.mark.parametrize("seed", SEEDS)
def test_random_texts(gpu_ctx, tmp, seed):
    lines = gen_spread(300, seed)
    M0 = PM.model(b"".join(lines), SPAN, MATCH, 1, None, NC)
    assert len(M0.excl) >= 1 and len(M0.names) >= 1 and int(M0.passed.sum()) - int(M0.stored.sum()) >= 1, "the seed does not exercise the exclusion"
    rs = np.random.RandomState(seed + 1000)
    sizes = [int(v) for v in rs.randint(0, 40, 12)]
    s, M = check(gpu_ctx, tmp, cut(lines, sizes), bi_dir=seed & 1 ^ 1)
    assert s.info["n_excl"] >= 1 and s.info["n_seq"] >= 1


# ------------------------------------------------------------------------------------------------ 13. no_cont = 0
def test_begin_excl_without_no_cont_is_begin(gpu_ctx, tmp):
    L = ma.lib()
    pieces = cut(base_lines(), [3, 50, 0, 100])
    a = S.streamed(gpu_ctx, pieces, SPAN, MATCH, 1)
    ma._chk(L.mahip_paf_stream_begin_excl(gpu_ctx.h, SPAN, MATCH, 1, 0, 0, C.c_float(0)), "paf_stream_begin_excl")
    for k, p in enumerate(pieces):
        buf = C.create_string_buffer(bytes(p), len(p)) if len(p) else None
        ma._chk(L.mahip_paf_stream_piece_mem(gpu_ctx.h, buf, len(p), 1 if k + 1 == len(pieces) else 0), "paf_stream_piece_mem")
    info = ma.PafInfo()
    ma._chk(L.mahip_paf_stream_end(gpu_ctx.h, C.byref(info)), "paf_stream_end")
    b = S._results(gpu_ctx, info)
    rep, x = S._copy(gpu_ctx.paf_stream_last()), gpu_ctx.paf_stream_excl_last()
    ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")
    assert b.info == a.info and b.info["n_excl"] == 0 and b.names == a.names and b.lens == a.lens and b.hits.tobytes() == a.hits.tobytes()
    timeless = lambda r: {k: v for k, v in r.items() if not k.startswith("t_")}  # noqa: E731
    assert timeless(rep) == timeless(a.rep), "the same report: no growth, no buffer the plain stream does not have"
    assert (x.n_early_lines, x.n_late_records, x.n_late_lines, x.n_flagged, x.n_renumbered, x.n_flag_grow, x.n_lens_grow) == (0,) * 7
    assert b"inner1" in b.names and b.names.index(b"inner3") == 6


# ------------------------------------------------------------------------------------------------ the host layer: the command line
cli, n_pieces = S.cli, S.n_pieces
ON = {"MA_STREAM_NOCONT": "1", "MA_INGEST_PIECE": "1024"}
ARGS = [["-R"], ["-R", "-p", "paf", "-S2"], ["-R", "-p", "bed"]]


@pytest.fixture(scope="module")
def paf_files(tmp):
    paf = R.pafgen(os.path.join(tmp, "stream_R.paf"), 400, 3000, 64, ["-d", "0.1"])
    gz = paf + ".gz"
    with open(paf, "rb") as f, gzip.open(gz, "wb", compresslevel=1) as g:
        g.write(f.read())
    assert os.path.getsize(paf) >= 100 << 10
    return paf, gz


@pytest.mark.parametrize("args", ARGS, ids=["ug", "paf_S2", "bed"])
def test_cli_R_streams_under_the_switch(paf_files, args):
    paf, gz = paf_files
    out, log, _ = cli(args, gz, env=ON)
    assert n_pieces(log) > 100, log[-1500:]
    assert "dropped 0 contained reads" not in log and "dropped " in log, "this input is supposed to trigger the -R pre-filter"
    assert "[T::ingest_gpu] stream: -R dropped early" in log
    off, log0, _ = cli(args, gz, env={"MA_INGEST_PIECE": "1024"})
    plain, log1, _ = cli(args, paf)
    assert n_pieces(log0) == 0 and n_pieces(log1) == 0 and out == off == plain and len(out) > 0
    assert R.counters(log) == R.counters(log0) == R.counters(log1), "the [M::...] lines do not say which road was taken"
    if R.have_ref():
        ref_out, ref_log = R.run_cli(R.REF_BIN, args, paf)
        assert R.norm_lines(out) == R.norm_lines(ref_out) and R.counters(log) == R.counters(ref_log)


def test_cli_R_streams_a_plain_file_when_every_input_is_streamed(paf_files):
    paf, gz = paf_files
    out, log, _ = cli(["-R"], paf, env=dict(ON, MA_INGEST_STREAM="1"))
    want, log0, _ = cli(["-R"], paf)
    assert n_pieces(log) > 100 and n_pieces(log0) == 0 and out == want


def test_cli_R_without_the_switch_does_not_stream(paf_files):
    paf, gz = paf_files
    want, _, _ = cli(["-R"], paf, env={"MA_INGEST_STREAM": "0"})
    for env in ({"MA_INGEST_PIECE": "1024"}, {"MA_INGEST_PIECE": "1024", "MA_INGEST_STREAM": "1"}, {"MA_INGEST_PIECE": "1024", "MA_STREAM_NOCONT": "0"}):
        out, log, _ = cli(["-R"], gz, env=env)
        assert out == want and n_pieces(log) == 0


def test_cli_R_on_stdin_stays_with_the_host_reader(paf_files):
    paf, gz = paf_files
    for src in (paf, gz):
        out, log, rc = cli(["-R"], stdin=src, env=ON, ok=False)
        off, log0, rc0 = cli(["-R"], stdin=src, env={"MA_INGEST_PIECE": "1024"}, ok=False)
        assert (out, rc) == (off, rc0) and n_pieces(log) == 0 and n_pieces(log0) == 0


def test_cli_R_with_two_ranks_does_not_stream(paf_files):
    paf, gz = paf_files
    want, _, _ = cli(["-R"], paf)
    out, log, _ = cli(["-R"], gz, env=dict(ON, MA_GPUS="2", MA_COMM="shm"))
    assert n_pieces(log) == 0 and out == want


def test_cli_R_a_refused_piece_goes_to_the_host_reader(paf_files):
    paf, gz = paf_files
    want, log0, _ = cli(["-R"], paf)
    out, log, _ = cli(["-R"], gz, env=dict(ON, MA_PAF_MAX_BYTES="512"))
    assert out == want and "using the host reader" in log and n_pieces(log) == 0
    assert R.counters(log) == R.counters(log0)
