"""The streamed PAF ingest (csrc/paf.hip: mahip_paf_stream_*; host/ingest_gpu.c: ma_hit_ingest_stream): one text handed over in pieces of whole lines must leave
exactly what mahip_paf_parse leaves on the concatenated text -- records (bytewise, HIT_DT), names, first-seen lengths, every mahip_paf_info_t field.  All are
integers: equality everywhere.  The oracle of every case is threefold: the same text through mahip_paf_load_mem + mahip_paf_parse, through the host reader
(ma_hit_ingest) and, where oracle/_ref is built, through the reference library's ma_hit_read.  Texts are a few hundred lines and pieces 0 - 4 KiB; each case
asserts from mahip_paf_stream_last (and, per piece, from the report behind that piece) that it met the edge it names.

The command-line cases drive the host layer -- producer thread, cut at the last newline, carry, grown buffers -- with MA_INGEST_PIECE=1024 on a pafgen file of a
few thousand lines and compare with MA_INGEST_STREAM=0 (the whole text inflated first) and, where built, with the reference binary."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import miniasm_amd as ma
import refapi as R
import stages as ST
import test_gpu_ingest_edges as E

pytestmark = pytest.mark.gpu

ln, forced_env = E.ln, E.forced_env
INFO_FIELDS = [f for f, _ in ma.PafInfo._fields_]
SHORT, TEXT = 1, 2  # MAHIP_PAF_DICT_*


@pytest.fixture(scope="module")
def tmp(tmpdir_s):
    return tmpdir_s


class Res:
    pass


def _results(ctx, info):
    """names, lengths and the unsorted records the context holds after a parse, whole or streamed"""
    L = ma.lib()
    r = Res()
    r.info = {f: int(getattr(info, f)) for f in INFO_FIELDS}
    names = C.create_string_buffer(max(int(info.name_bytes), 1))
    lens = np.zeros(max(info.n_seq, 1), dtype=np.uint32)
    ma._chk(L.mahip_paf_names(ctx.h, names, lens.ctypes.data), "paf_names")
    r.lens = [int(x) for x in lens[:info.n_seq]]
    r.names = names.raw[:int(info.name_bytes)].split(b"\0")[:-1] if info.n_seq else []
    r.hits = np.zeros(int(info.n_hits), dtype=ma.HIT_DT)
    if info.n_hits:
        ma._chk(L.mahip_hits_raw_download(ctx.h, r.hits.ctypes.data), "hits_raw_download")
    return r


def whole(ctx, text, min_span, min_match, bi_dir, release=True):
    L = ma.lib()
    buf = C.create_string_buffer(text, max(len(text), 1))
    ma._chk(L.mahip_paf_load_mem(ctx.h, buf, len(text)), "paf_load_mem")
    info = ma.PafInfo()
    ma._chk(L.mahip_paf_parse_excl(ctx.h, min_span, min_match, bi_dir, 0, 0, C.c_float(0), C.byref(info)), "paf_parse_excl")
    r = _results(ctx, info)
    r.rep = ma.PafReport()
    ma._chk(L.mahip_paf_last(ctx.h, C.byref(r.rep)), "paf_last")
    if release:
        ma._chk(L.mahip_paf_release(ctx.h), "paf_release")
    return r


def _copy(rep):
    return {f: getattr(rep, f) for f, _ in ma.PafStreamReport._fields_}


def streamed(ctx, pieces, min_span, min_match, bi_dir, release=True):
    per = []
    info, rep = ctx.paf_stream(pieces, min_span, min_match, bi_dir, each=lambda k, r: per.append(_copy(r)))
    r = _results(ctx, info)
    r.rep, r.per = _copy(rep), per
    r.last = ma.PafReport()
    ma._chk(ma.lib().mahip_paf_last(ctx.h, C.byref(r.last)), "paf_last")
    if release:
        ma._chk(ma.lib().mahip_paf_release(ctx.h), "paf_release")
    return r


def check(ctx, tmp, pieces, min_span=0, min_match=0, bi_dir=1, **env):
    """the pieces through the stream (under the switches in env), their concatenation through the whole parse, the host reader and the reference library"""
    text = b"".join(pieces)
    with forced_env(**env):
        s = streamed(ctx, pieces, min_span, min_match, bi_dir)
    w = whole(ctx, text, min_span, min_match, bi_dir)
    assert s.info == w.info, (s.info, w.info)
    assert s.names == w.names and s.lens == w.lens
    assert s.hits.tobytes() == w.hits.tobytes(), "records differ from the whole parse"
    assert s.rep["n_pieces"] == len(pieces) and s.rep["n_empty"] == sum(1 for p in pieces if not p)
    path = os.path.join(tmp, "stream.paf")
    with open(path, "wb") as f:
        f.write(text)
    h_hits, h_names, h_lens, _ = E.host_reader(path, min_span, min_match, bi_dir, None)
    assert h_names == s.names and h_lens == s.lens and h_hits.tobytes() == s.hits.tobytes(), "stream and host reader disagree"
    if os.path.exists(R.REF_LIB):
        r_hits, r_names, r_lens, _ = E.host_reader(path, min_span, min_match, bi_dir, None, R.ref())
        r_hits["bldel"] &= 0x7FFFFFFF
        assert r_names == s.names and r_lens == s.lens, "stream and reference library disagree"
        assert R.canon(r_hits).tobytes() == R.canon(s.hits).tobytes(), "stream and reference library disagree"
    return s, w


def gen(n, seed, n_names=40, prefix="r", ncol=None):
    """n lines over a pool of read names (all 1..8 bytes unless the prefix is long), spans around the usual thresholds, every line with its own numbers"""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        q, t = rs.randint(0, n_names, 2)
        qs, ts = int(rs.randint(0, 3000)), int(rs.randint(0, 3000))
        span = int(rs.randint(500, 6000))
        out.append(ln(q="%s%d" % (prefix, q), ql=10000 + q, qs=qs, qe=qs + span, st="+-"[i & 1], t="%s%d" % (prefix, t), tl=10000 + t, ts=ts, te=ts + span,
                      ml=int(rs.randint(50, 900)), bl=span + i, ncol=ncol) + b"\n")
    return out


def cut(lines, sizes):
    """the lines grouped into pieces of the given numbers of lines (the rest in a last piece)"""
    out, at = [], 0
    for k in sizes:
        out.append(b"".join(lines[at:at + k]))
        at += k
    out.append(b"".join(lines[at:]))
    return out


# ------------------------------------------------------------------------------------------------ one piece / no piece / empty text
def test_one_piece_equals_the_whole_parse(gpu_ctx, tmp):
    s, w = check(gpu_ctx, tmp, [b"".join(gen(200, 1))], 2000, 100)
    assert s.info["n_hits"] > 100 and s.rep["n_pieces"] == 1 and s.rep["n_rebuilds"] == 0 and s.rep["n_rec_grow"] == 0
    assert s.last.n_lines == 200


def test_begin_and_end_alone_give_zeros(gpu_ctx, tmp):
    s, w = check(gpu_ctx, tmp, [])
    assert all(v == 0 for v in s.info.values()) and s.rep["n_pieces"] == 0 and s.last.n_lines == 0
    s, w = check(gpu_ctx, tmp, [b""])
    assert all(v == 0 for v in s.info.values()) and s.rep["n_pieces"] == 1 and s.rep["n_empty"] == 1


def test_empty_pieces_first_in_the_middle_and_last(gpu_ctx, tmp):
    a, b = b"".join(gen(60, 2)), b"".join(gen(70, 3))
    s, w = check(gpu_ctx, tmp, [b"", a, b"", b"", b, b""], 2000, 100)
    assert s.rep["n_empty"] == 4 and s.info["n_lines"] == 130 and s.info["n_hits"] > 0
    assert s.last.n_lines == 70, "mahip_paf_last describes the last piece that had text"


def test_a_piece_that_stores_nothing(gpu_ctx, tmp):
    """a piece whose lines are all filtered out, and a piece of lines with fewer than 10 columns only: no local dictionary, no fold, no records -- and the ids
    of the pieces behind them go on where the pieces in front stopped"""
    a, b = gen(50, 4), gen(50, 5, n_names=80)
    flt = [ln(q="zz%d" % i, qs=0, qe=100, ts=0, te=100) + b"\n" for i in range(30)]  # spans of 100 < 2000
    junk = [ln(q="yy%d" % i, ncol=9) + b"\n" for i in range(30)]
    s, w = check(gpu_ctx, tmp, [b"".join(a), b"".join(flt), b"".join(junk), b"".join(b)], 2000, 100)
    assert (s.per[1]["last_local"], s.per[1]["last_form"]) == (0, 0) and (s.per[2]["last_local"], s.per[2]["last_form"]) == (0, 0)
    assert s.per[3]["last_new"] > 0 and s.info["n_records"] == 130 and s.info["n_lines"] == 160
    assert not any(n.startswith(b"zz") or n.startswith(b"yy") for n in s.names)


# ------------------------------------------------------------------------------------------------ the piece border contract
def test_a_piece_that_is_not_the_last_must_end_with_a_newline(gpu_ctx, tmp):
    L = ma.lib()
    a = b"".join(gen(10, 6))
    with pytest.raises(ma.GpuError, match="newline"):
        gpu_ctx.paf_stream([a[:-1], a], 0, 0, 1)
    rep = ma.PafStreamReport()
    assert L.mahip_paf_stream_last(gpu_ctx.h, C.byref(rep)) != 0, "the harness aborted the stream"
    ma._chk(L.mahip_paf_stream_begin(gpu_ctx.h, 0, 0, 1), "begin")
    buf = C.create_string_buffer(a, len(a))
    ma._chk(L.mahip_paf_stream_piece_mem(gpu_ctx.h, buf, len(a), 1), "piece")
    assert L.mahip_paf_stream_piece_mem(gpu_ctx.h, buf, len(a), 0) != 0 and b"behind the last piece" in L.mahip_strerror()
    ma._chk(L.mahip_paf_stream_abort(gpu_ctx.h), "abort")
    assert L.mahip_paf_stream_piece_mem(gpu_ctx.h, buf, len(a), 0) != 0 and b"mahip_paf_stream_begin" in L.mahip_strerror()
    info = ma.PafInfo()
    assert L.mahip_paf_stream_end(gpu_ctx.h, C.byref(info)) != 0
    check(gpu_ctx, tmp, [a, a])  # the context is as good as new


def test_the_last_piece_may_end_without_a_newline(gpu_ctx, tmp):
    lines = gen(40, 7)
    s, w = check(gpu_ctx, tmp, [b"".join(lines[:25]), b"".join(lines[25:])[:-1]], 2000, 100)
    assert w.rep.open_line == 1 and s.last.open_line == 1 and s.info["n_lines"] == 40
    s, w = check(gpu_ctx, tmp, [b"".join(lines[:39]), lines[39][:-1]])  # the open line is a piece of its own
    assert s.last.open_line == 1 and s.last.n_lines == 1 and s.info["n_lines"] == 40


# ------------------------------------------------------------------------------------------------ ids across pieces
def test_ids_and_first_seen_lengths_across_pieces(gpu_ctx, tmp):
    p0 = ln(q="a", ql=1000, t="b", tl=2000) + b"\n"
    p1 = ln(q="c", ql=3000, t="d", tl=4000) + b"\n"                                                # no `a`
    p2 = ln(q="a", ql=7777, t="e", tl=5000) + b"\n" + ln(q="b", ql=8888, t="c", tl=9999) + b"\n"  # `a` states another length; `b` was a target, is a query now
    p3 = ln(q="b", ql=1, t="a", tl=2) + b"\n" + ln(q="e", ql=3, t="d", tl=4) + b"\n"              # brings no new name
    p4 = ln(q="f", ql=6000, t="g", tl=7000) + b"\n" + ln(q="h", ql=8000, t="g", tl=1) + b"\n"     # brings only new names
    p5 = ln(q="a", ql=5, t="n1", tl=11) + b"\n" + ln(q="n2", ql=12, t="n3", tl=13) + b"\n" + ln(q="n3", ql=99, t="n1", tl=98) + b"\n"  # target new, query old
    s, w = check(gpu_ctx, tmp, [p0, p1, p2, p3, p4, p5])
    assert s.names == [b"a", b"b", b"c", b"d", b"e", b"f", b"g", b"h", b"n1", b"n2", b"n3"], "new ids follow 2 x line + column inside a piece"
    assert s.lens == [1000, 2000, 3000, 4000, 5000, 6000, 7000, 8000, 11, 12, 13], "the first length seen wins, whatever a later piece states"
    assert [(p["last_local"], p["last_new"]) for p in s.per] == [(2, 2), (2, 2), (4, 1), (4, 0), (3, 3), (4, 3)]
    assert [int(h["qns"] >> 32) for h in s.hits[::2]] == [0, 2, 0, 1, 1, 4, 5, 7, 0, 9, 10]


# ------------------------------------------------------------------------------------------------ name forms
def test_short_and_long_name_pieces_meet_in_one_table(gpu_ctx, tmp):
    """pieces 0 and 1 hold names of 1 - 8 bytes only (their local table is keyed by the bytes themselves), piece 2 brings a 9-byte name whose first 8 bytes are an
    earlier 8-byte name and a 7-byte name that is a prefix of it (its local table compares text), piece 3 is short again: one persistent table, decided by the
    bytes"""
    p0 = ln(q="ABCDEFGH", ql=100, t="x", tl=200) + b"\n" + ln(q="x", t="ABCDEFGH") + b"\n"
    p1 = ln(q="ABCD", ql=300, t="ABCDEFGH", tl=1) + b"\n"
    p2 = ln(q="ABCDEFGHI", ql=400, t="ABCDEFG", tl=500) + b"\n" + ln(q="ABCDEFGH", ql=2, t="ABCDEFGHIJKLMNOPQRSTUVWXYZ", tl=600) + b"\n" + ln(q="ABCD", ql=3, t="x", tl=4) + b"\n"
    p3 = ln(q="ABCDEFG", ql=5, t="ABCD", tl=6) + b"\n" + ln(q="y", ql=700, t="ABCDEFGH", tl=7) + b"\n"
    s, w = check(gpu_ctx, tmp, [p0, p1, p2, p3])
    assert [p["last_form"] for p in s.per] == [SHORT, SHORT, TEXT, SHORT] and (s.rep["n_short"], s.rep["n_text"]) == (3, 1)
    assert s.names == [b"ABCDEFGH", b"x", b"ABCD", b"ABCDEFGHI", b"ABCDEFG", b"ABCDEFGHIJKLMNOPQRSTUVWXYZ", b"y"]
    assert s.lens == [100, 200, 300, 400, 500, 600, 700]
    assert [(p["last_local"], p["last_new"]) for p in s.per] == [(2, 2), (2, 1), (6, 3), (4, 1)]


# ------------------------------------------------------------------------------------------------ growth
def test_the_name_table_is_rebuilt_larger(gpu_ctx, tmp):
    lines = []
    for k in range(16):  # 40 new names a piece and some old ones
        lines.append(b"".join(ln(q="n%d_%d" % (k, i), ql=100 + i, t="n%d_%d" % (max(k - 1, 0), (7 * i) % 40), tl=100 + (7 * i) % 40) + b"\n" for i in range(40)))
    s, w = check(gpu_ctx, tmp, lines, MA_STREAM_DICT_CAP_LOG2=4)
    assert s.info["n_seq"] == 640 and s.rep["n_rebuilds"] >= 2 and s.rep["tab_cap"] >= 2 * 640, s.rep
    t, _ = check(gpu_ctx, tmp, lines)
    assert t.rep["n_rebuilds"] == 0 and t.rep["tab_cap"] == 1 << 16 and t.names == s.names, "the same ids without the switch"


@pytest.mark.parametrize("bi_dir", [1, 0])
def test_the_record_buffer_grows_and_keeps_the_records(gpu_ctx, tmp, bi_dir):
    pieces = cut(gen(240, 8), [3, 5, 9, 17, 33, 65])
    s, w = check(gpu_ctx, tmp, pieces, 2000, 100, bi_dir, MA_STREAM_REC_CAP=8)
    assert s.rep["n_rec_grow"] >= 2 and s.info["n_hits"] > 64
    assert s.info["n_hits"] > s.info["n_stored_lines"] if bi_dir else s.info["n_hits"] == s.info["n_stored_lines"]


# ------------------------------------------------------------------------------------------------ the stale bl
def test_a_ten_column_line_inherits_across_pieces(gpu_ctx, tmp):
    """paf.c:54 leaves bl alone on a 10-column line: it keeps the value of the last line with an 11th column, however many pieces ago that was"""
    p0 = ln(q="a", t="b", bl=1111) + b"\n" + ln(q="a", t="c", bl=4242) + b"\n" + ln(q="short", ncol=9) + b"\n"
    p1 = b"".join(ln(q="a", t="d%d" % i, ncol=10) + b"\n" for i in range(5))                        # only 10-column lines
    p2 = ln(q="e", t="a", ncol=10) + b"\n" + ln(q="e", t="b", bl=77) + b"\n" + ln(q="e", t="c", ncol=10) + b"\n"
    p3 = ln(q="f", t="a", bl=5) + b"\n" + ln(q="f", t="b", ncol=10) + b"\n"                         # its first line has a bl of its own
    s, w = check(gpu_ctx, tmp, [p0, p1, p2, p3], bi_dir=0)
    assert [int(h["bldel"]) for h in s.hits] == [1111, 4242] + [4242] * 5 + [4242, 77, 77] + [5, 5]
    assert [p["last_before"] for p in s.per] == [0, 4242, 4242, 77] and s.rep["n_inherited"] == 2, s.rep
    assert [p["n_inherited"] for p in s.per] == [0, 1, 2, 2]


def test_a_ten_column_very_first_line(gpu_ctx, tmp):
    p0 = ln(q="a", t="b", ncol=10) + b"\n" + ln(q="a", t="c", bl=9) + b"\n"
    p1 = ln(q="a", t="d", ncol=10) + b"\n"
    s, w = check(gpu_ctx, tmp, [p0, p1], bi_dir=0)
    assert [int(h["bldel"]) for h in s.hits] == [0, 9, 9] and s.per[0]["last_before"] == 0 and [p["n_inherited"] for p in s.per] == [0, 1]
    s, w = check(gpu_ctx, tmp, [p1, p1, p0], bi_dir=0)  # nothing to inherit for two pieces
    assert [int(h["bldel"]) for h in s.hits] == [0, 0, 0, 9] and s.rep["n_inherited"] == 0


# ------------------------------------------------------------------------------------------------ one line per piece, and what follows the ingest
def test_one_line_per_piece_then_sort_and_pipeline(gpu_ctx, tmp):
    paf = R.pafgen(os.path.join(tmp, "stream300.paf"), 60, 340, 23, ["-L", "uniform", "-d", "0.3"])
    with open(paf, "rb") as f:
        lines = f.read().splitlines(keepends=True)[:300]
    assert len(lines) == 300
    with open(paf, "wb") as f:
        f.write(b"".join(lines))
    opt = ma.default_opt()
    s, w = check(gpu_ctx, tmp, lines, opt.min_span, opt.min_match)
    assert s.rep["n_pieces"] == 300 and s.info["n_hits"] > 100
    L = ma.lib()
    out = {}
    for how in ("whole", "stream"):
        r = whole(gpu_ctx, b"".join(lines), opt.min_span, opt.min_match, 1, release=False) if how == "whole" else streamed(gpu_ctx, lines, opt.min_span, opt.min_match, 1, release=False)
        gpu_ctx.sort()
        out[how] = (gpu_ctx.hits_download().tobytes(), ST.sort_last(gpu_ctx)["path"], gpu_ctx.sorted_runs())
        ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")
    assert out["stream"] == out["whole"] and out["whole"][2] > 0, "the sort takes runs of records after either parse"
    ing = ma.Ingest(paf, opt)  # (the dictionary for the pipeline's output: the same names and ids, checked above)
    gfa = {}
    for how in ("whole", "stream"):
        if how == "whole":
            whole(gpu_ctx, b"".join(lines), opt.min_span, opt.min_match, 1, release=False)
        else:
            streamed(gpu_ctx, lines, opt.min_span, opt.min_match, 1, release=False)
        gfa[how] = ma.run_resident(gpu_ctx, opt, ing, "ug")
        ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")
    ing.close()
    assert gfa["stream"] == gfa["whole"] and gfa["whole"].startswith(b"S\t")


# ------------------------------------------------------------------------------------------------ the host layer: the command line
def cli(args, paf=None, stdin=None, env=None, binary=None, ok=True):
    e = dict(os.environ)
    e.update({"MA_PIPE_TIMING": "1"})
    e.update(env or {})
    r = subprocess.run([binary or ma.CLI_PATH] + list(args) + [paf or "-"], stdin=open(stdin, "rb") if stdin else subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=e, timeout=600)
    if ok:
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr.decode(), r.returncode


def n_pieces(log):
    m = re.search(r"\[T::ingest_gpu\] stream: pieces=(\d+) piece=(\d+) B producer", log)
    return int(m.group(1)) if m else 0


@pytest.fixture(scope="module")
def paf_files(tmp):
    paf = R.pafgen(os.path.join(tmp, "stream_cli.paf"), 300, 2500, 31, ["-L", "uniform", "-d", "0.3", "-x", "0.03"])
    gz = paf + ".gz"
    with open(paf, "rb") as f, gzip.open(gz, "wb", compresslevel=1) as g:
        g.write(f.read())
    base, _, _ = cli([], paf, env={"MA_INGEST_STREAM": "0"})
    assert base.startswith(b"S\t")
    ref = R.run_cli(R.REF_BIN, [], paf)[0] if R.have_ref() else None
    return paf, gz, base, ref


PIECE = {"MA_INGEST_PIECE": "1024"}


@pytest.mark.parametrize("how", ["text_on_stdin", "gzip_on_stdin", "gz_file", "plain_file_forced"])
def test_cli_streams(paf_files, how):
    paf, gz, base, ref = paf_files
    env = dict(PIECE)
    if how == "plain_file_forced":
        env["MA_INGEST_STREAM"] = "1"
    src = dict(text_on_stdin=dict(stdin=paf), gzip_on_stdin=dict(stdin=gz), gz_file=dict(paf=gz), plain_file_forced=dict(paf=paf))[how]
    out, log, _ = cli([], env=env, **src)
    assert n_pieces(log) > 100, log[-1500:]
    off, log0, _ = cli([], env=dict(env, MA_INGEST_STREAM="0"), **src)
    assert n_pieces(log0) == 0 and out == off == base
    if ref is not None:
        assert R.norm_lines(out) == R.norm_lines(ref)
    assert R.counters(log) == R.counters(log0), "the [M::...] lines do not say which road was taken"


def test_cli_stream_unset_leaves_a_plain_file_whole(paf_files):
    paf, gz, base, ref = paf_files
    out, log, _ = cli([], paf, env=PIECE)
    assert out == base and n_pieces(log) == 0


def _rewrite(paf_files, tmp, name, change):
    with open(paf_files[0], "rb") as f:
        text = change(f.read())
    path = os.path.join(tmp, name)
    with open(path, "wb") as f:
        f.write(text)
    return path, text


def test_cli_a_line_longer_than_four_pieces(paf_files, tmp):
    def long_tag(text):
        lines = text.splitlines(keepends=True)
        k = len(lines) // 2
        lines[k] = lines[k][:-1] + b"\tzz:Z:" + b"Q" * 5000 + b"\n"
        return b"".join(lines)
    path, text = _rewrite(paf_files, tmp, "stream_long.paf", long_tag)
    out, log, _ = cli([], stdin=path, env=PIECE)
    assert out == paf_files[2] and n_pieces(log) > 100


def test_cli_text_ending_on_a_piece_border(paf_files, tmp):
    def on_border(text):  # the last line padded so that the text is a whole number of pieces
        need = -len(text) % 1024
        need += 1024 if 0 < need < 8 else 0
        return text if not need else text[:-1] + b"\tzz:Z:" + b"Q" * (need - 6) + b"\n"
    path, text = _rewrite(paf_files, tmp, "stream_border.paf", on_border)
    assert len(text) % 1024 == 0 and text.endswith(b"\n")
    out, log, _ = cli([], stdin=path, env=PIECE)
    assert out == paf_files[2] and n_pieces(log) > 100


def test_cli_an_unterminated_last_line(paf_files, tmp):
    path, text = _rewrite(paf_files, tmp, "stream_open.paf", lambda t: t[:-1])
    assert not text.endswith(b"\n")
    out, log, _ = cli([], stdin=path, env=PIECE)
    assert out == paf_files[2] and n_pieces(log) > 100


def test_cli_R_does_not_stream(paf_files):
    paf, gz, base, ref = paf_files
    want, _, _ = cli(["-R"], paf, env={"MA_INGEST_STREAM": "0"})
    for env in (PIECE, dict(PIECE, MA_INGEST_STREAM="1")):
        out, log, _ = cli(["-R"], gz, env=env)
        assert out == want and n_pieces(log) == 0


def test_cli_a_refused_piece(paf_files):
    """MA_PAF_MAX_BYTES below the piece size: the device refuses the first piece.  A file is read again by the host reader (a warning, the same output); what came
    from stdin is gone: an error of the run, not an empty result"""
    paf, gz, base, ref = paf_files
    env = dict(PIECE, MA_PAF_MAX_BYTES="512")
    out, log, _ = cli([], gz, env=env)
    assert out == base and "using the host reader" in log and n_pieces(log) == 0
    out, log, rc = cli([], stdin=gz, env=env, ok=False)
    assert rc != 0 and "[E::" in log and out == b""
