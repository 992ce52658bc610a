"""The device PAF reader (csrc/paf.hip) stage by stage, at the sizes its kernels branch on.  tests/test_gpu_ingest.py compares the END of the reader (records,
names, lengths) with the host reader on random text; it cannot say which kernel produced a line.  Here every text is small and built to sit ON an edge, the
parse is driven through mahip_paf_load_mem + mahip_paf_parse_excl, and what the kernels decided is read back through mahip_paf_last (tile size and form, lines
left to the byte-wise kernel, dictionary form, table attempts, stale-bl pass) and mahip_paf_cols_download (per-line flags with PF_QCONT, the snapshot of the
lines that waited for k_paf_parse_odd, the number columns, name offsets and lengths, line starts, first line start of every tile).  All of it is compared with
tests/pafmodel.py, a plain Python model of the reader that also states what the kernels SHOULD decide; the model is checked in turn: every text also goes
through the host reader (ma.Ingest / ma_hit_no_cont) and, where oracle/_ref is built, through the reference library's ma_hit_read.  All integers: equality
everywhere.  Every case asserts, from the report or the downloaded arrays, that the edge it names was met.

Out of scope: the sharded merge kernels (k_dict_merge and its kin need ranks: tests/test_gpu_ingest_shard_edges.py), texts over 4 GiB, more than 2^31 lines."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import miniasm_amd as ma
import pafmodel as PM
import refapi as R

pytestmark = pytest.mark.gpu

KIB = 1024
GROUP_BYTES = PM.GROUP * PM.GRAN


@contextlib.contextmanager
def forced_env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is not None:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Dev:
    pass


def device_parse(ctx, text, min_span, min_match, bi_dir, no_cont=None):
    """mahip_paf_load_mem + mahip_paf_parse_excl; report, columns, names, records; release"""
    L = ma.lib()
    d = Dev()
    ma._chk(L.mahip_paf_keep_odd(ctx.h, 1), "paf_keep_odd")
    buf = C.create_string_buffer(text, max(len(text), 1))
    ma._chk(L.mahip_paf_load_mem(ctx.h, buf, len(text)), "paf_load_mem")
    info = ma.PafInfo()
    mh, fr = (no_cont if no_cont is not None else (0, 0.0))
    ma._chk(L.mahip_paf_parse_excl(ctx.h, min_span, min_match, bi_dir, 1 if no_cont is not None else 0, mh, C.c_float(fr), C.byref(info)), "paf_parse_excl")
    d.info = info
    rep = ma.PafReport()
    ma._chk(L.mahip_paf_last(ctx.h, C.byref(rep)), "paf_last")
    d.rep = rep
    n, nt = int(rep.n_lines), int(rep.n_tiles)
    d.flags, d.odd = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    d.nums = np.zeros((8, max(n, 1)), dtype=np.uint32)
    d.tnoff, d.qlen, d.tlen = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
    d.lstart, d.tfirst = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(nt, 1), dtype=np.uint64)
    ma._chk(L.mahip_paf_cols_download(ctx.h, d.flags.ctypes.data, d.odd.ctypes.data, d.nums.ctypes.data, d.tnoff.ctypes.data, d.qlen.ctypes.data, d.tlen.ctypes.data,
                                      d.lstart.ctypes.data, d.tfirst.ctypes.data), "paf_cols_download")
    d.flags, d.odd, d.nums, d.tnoff, d.qlen, d.tlen, d.tfirst = d.flags[:n], d.odd[:n], d.nums[:, :n], d.tnoff[:n], d.qlen[:n], d.tlen[:n], d.tfirst[:nt]
    names = C.create_string_buffer(max(int(info.name_bytes), 1))
    d.lens = np.zeros(max(info.n_seq, 1), dtype=np.uint32)
    ma._chk(L.mahip_paf_names(ctx.h, names, d.lens.ctypes.data), "paf_names")
    d.lens = d.lens[:info.n_seq]
    d.names = names.raw[:int(info.name_bytes)].split(b"\0")[:-1] if info.n_seq else []
    d.hits = np.zeros(int(info.n_hits), dtype=ma.HIT_DT)
    if info.n_hits:
        ma._chk(L.mahip_hits_raw_download(ctx.h, d.hits.ctypes.data), "hits_raw_download")
    return d


def host_reader(path, min_span, min_match, bi_dir, no_cont, lib=None):
    """the host reader (or, lib = the reference library, its ma_hit_read) -> (records, names, lengths, n_excl)"""
    L = lib or ma.lib()
    verbose = C.c_int.in_dll(L, "ma_verbose")
    was, verbose.value = verbose.value, 1  # (no "[M::ma_hit_read] read ..." line per case)
    L.ma_hit_no_cont.restype = C.POINTER(ma.Sdict)
    L.ma_hit_no_cont.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_float]
    excl, n_excl = None, 0
    if no_cont is not None:
        excl = L.ma_hit_no_cont(path.encode(), min_span, min_match, no_cont[0], C.c_float(no_cont[1]))
        n_excl = excl.contents.n_seq
    d = L.sd_init()
    n = C.c_size_t(0)
    if lib is None:
        L.ma_hit_ingest.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(ma.Sdict), C.POINTER(C.c_size_t), C.c_int, C.POINTER(ma.Sdict)]
        p = L.ma_hit_ingest(path.encode(), min_span, min_match, d, C.byref(n), bi_dir, excl)
    else:
        L.ma_hit_read.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(ma.Sdict), C.POINTER(C.c_size_t), C.c_int, C.POINTER(ma.Sdict)]
        p = L.ma_hit_read(path.encode(), min_span, min_match, d, C.byref(n), bi_dir, excl)
    hits = R.np_from(p, n.value, ma.HIT_DT)
    if p:
        L.free_buf(p)
    names = [d.contents.seq[i].name for i in range(d.contents.n_seq)]
    lens = [d.contents.seq[i].len for i in range(d.contents.n_seq)]
    L.sd_destroy(d)
    if excl:
        L.sd_destroy(excl)
    verbose.value = was
    return hits, names, lens, n_excl


N_CASES = [0]


def check(ctx, tmp, text, min_span=0, min_match=0, bi_dir=1, K=None, cap_log2=None, no_cont=None, exact_text=None):
    """one text through the device, the model, the host reader and the reference library; -> (device results, model)"""
    N_CASES[0] += 1
    with forced_env(MA_PAF_TILE_K=K, MA_DICT_CAP_LOG2=cap_log2, MA_DICT_EXACT_TEXT=exact_text):
        d = device_parse(ctx, text, min_span, min_match, bi_dir, no_cont)
    ma._chk(ma.lib().mahip_paf_release(ctx.h), "paf_release")
    M = PM.model(text, min_span, min_match, bi_dir, K, no_cont)
    rep, info = d.rep, d.info
    # ---- the line census and the tiles
    assert (rep.n_lines, rep.n_gran, rep.open_line) == (M.L, M.n_gran, M.open_line)
    assert (d.lstart == M.lstart).all()
    if M.L:
        assert (rep.tile_k, rep.n_tiles, rep.tile_form) == (M.K, M.n_tiles, M.form)
        assert (d.tfirst == M.tfirst).all(), np.flatnonzero(d.tfirst != M.tfirst)[:8]
    # ---- which parser took a line, and what it made of it
    sure = np.array([o is not None for o in M.odd], dtype=bool)
    want_odd = np.array([bool(o) for o in M.odd], dtype=bool)
    bad = np.flatnonzero(sure & (d.odd.astype(bool) != want_odd))
    assert len(bad) == 0, "line %d: byte-wise kernel %d, model %s: %r" % (bad[0], d.odd[bad[0]], M.odd[bad[0]], text[int(M.lstart[bad[0]]):int(M.lstart[bad[0]]) + 120])
    assert rep.n_odd == int(d.odd.sum()) and rep.odd_ran == int(rep.n_odd > 0)
    v = M.valid
    assert ((d.flags & 1) == v).all() and ((d.flags >> 1 & 1) == M.stored).all() and ((d.flags >> 2 & 1) == M.hasbl).all() and ((d.flags >> 3 & 1) == M.rev).all()
    assert ((d.flags & 0xE0) == 0).all()
    for k, nm in enumerate(("ql", "qs", "qe", "tl", "ts", "te", "ml", "bl")):
        w = np.flatnonzero(v & (d.nums[k] != M.nums[k]))
        assert len(w) == 0, "%s of line %d: %d, model %d" % (nm, w[0], d.nums[k][w[0]], M.nums[k][w[0]])
    assert (d.tnoff[v] == M.tnoff[v]).all() and (d.qlen[v] == M.qlen[v]).all() and (d.tlen[v] == M.tlen[v]).all()
    qc = (d.flags & 0x10) != 0
    same_as_prev = np.zeros(M.L, dtype=bool)
    for i in range(1, M.L):
        same_as_prev[i] = bool(M.passed[i] and M.passed[i - 1] and M.qname[i] == M.qname[i - 1])
    assert not (qc & ~same_as_prev).any(), "PF_QCONT on a line whose query is not that of the stored line in front"
    if M.L:
        assert (qc == M.qcont).all(), np.flatnonzero(qc != M.qcont)[:8]
    # ---- counters, dictionary, records
    assert (info.n_lines, info.n_records, info.n_stored_lines) == (M.L, int(v.sum()), int(M.stored.sum()))
    assert rep.n_long == M.n_long and rep.bl_pass == int(M.n_nobl > 0)
    want_form = None if not M.passed.any() else "text" if (M.n_long or exact_text) else "short"
    assert ma.PAF_DICT_FORMS[rep.dict_form] == want_form
    if M.passed.any():
        assert rep.n_distinct == M.names_before_excl
        assert ma.PAF_TAB_ENDS[rep.end[rep.n_attempts - 1]] == "ok" and all(rep.end[a] != 0 for a in range(rep.n_attempts - 1))
    assert (info.n_excl, rep.n_excl) == (len(M.excl), len(M.excl))
    assert d.names == M.names and list(d.lens) == M.lens and info.n_seq == len(M.names)
    assert info.n_hits == len(M.hits) and d.hits.tobytes() == M.hits.tobytes(), "records differ from the model"
    if M.passed.any():
        assert info.max_qs == M.max_qs
    # ---- the model is not trusted alone
    path = os.path.join(tmp, "edge.paf")
    with open(path, "wb") as f:
        f.write(text)
    h_hits, h_names, h_lens, h_excl = host_reader(path, min_span, min_match, bi_dir, no_cont)
    assert h_names == M.names and h_lens == M.lens and h_hits.tobytes() == M.hits.tobytes() and h_excl == len(M.excl), "model and host reader disagree"
    if os.path.exists(R.REF_LIB):
        r_hits, r_names, r_lens, r_excl = host_reader(path, min_span, min_match, bi_dir, no_cont, R.ref())
        r_hits["bldel"] &= 0x7FFFFFFF
        assert r_names == M.names and r_lens == M.lens and r_excl == len(M.excl), "model and reference library disagree"
        assert R.canon(r_hits).tobytes() == R.canon(M.hits).tobytes(), "model and reference library disagree"
    return d, M


@pytest.fixture(scope="module")
def tmp(tmpdir_s):
    return tmpdir_s


def ln(q="q1", ql=9000, qs=10, qe=5000, st="+", t="t1", tl=8000, ts=20, te=5010, ml=800, bl=4990, more=("255",), ncol=None):
    """one PAF line (no newline); every argument may be bytes / str / int; ncol cuts the columns"""
    f = [q, ql, qs, qe, st, t, tl, ts, te, ml, bl] + list(more)
    f = [x if isinstance(x, bytes) else str(x).encode("latin-1") for x in f]
    return b"\t".join(f[:ncol] if ncol else f)


def filler(nbytes, width=40):
    """exactly nbytes of junk lines (fewer than 10 columns), the last byte a newline"""
    out = []
    while nbytes > 0:
        k = min(width, nbytes)
        if nbytes - k == 0 or nbytes - k >= 1:
            out.append(b"j" * (k - 1) + b"\n")
            nbytes -= k
    return b"".join(out)


def padded(line, total):
    """the line made exactly `total` bytes long (without its newline) by a tag column at its end"""
    need = total - len(line)
    assert need >= 2 or need == 0, need
    return line if need == 0 else line + b"\t" + b"Z" * (need - 1)


def test_accessors_need_a_parsed_text(gpu_ctx, tmp):
    L = ma.lib()
    rep = ma.PafReport()
    ma._chk(L.mahip_paf_release(gpu_ctx.h), "release")
    assert L.mahip_paf_last(gpu_ctx.h, C.byref(rep)) != 0 and b"mahip_paf_last" in L.mahip_strerror()
    buf = C.create_string_buffer(b"x\n")
    ma._chk(L.mahip_paf_load_mem(gpu_ctx.h, buf, 2), "load")
    assert L.mahip_paf_last(gpu_ctx.h, C.byref(rep)) != 0, "loaded, not parsed"
    d, M = check(gpu_ctx, tmp, ln() + b"\n")  # (check() releases)
    assert d.rep.n_lines == 1 and d.rep.dict_form == 1 and d.rep.n_attempts == 1
    assert L.mahip_paf_last(gpu_ctx.h, C.byref(rep)) != 0 and L.mahip_paf_cols_download(gpu_ctx.h, *([None] * 8)) != 0, "released"
    ma._chk(L.mahip_paf_keep_odd(gpu_ctx.h, 0), "keep_odd")
    ma._chk(L.mahip_paf_load_mem(gpu_ctx.h, buf, 2), "load")
    info = ma.PafInfo()
    ma._chk(L.mahip_paf_parse_excl(gpu_ctx.h, 0, 0, 1, 0, 0, C.c_float(0), C.byref(info)), "parse")
    odd = np.zeros(4, dtype=np.uint8)
    assert L.mahip_paf_cols_download(gpu_ctx.h, None, odd.ctypes.data, *([None] * 6)) != 0, "no snapshot was asked for"
    assert L.mahip_paf_cols_download(gpu_ctx.h, *([None] * 8)) == 0
    ma._chk(L.mahip_paf_release(gpu_ctx.h), "release")


# ------------------------------------------------------------------------------------------------ column windows
NUM_LENS, NAME_LENS = (1, 7, 8, 9, 31, 32, 33, 40), (1, 8, 9, 62, 63, 64, 65, 200)


def _col_value(col, n):
    """a column of n bytes made of digits only -- a name too, and the strand: if a window rule cuts a column in the wrong place, the pieces still look like
    numbers to the straight-line code and nothing sends the line to the byte-wise kernel by accident"""
    if col in (0, 5):
        return (b"7" if col == 0 else b"8") * n
    return (b"0" * (n - 3) + b"123")[-n:] if n > 3 else b"123"[:n]


@pytest.mark.parametrize("col,ncol", [(c, 12) for c in range(11)] + [(c, 9) for c in range(9)])
def test_column_windows(col, ncol, gpu_ctx, tmp):
    """a column of every length around its window, the line start moved through all 32 positions of a word of TAB bits (a junk line of 0..31 bytes in front);
    12 columns, and cut to 9 (a wrong cut would make it 10)"""
    parts, at = [], {}
    for n in (NAME_LENS if col in (0, 5) else NUM_LENS):
        for off in range(32):
            cur = sum(len(p) for p in parts)
            pad = (off - cur - 1) % 32  # junk bytes + their newline
            parts.append(b"j" * pad + b"\n")
            f = [b"5", b"9000", b"10", b"5000", b"1", b"6", b"8000", b"20", b"5010", b"800", b"4990", b"255"]
            f[col] = _col_value(col, n)
            at[(n, off)] = len(parts)
            parts.append(b"\t".join(f[:ncol]) + b"\n")
    text = b"".join(parts)
    d, M = check(gpu_ctx, tmp, text, K=1)
    idx = np.cumsum([p.count(b"\n") for p in parts]) - 1
    for (n, off), p in at.items():
        i = idx[p]
        assert int(M.lstart[i]) % 32 == off
        if ncol == 12:
            limit = 63 if col in (0, 5) else 32 if col == 4 else 8
            assert M.odd[i] == (n > limit or bool(M.long_first[i])), (n, off)
    assert d.odd.any() and not d.odd.all()


def test_column_counts_and_empty_columns(gpu_ctx, tmp):
    """9 / 10 / 11 / 12 / 15 columns, the last column cut by the line end, an empty column in every position"""
    lines = [ln(ncol=k) for k in (1, 2, 9, 10, 11, 12)] + [ln(more=("255", "a", "b", "c"))]
    lines += [ln(bl=b""), ln(bl=b"", ncol=11), ln(ml=b"", ncol=10), ln(ncol=10) + b"\t", ln(ncol=9) + b"\t"]
    for k in range(12):
        f = ln().split(b"\t")
        f[k] = b""
        lines.append(b"\t".join(f))
    lines += [b"", b"\t", b"\t" * 9, b"\t" * 10, b"\t" * 11, b"\t" * 40]
    d, M = check(gpu_ctx, tmp, b"\n".join(lines), K=1)
    assert d.odd.sum() >= 9 and M.n_nobl >= 3 and d.rep.open_line == 1


# ------------------------------------------------------------------------------------------------ numbers
def test_number_columns(gpu_ctx, tmp):
    """strtol on every number column: values around 8 / 9 digits, 2^31, 2^32, LONG_MAX, LONG_MIN; zeros in front; sign, blanks; junk, NUL, high-bit bytes"""
    vals = [0, 9, 99999999, 100000000, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, PM.LONG_MAX, PM.LONG_MAX + 1, 12345678901234567890123]
    toks = [str(x).encode() for x in vals] + [b"-" + str(x).encode() for x in vals] + [str(PM.LONG_MIN).encode(), str(PM.LONG_MIN - 1).encode()]
    toks += [b"0" * k + b"7" for k in range(0, 10)] + [b"0" * 8, b"0" * 9, b"00000000", b"99999999", b"999999999"]
    toks += [b"+5", b"-5", b" 5", b"\x0b5", b"\x0c5", b"\r5", b" \x0b -5", b"+-5", b"- 5", b"++5", b"+", b"-", b" ", b""]
    toks += [b"12x", b"12 ", b"1\x002", b"\x0012", b"12\x00", b"1\xb12", b"\xb912", b"12\xff", b"x12", b"1:2", b"1/2", b"12345678x", b"1234567x", b"/", b":"]
    lines = []
    for col in PM.NUM_COLS:
        for t in toks:
            f = ln().split(b"\t")
            f[col] = t
            lines.append(b"\t".join(f))
    for st in (b"", b"-", b"-x", b"+", b"x-", b"--", b"+-"):
        lines.append(ln(st=st))
    lines += [ln(ml=2 ** 31), ln(ml=2 ** 31 + 100), ln(ml=2 ** 32 - 1), ln(bl=2 ** 31), ln(bl=2 ** 31 + 7), ln(bl=2 ** 32 - 1), ln(ncol=10)]
    text = b"\n".join(lines) + b"\n"
    d, M = check(gpu_ctx, tmp, text, K=1)
    assert d.odd.sum() > 300 and (~d.odd.astype(bool)).sum() > 80
    check(gpu_ctx, tmp, text)
    # the filter: spans at min_span, one under, qe < qs (unsigned wrap); ml at min_match, one under; a negative min_span is a huge unsigned one
    flt = [ln(qs=100, qe=2100), ln(qs=100, qe=2099), ln(ts=100, te=2100), ln(ts=100, te=2099), ln(qs=5000, qe=100), ln(ts=5000, te=100), ln(ml=100), ln(ml=99),
           ln(ml=2 ** 31 + 5), ln(qs=" 100", qe=2100), ln(qs=" 100", qe=2099), ln(ml="+99"), ln(ml="+100")]
    d, M = check(gpu_ctx, tmp, b"\n".join(flt) + b"\n", min_span=2000, min_match=100, K=1)
    assert list(M.stored) == [True, False, True, False, True, True, True, False, False, True, False, False, True]
    check(gpu_ctx, tmp, b"\n".join(flt) + b"\n", min_span=-1, min_match=0, K=1)


def test_carriage_returns(gpu_ctx, tmp):
    lines = [ln(ncol=10) + b"\r", ln(ncol=11) + b"\r", ln() + b"\r", ln(bl=b"\r", ncol=11), ln(ncol=10) + b"\t\r", ln() + b"\t\r", b"\r", b"x\r", b"\r\r", ln(qs=b"10\r"), ln(t=b"t1\r"),
             ln(st=b"\r"), ln(bl=4990, ncol=11) + b"\r\r", ln(q=b"\rq"), ln(ncol=9) + b"\r", b"\t" * 9 + b"\r"]
    for tail in (b"\n", b"", b"\r"):
        d, M = check(gpu_ctx, tmp, b"\n".join(lines) + tail, K=1)
        assert d.odd.any() and M.valid.sum() >= 8


# ------------------------------------------------------------------------------------------------ line geometry
def _ordinary(k, q=None):
    return ln(q=q or "q%d" % (k % 37), t="t%d" % (k % 11), qs=k % 900, qe=3000 + k % 977, ts=k % 700, te=3000 + k % 911)


@pytest.mark.parametrize("K", [1, 2, 15, 16, 31])
def test_first_line_in_front_of_its_tile(K, gpu_ctx, tmp):
    """a tile keeps the 960 bytes in front of it: a line that starts exactly 960 bytes in front of the tile it ends in is parsed in place, one byte more and it is
    left to the byte-wise kernel; starts 0, 1, 63 and 64 past a multiple of 64"""
    T = K * KIB
    seen = set()
    for d_front in (1, 63, 64, 65, 895, 896, 897, 959, 960, 961, 1023, 1024, 1025):
        B = 2 * T
        S = B - d_front
        text = filler(S) + padded(ln(), d_front + 70) + b"\n" + b"".join(_ordinary(k) + b"\n" for k in range(30))
        d, M = check(gpu_ctx, tmp, text, K=K)
        i = int(np.searchsorted(M.lstart, S))
        assert int(M.lstart[i]) == S and M.tile_of[i] == 2 and M.rank_in_tile[i] == 0
        assert bool(d.odd[i]) == (d_front > 960) and M.stored[i] and d.rep.tile_form == (1 if K <= 15 else 2)
        seen.add(S % 64)
    assert {0, 1, 63} <= seen


def test_lines_on_tile_borders(gpu_ctx, tmp):
    """a line exactly one tile long, lines ending on the last byte of a tile and on the first byte of the next, tiles in which no line ends (one, and runs)"""
    for K in (1, 2):
        T = K * KIB
        pre = filler(T - 200)
        a = padded(ln(q="a"), 199)                      # newline on the last byte of tile 0
        b = padded(ln(q="b"), T - 1)                    # exactly one tile with its newline: ends on the last byte of tile 1
        c = padded(ln(q="c"), T)                        # newline on the first byte of tile 3: no line ends in tile 2
        e = padded(ln(q="e"), 5 * T + 17)               # tiles 3.. : a run of tiles without a line end
        text = pre + a + b"\n" + b + b"\n" + c + b"\n" + e + b"\n" + b"".join(_ordinary(k) + b"\n" for k in range(60)) + padded(ln(q="z"), 3 * T)
        d, M = check(gpu_ctx, tmp, text, K=K)
        ends = M.lstart[1:].astype(np.int64) - 1
        assert (T - 1) in ends and (2 * T - 1) in ends and (3 * T) in ends
        per_tile = np.bincount(M.tile_of, minlength=M.n_tiles)
        assert per_tile[2] == 0 and (per_tile[4:8] == 0).all() and d.rep.open_line == 1 and d.odd.sum() >= 3


@pytest.mark.parametrize("K", [1, None])
def test_text_sizes(K, gpu_ctx, tmp):
    """texts of exactly 1024 k and 1024 k +- 1 bytes with and without a final newline; a last 16-byte piece of 1 / 15 / 16 bytes; 1 .. 65 granules"""
    body = b"".join(_ordinary(k) + b"\n" for k in range(1700))
    seen_gran = set()
    for n in [KIB * k + dlt for k in (1, 2, 3) for dlt in (-1, 0, 1)] + [2000 + 16 * 3 + r for r in (1, 15, 16)] + \
             [(g - 1) * KIB + 500 for g in (1, 7, 8, 9, 31, 32, 33, 65)]:
        for text in (body[:n], body[:n - 1] + b"\n"):
            d, M = check(gpu_ctx, tmp, text, K=K)
            seen_gran.add(d.rep.n_gran)
    assert {1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 65} <= seen_gran
    for text in (b"", b"\n", b"x", b"\n\n\n", ln(), ln() + b"\n"):
        check(gpu_ctx, tmp, text, K=K)


@pytest.mark.parametrize("unit", [b"\n", b"x\n"])
def test_more_lines_than_lanes_in_a_tile(unit, gpu_ctx, tmp):
    """a tile hands its lines out in batches of 256: 255 .. 1024 lines ending in ONE tile, a stored line as the last of a batch and another as the first of the next"""
    K = 4
    for cnt in (255, 256, 257, 511, 512, 513, 1024):
        for split in (254, 255) if cnt > 256 else (cnt - 2,):
            # tile 0: `split` short lines, two stored lines of one query (ranks split, split + 1), the rest short lines; the line behind them ends in tile 1
            rest = cnt - split - 2
            text = unit * split + ln(q="same") + b"\n" + ln(q="same", t="t2") + b"\n" + unit * max(rest, 0)
            text += padded(ln(q="tail"), K * KIB - len(text) + 40) + b"\n" + _ordinary(1) + b"\n"
            d, M = check(gpu_ctx, tmp, text, K=K)
            per_tile = np.bincount(M.tile_of, minlength=M.n_tiles)
            assert per_tile[0] == cnt and M.stored[split] and M.stored[split + 1]
            assert bool(d.flags[split + 1] & 0x10) == ((split + 1) % 64 != 0)
    # every line of the tile is one of `unit`: exactly cnt of them, then nothing
    for cnt in (256, 257, 1024):
        d, M = check(gpu_ctx, tmp, unit * cnt, K=K)
        assert d.rep.n_lines == cnt and d.rep.n_tiles == 1


# ------------------------------------------------------------------------------------------------ group fallback
def _group_case(start, end, K, gpu_ctx, tmp, junk_front=False):
    """ordinary lines, then ONE stored line from `start` to its newline at `end`, then ordinary lines"""
    head = b"".join(_ordinary(k) + b"\n" for k in range(12))
    if junk_front:
        head += b"j" * (start - len(head) - 1) + b"\n"
    else:
        head += filler(start - len(head))
    text = head + padded(ln(q="longline"), end - start) + b"\n" + b"".join(_ordinary(k) + b"\n" for k in range(40))
    d, M = check(gpu_ctx, tmp, text, K=K)
    i = int(np.searchsorted(M.lstart, start))
    assert int(M.lstart[i]) == start and int(M.lstart[i + 1]) == end + 1 and M.stored[i] and d.odd[i]
    return d, M


def test_first_line_of_a_tile_from_an_earlier_group(gpu_ctx, tmp):
    """k_paf_tile_first scans back to the start of its group of 4096 granules only; a line that leaves a group's granules up to a tile border without a newline
    sends it to the per-group table (k_paf_gran_bmax): one group back, two groups back, the newline found in the table's second step of 64 granules, and a
    line ending on a group border +- one granule"""
    G = GROUP_BYTES
    d, M = _group_case(2000, G + 200 * KIB, None, gpu_ctx, tmp)
    assert d.rep.tile_k == 31 and M.needs_group_table.sum() >= 5 and M.groups_back.max() == 1
    d, M = _group_case(2000, 2 * G + 300 * KIB, None, gpu_ctx, tmp)
    assert M.needs_group_table.any() and M.groups_back.max() == 2, "the table loop runs twice"
    # the group's last newline lies 100 granules in front of its end: the second step of k_paf_gran_bmax finds it
    d, M = _group_case(G - 100 * KIB, G + 100 * KIB, None, gpu_ctx, tmp, junk_front=True)
    assert M.needs_group_table.any() and (M.tfirst[M.needs_group_table] == G - 100 * KIB).all()
    for K in (1, 31):  # (K = 1: tile 4097 starts one granule behind the border and scans that granule only)
        for end in (G - 1, G - 1 - KIB, G - 1 + KIB, G + KIB + 5):
            d, M = _group_case(2000, end, K, gpu_ctx, tmp)
            assert bool(M.needs_group_table.any()) == (K == 1 and end >= G + KIB)


# ------------------------------------------------------------------------------------------------ stale bl
def test_stale_bl(gpu_ctx, tmp):
    ten = lambda k: ln(q="q%d" % k, ncol=10)
    cases = {
        "first line": [ten(0), ln(bl=111), ten(1)],
        "after a dropped 11-column line": [ln(bl=111), ln(bl=222, ncol=11, qs=10, qe=20), ten(0)],
        "after an odd line": [ln(bl=111), ln(bl=b" 333"), ten(0), ln(bl=b"-1"), ten(1)],
        "after a short line": [ln(bl=111), ln(ncol=9), ten(0), b"", ten(1)],
        "none": [ln(bl=5), ln(bl=6, ncol=11)],
    }
    for name, lines in cases.items():
        d, M = check(gpu_ctx, tmp, b"\n".join(lines) + b"\n", min_span=2000, min_match=100, K=1)
        assert d.rep.bl_pass == (name != "none"), name
    d, M = check(gpu_ctx, tmp, b"\n".join(cases["after an odd line"]) + b"\n", K=1)
    assert d.odd[1] and d.nums[7][2] == 333 and d.nums[7][4] == 0xFFFFFFFF
    # runs of 10-column lines over the 256-line blocks of the fill kernels and the tiles of the scan, every run behind another bl
    lines, k = [], 0
    for run in (1, 2, 255, 256, 257, 1023, 1024, 1025, 3000):
        lines.append(ln(bl=1000 + run))
        lines += [ten(k + j) for j in range(run)]
        k += run
    d, M = check(gpu_ctx, tmp, b"\n".join(lines) + b"\n")
    assert d.rep.bl_pass == 1 and M.n_nobl == k and len(set(d.nums[7])) == 9


# ------------------------------------------------------------------------------------------------ dictionary
def test_dictionary_forms(gpu_ctx, tmp):
    short = [ln(q=a, t=b) for a, b in (("a", "b"), ("abcdefgh", "abcdefg"), ("b", "a"), ("12345678", "a"))]
    d, M = check(gpu_ctx, tmp, b"\n".join(short) + b"\n")
    assert d.rep.dict_form == 1 and d.rep.n_long == 0
    d, M = check(gpu_ctx, tmp, b"\n".join(short) + b"\n", exact_text="1")
    assert d.rep.dict_form == 2
    for long_name in ("abcdefghi", ""):
        d, M = check(gpu_ctx, tmp, b"\n".join(short + [ln(q="a", t=long_name)]) + b"\n")
        assert d.rep.dict_form == 2 and d.rep.n_long == 1, "one stored line with a name that is not 1..8 bytes"
        d, M = check(gpu_ctx, tmp, b"\n".join(short + [ln(q="a", t=long_name, qs=10, qe=20)]) + b"\n", min_span=2000)
        assert d.rep.dict_form == 1 and d.rep.n_long == 0, "the long name stands in a dropped line only"


def test_dictionary_names(gpu_ctx, tmp):
    """key forms at 8 / 9 bytes, names that differ in the last byte only, a NUL (the C-string prefix meets another name), the first length wins"""
    names = [b"abcdefgh", b"abcdefghi", b"abcdefghj", b"abcdefg", b"abcdefgi"]
    for n in (9, 16, 17, 63, 64):
        names += [b"n" * (n - 1) + b"x", b"n" * (n - 1) + b"y"]
    names += [b"r\x001", b"r", b"r\x002", b"abcdefgh\x00zz", b"\x00", b""]
    lines = []
    for k, a in enumerate(names):
        for j, b in enumerate(names):
            if (k + j) % 3 == 0 or k == j:
                lines.append(ln(q=a, t=b, ql=1000 + k, tl=2000 + j, qs=k, ts=j, qe=4000, te=4100))
    d, M = check(gpu_ctx, tmp, b"\n".join(lines) + b"\n", K=1)
    assert d.rep.dict_form == 2 and len(M.names) == len({n.split(b"\0")[0] for n in names}) and d.odd.any()
    assert (M.qid == M.tid)[M.stored].any() and len(M.hits) < 2 * M.stored.sum(), "self hits: no mirror"
    check(gpu_ctx, tmp, b"\n".join(lines) + b"\n", bi_dir=0)
    # first seen as a target, later as a query (and the other way round); different lengths for one name: the first wins, a target column's too
    for nm in ("a", "a_long_name"):
        lines = [ln(q="x", t=nm, ql=1, tl=2), ln(q=nm, t="y", ql=3, tl=4), ln(q="y", t="x", ql=5, tl=6), ln(q=nm, t=nm, ql=7, tl=8), ln(q="z", t="z", ql=9, tl=10)]
        d, M = check(gpu_ctx, tmp, b"\n".join(lines) + b"\n")
        assert M.names == [b"x", nm.encode(), b"y", b"z"] and M.lens == [1, 2, 4, 9]


def _many_names(n_names, long_names=False):
    fmt = "name_number_%05d" if long_names else "%d"
    return b"".join(ln(q=fmt % (k % n_names), t=fmt % ((k * 7 + 1) % n_names), qs=k) + b"\n" for k in range(n_names if n_names > 1000 else 2 * n_names))


@pytest.mark.parametrize("long_names", [False, True])
def test_name_table_growth(long_names, gpu_ctx, tmp):
    """MA_DICT_CAP_LOG2: the first attempt ends on the load factor, on an exhausted probe sequence, three attempts; distinct names at half the table and one more"""
    ends = lambda d: [ma.PAF_TAB_ENDS[d.rep.end[a]] for a in range(d.rep.n_attempts)]
    caps = lambda d: [d.rep.cap[a] for a in range(d.rep.n_attempts)]
    d, M = check(gpu_ctx, tmp, _many_names(8, long_names), cap_log2=4)
    assert len(M.names) == 8 and ends(d) == ["ok"] and caps(d) == [16], "8 names in 16 slots: load factor exactly 1/2"
    d, M = check(gpu_ctx, tmp, _many_names(9, long_names), cap_log2=4)
    assert len(M.names) == 9 and ends(d) == ["load", "ok"] and caps(d) == [16, 65536 * 2]
    d, M = check(gpu_ctx, tmp, _many_names(16, long_names), cap_log2=4)
    assert ends(d) == ["load", "ok"], "a full table: every probe sequence still ends on a slot"
    d, M = check(gpu_ctx, tmp, _many_names(17, long_names), cap_log2=4)
    assert ends(d)[0] == "probes" and ends(d)[-1] == "ok", "17 names cannot sit in 16 slots"
    d, M = check(gpu_ctx, tmp, _many_names(70000, long_names), cap_log2=4)  # the first attempt counts 16 names, the second table is sized for those
    assert ends(d) == ["probes", "load", "ok"] and caps(d) == [16, 131072, 524288] and d.rep.n_distinct == 70000, "three attempts"


# ------------------------------------------------------------------------------------------------ query runs
@pytest.mark.parametrize("long_names", [False, True])
@pytest.mark.parametrize("run", [1, 2, 63, 64, 65, 128, 256, 257])
def test_query_runs(run, long_names, gpu_ctx, tmp):
    """runs of one query name, the run start moved through line indices 0 .. 64 (mod 64: k_dict_insert's lane) while the tile parser's lane is the line's rank in
    its tile: the two numberings disagree in every way.  Long names are equal in length and differ in the last byte only (bytes compared in LDS)."""
    fmt = "a_query_name_that_is_long_%03d%s" if long_names else "%03d%s"
    lines = []
    for s in range(65):
        for j in range((s - len(lines)) % 64):
            lines.append(ln(q=fmt % (j % 50, "s"), t="t%d" % j))
        assert len(lines) % 64 == s % 64
        lines += [ln(q=fmt % (s // 2, "ab"[s & 1]), t="t%d" % (j % 9), qs=j) for j in range(run)]  # (the run in front, if it stands right there, differs in the last byte)
    d, M = check(gpu_ctx, tmp, b"\n".join(lines) + b"\n", K=None if run >= 63 else 2)  # (short runs: small tiles, so that the text has more than one)
    qc = (d.flags & 0x10) != 0
    idx, rank = np.arange(M.L) % 64, M.rank_in_tile % 64
    assert d.rep.dict_form == (2 if long_names else 1) and (idx != rank).any()
    assert qc.any() == (run > 1)
    if run >= 63:
        assert (qc & (idx == 0)).any(), "a line the parser calls a continuation stands on lane 0 of the insert kernel"
    if run >= 64:
        assert (~qc & (rank == 0) & (idx != 0) & M.passed & np.r_[False, M.passed[:-1]]).any(), "a run the parser breaks at ITS lane 0 goes on in the insert kernel's wave"


def test_query_runs_broken(gpu_ctx, tmp):
    """runs over a tile border and a batch border; runs broken by a dropped, an invalid and an odd line"""
    for q in ("q", "a_query_name_that_is_long"):
        run = [ln(q=q, t="t%d" % (j % 5), qs=j) for j in range(40)]
        for breaker in (ln(q=q, qs=10, qe=20), ln(q=q, ncol=9), ln(q=q, qs=b" 7"), b""):
            lines = run[:20] + [breaker] + run[20:]
            d, M = check(gpu_ctx, tmp, b"\n".join(lines) + b"\n", min_span=2000, K=1)
            qc = (d.flags & 0x10) != 0
            assert not qc[20] and not qc[21] and qc.sum() >= 30 and (M.tile_of[1:] != M.tile_of[:-1]).any()
        d, M = check(gpu_ctx, tmp, b"\n" * 250 + b"\n".join(run) + b"\n", K=8)
        qc = (d.flags & 0x10) != 0
        assert d.rep.n_tiles == 1 and qc[255] and not qc[256] and qc[257], "the batch border is a wave border"


# ------------------------------------------------------------------------------------------------ records
@pytest.mark.parametrize("L", [1, 63, 64, 65, 4095, 4096, 4097, 8192, 8193])
def test_records(L, gpu_ctx, tmp):
    """k_paf_emit_chain: tiles of 4096 lines chained, the last one writes the total; stored patterns, mirrored records, self hits"""
    pats = {"all": lambda k: True, "none": lambda k: False, "first": lambda k: k == 0, "last": lambda k: k == L - 1, "alternating": lambda k: k % 2 == 0,
            "tile 1 unstored": lambda k: not (4096 <= k < 8192)}
    for name, keep in pats.items():
        if name == "tile 1 unstored" and L < 8192:
            continue
        lines = [ln(q="r%d" % (k % 61), t="r%d" % (k % 61 if k % 5 == 0 else (k * 3) % 67), qs=k % 1000, qe=(k % 1000) + (3000 if keep(k) else 10), ml=100 + k % 7) for k in range(L)]
        text = b"\n".join(lines) + b"\n"
        for bi_dir in (1, 0) if name in ("all", "alternating") else (1,):
            d, M = check(gpu_ctx, tmp, text, min_span=2000, bi_dir=bi_dir)
            assert d.rep.n_lines == L and M.stored.sum() == sum(keep(k) for k in range(L))
            if name == "all":
                assert (M.qid == M.tid).any() and len(M.hits) == (2 * L - int((M.qid == M.tid).sum()) if bi_dir else L)


def test_records_by_read_range(gpu_ctx, tmp):
    """mahip_hits_raw_extract_pos on the parser's records: read ranges cut at id 0, 1, n_seq - 1 and n_seq"""
    def _dev_buffer(nbytes):  # device memory for the C ABI: a torch tensor; on the CPU build of the kernels device pointers are host pointers
        if getattr(ma, "IS_EMU", False):
            a = np.zeros(max(nbytes, 1), dtype=np.uint8)
            return a, a.ctypes.data
        import torch
        t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        return t, t.data_ptr()
    Lb = ma.lib()
    vp = C.c_void_p
    Lb.mahip_hits_raw_extract_pos.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.POINTER(C.c_size_t)]
    text = b"".join(ln(q="r%d" % (k % 61), t="r%d" % ((k * 3) % 67), qs=k) + b"\n" for k in range(4097))
    M = PM.model(text, 0, 0, 1)
    d = device_parse(gpu_ctx, text, 0, 0, 1)
    assert d.hits.tobytes() == M.hits.tobytes()
    n_seq = len(M.names)
    qid = (M.hits["qns"] >> np.uint64(32)).astype(np.int64)
    for q0, q1 in ((0, 0), (0, 1), (1, n_seq - 1), (n_seq - 1, n_seq), (0, n_seq), (n_seq, n_seq), (1, 1)):
        sel = (qid >= q0) & (qid < q1)
        n = C.c_size_t(0)
        keep_r, ptr_r = _dev_buffer(max(int(sel.sum()), 1) * 32)
        keep_p, ptr_p = _dev_buffer(max(int(sel.sum()), 1) * 4)
        ma._chk(Lb.mahip_hits_raw_extract_pos(gpu_ctx.h, q0, q1, vp(ptr_r), vp(ptr_p), C.byref(n)), "raw_extract_pos")
        Lb.mahip_sync(gpu_ctx.h)
        pos, rec = np.zeros(max(n.value, 1), dtype=np.uint32), np.zeros(max(n.value, 1), dtype=ma.HIT_DT)
        if n.value:
            ma._chk(Lb.mahip_memcpy_d2h(gpu_ctx.h, pos.ctypes.data, vp(ptr_p), n.value * 4), "d2h")
            ma._chk(Lb.mahip_memcpy_d2h(gpu_ctx.h, rec.ctypes.data, vp(ptr_r), n.value * 32), "d2h")
        assert n.value == int(sel.sum()) and (pos[:n.value] == np.flatnonzero(sel)).all() and rec[:n.value].tobytes() == M.hits[sel].tobytes()
    ma._chk(Lb.mahip_paf_release(gpu_ctx.h), "release")


# ------------------------------------------------------------------------------------------------ -R
def test_no_cont_prefilter(gpu_ctx, tmp):
    """-R on the parsed columns: containments in both directions, an excluded name whose removal shifts every later id, an excluded name in dropped lines only"""
    lines = [ln(q="first", t="second", ql=9000, tl=9000, qs=100, qe=5000, ts=100, te=5000),
             ln(q="big1", ql=30000, qs=5000, qe=14000, t="inner1", tl=9000, ts=10, te=8990),           # the target is inside the query
             ln(q="inner2", ql=9000, qs=10, qe=8990, t="big2", tl=30000, ts=5000, te=14000, st="-"),    # the query is inside the target
             ln(q="inner3", ql=9000, qs=10, qe=8990, t="big3", tl=30000, ts=5000, te=14000, ml=10)]     # ... in a line the filter drops: not excluded
    lines.append(ln(q="inner3", t="first"))
    for k in range(300):
        q, t = ("inner1", "big2") if k % 17 == 0 else ("r%d" % (k % 40), "inner2" if k % 13 == 0 else "r%d" % ((k * 7) % 43))
        lines.append(ln(q=q, t=t, qs=k, qe=4000 + k, ts=k, te=4100))
    text = b"\n".join(lines) + b"\n"
    d, M = check(gpu_ctx, tmp, text, min_span=2000, min_match=100, no_cont=(1000, 0.8))
    assert M.excl == {b"inner1", b"inner2"} and d.info.n_excl == 2 and b"inner3" in M.names and b"inner1" not in M.names
    plain = PM.model(text, 2000, 100, 1)
    assert b"big1" not in M.names and plain.names.index(b"inner3") == 6 and M.names.index(b"inner3") == 2, "its only line touched an excluded read; later ids shift"
    assert M.stored.sum() < M.passed.sum() and d.rep.n_distinct == len(plain.names)
    check(gpu_ctx, tmp, text, min_span=2000, min_match=100, no_cont=(1000, 0.8), bi_dir=0, K=1)
    d, M = check(gpu_ctx, tmp, b"\n".join(lines[1:3]) + b"\n", min_span=2000, min_match=100, no_cont=(1000, 0.8))
    assert M.stored.sum() == 0 and d.info.n_seq == 0 and d.info.n_excl == 2, "every stored line touches an excluded read"
