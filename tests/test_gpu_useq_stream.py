"""The reads file of `miniasm -f` read on the device A PIECE AT A TIME (csrc/useq.hip, host/unitig_gfa.c: ma_ug_seq with MA_FASTX_STREAM): the
window = carry + piece, its consumed prefix, the verdict per window, the probe with its match list, the placement by match, the handover to the host reader.

Yardsticks of a stage case: the arena the WHOLE-FILE reader (Ctx.useq_place_text, unchanged code) makes of the concatenated text, and the small Python model of
the window rules below (consumed records, carry, verdict, matched / dup / jobs).  End to end: the unmodified reference binary, byte for byte, through the CLI
and the drop-in; the `[T::ug_seq]` line says that the streamed reader ran and whether (and where) it handed over."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bgzfmodel as B
import miniasm_amd as ma
import refapi as R

pytestmark = pytest.mark.gpu

needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not built")

COMP = bytes.maketrans(b"ABCDGHKMRTUVYabcdghkmrtuvy`", b"TVGHCDMKYAABRtvghcdmkyaabr@")


# ------------------------------------------------------------------------------------------------ inputs
def _bases(rs, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rs.randint(0, len(alphabet), n)].tobytes()


def _wrap(seq, w):
    return b"\n".join(seq[i:i + w] for i in range(0, len(seq), w)) if w and len(seq) > w else seq


def _record(name, seq, fmt, wrap=0):
    if fmt == "fq":
        return b"@" + name + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"
    return b">" + name + b"\n" + _wrap(seq, wrap) + b"\n"


def _by_lines(text, k):
    """pieces of k lines each (the last piece takes what is left, with or without its newline)"""
    lines = text.split(b"\n")
    tail = lines.pop()
    lines = [l + b"\n" for l in lines] + ([tail] if tail else [])
    return [b"".join(lines[i:i + k]) for i in range(0, len(lines), k)]


def _want(name, dst_off, ln, rev=False, s=0, e=None):
    return dict(name=name, dst_off=dst_off, len=ln, rev=rev, s=s, e=e)


# ------------------------------------------------------------------------------------------------ the model of the window rules
def _lines(win):
    lines = win.split(b"\n")
    if win.endswith(b"\n"):
        lines.pop()
    return lines


def _name(header):
    return re.split(rb"[ \t\v\f]", header[1:])[0]


def _place(arena, w, seq):
    s, e = (w["s"], w["e"]) if w.get("e") is not None else (0, len(seq))
    part = seq[s:e]
    n = min(w["len"], len(part))
    arena[w["dst_off"]:w["dst_off"] + n] = part[:n] if not w["rev"] else bytes(78 if c >= 128 else c for c in part[::-1][:n]).translate(COMP)


def model(pieces, wanted, arena_bytes):
    """-> (arena, verdicts, report, refused window or None): the rules of DESIGN 3.18 in fifty lines"""
    arena, carry, fmt, seen, verdicts, refused = bytearray(b"N" * arena_bytes), b"", None, set(), [], None
    by_name = {w["name"]: w for w in wanted}
    rep = dict(records=0, matched=0, dup=0, jobs=0, max_carry=0, refused_piece=-1, refused_reason="OK", pieces=0)
    for k, p in enumerate(pieces):
        last, win = k + 1 == len(pieces), carry + p
        rep["pieces"] += 1
        if not win:
            verdicts.append(dict(reason="OK", records=0, consumed=0, carry=0, placed=0))
            continue
        reason = "OK"
        if fmt is None:
            fmt = {62: "fasta", 64: "fastq"}.get(win[0])
        if fmt is None:
            reason, recs, consumed = "FIRST_BYTE", [], 0
        else:
            lines = _lines(win)
            L = len(lines)
            if fmt == "fastq":
                Lc = L if last else L - L % 4
                recs = [(lines[i], lines[i + 1], lines[i + 2], lines[i + 3]) for i in range(0, L - L % 4, 4)]
            else:
                heads = [i for i, l in enumerate(lines) if l[:1] == b">"]
                Lc = L if last else heads[-1]
                heads = [i for i in heads if i < Lc] + [Lc]
                recs = [(lines[a], b"".join(lines[a + 1:b])) for a, b in zip(heads, heads[1:])]
            consumed = min(sum(len(l) + 1 for l in lines[:Lc]), len(win))
            prefix = win[:consumed]
            hits = [(_name(r[0]), r[1]) for r in recs if _name(r[0]) in by_name and _name(r[0])]
            need = lambda w: w["len"] if w.get("e") is None else w["e"]  # noqa: E731
            if b"\r" in prefix:
                reason = "CR"
            elif b"\0" in prefix:
                reason = "NUL_BYTE"
            elif fmt == "fastq" and last and L % 4:
                reason = "FASTQ_SHAPE"
            elif fmt == "fasta" and any(l[:1] in (b"@", b"+") for l in lines[:Lc]):
                reason = "FASTA_LINE_START"
            elif fmt == "fastq" and any(r[0][:1] != b"@" or r[1][:1] in (b">", b"@", b"+") or r[2][:1] != b"+" for r in recs):
                reason = "FASTQ_SHAPE"
            elif fmt == "fastq" and any(len(r[1]) != len(r[3]) for r in recs):
                reason = "FASTQ_QUAL_LEN"
            elif any(len(s) < need(by_name[nm]) for nm, s in hits):
                reason = "SHORT_READ"
        if reason != "OK":
            verdicts.append(dict(reason=reason))
            rep["refused_piece"], rep["refused_reason"], refused = k, reason, win
            break
        lastrec = dict(hits)
        for nm, s in lastrec.items():
            _place(arena, by_name[nm], s)
        new = set(lastrec) - seen
        seen |= new
        carry = win[consumed:]
        rep["records"] += len(recs); rep["matched"] += len(new); rep["dup"] += len(hits) - len(new); rep["jobs"] += len(lastrec)
        rep["max_carry"] = max(rep["max_carry"], len(carry))
        verdicts.append(dict(reason="OK", records=len(recs), consumed=consumed, carry=len(carry), placed=len(lastrec)))
    return bytes(arena), verdicts, rep, refused


def _whole(ctx, text, wanted, arena_bytes):
    """the whole-file reader on the concatenated text -> (arena, n_matched, n_dup)"""
    ctx.fastx_load(text)
    info = ctx.fastx_index()
    assert info["regular"], info
    arena, n_matched, n_dup, n_short = ctx.useq_place_text(arena_bytes, wanted)
    assert n_short == 0
    ctx.fastx_release()
    return arena, n_matched, n_dup


def _stream(ctx, pieces, wanted, arena_bytes, whole=True):
    """the stream against the model, and (for a text the whole-file reader takes) against the whole-file reader; -> (arena, verdicts, report)"""
    arena, verdicts, rep = ctx.useq_stream(pieces, arena_bytes, wanted)
    m_arena, m_verdicts, m_rep, m_refused = model(pieces, wanted, arena_bytes)
    assert [v["reason"] for v in verdicts] == [v["reason"] for v in m_verdicts]
    assert [v for v in verdicts if v["reason"] == "OK"] == [v for v in m_verdicts if v["reason"] == "OK"], "records consumed / bytes / carry / placed differ from the model"
    assert arena == m_arena, "the arena differs from the model's"
    for key in ("records", "matched", "dup", "jobs", "max_carry", "refused_piece", "refused_reason", "pieces"):
        assert rep[key] == m_rep[key], (key, rep, m_rep)
    if m_refused is None:
        if whole:
            w_arena, w_matched, w_dup = _whole(ctx, b"".join(pieces), wanted, arena_bytes)
            assert arena == w_arena, "the arena differs from the whole-file reader's"
            assert (rep["matched"], rep["dup"]) == (w_matched, w_dup)
    else:
        assert ctx.useq_stream_window() == m_refused, "the refused window is not carry + piece"
        with pytest.raises(Exception):
            ctx.useq_stream_piece(b"", True)
        ctx.useq_stream_abort()
    ctx.fastx_release()
    return arena, verdicts, rep


def _wanted_all(recs, rs):
    """every distinct name wanted once: strands alternate, whole records and kept intervals alternate"""
    out, at, done = [], 0, set()
    for k, (nm, s) in enumerate(recs):
        if nm in done:
            continue
        done.add(nm)
        n = len(s)
        if k % 3 == 0:
            a, b, ln = 0, None, int(rs.randint(0, n + 1))
        else:
            a = int(rs.randint(0, n + 1)); b = int(rs.randint(a, n + 1)); ln = int(rs.randint(0, b - a + 1))
        if k % 4 == 1:
            a, b, ln = 0, n, n
        out.append(_want(nm, at, ln, k % 2 == 1, a, b))
        at += ln + 1
    return out, at


# ------------------------------------------------------------------------------------------------ cut phase
SIX = [(b"r%d" % k, n) for k, n in enumerate([30, 1, 300, 64, 0, 257])]


@pytest.mark.parametrize("variant", ["plain", "empty_piece", "no_final_newline"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7])
def test_fastq_cut_on_every_phase(k, variant, gpu_ctx):
    """six records in pieces of k lines: the cut falls on every phase mod 4 and inside every record; an empty piece in the middle; the last line without '\\n'"""
    rs = np.random.RandomState(k)
    recs = [(nm, _bases(rs, n)) for nm, n in SIX]
    text = b"".join(_record(nm + (b" c" if i % 2 else b""), s, "fq") for i, (nm, s) in enumerate(recs))
    if variant == "no_final_newline":
        text = text[:-1]
    pieces = _by_lines(text, k)
    if variant == "empty_piece":
        pieces.insert(len(pieces) // 2, b"")
    wanted, ab = _wanted_all(recs, rs)
    _, verdicts, rep = _stream(gpu_ctx, pieces, wanted, ab)
    assert rep["format"] == "fastq" and rep["records"] == 6 and rep["matched"] == 6 and rep["refused_piece"] == -1
    if k % 4:
        assert rep["max_carry"] > 0


@pytest.mark.parametrize("variant", ["plain", "header_last", "empty_lines", "no_final_newline"])
@pytest.mark.parametrize("wrap", [0, 7])
def test_fasta_one_line_per_piece(wrap, variant, gpu_ctx):
    """a record spans many pieces: it is carried until the next header (or the last piece) comes, and the window grows past its first size"""
    rs = np.random.RandomState(wrap + 1)
    recs = [(b"a", _bases(rs, 40)), (b"bb", _bases(rs, 300)), (b"c", _bases(rs, 7)), (b"d", _bases(rs, 100))]
    body = [_record(nm, s, "fa", wrap) for nm, s in recs]
    if variant == "empty_lines":
        body = [b + b"\n\n" for b in body]
    text = b"".join(body)
    if variant == "header_last":
        text += b">tail comment\n"
        recs.append((b"tail", b""))
    if variant == "no_final_newline":
        text = text[:-1]
    pieces = _by_lines(text, 1)
    wanted, ab = _wanted_all(recs, rs)
    _, verdicts, rep = _stream(gpu_ctx, pieces, wanted, ab)
    assert rep["format"] == "fasta" and rep["records"] == len(recs) and rep["refused_piece"] == -1
    assert verdicts[-1]["records"] >= 1 and verdicts[-1]["carry"] == 0, "the last record is consumed by the last piece only"
    assert all(v["placed"] == 0 for v in verdicts[:2])
    if wrap:
        assert rep["window_growths"] >= 1 and rep["max_carry"] > 300


def test_wrapped_placement_across_the_seam(gpu_ctx):
    """records of 257 and 513 lines of width 3, 100 lines a piece: the 256-line chunk edges of the placement, over lines that came in different pieces"""
    rs = np.random.RandomState(7)
    recs = [(b"n257", _bases(rs, 257 * 3 - 1)), (b"n513", _bases(rs, 513 * 3)), (b"z", _bases(rs, 5))]
    text = b"".join(_record(nm, s, "fa", 3) for nm, s in recs)
    wanted = [_want(b"n257", 0, 700, True, 3, 769), _want(b"n513", 701, 1539, False), _want(b"z", 2300, 5, True)]
    _, _, rep = _stream(gpu_ctx, _by_lines(text, 100), wanted, 2310)
    assert rep["records"] == 3 and rep["jobs"] == 3


def test_carry_moves_over_itself(gpu_ctx):
    """a carry longer than what was consumed in front of it, in a window that needs no larger buffer: the copy kernel, over several of its 4 KiB tiles"""
    rs = np.random.RandomState(11)
    big = _bases(rs, 9001)
    text = _record(b"a", b"ACGT", "fa") + _record(b"big", big, "fa", 61) + _record(b"c", b"GGA", "fa")
    cut = text.index(b"\n", 9000) + 1
    first, rest = text[:cut], text[cut:]
    pieces = [first] + _by_lines(rest, 2)
    wanted = [_want(b"a", 0, 4), _want(b"big", 5, 9001, True), _want(b"c", 9010, 3)]
    _, verdicts, rep = _stream(gpu_ctx, pieces, wanted, 9014)
    assert verdicts[0]["consumed"] == 8 and verdicts[0]["carry"] > 8900 and rep["window_growths"] == 0


# ------------------------------------------------------------------------------------------------ last wins, win[] between windows
@pytest.mark.parametrize("fmt", ["fq", "fa"])
def test_last_record_of_a_name_wins(fmt, gpu_ctx):
    rs = np.random.RandomState(5)
    recs = [(b"x", _bases(rs, 50)), (b"twice", _bases(rs, 40)), (b"twice", _bases(rs, 60)), (b"y", _bases(rs, 9)),     # window 0: one name twice
            (b"far", _bases(rs, 80)), (b"p", _bases(rs, 10)), (b"q", _bases(rs, 10)), (b"s", _bases(rs, 10)),          # window 1
            (b"t", _bases(rs, 10)), (b"u", _bases(rs, 10)), (b"v", _bases(rs, 10)), (b"w", _bases(rs, 10)),            # window 2
            (b"far", _bases(rs, 33)), (b"x", _bases(rs, 50)), (b"o", _bases(rs, 3)), (b"oo", _bases(rs, 3)), (b"end", b"A")]  # window 3: other bases, another length
    text = b"".join(_record(nm, s, fmt) for nm, s in recs)
    pieces = _by_lines(text, 16 if fmt == "fq" else 8)
    wanted = [_want(b"x", 0, 50, True), _want(b"twice", 50, 40, False), _want(b"far", 90, 30, True, 2, 33), _want(b"absent", 120, 10), _want(b"y", 130, 9, False, 0, 9)]
    arena, verdicts, rep = _stream(gpu_ctx, pieces, wanted, 140)
    assert arena[120:130] == b"N" * 10 and (rep["matched"], rep["dup"]) == (4, 3)
    assert arena[50:90] == recs[2][1][:40]


def test_win_is_clean_between_windows(gpu_ctx):
    """A matches record 2 of window 1; window 2 has other names at record 2 and no A: A keeps window 1's bases, and one job runs per (window, name) pair"""
    rs = np.random.RandomState(13)
    names = [[b"k0", b"k1", b"k2", b"k3"], [b"m0", b"m1", b"A", b"m3"], [b"n0", b"n1", b"n2", b"n3"], [b"z0", b"m1", b"z2", b"z3"]]
    recs = [(nm, _bases(rs, 20)) for win in names for nm in win]
    text = b"".join(_record(nm, s, "fq") for nm, s in recs)
    wanted = [_want(b"A", 0, 20), _want(b"n2", 20, 20, True), _want(b"m1", 40, 20), _want(b"k3", 60, 20), _want(b"n0", 80, 20)]
    arena, verdicts, rep = _stream(gpu_ctx, _by_lines(text, 16), wanted, 100)
    assert [v["placed"] for v in verdicts] == [1, 2, 2, 1] and rep["jobs"] == 6 and (rep["matched"], rep["dup"]) == (5, 1)
    assert arena[:20] == recs[6][1]


@pytest.mark.parametrize("fmt,wrap", [("fq", 0), ("fa", 0), ("fa", 5)])
def test_both_strands_and_both_placement_kinds(fmt, wrap, gpu_ctx):
    rs = np.random.RandomState(17)
    alpha = b"ACGTacgtRYKMSWBDHVNrykmswbdhvnUu" + bytes([128, 200, 255]) + b"*-."
    recs = [(b"r%d" % k, _bases(rs, 90 + k, alpha)) for k in range(8)]
    recs[1] = (b"r1", b"AC" + bytes([129, 255]) + b"GT" * 40)
    text = b"".join(_record(nm, s, fmt, wrap) for nm, s in recs)
    wanted, at = [], 0
    for k, (nm, s) in enumerate(recs):
        whole, rev = k % 2 == 0, (k // 2) % 2 == 1
        wanted.append(_want(nm, at, 60, rev, 0 if whole else 10, None if whole else 80))
        at += 61
    wanted[1] = _want(b"r1", wanted[1]["dst_off"], 60, True, 0, len(recs[1][1]))  # the bytes >= 128 are among the last 60 of the reverse strand
    wanted[1]["len"] = len(recs[1][1])
    at += 40
    arena, _, _ = _stream(gpu_ctx, _by_lines(text, 5), wanted[:1] + [dict(wanted[1], dst_off=at)] + wanted[2:], at + 100)
    assert arena[at:at + len(recs[1][1])].endswith(b"NNGT")


# ------------------------------------------------------------------------------------------------ verdicts
def _five(fmt, bad_record):
    """five pieces of four records each; record 9 (in piece 2) is replaced"""
    rs = np.random.RandomState(23)
    recs = [(b"v%d" % k, _bases(rs, 30)) for k in range(20)]
    body = [_record(nm, s, fmt) for nm, s in recs]
    body[9] = bad_record(recs[9])
    pieces = [b"".join(body[i:i + 4]) for i in range(0, 20, 4)]
    wanted = [_want(nm, 31 * k, 30, k % 2 == 1) for k, (nm, s) in enumerate(recs)]
    return pieces, wanted, 31 * 20


VERDICTS = {
    "cr": ("fq", lambda r: b"@" + r[0] + b"\n" + r[1] + b"\r\n+\n" + b"I" * 30 + b"\r\n", "CR"),
    "nul": ("fa", lambda r: b">" + r[0] + b"\0x\n" + r[1] + b"\n", "NUL_BYTE"),
    "qual_one_short": ("fq", lambda r: b"@" + r[0] + b"\n" + r[1] + b"\n+\n" + b"I" * 29 + b"\n", "FASTQ_QUAL_LEN"),
    "fasta_plus_line": ("fa", lambda r: b">" + r[0] + b"\n" + r[1][:10] + b"\n+" + r[1][11:] + b"\n", "FASTA_LINE_START"),
    "short_read": ("fq", lambda r: b"@" + r[0] + b"\nACGT\n+\nIIII\n", "SHORT_READ"),
}


@pytest.mark.parametrize("what", list(VERDICTS))
def test_verdict_in_the_middle_piece(what, gpu_ctx):
    """the reason and the piece; the arena holds what the windows before placed; the refused window comes back byte for byte; a further piece is an error"""
    fmt, bad, reason = VERDICTS[what]
    pieces, wanted, ab = _five(fmt, bad)
    arena, verdicts, rep = _stream(gpu_ctx, pieces, wanted, ab)
    assert (rep["refused_piece"], rep["refused_reason"]) == (2, reason) and len(verdicts) == 3
    assert arena[31 * 8:] == (b"N" * 31 * 12) and b"N" * 30 not in arena[:31 * 7]


def test_fastq_last_window_of_a_broken_shape(gpu_ctx):
    rs = np.random.RandomState(29)
    recs = [(b"s%d" % k, _bases(rs, 20)) for k in range(6)]
    text = b"".join(_record(nm, s, "fq") for nm, s in recs) + b"@tail\nACGT\n"  # L mod 4 = 2 in the last window
    wanted = [_want(nm, 21 * k, 20) for k, (nm, s) in enumerate(recs)]
    arena, verdicts, rep = _stream(gpu_ctx, _by_lines(text, 10), wanted, 126)
    assert (rep["refused_piece"], rep["refused_reason"]) == (2, "FASTQ_SHAPE")


def test_first_byte_of_the_input(gpu_ctx):
    _, verdicts, rep = _stream(gpu_ctx, [b"", b"ACGT\n", b">a\nAC\n"], [_want(b"a", 0, 2)], 2)
    assert (rep["refused_piece"], rep["refused_reason"], rep["format"]) == (1, "FIRST_BYTE", None)


def test_later_fasta_window_is_checked_as_fasta(gpu_ctx):
    """a later window that holds a line beginning with '@': the format comes from window 0, not from the window"""
    pieces = [b">a\nACGT\n>b\nAC\n", b">c\nGG\n", b"@CGT\n>d\nTT\n", b">e\nAA\n"]
    wanted = [_want(nm, 4 * k, 2) for k, nm in enumerate([b"a", b"b", b"c", b"d", b"e"])]
    arena, verdicts, rep = _stream(gpu_ctx, pieces, wanted, 20)
    assert (rep["refused_piece"], rep["refused_reason"], rep["format"]) == (2, "FASTA_LINE_START", "fasta")
    assert arena == b"ACNNACNN" + b"N" * 12  # b is placed by window 1, c is still carried when window 2 is refused


def test_stream_misuse_is_an_error(gpu_ctx):
    with pytest.raises(Exception):
        gpu_ctx.useq_stream([b">a\nAC", b"GT\n"], 4, [_want(b"a", 0, 4)])  # a piece that is not the last ends inside a line
    gpu_ctx.useq_stream_abort()
    with pytest.raises(Exception):
        gpu_ctx.useq_stream_piece(b">a\n", False)  # no stream
    arena, verdicts, rep = gpu_ctx.useq_stream([], 4, [_want(b"a", 0, 4)])
    assert arena == b"NNNN" and rep["pieces"] == 0
    arena, verdicts, rep = gpu_ctx.useq_stream([b">a\nACGT\n"], 0, [])
    assert arena is None and rep["records"] == 1 and rep["jobs"] == 0
    gpu_ctx.fastx_release()


def test_cost_follows_the_window_not_the_wanted_list(gpu_ctx):
    """one wanted read, and 5000 of which 4999 are in no window: the same ten pieces give the same verdicts and jobs (that no launch of a window sweeps the wanted
    list is a point for the reader of csrc/useq.hip; this guards the behaviour)"""
    rs = np.random.RandomState(31)
    recs = [(b"w%d" % k, _bases(rs, 25)) for k in range(40)]
    pieces = _by_lines(b"".join(_record(nm, s, "fq") for nm, s in recs), 16)
    assert len(pieces) == 10
    one = [_want(b"w17", 0, 25, True)]
    many = one + [_want(b"absent%d" % k, 26 + k, 1) for k in range(4999)]
    a1, v1, r1 = _stream(gpu_ctx, pieces, one, 26 + 4999)
    a2, v2, r2 = _stream(gpu_ctx, pieces, many, 26 + 4999)
    assert v1 == v2 and r1["jobs"] == r2["jobs"] == 1 and a1 == a2


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def paf(tmpdir_s):
    return R.pafgen(os.path.join(tmpdir_s, "ustream.paf"), 400, 12000, 23, ["-L", "uniform"])


@pytest.fixture(scope="module")
def reads(paf):
    lens = {}
    for ln in open(paf, "rb"):
        f = ln.split(b"\t")
        lens.setdefault(f[0], int(f[1]))
        lens.setdefault(f[5], int(f[6]))
    rs = np.random.RandomState(5)
    return {nm: _bases(rs, n) for nm, n in lens.items()}


def _file(reads, fmt, wrap=0):
    return b"".join(_record(nm, s, fmt, wrap) for nm, s in reads.items())


def _write(tmpdir_s, tag, data, gz=False):
    p = os.path.join(tmpdir_s, "ustream_%s" % tag)
    with (gzip.open(p, "wb", 1) if gz else open(p, "wb")) as f:
        f.write(data)
    return p


def _e2e(reads_fn, paf, env, stdin_fn=None):
    """reference, then CLI and drop-in under `env` -> [(the [T::ug_seq] line, the [W::ma_ug_seq] lines)], outputs compared byte for byte"""
    def inp():
        return open(stdin_fn, "rb") if stdin_fn else None
    r = subprocess.run([R.REF_BIN, "-f", reads_fn, paf], stdin=inp(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert b"\nS\t" in b"\n" + r.stdout, "the case is supposed to have unitigs"
    out = []
    for binary in (ma.CLI_PATH, R.DROPIN_BIN):
        e = dict(os.environ, MA_PIPE_TIMING="1")
        for k in ("MA_FASTX_HOST", "MA_FASTX_STREAM", "MA_FASTX_PIECE", "MA_BGZF_HOST"):
            e.pop(k, None)
        e.update(env)
        g = subprocess.run([binary, "-f", reads_fn, paf], stdin=inp(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=600)
        log = g.stderr.decode(errors="replace")
        assert g.returncode == 0, log[-2000:]
        assert g.stdout == r.stdout, "%s: output differs from the reference" % os.path.basename(binary)
        t = [ln for ln in log.splitlines() if ln.startswith("[T::ug_seq]")]
        assert len(t) == 1, log[-2000:]
        out.append((t[0], [ln for ln in log.splitlines() if ln.startswith("[W::ma_ug_seq]")]))
    return out


STREAM = {"MA_FASTX_STREAM": "1", "MA_FASTX_PIECE": "4096"}
REGULAR = ["gzip_fastq", "gzip_fasta_wrap60", "stdin_fastq", "stdin_gzip", "bgzf_host_forced", "plain_file_mode_2"]


@needs_ref
@pytest.mark.parametrize("what", REGULAR)
def test_regular_input_is_streamed_through_the_device(what, reads, paf, tmpdir_s):
    """pieces of 4 KiB, so reads longer than a piece occur; fails without the streamed reader: reader=host there"""
    env, stdin_fn = dict(STREAM), None
    if what == "gzip_fastq":
        fn = _write(tmpdir_s, "a.fq.gz", _file(reads, "fq"), gz=True)
    elif what == "gzip_fasta_wrap60":
        fn = _write(tmpdir_s, "b.fa.gz", _file(reads, "fa", 60), gz=True)
    elif what == "stdin_fastq":
        fn, stdin_fn = "-", _write(tmpdir_s, "c.fq", _file(reads, "fq"))
    elif what == "stdin_gzip":
        fn, stdin_fn = "-", _write(tmpdir_s, "d.fq.gz", _file(reads, "fq"), gz=True)
    elif what == "bgzf_host_forced":
        fn = _write(tmpdir_s, "e.fq.bgz", B.bgzf(_file(reads, "fq")))
        env["MA_BGZF_HOST"] = "1"
    else:
        fn = _write(tmpdir_s, "f.fa", _file(reads, "fa", 60))
        env["MA_FASTX_STREAM"] = "2"
    for t, warn in _e2e(fn, paf, env, stdin_fn):
        assert "reader=stream" in t and "handover=none" in t and "reason=0" in t, t
        assert int(re.search(r"pieces=(\d+)", t).group(1)) > 10 and "piece=4096 B" in t
        assert warn == []


@needs_ref
@pytest.mark.parametrize("what", ["cr", "qual_len"])
def test_handover_to_the_host_reader_in_the_middle(what, reads, paf, tmpdir_s):
    """a record in the middle of a gzip FASTQ that the device refuses: the windows before it stay placed, the host reader takes over from the window's first byte"""
    names = list(reads)
    mid = names[len(names) // 2]
    s = reads[mid]
    alt = b"@" + mid + b"\n" + s + (b"\r\n+\n" + b"I" * len(s) + b"\r\n" if what == "cr" else b"\n+\n" + b"I" * (len(s) + 3) + b"\n")
    data = b"".join(alt if nm == mid else _record(nm, q, "fq") for nm, q in reads.items())
    fn = _write(tmpdir_s, "h_%s.fq.gz" % what, data, gz=True)
    for t, warn in _e2e(fn, paf, STREAM):
        m = re.search(r"handover=(\d+) reason=(\d+)", t)
        assert "reader=stream" in t and m and int(m.group(1)) > 0, t
        assert ma.FASTX_REASONS[int(m.group(2))] == ("CR" if what == "cr" else "FASTQ_QUAL_LEN")
        assert len(warn) == 1 and "piece %s" % m.group(1) in warn[0], warn


def test_default_is_unchanged(reads, paf, tmpdir_s):
    """MA_FASTX_STREAM unset or 0: a gzip reads file takes the host reader, with its warning, as before"""
    fn = _write(tmpdir_s, "g.fq.gz", _file(reads, "fq"), gz=True)
    for val in (None, "0"):
        e = dict(os.environ, MA_PIPE_TIMING="1")
        e.pop("MA_FASTX_STREAM", None)
        if val:
            e["MA_FASTX_STREAM"] = val
        g = subprocess.run([ma.CLI_PATH, "-f", fn, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=600)
        log = g.stderr.decode(errors="replace")
        assert g.returncode == 0 and "reader=host reason=9" in log and log.count("[W::ma_ug_seq]") == 1, log[-2000:]
