"""The reads file of `miniasm -f` read on the device (csrc/useq.hip, host/unitig_gfa.c: ma_ug_seq): FASTA/FASTQ text in HBM -> line index -> form check ->
name lookup -> placement.  Every end-to-end case is compared byte for byte with the unmodified reference binary (oracle/_ref/miniasm_ref), through the CLI and
through the drop-in, once with the device reader allowed and once with MA_FASTX_HOST=1; the `[T::ug_seq]` line says which reader ran and why, so a regular
input that falls back -- or an irregular one that does not, or falls back for another reason -- fails.  The stage tests drive the C ABI through the ctypes harness
against a small Python model of the regular form, on every size edge the kernels branch on (16-byte pieces and 1 KiB granules of the census, 64 lanes, 256-line
chunks of the wrapped placement, the three forms of the device-wide scan)."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import miniasm_amd as ma
import refapi as R

pytestmark = pytest.mark.gpu

needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not built")


# ------------------------------------------------------------------------------------------------ inputs
def _bases(rs, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rs.randint(0, len(alphabet), n)].tobytes()


def _wrap(seq, w):
    return b"\n".join(seq[i:i + w] for i in range(0, len(seq), w)) if w and len(seq) > w else seq


def _record(name, seq, fmt, wrap=0):
    if fmt == "fq":
        return b"@" + name + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"
    return b">" + name + b"\n" + _wrap(seq, wrap) + b"\n"


@pytest.fixture(scope="module")
def paf(tmpdir_s):
    return R.pafgen(os.path.join(tmpdir_s, "fastx.paf"), 400, 12000, 23, ["-L", "uniform"])


def _reads_of(paf, seed):
    lens = {}
    for ln in open(paf, "rb"):
        f = ln.split(b"\t")
        lens.setdefault(f[0], int(f[1]))
        lens.setdefault(f[5], int(f[6]))
    rs = np.random.RandomState(seed)
    return {nm: _bases(rs, n) for nm, n in lens.items()}


@pytest.fixture(scope="module")
def reads(paf):
    """name -> bases, in the PAF's order of first appearance, with the PAF's lengths"""
    return _reads_of(paf, 5)


@pytest.fixture(scope="module")
def paf_b(tmpdir_s):
    """a second PAF, for `-b -S 5 -p ug`: with both strands kept apart and five cleaning rounds the unitigs of many inputs (the one above among them) hold a read
    twice, and the reference stops at its assertion asm.c:255 there; this one it answers"""
    return R.pafgen(os.path.join(tmpdir_s, "fastx_b.paf"), 300, 9000, 2)


def _write(tmpdir_s, tag, data):
    p = os.path.join(tmpdir_s, "fastx_%s" % tag)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _file(reads, fmt, wrap=0):
    return b"".join(_record(nm, s, fmt, wrap) for nm, s in reads.items())


# ------------------------------------------------------------------------------------------------ running
def _run(binary, args, reads_fn, paf, host=False, stdin=None):
    env = dict(os.environ, MA_PIPE_TIMING="1")
    env.pop("MA_FASTX_HOST", None)
    if host:
        env["MA_FASTX_HOST"] = "1"
    r = subprocess.run([binary] + list(args) + ["-f", reads_fn, paf], stdin=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode == 0, "%s: exit %d: %s" % (binary, r.returncode, r.stderr.decode(errors="replace")[-2000:])
    log = r.stderr.decode(errors="replace")
    t = [ln for ln in log.splitlines() if ln.startswith("[T::ug_seq]")]
    assert len(t) == 1, "one [T::ug_seq] line expected:\n" + log[-2000:]
    m = re.search(r"reader=(\w+)", t[0])
    why = re.search(r"reason=(\d+)", t[0])
    warn = [ln for ln in log.splitlines() if ln.startswith("[W::ma_ug_seq]")]
    assert len(warn) == (1 if m.group(1) == "host" else 0), "a fallback prints exactly one [W::ma_ug_seq] line:\n" + log[-2000:]
    return r.stdout, log, m.group(1), ma.FASTX_REASONS[int(why.group(1))] if why else "OK"


def _check(reads_fn, paf, args=(), reader="device", reason="OK", stdin_data=None):
    """CLI and drop-in, with and without MA_FASTX_HOST=1, equal the reference; the reader and the reason are the expected ones"""
    def inp():
        return open(stdin_data, "rb") if stdin_data else None
    r = subprocess.run([R.REF_BIN] + list(args) + ["-f", reads_fn, paf], stdin=inp(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    ref_out, ref_cnt = r.stdout, R.counters(r.stderr.decode(errors="replace"))
    assert b"\nS\t" in b"\n" + ref_out, "the case is supposed to have unitigs"
    for binary in (ma.CLI_PATH, R.DROPIN_BIN):
        for host in (False, True):
            out, log, got_reader, got_reason = _run(binary, args, reads_fn, paf, host, inp())
            what = "%s %s%s" % (os.path.basename(binary), " ".join(args), " MA_FASTX_HOST=1" if host else "")
            assert out == ref_out, what + ": output differs from the reference"
            assert [x for x in R.counters(log) if not x.startswith("main: Version")] == ref_cnt, what + ": log counters differ"
            if host:
                assert (got_reader, got_reason) == ("host", "FORCED"), what
            else:
                assert (got_reader, got_reason) == (reader, reason), "%s: reader %s (%s), expected %s (%s)" % (what, got_reader, got_reason, reader, reason)
    return ref_out


# ------------------------------------------------------------------------------------------------ end to end: regular inputs
REGULAR = {"fastq": ("fq", 0), "fasta": ("fa", 0), "fasta_wrap60": ("fa", 60), "fasta_wrap1000": ("fa", 1000)}


@needs_ref
@pytest.mark.parametrize("form", list(REGULAR))
def test_regular_file_is_read_on_the_device(form, reads, paf, tmpdir_s):
    """no case of this list may fall back (the cap is zero); fails without the device reader: the [T::ug_seq] line does not exist there"""
    fmt, wrap = REGULAR[form]
    fn = _write(tmpdir_s, form, _file(reads, fmt, wrap))
    out = _check(fn, paf)
    assert not out.split(b"\n")[0].split(b"\t")[2].startswith(b"*")


@needs_ref
@pytest.mark.parametrize("args", [["-R"], ["-1", "-2"], ["-S", "5", "-p", "ug"], ["-b", "-S", "4", "-p", "ug"]], ids=lambda a: "".join(a))
@pytest.mark.parametrize("form", ["fastq", "fasta_wrap60"])
def test_options_that_change_the_placement(form, args, reads, paf, tmpdir_s):
    """-1 -2: no read selection, whole records (the reverse strand counts from the record's end); -R, -S 5 -p ug, -b -S 4 -p ug: other unitigs"""
    fmt, wrap = REGULAR[form]
    _check(_write(tmpdir_s, form, _file(reads, fmt, wrap)), paf, args)


@needs_ref
@pytest.mark.parametrize("form", ["fastq", "fasta_wrap60"])
def test_asymmetric_graph_unitigs_from_text(form, paf_b, tmpdir_s):
    """-b -S 5 -p ug: the unitigs of the graph whose two strands were cleaned apart, their bases placed from the text"""
    fmt, wrap = REGULAR[form]
    out = _check(_write(tmpdir_s, "b_" + form, _file(_reads_of(paf_b, 6), fmt, wrap)), paf_b, ["-b", "-S", "5", "-p", "ug"])
    assert out.count(b"\nS\t") + out.startswith(b"S\t") >= 5


def _readgen():
    """tools/readgen.c -> miniasm_amd/bin/readgen (the build makes it; a tree built before it existed gets it here)"""
    exe = os.path.join(os.path.dirname(ma.PAFGEN_PATH), "readgen")
    if not os.path.exists(exe):
        root = os.path.dirname(os.path.dirname(os.path.abspath(ma.__file__)))
        subprocess.run(["gcc", "-O2", "-Wall", "-o", exe, os.path.join(root, "tools", "readgen.c")], check=True)
    return exe


@needs_ref
@pytest.mark.parametrize("opts", [["-q"], [], ["-w", "60", "-x", "0.1", "-e", "50"]], ids=["fastq", "fasta", "fasta_wrap60_left_out_and_extra"])
def test_reads_file_made_by_readgen(opts, paf, tmpdir_s):
    """the generator of the timing tool: the PAF's names in the order of first appearance with the lengths seen first; -x leaves reads out, -e adds reads the PAF never names"""
    fn = os.path.join(tmpdir_s, "fastx_readgen_%d" % len(opts))
    subprocess.run([_readgen()] + opts + ["-s", "7", "-o", fn, paf], check=True, stderr=subprocess.DEVNULL)
    text = open(fn, "rb").read()
    _, recs = _model(text)
    lens = {}
    for ln in open(paf, "rb"):
        f = ln.split(b"\t")
        lens.setdefault(f[0], int(f[1]))
        lens.setdefault(f[5], int(f[6]))
    named = [(nm, len(s)) for nm, s in recs if nm in lens]
    if "-x" not in opts:
        assert named == list(lens.items()) and len(recs) == len(lens)
    else:
        order = list(lens)
        assert 0 < len(named) < len(lens) and len(recs) - len(named) == 50 and all(lens[nm] == n for nm, n in named)
        assert [order.index(nm) for nm, _ in named] == sorted(order.index(nm) for nm, _ in named)
    assert set(b"".join(s for _, s in recs)) <= set(b"ACGT")
    _check(fn, paf)


# ------------------------------------------------------------------------------------------------ end to end: irregular inputs, one per reason
def _irregular(reads, what):
    names = list(reads)
    if what == "crlf":
        return _file(reads, "fa").replace(b"\n", b"\r\n"), "CR"
    if what == "leading_blank":
        return b"\n" + _file(reads, "fa"), "FIRST_BYTE"
    if what == "fasta_at_line":
        return _file(reads, "fa", 60) + b">odd\nACGT\n@CGT\n", "FASTA_LINE_START"
    if what == "fastq_two_line_seq":
        s = reads[names[3]]
        alt = b"@" + names[3] + b"\n" + s[:50] + b"\n" + s[50:] + b"\n+\n" + b"I" * len(s) + b"\n"
        return b"".join(alt if nm == names[3] else _record(nm, q, "fq") for nm, q in reads.items()), "FASTQ_SHAPE"
    if what in ("fastq_short_qual", "fastq_long_qual"):  # the third record: the reference's reader returns -2 there and the file ends for it (asm.c:262)
        s = reads[names[2]]
        q = b"I" * (len(s) - 5 if what == "fastq_short_qual" else len(s) + 5)
        alt = b"@" + names[2] + b"\n" + s + b"\n+\n" + q + b"\n"
        return b"".join(alt if nm == names[2] else _record(nm, b, "fq") for nm, b in reads.items()), "FASTQ_QUAL_LEN"
    if what == "nul_in_a_name":  # the reference's names are C strings (asm.c:266): `name\0x` IS `name` for it, and this later record wins
        rs = np.random.RandomState(29)
        return _file(reads, "fa", 60) + b"".join(_record(nm + b"\0x", _bases(rs, len(reads[nm])), "fa", 60) for nm in names[::7]), "NUL_BYTE"
    raise KeyError(what)


@needs_ref
@pytest.mark.parametrize("what", ["crlf", "leading_blank", "fasta_at_line", "fastq_two_line_seq", "fastq_short_qual", "fastq_long_qual", "nul_in_a_name"])
def test_irregular_file_takes_the_host_reader(what, reads, paf, tmpdir_s):
    data, reason = _irregular(reads, what)
    _check(_write(tmpdir_s, what, data), paf, reader="host", reason=reason)


@needs_ref
def test_gzip_and_stdin_take_the_host_reader(reads, paf, tmpdir_s):
    data = _file(reads, "fq")
    gz = os.path.join(tmpdir_s, "fastx_reads.fq.gz")
    with gzip.open(gz, "wb") as f:
        f.write(data)
    _check(gz, paf, reader="host", reason="NOT_PLAIN")
    _check("-", paf, reader="host", reason="NOT_PLAIN", stdin_data=_write(tmpdir_s, "stdin.fq", data))


def test_short_read_takes_the_host_reader(reads, paf, tmpdir_s):
    """wanted reads with fewer bases than their placement needs, under -1 -2 (the reference reads outside its buffer there, so it is no yardstick; the host reader's
    'missing bases stay N' is: tests/test_gpu_cli.py::test_cli_reads_file_shorter_than_the_paf_says) -- the device path must hand such a file over"""
    short = {nm: (s[:40] if k % 2 == 0 else s) for k, (nm, s) in enumerate(reads.items())}
    for fmt, wrap in (("fq", 0), ("fa", 60)):
        fn = _write(tmpdir_s, "short_%s" % fmt, _file(short, fmt, wrap))
        out, _, reader, reason = _run(ma.CLI_PATH, ["-1", "-2"], fn, paf)
        assert (reader, reason) == ("host", "SHORT_READ")
        forced, _, _, _ = _run(ma.CLI_PATH, ["-1", "-2"], fn, paf, host=True)
        assert out == forced and b"N" in b"".join(l.split(b"\t")[2] for l in out.split(b"\n") if l.startswith(b"S\t"))


# ------------------------------------------------------------------------------------------------ end to end: semantics
def _semantic(reads, what, fmt, wrap):
    rs = np.random.RandomState(17)
    names = list(reads)
    rec = lambda nm, s: _record(nm, s, fmt, wrap)  # noqa: E731
    body = [rec(nm, s) for nm, s in reads.items()]
    if what == "duplicates_last_wins":  # wrong bases first, the right ones later; and the right ones first, other bases of the same length last
        head = [rec(nm, _bases(rs, len(reads[nm]))) for nm in names[::5]]
        tail = [rec(nm, _bases(rs, len(reads[nm]))) for nm in names[1::9]]
        return b"".join(head + body + tail)
    if what == "comments":
        return b"".join(_record(nm + (b" a comment\tx" if k % 2 else b"\tcomment no %d" % k), s, fmt, wrap) for k, (nm, s) in enumerate(reads.items()))
    if what == "prefix_names":  # records whose names are prefixes / extensions of wanted names, before and after them
        pre = [rec(nm[:-1], _bases(rs, len(reads[nm]))) for nm in names[::3] if nm[:-1] not in reads]
        ext = [rec(nm + b"0", _bases(rs, len(reads[nm]))) for nm in names[::4] if nm + b"0" not in reads]
        return b"".join(pre + body + ext)
    if what == "empty_name":
        return rec(b"", b"ACGTACGT") + b"".join(body[:50]) + rec(b" only a comment", b"TTTT") + b"".join(body[50:])
    if what == "missing_reads":
        return b"".join(b for k, b in enumerate(body) if k % 10 != 3)
    if what == "unnamed_extras":
        return b"".join(rec(b"extra%d" % k, _bases(rs, 700)) + b for k, b in enumerate(body))
    if what == "letters":  # lower case, IUPAC and bytes >= 128 (the reverse strand turns those into N, asm.c:281)
        alpha = b"ACGTacgtRYKMSWBDHVNrykmswbdhvnUu" + bytes([128, 200, 255]) + b"*-."
        return b"".join(rec(nm, _bases(rs, len(s), alpha)) for nm, s in reads.items())
    if what == "no_final_newline":
        return b"".join(body)[:-1]
    if what == "single_record":
        return body[len(body) // 2]
    raise KeyError(what)


SEMANTICS = ["duplicates_last_wins", "comments", "prefix_names", "empty_name", "missing_reads", "unnamed_extras", "letters", "no_final_newline", "single_record"]


@needs_ref
@pytest.mark.parametrize("what", SEMANTICS)
@pytest.mark.parametrize("form", ["fastq", "fasta_wrap60"])
def test_semantics_match_the_reference_on_the_device(form, what, reads, paf, tmpdir_s):
    fmt, wrap = REGULAR[form]
    _check(_write(tmpdir_s, "%s_%s" % (what, form), _semantic(reads, what, fmt, wrap)), paf)


@needs_ref
def test_wanted_read_first_and_last(reads, paf, tmpdir_s):
    """the file holds exactly the reads the unitigs take, one of them first and one of them last"""
    out, _ = R.run_cli(R.REF_BIN, ["-p", "ug"], paf)
    used = [ln.split(b"\t")[3].rsplit(b":", 1)[0] for ln in out.split(b"\n") if ln.startswith(b"a\t")]
    assert len(used) > 2
    only = {nm: reads[nm] for nm in used}
    for form in ("fastq", "fasta_wrap60"):
        fmt, wrap = REGULAR[form]
        _check(_write(tmpdir_s, "only_%s" % form, _file(only, fmt, wrap)), paf)


# ------------------------------------------------------------------------------------------------ stage tests against a Python model
def _model(text):
    """the regular form in ten lines: line starts, record names, record bases"""
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    starts = np.cumsum([0] + [len(l) + 1 for l in lines])
    if text[:1] == b">":
        heads = [i for i, l in enumerate(lines) if l[:1] == b">"] + [len(lines)]
        recs = [(lines[a], b"".join(lines[a + 1:b])) for a, b in zip(heads, heads[1:])]
    else:
        recs = [(lines[i], lines[i + 1]) for i in range(0, len(lines), 4)]
    return starts, [(re.split(rb"[ \t\v\f]", h[1:])[0], s) for h, s in recs]


COMP = bytes.maketrans(b"ABCDGHKMRTUVYabcdghkmrtuvy`", b"TVGHCDMKYAABRtvghcdmkyaabr@")


def _place_model(recs, wanted, arena_bytes):
    arena = bytearray(b"N" * arena_bytes)
    last = {nm: s for nm, s in recs if nm}
    for w in wanted:
        if w["name"] not in last:
            continue
        seq = last[w["name"]]
        s, e = (w["s"], w["e"]) if w.get("e") is not None else (0, len(seq))
        part = seq[s:e]
        n = min(w["len"], len(part))
        piece = part[:n] if not w["rev"] else bytes(78 if c >= 128 else c for c in part[::-1][:n]).translate(COMP)
        arena[w["dst_off"]:w["dst_off"] + n] = piece
    return bytes(arena)


def _stage(ctx, text, wanted=None, arena_bytes=0):
    starts, recs = _model(text)
    ctx.fastx_load(text)
    info = ctx.fastx_index()
    assert info["regular"] and info["reason"] == "OK", info
    assert info["n_lines"] == len(starts) - 1 and info["n_records"] == len(recs) and info["n_cr"] == 0
    assert info["format"] == ("fasta" if text[:1] == b">" else "fastq")
    got = ctx.fastx_line_starts(info["n_lines"])
    assert np.array_equal(got, starts.astype(np.uint64)), "line starts differ from the model"
    assert ctx.fastx_names(text, len(recs)) == [nm for nm, _ in recs], "names differ from the model"
    if wanted is not None:
        arena, n_matched, n_dup, n_short = ctx.useq_place_text(arena_bytes, wanted)
        assert n_short == 0
        have = [nm for nm, _ in recs if nm]
        assert n_matched == len({w["name"] for w in wanted} & set(have))
        assert n_dup == sum(have.count(w["name"]) - 1 for w in wanted if w["name"] in have)
        assert arena == _place_model(recs, wanted, arena_bytes), "placement differs from the model"
    ctx.fastx_release()
    return info


def _wanted_for(recs, rs, whole):
    """every record wanted once: forward and reverse alternate, sub-intervals and lengths drawn inside the read (or the whole read: `whole`)"""
    out, at = [], 0
    for k, (nm, s) in enumerate(recs):
        if not nm or any(w["name"] == nm for w in out):
            continue
        n = len(s)
        if whole:
            a, b, ln = 0, None, int(rs.randint(0, n + 1))
        else:
            a = int(rs.randint(0, n + 1))
            b = int(rs.randint(a, n + 1))
            ln = int(rs.randint(0, b - a + 1))
        if k % 5 == 0:  # a read that needs exactly all of its bases
            a, b, ln = (0, None, n) if whole else (0, n, n)
        out.append(dict(name=nm, dst_off=at, len=ln, rev=k % 2 == 1, s=a, e=b))
        at += ln + 1
    return out, at


LINE_LENS = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
NAME_LENS = [1, 8, 9, 64, 255]


@pytest.mark.parametrize("whole", [False, True], ids=["sub", "whole"])
@pytest.mark.parametrize("form", ["fastq", "fasta", "fasta_wrapped"])
def test_size_edges_of_lines_and_names(form, whole, gpu_ctx):
    """sequence lines of 0 .. 4097 bytes (the 16-byte pieces, the 64 lanes and the 1 KiB granules of the census; 256 threads of the copy), names of 1 .. 255 bytes,
    wrapped records of 1, 2, 255, 256, 257 and 600 lines (the 256-line chunks of the wrapped placement), reads that need exactly all of their bases"""
    rs = np.random.RandomState(3)
    recs, k = [], 0
    for a, ll in enumerate(LINE_LENS):
        for nl in NAME_LENS:
            recs.append((bytes([97 + a]) if nl == 1 else (b"%d_" % k).ljust(nl, b"n"), _bases(rs, ll, b"ACGTNacgtRY" + bytes([129, 255]))))
            k += 1
    assert sorted({len(nm) for nm, _ in recs}) == NAME_LENS and len({nm for nm, _ in recs}) == len(recs)
    if form == "fasta_wrapped":
        text = b""
        for (nm, s), w in zip(recs, [1, 7, 60, 61, 64, 1000] * len(recs)):
            text += _record(nm, s, "fa", w)
        for n_lines in (1, 2, 255, 256, 257, 600):  # records of that many sequence lines, an empty line among them
            s = _bases(rs, n_lines * 13 - 5)
            recs.append((b"lines%d" % n_lines, s))
            text += b">lines%d\tc\n" % n_lines + _wrap(s, 13).replace(b"\n", b"\n\n", 1) + b"\n"
        _, recs = _model(text)
    else:
        text = b"".join(_record(nm, s, "fq" if form == "fastq" else "fa") for nm, s in recs)
    wanted, arena = _wanted_for(recs, rs, whole)
    info = _stage(gpu_ctx, text, wanted, arena)
    assert info["n_records"] == len(recs)
    _stage(gpu_ctx, text[:-1], wanted, arena)  # the same without the final newline


def test_duplicates_prefixes_and_missing_names_at_stage_level(gpu_ctx):
    rs = np.random.RandomState(9)
    recs = [(b"r%d" % (k % 37), _bases(rs, 300)) for k in range(100)] + [(b"", b"ACGT"), (b"r1x", _bases(rs, 300)), (b"r", _bases(rs, 300))]
    text = b"".join(_record(nm + (b" c" if k % 3 == 0 else b""), s, "fa", 70) for k, (nm, s) in enumerate(recs))
    _, recs = _model(text)
    wanted, arena = _wanted_for(recs, rs, False)
    wanted.append(dict(name=b"absent", dst_off=arena, len=40, rev=False, s=0, e=40))
    _stage(gpu_ctx, text, wanted, arena + 41)


def test_short_record_is_reported_and_nothing_is_placed(gpu_ctx):
    text = b">a\nACGTACGT\n>b\nACGT\n>b\nACGTACGTAC\n"
    gpu_ctx.fastx_load(text)
    assert gpu_ctx.fastx_index()["regular"]
    wanted = [dict(name=b"a", dst_off=0, len=8, rev=False, s=0, e=8), dict(name=b"b", dst_off=8, len=6, rev=True, s=2, e=8)]  # the first `b` holds 4 < 8 bases
    arena, n_matched, n_dup, n_short = gpu_ctx.useq_place_text(14, wanted)
    assert (n_matched, n_dup, n_short) == (2, 1, 1) and arena == b"N" * 14
    gpu_ctx.fastx_release()


@pytest.mark.parametrize("text,reason", [(b">a\r\nAC\r\n", "CR"), (b"\n>a\nAC\n", "FIRST_BYTE"), (b"ACGT\n", "FIRST_BYTE"), (b">a\nAC\n+C\n", "FASTA_LINE_START"),
                                         (b">a\nAC\n@b\nAC\n", "FASTA_LINE_START"), (b"@a\nAC\n+\nII\n@b\nAC\n+\n", "FASTQ_SHAPE"), (b"@a\nAC\nGT\n+\nIIII\n@b\nA\n+\n", "FASTQ_SHAPE"),
                                         (b"@a\n>C\n+\nII\n", "FASTQ_SHAPE"), (b"@a\nAC\n+\nI\n", "FASTQ_QUAL_LEN"), (b"@a\nAC\n+\nIII\n", "FASTQ_QUAL_LEN"),
                                         (b">a\0b\nAC\n", "NUL_BYTE"), (b"@a\nA\0\n+\nII\n", "NUL_BYTE"), (b">a\n" + b"A" * (1 << 24) + b"\nAC\n", "LONG_LINE"),
                                         (b">a\nAC\n" + b"A" * (1 << 24) + b"\n>b\nAC\n", "LONG_LINE")], ids=lambda v: None if isinstance(v, str) else "%d_bytes" % len(v))
def test_form_check_reasons(text, reason, gpu_ctx):
    gpu_ctx.fastx_load(text)
    info = gpu_ctx.fastx_index()
    assert not info["regular"] and info["reason"] == reason, info
    gpu_ctx.fastx_release()


def test_long_line_alone_in_its_record_is_regular(gpu_ctx):
    """16 MiB on ONE line is copied without the 32-bit sums of the wrapped placement; one byte less is fine in a wrapped record too"""
    rs = np.random.RandomState(41)
    big, less = _bases(rs, 1 << 24), _bases(rs, (1 << 24) - 1)
    text = b">one\n" + big + b"\n>two\n" + less + b"\nACGTT\n>three\nAC\n"
    wanted = [dict(name=b"one", dst_off=0, len=100, rev=True, s=0, e=None), dict(name=b"two", dst_off=100, len=50, rev=True, s=(1 << 24) - 30, e=(1 << 24) + 4),
              dict(name=b"three", dst_off=150, len=2, rev=False, s=0, e=2)]
    _stage(gpu_ctx, text, wanted, 152)


def _scan_form(n):
    return 0 if n <= 2048 else 1 if n <= 524288 else 2


@pytest.mark.parametrize("n_records,form", [(1000, 0), (200000, 1), (262200, 2)])
def test_line_counts_on_every_form_of_the_scan(n_records, form, gpu_ctx):
    """FASTA: the header flags of all lines are scanned (record numbers): <= 2048 lines one tile, <= 524 288 the chained launch, above the three-phase scan.
    The index scans twice -- the newline counts of the 1 KiB granules, then the header flags of the lines -- and nothing else: the increments are exactly those two."""
    rs = np.random.RandomState(n_records)
    seqs = _bases(rs, 8 * n_records)
    recs = [(b"q%d" % k, seqs[8 * k:8 * k + 5 + k % 4]) for k in range(n_records)]
    text = b"".join(b">%s\n%s\n" % r for r in recs)
    n_lines = 2 * n_records
    assert (n_lines <= 2048, 2048 < n_lines <= 524288, n_lines > 524288) == (form == 0, form == 1, form == 2)
    before = gpu_ctx.scan_forms()
    pick = sorted(set(int(x) for x in rs.randint(0, n_records, 300)) | {0, n_records - 1})
    wanted = [dict(name=recs[k][0], dst_off=8 * j, len=len(recs[k][1]), rev=j % 2 == 1, s=0, e=None) for j, k in enumerate(pick)]
    gpu_ctx.fastx_load(text)
    info = gpu_ctx.fastx_index()
    assert info["regular"] and info["n_lines"] == n_lines and info["n_records"] == n_records
    after = gpu_ctx.scan_forms()
    expect = [0, 0, 0]
    expect[_scan_form((len(text) + 1023) // 1024)] += 1
    expect[form] += 1
    assert [int(a) - int(b) for a, b in zip(after, before)] == expect, "granule scan + header scan over %d lines (form %d): %s -> %s" % (n_lines, form, before, after)
    starts = gpu_ctx.fastx_line_starts(n_lines)
    assert np.array_equal(starts, np.cumsum([0] + [len(x) + 1 for r in recs for x in (b">" + r[0], r[1])]).astype(np.uint64))
    arena, n_matched, n_dup, n_short = gpu_ctx.useq_place_text(8 * len(pick), wanted)
    assert (n_matched, n_dup, n_short) == (len(pick), 0, 0)
    assert arena == _place_model(recs, wanted, 8 * len(pick))
    gpu_ctx.fastx_release()
