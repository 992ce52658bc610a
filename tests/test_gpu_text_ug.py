"""The unitig GFA (-p ug, with -f sequences) written on the device (csrc/text_dev.hpp over csrc/text_core.h: the ug kind).
Stage cases through Ctx.text_format_ug -- hand-made unitigs, links, counts, names, kept intervals, sequences; the yardstick is the Python model of
tests/ugtextmodel.py, byte for byte, and the report: lines, bytes, sequence bytes, slabs, records that took the slow path -- at every count, chunk and slab edge
the kernels branch on; then the command line with MA_TEXT_DEVICE=1 against the reference binary (against MA_TEXT_DEVICE=0 where oracle/_ref is not built), with
and without a reads file, and the memory sink."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import miniasm_amd as ma
import refapi as R
import textmodel as TM
import ugtextmodel as UM

pytestmark = pytest.mark.gpu

NONE = UM.NONE
SLABS = (None, 1, 7, 64, 100)


def short_names(n, seed=3):
    rnd = np.random.RandomState(seed)
    return [b"n%d_" % i + b"x" * rnd.randint(0, 12) for i in range(n)]


def check(ctx, units, links, counts, names, sub=None, seqs=None, slab=None, want_slow=None):
    text, info = ctx.text_format_ug(units, links, counts, names, sub=sub, seqs=seqs, slab=slab)
    chunk = info["seq_chunk"]
    assert chunk >= 16
    recs = UM.records(units, links, counts, names, sub, seqs, chunk)
    what = "%d unitigs, %d links, slab %r, %s" % (len(units), len(links), slab, "sequences" if seqs is not None else "no sequences")
    assert info["road"] == "device" and info["reason"] == "OK" and info["kind"] == "ug", what
    assert text == b"".join(recs), what + ": the text differs from the model"
    assert info["n_lines"] == text.count(b"\n") and info["text_bytes"] == len(text) and info["n_records"] == len(recs), what
    assert info["n_seq_bytes"] == (sum(len(s) for s in seqs) if seqs is not None else 0), what
    max_name = max([len(x) for x in names] + [0])
    eff = info["slab_records"]
    assert eff == UM.slab_records(slab, max_name, chunk if seqs is not None else 0) and info["max_name"] == max_name
    assert info["n_slabs"] == (len(recs) + eff - 1) // eff
    if slab is not None and len(recs) > slab:
        assert info["n_slabs"] >= 2
    if want_slow is None:  # the model's wave arithmetic over the records' lengths (None: a wave is too close to the tile to call)
        want_slow = TM.slow_lines([len(r) for r in recs], eff)
    if want_slow is not None:
        assert info["n_slow_lines"] == want_slow, what
    return text, info


# ---- 1. counts at the wave edge
@pytest.mark.parametrize("U,n_links", [(0, 0), (1, 1), (2, 63), (63, 64), (64, 65), (65, 1000)])
def test_counts_at_the_wave_edge(gpu_ctx, U, n_links):
    """0, 1, 2, 63, 64, 65 unitigs of 1, 2, 63, 64, 65 or 200 members, linear and circular mixed, with 0, 1, 63, 64, 65, 1000 links whose ends name both kinds, with
    and without kept intervals, under the default slab and slabs of 1, 7, 64 and 100 records"""
    rnd = np.random.RandomState(100 + U)
    names = short_names(37)
    units = UM.make_units(U, len(names), rnd)
    links = UM.make_links(n_links, max(U, 1), rnd)
    counts = [(int(rnd.randint(0, 5)), int(rnd.randint(0, 5))) for _ in units]
    sub = UM.make_sub(len(names), rnd)
    if U >= 63:
        letters = {(units[int(a["ul"]) >> 33][1] == NONE, units[int(a["v"]) >> 1][1] == NONE) for a in links}
        assert len(letters) == 4, "both letters at both ends of a link"
    for slab in SLABS:
        check(gpu_ctx, units, links, counts, names, sub, None, slab)
        if slab != 1:
            check(gpu_ctx, units, links, counts, names, None, None, slab)
    if U == 0:
        assert check(gpu_ctx, units, links, counts, names, None, None, None)[0] == b""


# ---- 2. sequences at the chunk edge
def _chunk(ctx):
    return ctx.text_format_ug([], [], [], [b"a"])[1]["seq_chunk"]


def test_sequences_at_the_chunk_edge(gpu_ctx):
    """unitigs of 0, 1, C - 1, C, C + 1, 2 C, 64 C - 1, 64 C, 64 C + 1 and 5 * 64 C + 17 bases (C from the report), circular ones among them; slabs that cut inside a
    unitig's chunks, between its head and its first chunk and between its tail and its first a line (a slab of one record cuts everywhere)"""
    c = _chunk(gpu_ctx)
    lens = [0, 1, c - 1, c, c + 1, 2 * c, 64 * c - 1, 64 * c, 64 * c + 1, 5 * 64 * c + 17]
    rnd = np.random.RandomState(7)
    names = short_names(37)
    units = UM.make_units(len(lens), len(names), rnd, members=(1, 2, 3, 70), lens=lens)
    assert {u[1] == NONE for u in units} == {True, False}
    seqs = [UM.make_seq(n, rnd) for n in lens]
    links = UM.make_links(20, len(units), rnd)
    counts = [(1, 2)] * len(units)
    sub = UM.make_sub(len(names), rnd)
    for slab in (None, 1, 3, 7, 64, 100, 67):
        check(gpu_ctx, units, links, counts, names, sub if slab != 3 else None, seqs, slab)


@pytest.mark.parametrize("first", range(16))
def test_sequences_on_every_residue_mod_16(gpu_ctx, first):
    """16 unitigs, the first of 0 ... 15 bases: where a unitig's bases start in the arena and where they land in the text meet every pair of residues mod 16"""
    c = _chunk(gpu_ctx)
    rnd = np.random.RandomState(first)
    lens = [first] + [c + 3 * k + (k % 5) * c for k in range(1, 16)]
    names = short_names(20)
    units = UM.make_units(16, len(names), rnd, members=(1, 2), lens=lens, circ_every=4)
    seqs = [UM.make_seq(n, rnd) for n in lens]
    src = np.cumsum([0] + [n + 1 for n in lens[:-1]]) % 16
    assert len(set(src.tolist())) >= 8
    check(gpu_ctx, units, [], [(0, 0)] * 16, names, None, seqs, None)
    check(gpu_ctx, units, [], [(0, 0)] * 16, names, None, seqs, 50)


# ---- 3. value edges
def test_value_edges_in_every_field(gpu_ctx):
    """member low words and u_len over 0, 9, 10, ..., 2^31 - 1, 2^31, 2^32 - 1; the offset l wrapping through 2^32; ol, the arc length, the counts and the kept
    intervals over their edge lists"""
    n = len(UM.E32)
    names = [b"r" * (1 + i % 5) + b"%d" % i for i in range(2 * n)]
    sub = np.zeros(len(names), dtype=ma.SUB_DT)
    for i in range(len(names)):
        sub["sdel"][i] = UM.S_PLUS1[i % len(UM.S_PLUS1)]
        sub["e"][i] = UM.E32[(i + 5) % n]
    units, counts = [], []
    for i in range(n):  # unitig i: length edge i, three members whose low words are edges, alternately circular
        mem = [(((2 * i + k) % len(names)) << 33) | ((i + k) & 1) << 32 | UM.E32[(i + 3 * k) % n] for k in range(3)]
        if i % 2:
            units.append((UM.E32[i], NONE, NONE, mem))
        else:
            units.append((UM.E32[i], (i % len(names)) << 1 | (i >> 1 & 1), ((i + 7) % len(names)) << 1 | (i >> 2 & 1), mem))
        counts.append((UM.E32[(i + 1) % n], UM.E32[(i + 2) % n]))
    units.append((5, 0, 3, [(0 << 33) | 2**31, (1 << 33) | 1 << 32 | 2**31, (2 << 33) | 5, (3 << 33) | 9]))  # l = 0, 2^31, 0, 5
    counts.append((0, 0))
    links = np.zeros(2 * n, dtype=ma.ARC_DT)
    for i in range(2 * n):
        links["ul"][i] = (((i % len(units)) << 1 | (i & 1)) << 32) | UM.E32[i % n]
        links["v"][i] = ((i * 7 + 3) % len(units)) << 1 | (i >> 1 & 1)
        links["oldel"][i] = UM.E31[i % len(UM.E31)]
    for s in (sub, None):
        text, _ = check(gpu_ctx, units, links, counts, names, s, None, None)
        check(gpu_ctx, units, links, counts, names, s, None, 7)
        assert b"\t-2147483648\t" in text and b"2147483647" in text and b"SD:i:-1\n" in text
        offs = [ln.split(b"\t")[2] for ln in text.splitlines() if ln.startswith(b"a\t" + UM.utg(len(units), False))]
        assert offs == [b"0", b"-2147483648", b"0", b"5"]


# ---- 4. the slow path
@pytest.mark.parametrize("where", ["a_line_next_to_chunks", "x_line", "first_member"])
def test_a_name_longer_than_the_tile_takes_the_slow_path(gpu_ctx, where):
    """one name of 13 000 bytes: the wave that holds its record does not fit the 12 KiB tile and writes straight to device memory -- chunk records included when
    they share that wave; the report counts the records of such waves"""
    c = _chunk(gpu_ctx)
    rnd = np.random.RandomState(5)
    names = short_names(50)
    names[17] = b"L" * 13000
    lens = [40 * c + 5, 3 * c, 7, 64 * c]
    units = UM.make_units(4, len(names), rnd, members=(3, 5, 70), lens=lens, circ_every=0)
    clean = lambda mem: [m if (m >> 33) != 17 else (m ^ (1 << 33)) for m in mem]  # noqa: E731  (the long name only where the case puts it)
    units = [(ln, st if (st >> 1) != 17 else st ^ 2, en if (en >> 1) != 17 else en ^ 2, clean(mem)) for ln, st, en, mem in units]
    ln, st, en, mem = units[0]
    if where == "a_line_next_to_chunks":
        mem[2] = (17 << 33) | 1 << 32 | 1234
        seqs = [UM.make_seq(n, rnd) for n in lens]
    elif where == "x_line":
        units[1] = (units[1][0], 17 << 1 | 1, units[1][2], units[1][3])
        seqs = None
    else:
        units[2][3][0] = (17 << 33) | 99
        seqs = [UM.make_seq(n, rnd) for n in lens]
    links = UM.make_links(30, 4, rnd)
    counts = [(1, 1)] * 4
    sub = UM.make_sub(len(names), rnd)
    for slab in (None, 64, 100):
        recs = UM.records(units, links, counts, names, sub, seqs, c)
        slow = TM.slow_lines([len(r) for r in recs], UM.slab_records(slab, 13000, c if seqs is not None else 0))
        assert slow is None or slow >= 1
        _, info = check(gpu_ctx, units, links, counts, names, sub, seqs, slab, want_slow=slow)
        assert info["n_slow_lines"] >= 1
        if where == "a_line_next_to_chunks" and slab is None:
            assert slow is not None and slow >= 40, "the chunk records in front of the a line share its wave"


# ---- 5. refusals
def test_refusals(gpu_ctx):
    rnd = np.random.RandomState(9)
    names = short_names(10)
    units = UM.make_units(3, len(names), rnd, members=(2,), lens=[300, 5, 0])
    seqs = [UM.make_seq(n, rnd) for n in (300, 5, 0)]
    bad = [seqs[0][:131] + b"\0" + seqs[0][132:], seqs[1], seqs[2]]
    text, info = gpu_ctx.text_format_ug(units, [], [(0, 0)] * 3, names, seqs=bad)
    assert text is None and (info["road"], info["reason"], info["kind"]) == ("host", "SEQ_NUL", "ug")
    text, info = gpu_ctx.text_format_ug(units, [], [(0, 0)] * 3, names, seqs=False)
    assert text is None and (info["road"], info["reason"]) == ("host", "NO_SEQ")
    text, info = gpu_ctx.text_format_ug(units, [], [(0, 0)] * 3, names, seqs=b"".join(x + b"N" for x in seqs) + b"N")  # an arena of another size than these unitigs'
    assert text is None and (info["road"], info["reason"]) == ("host", "NO_SEQ")
    check(gpu_ctx, units, [], [(0, 0)] * 3, names, None, seqs, None)  # and the same unitigs with a sound arena


# ---- 6. the command line
NOISY = dict(reads=4000, lines=90000, seed=63, extra=["-L", "uniform", "-d", "0.35", "-x", "0.03"])  # tests/test_gpu_cli.py: INPUTS["noisy"]
UG_ARGS = [[], ["-S6"], ["-S9"], ["-1", "-2"], ["-R"], ["-b", "-S5"], ["-b", "-S4"]]
_made = {}


def _noisy(tmpdir_s):
    if "paf" not in _made:
        _made["paf"] = R.pafgen(os.path.join(tmpdir_s, "text_ug_noisy.paf"), NOISY["reads"], NOISY["lines"], NOISY["seed"], NOISY["extra"])
    return _made["paf"]


def _readgen(tmpdir_s, paf, tag, opts):
    key = (paf, tag)
    if key not in _made:
        exe = os.path.join(os.path.dirname(ma.PAFGEN_PATH), "readgen")
        fn = os.path.join(tmpdir_s, "text_ug_reads_%s" % tag)
        subprocess.run([exe] + opts + ["-s", "7", "-o", fn, paf], check=True, stderr=subprocess.DEVNULL)
        _made[key] = fn
    return _made[key]


def _run(binary, args, paf, reads=None, **env):
    e = dict(os.environ, MA_PIPE_TIMING="1")
    for k in ("MA_TEXT_DEVICE", "MA_TEXT_SLAB"):
        e.pop(k, None)
    e.update({k: v for k, v in env.items() if v is not None})
    r = subprocess.run([binary] + list(args) + (["-f", reads] if reads else []) + [paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=900)
    assert r.returncode == 0, "%s %s: exit %d: %s" % (binary, " ".join(args), r.returncode, r.stderr.decode(errors="replace")[-2000:])
    return r.stdout, r.stderr.decode(errors="replace")


def _on_the_device(args, paf, reads=None, want_units=None, seq_bytes=None):
    """MA_TEXT_DEVICE=1 under the default slab and slabs of 1000 records: the reference's bytes (the host formatter's where oracle/_ref is not built); the log says `ug device`"""
    host_out, host_log = _run(ma.CLI_PATH, args + ["-p", "ug"], paf, reads, MA_TEXT_DEVICE="0")
    assert "[T::text]" not in host_log, "with the switch off a -p ug run prints what it always printed"
    if R.have_ref():
        want, _ = _run(R.REF_BIN, args + ["-p", "ug"], paf, reads)
        assert host_out == want
    else:
        want = host_out
    if want_units:
        assert (want.count(b"\nS\t") + want.startswith(b"S\t"), sum(1 for ln in want.split(b"\n") if ln[:2] == want_units[1])) == (want_units[0], want_units[2])
    for slab in (None, "1000"):
        out, log = _run(ma.CLI_PATH, args + ["-p", "ug"], paf, reads, MA_TEXT_DEVICE="1", MA_TEXT_SLAB=slab)
        assert out == want, "%s -p ug%s, MA_TEXT_SLAB=%s: bytes differ" % (" ".join(args), " -f" if reads else "", slab)
        m = re.search(r"^\[T::text\] ug (device|host)\b(.*)$", log, flags=re.M)
        assert m and m.group(1) == "device", log[-1500:]
        lines, nbytes, sbytes = (int(x) for x in re.search(r"(\d+) lines, (\d+) bytes, (\d+) sequence bytes", m.group(2)).groups())
        assert lines == out.count(b"\n") and nbytes == len(out)
        s_bases = sum(len(ln.split(b"\t")[2]) for ln in out.split(b"\n") if ln.startswith(b"S\t")) if reads else 0
        assert sbytes == s_bases
        if slab:  # without sequences a record is a line, but for the S record of a circular unitig, which is three
            n_slabs, records = int(re.search(r"(\d+) slabs of 1000 records", m.group(2)).group(1)), lines - 2 * out.count(b"\t+\t0M\n")
            assert n_slabs == (records + 999) // 1000 if not reads else n_slabs >= (records + 999) // 1000  # (and a head, chunks and a tail per unitig)
    return want, log


@pytest.mark.parametrize("args,shape", list(zip(UG_ARGS, [(1, b"a\t", 976), (1786, b"L\t", 8308), (227, b"L\t", 818), None, None, (1402, b"L\t", 11132), (2201, b"L\t", 24500)])),
                         ids=lambda a: " ".join(a) if isinstance(a, list) else None)
def test_cli_ug_written_on_the_device(args, shape, tmpdir_s):
    """-p ug alone and with -S6, -S9, -1 -2, -R, -b -S5, -b -S4 on the noisy input: every block has more than one wave of records"""
    want, _ = _on_the_device(list(args), _noisy(tmpdir_s), want_units=shape)
    assert len(want) > 1000


@pytest.mark.parametrize("args", [[], ["-S6"], ["-S9"]], ids=lambda a: " ".join(a) or "alone")
def test_cli_ug_with_a_reads_file(args, tmpdir_s):
    """-f with a FASTQ the device reader takes: the S lines carry the unitigs' bases, copied from the arena in HBM"""
    paf = _noisy(tmpdir_s)
    fq = _readgen(tmpdir_s, paf, "fq", ["-q"])
    want, log = _on_the_device(list(args), paf, fq)
    assert "reader=device" in log and "download 0.000 ms" in log
    assert max(len(ln.split(b"\t")[2]) for ln in want.split(b"\n") if ln.startswith(b"S\t")) > 7000


def test_cli_ug_with_a_fasta_and_a_gzipped_reads_file(tmpdir_s):
    """a FASTA through the device reader; the same file gzip'ed: the host reader fills the arena, and the text road is still the device's"""
    paf = _noisy(tmpdir_s)
    fa = _readgen(tmpdir_s, paf, "fa", [])
    want, log = _on_the_device(["-S9"], paf, fa)
    assert "reader=device" in log
    gz = fa + ".gz"
    with open(fa, "rb") as f, gzip.open(gz, "wb", compresslevel=1) as g:
        g.write(f.read())
    want_gz, log = _on_the_device(["-S9"], paf, gz)
    assert want_gz == want and "reader=host" in log
    out, log = _run(ma.CLI_PATH, ["-S9", "-p", "ug"], paf, os.path.join(tmpdir_s, "no_such_reads_file"), MA_TEXT_DEVICE="1")  # cannot be opened: "*", as ever
    assert out == _run(ma.CLI_PATH, ["-S9", "-p", "ug"], paf)[0] and re.search(r"^\[T::text\] ug device", log, flags=re.M)


def test_cli_ring_and_chain(tmpdir_s):
    """a hand-written input: seven reads c0 ... c6 of 10 000 bases, each one's 5000-10000 overlapping the next one's 0-5000, c6 closing on c0; then a chain l0 ... l5.
    -1 -2 gives one circular and one linear unitig: the circularising links, both x forms, both letters"""
    rows = []
    for k in range(7):
        rows.append("c%d\t10000\t5000\t10000\t+\tc%d\t10000\t0\t5000\t5000\t5000\t255\n" % (k, (k + 1) % 7))
    for k in range(5):
        rows.append("l%d\t10000\t5000\t10000\t+\tl%d\t10000\t0\t5000\t5000\t5000\t255\n" % (k, k + 1))
    paf = os.path.join(tmpdir_s, "text_ug_ring.paf")
    with open(paf, "w") as f:
        f.write("".join(rows))
    want, _ = _on_the_device(["-1", "-2"], paf)
    assert want.count(b"\nS\t") + 1 == 2 and b"\t+\t0M\n" in want and b"\t-\t0M\n" in want and re.search(rb"^x\tutg00000\dc\t", want, flags=re.M) and re.search(rb"^x\tutg00000\dl\t", want, flags=re.M)
    rnd = np.random.RandomState(3)
    fa = os.path.join(tmpdir_s, "text_ug_ring.fa")
    with open(fa, "wb") as f:
        for nm in ["c%d" % k for k in range(7)] + ["l%d" % k for k in range(6)]:
            f.write(b">" + nm.encode() + b"\n" + UM.make_seq(10000, rnd).upper() + b"\n")
    with_seq, _ = _on_the_device(["-1", "-2"], paf, fa)
    assert sorted(len(ln.split(b"\t")[2]) for ln in with_seq.split(b"\n") if ln.startswith(b"S\t")) == [35000, 35000]


# ---- 7. the memory sink
def test_memory_sink_gives_the_file_sinks_bytes(tmpdir_s, monkeypatch):
    """ma_pipeline_device_mem and, over two contexts, ma_pipeline_tail_mem after mahip_tail_handoff: the block holds what the command line writes; the context
    reports kind ug, road device"""
    paf = _noisy(tmpdir_s)
    opt = ma.default_opt()
    outs = {}
    monkeypatch.setenv("MA_TEXT_SLAB", "500")
    for dev in ("0", "1"):
        monkeypatch.setenv("MA_TEXT_DEVICE", dev)
        ing = ma.Ingest(paf, opt)
        ctx = ma.Ctx(0)
        ctx.hits_upload(ing.hits, ing.n_seq)
        outs[dev] = ma.run_resident(ctx, opt, ing, "ug", 6)
        last = ctx.text_last()
        if dev == "1":
            assert last["road"] == "device" and last["kind"] == "ug" and last["text_bytes"] == len(outs[dev]) and last["n_slabs"] >= 2 and last["n_slow_lines"] == 0
            assert last["n_lines"] == outs[dev].count(b"\n") and last["n_seq_bytes"] == 0
            ctx2 = ma.Ctx(0)
            ctx.hits_upload(ing.hits, ing.n_seq)
            outs["handoff"] = ma.run_resident_handoff(ctx, ctx2, opt, ing, "ug", 6)
            last2 = ctx2.text_last()
            assert last2["road"] == "device" and last2["kind"] == "ug" and last2["text_bytes"] == len(outs["handoff"])
            ctx2.close()
        else:
            assert last["road"] in (None, "host")
        ing.close()
        ctx.close()
    assert len(outs["1"]) > 100000 and outs["1"] == outs["0"] == outs["handoff"]
    monkeypatch.delenv("MA_TEXT_DEVICE")
    monkeypatch.delenv("MA_TEXT_SLAB")
    cli, _ = R.run_cli(ma.CLI_PATH, ["-p", "ug", "-S6"], paf)
    assert cli == outs["1"]
