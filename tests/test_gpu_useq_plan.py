"""The placement plan of -p ug -f made on the device (csrc/useq.hip: mahip_useq_plan): where every unitig's string starts in the arena, where every
read that sits on a unitig lands, and the wanted table of the device readers -- from the unitig members where they lie.
Stage cases through Ctx.useq_plan_mem (hand-made unitigs, names, kept intervals; no arena is allocated, so lengths may be anything); the yardstick is the Python
model of tests/useqplanmodel.py (asm.c:248-260 + ug_seq_wanted): entries as (name bytes, dst_off, len, s, e, rev, whole) in order, uoff and arena_bytes exactly.
Then the placement through the plan against the placement from the model's table, whole file and streamed; then the command line: MA_TEXT_DEVICE=1 -p ug -f
against the reference binary (MA_TEXT_DEVICE=0 where oracle/_ref is not built) on the device road and on every fallback, each seen to have been taken."""
import os
import re
import subprocess

import numpy as np
import pytest

import bgzfmodel as BM
import miniasm_amd as ma
import refapi as R
import ugtextmodel as UM
import useqplanmodel as PM

pytestmark = pytest.mark.gpu

NONE = UM.NONE
CSRC = os.path.join(ma.PKG, "csrc")


def _define(fn, name):
    src = open(os.path.join(CSRC, fn)).read()
    m = re.search(r"^#define %s \(?(\d+)u?\b" % name, src, flags=re.M)
    assert m, (fn, name)
    return int(m.group(1))


SCAN_TILE = _define("scan.hip", "SCAN_THREADS") * _define("scan.hip", "SCAN_ITEMS")  # scan_exclusive_u32 takes one block up to here
PL_TILE = 256 * _define("useq.hip", "PL_ITEMS")                                      # and so does the 64-bit scan of the unitig offsets


def read_names(n, empty=()):
    return [b"" if i in empty else b"rd%d" % i + b"y" * (i % 7) for i in range(n)]


def make_units(counts, n_reads, rnd, lows=None, lens=None, circ_every=3, reads=None):
    """unitigs of counts[i] members over DISTINCT reads (a random choice of the n_reads ids unless `reads` lists them), both strands, low words random (a few 0) unless
    `lows` gives them; every circ_every-th unitig circular; lens: their lengths (default: the sum of the low words mod 2^32)"""
    ids = list(reads) if reads is not None else [int(x) for x in rnd.permutation(n_reads)[:sum(counts)]]
    assert len(ids) >= sum(counts) and len(set(ids)) == len(ids)
    units, at = [], 0
    for i, k in enumerate(counts):
        mem = []
        for j in range(k):
            low = int(lows[i][j]) if lows is not None else (0 if rnd.randint(0, 9) == 0 else int(rnd.randint(1, 10 ** rnd.randint(1, 6))))
            mem.append(((ids[at] << 1 | int(rnd.randint(0, 2))) << 32) | low)
            at += 1
        ln = sum(m & 0xffffffff for m in mem) & 0xffffffff if lens is None else lens[i]
        if not mem or (circ_every and i % circ_every == circ_every - 1):
            units.append((ln, NONE, NONE, mem))
        else:
            units.append((ln, mem[0] >> 32, (mem[-1] >> 32) ^ 1, mem))
    return units


def check(ctx, units, names, sub=None):
    """plan on the device, bring it down, compare everything with the model"""
    info = ctx.useq_plan_mem(units, names, sub)
    want = PM.plan(units, names, sub)
    what = "%d unitigs, %d members, %d reads, %s" % (len(units), sum(len(u[3]) for u in units), len(names), "kept intervals" if sub is not None else "whole reads")
    assert (info["road"], info["reason"]) == ("device", "OK"), what
    assert ctx.useq_plan_last() == info
    uoff, pl, tab, blob = ctx.useq_plan_download()
    assert [int(x) for x in uoff] == want["uoff"], what + ": uoff"
    assert info["arena_bytes"] == want["arena_bytes"] == int(uoff[-1]), what
    got = [(blob[int(w["name_off"]):int(w["name_off"]) + int(w["name_len"])], int(w["dst_off"]), int(w["len"]), int(w["s"]), int(w["e"]), int(w["rev"]), int(w["whole"])) for w in tab]
    assert got == want["entries"], what + ": the wanted table differs from the model"
    assert (info["n_utg"], info["n_members"], info["n_reads"], info["n_wanted"], info["name_bytes"], info["n_multi"]) == \
        (len(units), sum(len(u[3]) for u in units), len(names), len(want["entries"]), want["name_bytes"], 0), what
    assert info["blob_bytes"] == sum(len(x) for x in names) and info["uoff_tiles"] == (len(units) + PL_TILE - 1) // PL_TILE
    for r in range(len(names)):  # the per-read plan: utg_place_t of every read; a read on no unitig has len 0
        p = want["place"].get(r)
        if p is None:
            assert int(pl["len"][r]) == 0, what
        else:
            assert (int(pl["utg"][r]), int(pl["start"][r]), int(pl["len"][r]), int(pl["ori"][r])) == p, what + ": read %d" % r
    return info, want


# ---- 1. counts
@pytest.mark.parametrize("U", [1, 2, 63, 64, 65])
def test_counts_at_the_wave_edge(gpu_ctx, U):
    """1, 2, 63, 64, 65 unitigs of 1, 2, 63, 64, 65 or 200 members, linear and circular mixed, with and without kept intervals"""
    rnd = np.random.RandomState(500 + U)
    counts = [(1, 2, 63, 64, 65, 200)[(i + U) % 6] for i in range(U)]
    n = sum(counts) + 11
    names = read_names(n)
    units = make_units(counts, n, rnd)
    if U >= 3:
        assert {u[1] == NONE for u in units} == {True, False}
    assert U < 6 or set(counts) == {1, 2, 63, 64, 65, 200}
    sub = UM.make_sub(n, rnd)
    _, w = check(gpu_ctx, units, names, sub)
    assert {e[5] for e in w["entries"]} == ({0, 1} if U >= 2 else {e[5] for e in w["entries"]}) and all(e[6] == 0 for e in w["entries"])
    _, w = check(gpu_ctx, units, names, None)
    assert all(e[3:5] == (0, 0) and e[6] == 1 for e in w["entries"])


def test_no_unitigs(gpu_ctx):
    info = gpu_ctx.useq_plan_mem([], read_names(5))
    assert (info["road"], info["reason"]) == ("host", "NO_UG")


# ---- 2. the scans past one block
@pytest.mark.parametrize("U,M,n", [(1, SCAN_TILE - 1, SCAN_TILE - 1), (1, SCAN_TILE, SCAN_TILE), (1, SCAN_TILE, SCAN_TILE + 1), (1, SCAN_TILE + 1, SCAN_TILE + 1),
                                   (PL_TILE - 1, PL_TILE - 1, PL_TILE + 5), (PL_TILE, PL_TILE, PL_TILE + 5), (PL_TILE + 1, PL_TILE + 1, PL_TILE + 5), (3 * PL_TILE + 7, 3 * PL_TILE + 7, 4 * PL_TILE)])
def test_scans_one_below_at_and_above_one_block(gpu_ctx, U, M, n):
    """the scan of the members' low words (M values), the compaction of the reads (n flags) and the 64-bit scan of the unitig offsets (U values), each one below, at
    and one above the size at which it leaves its one-block form; which form ran is read from Ctx.scan_forms() and from the report's uoff_tiles"""
    rnd = np.random.RandomState(U + M + n)
    counts = [M] if U == 1 else [1] * U
    names = read_names(n)
    units = make_units(counts, n, rnd, circ_every=0)
    before = gpu_ctx.scan_forms()
    info, _ = check(gpu_ctx, units, names, UM.make_sub(n, rnd) if n % 2 else None)
    after = gpu_ctx.scan_forms()
    sizes = (U, M, n)  # the first members of the hand-made unitigs, the members' low words, the reads' flags
    assert after[1] - before[1] == sum(1 for x in sizes if x > SCAN_TILE), "scans that took the chained form"
    assert after[0] - before[0] == sum(1 for x in sizes if x <= SCAN_TILE) and after[2] == before[2]
    assert info["uoff_tiles"] == (U + PL_TILE - 1) // PL_TILE and (info["uoff_tiles"] > 1) == (U > PL_TILE)


# ---- 3. / 4. 32 and 64 bits
def test_start_wraps_mod_2_32_and_dst_off_does_not(gpu_ctx):
    """one unitig whose low words 0xC0000000, 0xC0000000, 5 sum past 2^32: the third member starts at 0x80000000 (the reference's uint32_t l), the fourth at
    0x80000005; dst_off is the 64-bit sum uoff + start behind a first unitig of 2^32 - 1 bases"""
    rnd = np.random.RandomState(1)
    names = read_names(9)
    units = make_units([2, 4, 1], 9, rnd, lows=[[7, 9], [0xC0000000, 0xC0000000, 5, 11], [3]], lens=[0xffffffff, 0x80000010, 3], reads=[4, 1, 8, 2, 6, 3, 5])
    _, w = check(gpu_ctx, units, names, None)
    by_name = {e[0]: e for e in w["entries"]}
    assert [w["place"][r][1] for r in (8, 2, 6, 3)] == [0, 0xC0000000, 0x80000000, 0x80000005]
    assert by_name[names[6]][1] == (1 << 32) + 0x80000000 and by_name[names[2]][1] == (1 << 32) + 0xC0000000
    check(gpu_ctx, units, names, UM.make_sub(9, rnd))


def test_uoff_passes_2_32(gpu_ctx):
    """three unitigs of 2^32 - 1 bases: uoff = 0, 2^32, 2^33, the arena 3 * 2^32 bytes"""
    rnd = np.random.RandomState(2)
    names = read_names(6)
    units = make_units([1, 2, 1], 6, rnd, lens=[0xffffffff] * 3)
    info, w = check(gpu_ctx, units, names, None)
    assert w["uoff"] == [0, 1 << 32, 1 << 33, 3 << 32] and info["arena_bytes"] == 3 << 32
    assert max(e[1] for e in w["entries"]) >= 1 << 33


# ---- 5. reads that are not wanted
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_unwanted_reads(gpu_ctx, n):
    """a member of length 0 and a read without a name are not wanted; reads 0 and n - 1 sit on no unitig, and so does every third read between the wanted ones"""
    rnd = np.random.RandomState(n)
    if n == 1:  # the only read: wanted; not wanted (length 0; no name); on no unitig
        check(gpu_ctx, [(5, 0, 1, [5])], [b"only"])
        info, _ = check(gpu_ctx, [(0, 0, 1, [1 << 32])], [b"only"])
        assert info["n_wanted"] == 0
        info, _ = check(gpu_ctx, [(5, 0, 1, [5])], [b""])
        assert info["n_wanted"] == 0
        info, _ = check(gpu_ctx, [(5, NONE, NONE, [])], [b"only"])
        assert (info["n_wanted"], info["n_members"]) == (0, 0)
        return
    on = [r for r in range(1, n - 1) if r % 3]
    rnd.shuffle(on)
    counts = [len(on) // 2, len(on) - len(on) // 2]
    lows = [[0 if (i + j) % 5 == 0 else 10 + i + j for j in range(k)] for i, k in enumerate(counts)]
    units = make_units(counts, n, rnd, lows=lows, reads=on)
    names = read_names(n, empty=set(on[::4]))
    for sub in (None, UM.make_sub(n, rnd)):
        info, w = check(gpu_ctx, units, names, sub)
        zero = {m >> 33 for u in units for m in u[3] if m & 0xffffffff == 0}
        assert zero and set(on[::4]) - zero and info["n_wanted"] == len(set(on) - zero - set(on[::4])) > 0
        assert {e[5] for e in w["entries"]} == {0, 1}, "both strands"


# ---- 6. refusals
FA = b">a desc\nACGTACGTAC\n>b\nGGGGGCCCCCTTTTT\n>c\nAC\n"
HOST_TABLE = [dict(name=b"a", dst_off=0, len=6, rev=False, s=2, e=10), dict(name=b"b", dst_off=6, len=4, rev=True, s=0, e=None)]
HOST_ARENA = b"GTACGT" + b"AAAA" + b"N"


def _still_works(ctx):
    """the refusal left no plan and changed nothing else: the planned entries refuse, the text indexed before is still there, and the host-table placement works"""
    assert ctx.useq_plan_last()["road"] == "host"
    with pytest.raises(RuntimeError):
        ctx.useq_place_text_planned()
    with pytest.raises(RuntimeError):
        ctx.useq_plan_download()
    assert ctx.useq_place_text(len(HOST_ARENA), HOST_TABLE) == (HOST_ARENA, 2, 0, 0)


def test_refusals_leave_the_context_as_it_was(gpu_ctx, monkeypatch):
    """MULTI (a read in two unitigs; a read twice in one), NO_NAMES, FORCED (MA_USEQ_PLAN_HOST=1), NO_UG: road host with the reason, no plan, and the host-table
    placement on the text that was indexed BEFORE the refusal gives its bytes"""
    ctx = gpu_ctx
    names = read_names(8)
    ctx.fastx_load(FA)
    assert ctx.fastx_index()["regular"]
    two = [(20, NONE, NONE, [(3 << 33) | 10, (5 << 33) | 10]), (9, NONE, NONE, [(5 << 33 | 1 << 32) | 9])]
    twice = [(30, NONE, NONE, [(3 << 33) | 10, (5 << 33) | 10, (3 << 33) | 10])]
    for units in (two, twice):
        with pytest.raises(PM.Multi):
            PM.plan(units, names)
        info = ctx.useq_plan_mem(units, names)
        assert (info["road"], info["reason"], info["n_multi"]) == ("host", "MULTI", 1)
        _still_works(ctx)
    fine = [(20, NONE, NONE, [(3 << 33) | 10, (5 << 33) | 10])]
    info = ctx.useq_plan_mem(fine, None)
    assert (info["road"], info["reason"]) == ("host", "NO_NAMES")
    _still_works(ctx)
    monkeypatch.setenv("MA_USEQ_PLAN_HOST", "1")
    info = ctx.useq_plan_mem(fine, names)
    assert (info["road"], info["reason"]) == ("host", "FORCED")
    _still_works(ctx)
    monkeypatch.delenv("MA_USEQ_PLAN_HOST")
    info = ctx.useq_plan_mem([], names)
    assert (info["road"], info["reason"]) == ("host", "NO_UG")
    _still_works(ctx)
    check(ctx, fine, names)  # and the same unitigs plan once nothing is in the way
    ctx.fastx_release()


def test_a_member_outside_the_dictionary_is_an_error(gpu_ctx):
    with pytest.raises(RuntimeError, match="outside"):
        gpu_ctx.useq_plan_mem([(5, NONE, NONE, [(9 << 33) | 5])], read_names(9))


# ---- 7. placement through the plan
def _reads_and_units(rnd, n, with_sub):
    """n reads of 40 ... 400 bases; three unitigs over two thirds of them whose members take no more bases than the read (its kept interval) holds"""
    names = read_names(n)
    seqs = [UM.make_seq(int(rnd.randint(40, 400)), rnd) for _ in range(n)]
    sub = None
    if with_sub:
        sub = np.zeros(n, dtype=ma.SUB_DT)
        sub["sdel"] = [rnd.randint(0, len(s) // 3) for s in seqs]
        sub["e"] = [len(s) - rnd.randint(0, len(s) // 3) for s in seqs]
    on = [int(x) for x in rnd.permutation(n)[:2 * n // 3]]
    counts = [len(on) // 3, len(on) // 3, len(on) - 2 * (len(on) // 3)]
    room = [len(seqs[r]) if sub is None else int(sub["e"][r]) - int(sub["sdel"][r]) for r in on]
    it = iter(room)
    lows = [[int(rnd.randint(0, next(it) + 1)) for _ in range(k)] for k in counts]
    units = make_units(counts, n, rnd, lows=lows, reads=on)
    return names, seqs, sub, units


def _fasta(names, seqs, width):
    return b"".join(b">%s\n" % nm + b"".join(s[k:k + width] + b"\n" for k in range(0, len(s), width)) for nm, s in zip(names, seqs))


def _fastq(names, seqs):
    return b"".join(b"@%s extra\n%s\n+\n%s\n" % (nm, s, b"I" * len(s)) for nm, s in zip(names, seqs))


def _pieces(text, most=256):
    out, cur = [], b""
    for ln in text.splitlines(keepends=True):
        if cur and len(cur) + len(ln) > most:
            out.append(cur)
            cur = b""
        cur += ln
    return out + [cur]


@pytest.mark.parametrize("fmt,with_sub", [("fasta", False), ("fasta", True), ("fastq", False), ("fastq", True)])
def test_placement_through_the_plan(gpu_ctx, fmt, with_sub):
    """plan, then the planned placement of a small FASTA (wrapped at 60) / FASTQ: the arena is byte for byte what Ctx.useq_place_text gives for the model's table;
    the same through the streamed reader in pieces of at most 256 bytes"""
    ctx = gpu_ctx
    rnd = np.random.RandomState(17 + with_sub)
    names, seqs, sub, units = _reads_and_units(rnd, 70, with_sub)
    text = _fasta(names, seqs, 60) if fmt == "fasta" else _fastq(names, seqs)
    w = PM.plan(units, names, sub)
    table = PM.wanted(w["entries"])
    ctx.fastx_load(text)
    assert ctx.fastx_index()["regular"]
    want = ctx.useq_place_text(w["arena_bytes"], table)
    assert want[1:] == (len(table), 0, 0) and set(want[0]) - set(b"N") and b"N" in want[0]
    info = ctx.useq_plan_mem(units, names, sub)
    assert (info["road"], info["n_wanted"], info["arena_bytes"]) == ("device", len(table), w["arena_bytes"])
    assert ctx.useq_place_text_planned() == want
    ctx.fastx_release()
    pieces = _pieces(text)
    assert len(pieces) > 20
    arena, verdicts, rep = ctx.useq_stream(pieces, w["arena_bytes"], table)
    assert arena == want[0] and all(v["reason"] == "OK" for v in verdicts)
    ctx.useq_plan_mem(units, names, sub)
    arena2, verdicts2, rep2 = ctx.useq_stream_planned(pieces)
    assert arena2 == want[0] and verdicts2 == verdicts and (rep2["matched"], rep2["jobs"]) == (rep["matched"], rep["jobs"]) == (len(table), len(table))
    ctx.fastx_release()


def test_planned_readers_refuse_a_table_that_leaves_the_arena(gpu_ctx):
    """unitig lengths that do not hold their members: the plan is made (it allocates nothing), the planned readers refuse it before anything is placed"""
    ctx = gpu_ctx
    names = read_names(4)
    ctx.fastx_load(FA)
    assert ctx.fastx_index()["regular"]
    info = ctx.useq_plan_mem([(3, NONE, NONE, [(1 << 33) | 2, (2 << 33) | 9])], names)
    assert info["road"] == "device" and info["arena_bytes"] == 4
    with pytest.raises(RuntimeError, match="outside the arena"):
        ctx.useq_place_text_planned()
    ctx.fastx_release()


# ---- 8. the command line
NOISY = dict(reads=4000, lines=90000, seed=63, extra=["-L", "uniform", "-d", "0.35", "-x", "0.03"])  # tests/test_gpu_text_ug.py: the same input, made the same way
_made = {}


def _noisy(tmpdir_s):
    if "paf" not in _made:
        _made["paf"] = R.pafgen(os.path.join(tmpdir_s, "useq_plan_noisy.paf"), NOISY["reads"], NOISY["lines"], NOISY["seed"], NOISY["extra"])
    return _made["paf"]


def _readgen(tmpdir_s, paf, tag, opts):
    key = (paf, tag)
    if key not in _made:
        exe = os.path.join(os.path.dirname(ma.PAFGEN_PATH), "readgen")
        fn = os.path.join(tmpdir_s, "useq_plan_reads_%s" % tag)
        subprocess.run([exe] + opts + ["-s", "7", "-o", fn, paf], check=True, stderr=subprocess.DEVNULL)
        _made[key] = fn
    return _made[key]


SWITCHES = ("MA_TEXT_DEVICE", "MA_TEXT_SLAB", "MA_USEQ_PLAN_HOST", "MA_FASTX_HOST", "MA_FASTX_STREAM", "MA_FASTX_PIECE", "MA_BGZF_HOST")


def _run(binary, args, paf, reads, timing="1", **env):
    e = dict(os.environ)
    for k in SWITCHES + ("MA_PIPE_TIMING",):
        e.pop(k, None)
    if timing:
        e["MA_PIPE_TIMING"] = timing
    e.update(env)
    r = subprocess.run([binary] + list(args) + ["-p", "ug", "-f", reads, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=900)
    assert r.returncode == 0, "%s %s: exit %d: %s" % (binary, " ".join(args), r.returncode, r.stderr.decode(errors="replace")[-2000:])
    return r.stdout, r.stderr.decode(errors="replace")


def _want(args, paf, reads):
    """the reference's bytes (MA_TEXT_DEVICE=0's where oracle/_ref is not built)"""
    key = ("want", tuple(args), paf, reads)
    if key not in _made:
        host, log = _run(ma.CLI_PATH, args, paf, reads, MA_TEXT_DEVICE="0")
        assert "[T::ug_plan]" not in log and "[T::text]" not in log
        if R.have_ref():
            ref, _ = _run(R.REF_BIN, args, paf, reads)
            assert host == ref
        _made[key] = host
    return _made[key]


def _bgzip(fn):
    """the file as bgzip writes it (tests/bgzfmodel.py)"""
    out = fn + ".bgz"
    if not os.path.exists(out):
        with open(fn, "rb") as f, open(out, "wb") as g:
            g.write(BM.bgzf(f.read()))
    return out


PLAN_DEVICE = re.compile(r"^\[T::ug_plan\] device: (\d+) unitigs, (\d+) members, (\d+) wanted reads, (\d+) name bytes, (\d+) arena bytes; [\d.]+ ms$", flags=re.M)


@pytest.mark.parametrize("args", [[], ["-R"]], ids=["alone", "-R"])
@pytest.mark.parametrize("packed", [False, True], ids=["fastq", "bgzip"])
def test_cli_plans_on_the_device(args, packed, tmpdir_s):
    """-p ug -f under MA_TEXT_DEVICE=1, a plain FASTQ and the same file bgzip'ed, with and without -R: the reference's bytes, the plan made on the device, the
    text written on the device, nothing downloaded"""
    paf = _noisy(tmpdir_s)
    fq = _readgen(tmpdir_s, paf, "fq", ["-q"])
    want = _want(args, paf, fq)
    assert max(len(ln.split(b"\t")[2]) for ln in want.split(b"\n") if ln.startswith(b"S\t")) > 7000
    out, log = _run(ma.CLI_PATH, args, paf, _bgzip(fq) if packed else fq, MA_TEXT_DEVICE="1")
    assert out == want
    m = PLAN_DEVICE.search(log)
    assert m, log[-1500:]
    n_utg, n_mem, n_want, _, arena = (int(x) for x in m.groups())
    s_lines = [ln for ln in out.split(b"\n") if ln.startswith(b"S\t")]
    assert n_utg == len(s_lines) and n_mem == sum(1 for ln in out.split(b"\n") if ln.startswith(b"a\t")) and 0 < n_want <= n_mem
    assert arena == sum(len(ln.split(b"\t")[2]) + 1 for ln in s_lines)
    assert "reader=device" in log and "download 0.000 ms" in log and re.search(r"^\[T::text\] ug device", log, flags=re.M)


TEXT_DEVICE = re.compile(r"^\[T::text\] ug device", flags=re.M)


@pytest.mark.parametrize("env,seen", [(dict(MA_USEQ_PLAN_HOST="1"), ("[T::ug_plan] host (MA_USEQ_PLAN_HOST is set)", "reader=device")),
                                      (dict(MA_FASTX_HOST="1"), ("[T::ug_plan] device", "reads file read on the host: MA_FASTX_HOST is set", "reader=host")),
                                      (dict(MA_FASTX_STREAM="2", MA_FASTX_PIECE="65536"), ("[T::ug_plan] device", "reader=stream", "handover=none"))], ids=["plan_host", "fastx_host", "stream"])
def test_cli_switches_off_the_device_plan_give_the_same_bytes(env, seen, tmpdir_s):
    """the host plan (MA_USEQ_PLAN_HOST=1), the host reader on the downloaded plan (MA_FASTX_HOST=1), the streamed reader on the plan's table (MA_FASTX_STREAM=2): the
    device road's bytes, the road seen in stderr, the text still written on the device"""
    paf = _noisy(tmpdir_s)
    fq = _readgen(tmpdir_s, paf, "fq", ["-q"])
    out, log = _run(ma.CLI_PATH, [], paf, fq, MA_TEXT_DEVICE="1", **env)
    assert out == _want([], paf, fq)
    for x in seen:
        assert x in log, (x, log[-1500:])
    assert TEXT_DEVICE.search(log) and ("MA_USEQ_PLAN_HOST" in env) == (PLAN_DEVICE.search(log) is None)


def _records(fq):
    lines = open(fq, "rb").read().split(b"\n")
    return lines, lambda name: next(i for i in range(0, len(lines) - 3, 4) if lines[i][1:].split()[0] == name)


def test_cli_short_read_goes_to_the_host_reader(tmpdir_s):
    """SHORT_READ behind a device plan: the host reader runs on the downloaded plan.  Under -1 -2 (whole reads: with kept intervals the reference, and the host reader,
    assert on such a record) the first read of the first unitig is cut to 10 bases; the missing ones stay N
    (tests/test_gpu_cli.py::test_cli_reads_file_shorter_than_the_paf_says), so MA_TEXT_DEVICE=0 on the same file is the yardstick"""
    paf = _noisy(tmpdir_s)
    fq = _readgen(tmpdir_s, paf, "fq", ["-q"])
    want12 = _want(["-1", "-2"], paf, fq)
    a = next(ln for ln in want12.split(b"\n") if ln.startswith(b"a\t")).split(b"\t")
    assert int(a[5]) > 10
    lines, record_of = _records(fq)
    k = record_of(a[3])
    lines[k + 1], lines[k + 3] = lines[k + 1][:10], lines[k + 3][:10]
    fn = fq + ".short"
    open(fn, "wb").write(b"\n".join(lines))
    host, _ = _run(ma.CLI_PATH, ["-1", "-2"], paf, fn, MA_TEXT_DEVICE="0")
    out, log = _run(ma.CLI_PATH, ["-1", "-2"], paf, fn, MA_TEXT_DEVICE="1")
    assert out == host and out != want12 and len(out) == len(want12)
    assert PLAN_DEVICE.search(log) and "reads file read on the host: a wanted read is shorter than its placement" in log and "reader=host" in log, log[-1500:]
    assert TEXT_DEVICE.search(log)


def test_cli_nul_in_a_wanted_read_goes_to_the_host_formatter(tmpdir_s):
    """SEQ_NUL behind a device plan: a NUL byte among the bases a unitig takes from its first read ("name:s-e", s printed 1-based: forward the first len bases of
    [s, e), reverse the last).  The file is read on the host (NUL_BYTE), the arena holds the NUL, mahip_text_prepare_ug refuses, ma_ug_t is fetched at that moment
    and the arena is cut with the plan's uoff: the reference's bytes"""
    paf = _noisy(tmpdir_s)
    fq = _readgen(tmpdir_s, paf, "fq", ["-q"])
    want = _want([], paf, fq)
    a = next(ln for ln in want.split(b"\n") if ln.startswith(b"a\t")).split(b"\t")
    name, span = a[3].rsplit(b":", 1)
    s1, e = (int(x) for x in span.split(b"-"))
    assert int(a[5]) > 0
    at = s1 - 1 if a[4] == b"+" else e - 1
    lines, record_of = _records(fq)
    k = record_of(name)
    lines[k + 1] = lines[k + 1][:at] + b"\0" + lines[k + 1][at + 1:]
    fn = fq + ".nul"
    open(fn, "wb").write(b"\n".join(lines))
    host, _ = _run(ma.CLI_PATH, [], paf, fn, MA_TEXT_DEVICE="0")
    if R.have_ref():
        assert host == _run(R.REF_BIN, [], paf, fn)[0]
    out, log = _run(ma.CLI_PATH, [], paf, fn, MA_TEXT_DEVICE="1")
    assert out == host and out != want
    assert PLAN_DEVICE.search(log) and "reads file read on the host: NUL bytes in the file" in log and "reader=host" in log, log[-1500:]
    assert re.search(r"^\[T::text\] ug host \(a NUL byte in the sequences\)", log, flags=re.M) and "download 0.000 ms" not in log, log[-1500:]


def _prefixes(log):
    return set(re.findall(r"^\[[MTW]::[A-Za-z_0-9]+", log, flags=re.M))


# the parent commit's stderr on this input with MA_TEXT_DEVICE unset, as the set of its line prefixes: a plain run, and what MA_PIPE_TIMING=1 adds
PARENT_PREFIXES = {"[M::" + x for x in ("main", "ma_hit_read", "ma_hit_sub", "ma_hit_cut", "ma_hit_flt", "ma_hit_contained", "ma_sg_gen", "asg_arc_del_trans", "asg_arc_del_multi", "asg_arc_del_asymm",
                                        "asg_arc_del_short", "asg_cut_tip", "asg_pop_bubble", "asg_cut_internal", "asg_cut_biloop")}
PARENT_TIMING_PREFIXES = {"[T::" + x for x in ("init", "paf", "xfer", "ingest_gpu", "ties", "pipeline", "tail", "ug_seq", "ug_print")}


def test_cli_with_the_switch_unset_prints_what_it_printed(tmpdir_s):
    """MA_TEXT_DEVICE unset: the reference's bytes, and a stderr of the parent commit's shape -- the set of its [M:: / [T:: / [W:: line prefixes, recorded above from the
    parent commit: no [T::ug_plan], no [T::text], no warning, one [T::ug_seq] line of the device reader; without MA_PIPE_TIMING no [T:: line at all"""
    paf = _noisy(tmpdir_s)
    fq = _readgen(tmpdir_s, paf, "fq", ["-q"])
    want = _want([], paf, fq)
    out, log = _run(ma.CLI_PATH, [], paf, fq)
    assert out == want
    assert _prefixes(log) == PARENT_PREFIXES | PARENT_TIMING_PREFIXES, sorted(_prefixes(log) ^ (PARENT_PREFIXES | PARENT_TIMING_PREFIXES))
    assert len(re.findall(r"^\[T::ug_seq\] reader=device ", log, flags=re.M)) == 1
    out, log = _run(ma.CLI_PATH, [], paf, fq, timing=None)
    assert out == want and _prefixes(log) == PARENT_PREFIXES, sorted(_prefixes(log) ^ PARENT_PREFIXES)
