"""GPU: the sharded multi-GPU mode on real hardware.  One box has one GPU, and RCCL refuses two ranks on one device, so N ranks run as N processes
that share the GPU and exchange through the shared-memory double of the collectives (MA_COMM=shm).  Everything else is the production path: host/sharded.c,
host/ingest_sharded.c, mahip_set_shard, the split contained / sg passes, arc row import/export, ranged transitive reduction.  (Until round 3 this module
also ran N virtual ranks as threads through a Python copy of the exchange sequence; that copy is gone -- tests/test_dist_gloo.py runs the C code over gloo.)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import miniasm_amd as ma
import refapi as R
import stages as ST

pytestmark = pytest.mark.gpu


# ---- the product path: orchestration in C (host/sharded.c), collectives from C (csrc/comm.hip) ----
@pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", ["lognormal", "noisy", "fixed"])
def test_cli_on_n_ranks_matches_one_gpu_and_reference(world, case, tmpdir_s):
    """MA_GPUS=N miniasm: one process per rank, read-range shards, the C orchestration end to end.  This box has one GPU, where RCCL
    refuses several ranks, so the collectives run through the host-staged shared-memory double (MA_COMM=shm); everything else --
    shard bookkeeping, exchange points, buffer layout, rank-0 tail -- is the production code."""
    import subprocess
    extra = {"lognormal": [], "noisy": ["-L", "uniform", "-d", "0.35", "-x", "0.03"], "fixed": ["-L", "fixed"]}[case]
    paf = R.pafgen(os.path.join(tmpdir_s, "shc_%s.paf" % case), 3001, 80000, 81, extra)
    one, _ = R.run_cli(ma.CLI_PATH, [], paf)
    env = dict(os.environ, MA_GPUS=str(world), MA_COMM="shm")
    r = subprocess.run([ma.CLI_PATH, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == one, "N-rank GFA differs from the single-GPU GFA"
    ref_sg, _ = R.run_cli(R.REF_BIN, ["-p", "sg", "-S5"], paf)
    if R.arc_tie_groups(ref_sg) == 0:
        ref, _ = R.run_cli(R.REF_BIN, [], paf)
        assert r.stdout == ref
    r = subprocess.run([ma.CLI_PATH, "-p", "sg", paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout == R.run_cli(ma.CLI_PATH, ["-p", "sg"], paf)[0]


@pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("world", [2, 3])
def test_cli_on_n_ranks_reproduces_the_reference_tie_order(world, tmpdir_s):
    """tie-rich input on shards: the census runs on the merged graph, the ranks restore the reference's hit order for their own pushed arcs
    (every rank holds the whole input) and rebuild the reference's arc order from the global push sequence -- GFA and string-graph dump
    byte-identical to the reference's, as on one GPU"""
    import subprocess
    paf = R.pafgen(os.path.join(tmpdir_s, "shc_ties.paf"), 3000, 80000, 5, ["-q", "16", "-L", "uniform", "-d", "0.3", "-x", "0.03"])
    ref_sg, _ = R.run_cli(R.REF_BIN, ["-p", "sg", "-S5"], paf)
    assert R.arc_tie_groups(ref_sg) >= 5
    env = dict(os.environ, MA_GPUS=str(world), MA_COMM="shm")
    env.pop("MA_EXACT_TIES", None)
    for args in ([], ["-p", "sg", "-S6"], ["-p", "sg"]):
        ref, _ = R.run_cli(R.REF_BIN, args, paf)
        r = subprocess.run([ma.CLI_PATH] + args + [paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"left in the stable order" not in r.stderr
        assert r.stdout == ref, "%d ranks, %s: bytes differ from the reference" % (world, " ".join(args))


@pytest.mark.parametrize("tail_ctx", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_that_hold_only_their_own_records(world, tail_ctx, tmpdir_s, monkeypatch):
    """the shape of `bench.py --gpus N` without torch: every rank is a process that holds ONLY the records of its read range, three steps over
    the shared-memory double, rank 0 finishes each batch on its own context or (tail_ctx) on a second one (mahip_tail_handoff); every step's GFA
    equals the single-context run and the reference's"""
    import subprocess
    import sys
    paf = R.pafgen(os.path.join(tmpdir_s, "own_%d.paf" % world), 2500, 70000, 55, ["-L", "uniform", "-d", "0.3"])
    out = os.path.join(tmpdir_s, "own_%d_%d.out" % (world, tail_ctx))
    # tail_ctx runs also use read ranges balanced by hit count (unequal ranges: the all-gathers' slots are as long as the longest one)
    env = dict(os.environ, MA_WORKER_EMU="1" if getattr(ma, "IS_EMU", False) else "0", MA_WORKER_BALANCE="1" if tail_ctx else "0")
    env.pop("MA_GPUS", None)
    name = "ma_own_%d_%d_%d" % (os.getpid(), world, tail_ctx)
    procs = [subprocess.Popen([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "shard_step_worker.py"), paf, str(r), str(world), name, str(tail_ctx), out],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(world)]
    for p in procs:
        try:
            _, err = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, err.decode()[-2000:]
    data = open(out, "rb").read()
    assert data.startswith(b"OK\n"), "a step's GFA differs from the single-context run"
    if R.have_ref():
        ref_sg, _ = R.run_cli(R.REF_BIN, ["-p", "sg", "-S5"], paf)
        if R.arc_tie_groups(ref_sg) == 0:
            assert data[3:] == R.run_cli(R.REF_BIN, [], paf)[0]


@pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_with_their_own_records_restore_the_reference_tie_order(world, tmpdir_s):
    """own-records shards on a tie-rich input: each rank knows where its records stood in the input (mahip_hits_set_positions), the ranks put the hit keys
    of the whole input together, every rank runs the walk (hit.c:19-22 is a function of ALL records) and orders its own pushed arcs by it; the GFA of every
    step is the reference's, byte for byte -- without positions the same run reports the groups as unrepaired"""
    import subprocess
    import sys
    paf = R.pafgen(os.path.join(tmpdir_s, "own_ties_%d.paf" % world), 3000, 80000, 5, ["-q", "16", "-L", "uniform", "-d", "0.3", "-x", "0.03"])
    ref_sg, _ = R.run_cli(R.REF_BIN, ["-p", "sg", "-S5"], paf)
    assert R.arc_tie_groups(ref_sg) >= 5
    out = os.path.join(tmpdir_s, "own_ties_%d.out" % world)
    env = dict(os.environ, MA_WORKER_EMU="1" if getattr(ma, "IS_EMU", False) else "0", MA_WORKER_BALANCE="1" if world == 3 else "0", MA_WORKER_POS="1")
    env.pop("MA_GPUS", None)
    name = "ma_ownt_%d_%d" % (os.getpid(), world)
    procs = [subprocess.Popen([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "shard_step_worker.py"), paf, str(r), str(world), name, "0", out],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(world)]
    for p in procs:
        try:
            _, err = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, err.decode()[-2000:]
    data = open(out, "rb").read()
    assert data.startswith(b"OK\n"), "a step's GFA differs from the single-context run"
    assert data[3:] == R.run_cli(R.REF_BIN, [], paf)[0]


@pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("world", [2, 3, 5])
def test_every_rank_ingests_its_own_byte_range(world, tmpdir_s):
    """round-3 review, What's missing #2 (ingest routing option B): `MA_GPUS=N miniasm plain.paf` no longer parses the whole text on every rank.
    Rank g loads the bytes [g S/N, (g+1) S/N) cut at line starts, the ranks merge the name tables of their ranges into the reference's first-appearance ids
    and send every record to the owner of its query read (host/ingest_sharded.c, csrc/paf.hip, csrc/hits.hip: mahip_hits_route).  Checked here: the byte ranges
    tile the file, the output is the reference's byte for byte -- also where the reference's sequential reader carries state across a range border (a name first
    seen as a TARGET in an earlier range, 10-column lines that inherit `bl` from a line of an earlier range, CR LF, an unterminated last line, tied sort keys) --
    and MA_INGEST_WHOLE=1 (every rank parses everything: round 3) and gzip input (falls back to it) give the same bytes."""
    import gzip
    import random
    import re
    import subprocess
    base = R.pafgen(os.path.join(tmpdir_s, "ing_%d.paf" % world), 2500, 60000, 91 + world, ["-q", "16", "-L", "uniform", "-d", "0.3", "-x", "0.03"])
    rnd = random.Random(world)
    lines = open(base, "rb").read().split(b"\n")[:-1]
    out = []
    for k, ln in enumerate(lines):  # damage that crosses range borders: runs of 10-column lines (stale bl), CR LF, short lines
        f = ln.split(b"\t")
        if rnd.random() < 0.25:
            ln = b"\t".join(f[:10])
        elif rnd.random() < 0.02:
            ln = b"\t".join(f[:rnd.randint(1, 9)])
        if rnd.random() < 0.05:
            ln += b"\r"
        out.append(ln)
    paf = os.path.join(tmpdir_s, "ing_%d_damaged.paf" % world)
    with open(paf, "wb") as fo:
        fo.write(b"\n".join(out))  # no newline behind the last line
    size = os.path.getsize(paf)
    ref, _ = R.run_cli(R.REF_BIN, [], paf)
    env = dict(os.environ, MA_GPUS=str(world), MA_COMM="shm", MA_PIPE_TIMING="1")
    r = subprocess.run([ma.CLI_PATH, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == ref, "N-rank GFA (own byte ranges) differs from the reference's"
    spans = sorted((int(a), int(b)) for a, b in re.findall(r"rank \d+ of \d+: bytes \[(\d+), (\d+)\) of %d" % size, r.stderr.decode()))
    assert len(spans) == world and spans[0][0] == 0 and spans[-1][1] == size and all(spans[k][1] == spans[k + 1][0] for k in range(world - 1)), spans
    assert max(b - a for a, b in spans) < size / world * 1.5 + 4096, "a rank loaded far more than its share: %r" % spans
    for sg_args in (["-p", "sg"], ["-p", "sg", "-S6"]):
        r2 = subprocess.run([ma.CLI_PATH] + sg_args + [paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
        assert r2.returncode == 0 and r2.stdout == R.run_cli(R.REF_BIN, sg_args, paf)[0], sg_args
    if world == 2:  # the shared-memory double moves a rank's pieces a slot's worth at a time (BASELINE configs[3] on two ranks: 3.2 GB from each through 1 GB slots): here with 512 KB slots
        small = subprocess.run([ma.CLI_PATH, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, MA_SHM_SLOT_LOG2="19"), timeout=900)
        assert small.returncode == 0 and small.stdout == ref, small.stderr.decode()[-500:]
    whole = subprocess.run([ma.CLI_PATH, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, MA_INGEST_WHOLE="1"), timeout=900)
    assert whole.returncode == 0 and whole.stdout == ref and b"bytes [" not in whole.stderr
    with open(paf, "rb") as fi, gzip.open(paf + ".gz", "wb") as fo:
        fo.write(fi.read())
    gz = subprocess.run([ma.CLI_PATH, paf + ".gz"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert gz.returncode == 0 and gz.stdout == ref


# ---- the byte-range ingest at its edges: hand-made texts whose lines are padded to one length, so that the [g S/N, (g+1) S/N) cut puts chosen lines on chosen ranks
_EDGE_READS, _EDGE_LEN, _EDGE_STEP = 12, 10000, 2000
_EDGE_POISON = 999999  # a `bl` under which ma_hit_sub drops the hit (hit.c:125: ml < bl * min_iden); the lines that inherit it are dropped with it


def _edge_chain():
    """twelve reads of 10 kb every 2 kb, every overlap of at least 2 kb once, grouped by query: 38 lines on which the reference writes one unitig of six reads"""
    out = []
    for i in range(_EDGE_READS):
        for j in range(i + 1, _EDGE_READS):
            d = _EDGE_STEP * (j - i)
            if _EDGE_LEN - d < 2000:
                break
            out.append(dict(q="r%02d" % i, ql=_EDGE_LEN, qs=d, qe=_EDGE_LEN, t="r%02d" % j, tl=_EDGE_LEN, ts=0, te=_EDGE_LEN - d, ml=_EDGE_LEN - d, bl=_EDGE_LEN - d))
    return out


def _edge_unstored(k):
    """a valid line that is not stored (spans below min_span), with names no other line has"""
    return dict(q="u%02d" % k, ql=_EDGE_LEN, qs=0, qe=1000, t="v%02d" % k, tl=_EDGE_LEN, ts=0, te=1000, ml=900, bl=1000)


def _edge_text(recs, width):
    """every record as a line of exactly `width` bytes (newline included).  bl=None: a 10-column line, padded with leading zeros in its numbers (at most 8 digits each:
    the tile parser's own form); otherwise 12 columns and a tag column that takes the padding"""
    lines = []
    for r in recs:
        num = ["%05d" % r[k] for k in ("ql", "qs", "qe", "tl", "ts", "te", "ml")]
        def cols():
            return [r["q"], num[0], num[1], num[2], "+", r["t"], num[3], num[4], num[5], num[6]]
        if r["bl"] is None:
            k = 0
            while len("\t".join(cols())) + 1 < width:
                assert any(len(x) < 8 for x in num), "width too large for a 10-column line"
                if len(num[k % 7]) < 8:
                    num[k % 7] = "0" + num[k % 7]
                k += 1
            ln = "\t".join(cols())
        else:
            ln = "\t".join(cols() + ["%d" % r["bl"], "255"])
            if len(ln) + 1 < width:
                assert len(ln) + 1 + 6 <= width, "width too small for the tag column"
                ln += "\tpd:Z:" + "x" * (width - len(ln) - 7)
        assert len(ln) + 1 == width, (len(ln) + 1, width, ln)
        lines.append(ln.encode() + b"\n")
    return lines


def _edge_split(lines, world):
    """the line ranges of the ranks (host/ingest_sharded.c: a range begins at the first line start at or behind its nominal start): [(first line, end line, first byte, end byte)]"""
    starts = [0]
    for ln in lines:
        starts.append(starts[-1] + len(ln))
    size = starts[-1]
    def cut(g):
        at = size * g // world
        return next(k for k, s in enumerate(starts) if s >= at) if g < world else len(lines)
    return [(cut(g), cut(g + 1), starts[cut(g)], starts[cut(g + 1)]) for g in range(world)]


def _edge_cases():
    """name -> (records, width, worlds, check(records, ranges of line numbers) that the text is the case it claims to be)"""
    chain = _edge_chain()
    assert len(chain) == 38
    cases = {}
    def names(recs):
        return {r["q"] for r in recs} | {r["t"] for r in recs}
    def stored(r):
        return r["qe"] - r["qs"] >= 2000 and r["te"] - r["ts"] >= 2000 and r["ml"] >= 100
    def with_bl(recs, has, poison=()):
        return [dict(r, bl=(_EDGE_POISON if k in poison else r["bl"]) if has(k) else None) for k, r in enumerate(recs)]

    # more ranks than lines: some ranks get an empty range (L == 0, no local names, no local table)
    def chk(recs, rg):
        assert sum(1 for a, b in rg if a == b) == len(rg) - 2 and all(b - a <= 1 for a, b in rg)
    cases["more_ranks_than_lines"] = (chain[:2], 72, (3, 5), chk)

    # a range whose lines are all below min_span between two ranges with names: L > 0, n_pass == 0, R_loc == 0
    def chk(recs, rg):
        assert rg == [(0, 19), (19, 38), (38, 57)] and not any(stored(r) for r in recs[19:38]) and all(stored(r) for r in recs[:19] + recs[38:])
    cases["range_without_names"] = (chain[:19] + [_edge_unstored(k) for k in range(19)] + chain[19:], 72, (3,), chk)

    # stale bl.  Only the first range has 11-column lines, and the last of them leaves a bl behind under which every line of the second range is dropped
    def chk(recs, rg):
        assert rg == [(0, 19), (19, 38)] and all(r["bl"] is not None for r in recs[:19]) and all(r["bl"] is None for r in recs[19:]) and recs[18]["bl"] == _EDGE_POISON
    cases["bl_first_range_only"] = (with_bl(chain, lambda k: k < 19, poison=(18,)), 72, (2,), chk)
    # only the last range has them: the first inherits 0
    def chk(recs, rg):
        assert rg == [(0, 19), (19, 38)] and all(r["bl"] is None for r in recs[:19]) and all(r["bl"] is not None for r in recs[19:])
    cases["bl_last_range_only"] = (with_bl(chain, lambda k: k >= 19), 72, (2,), chk)
    # three ranks, the middle range has none: the third range's lines in front of its first 11-column line inherit the first range's last bl ACROSS the second
    def chk(recs, rg):
        assert rg == [(0, 13), (13, 26), (26, 38)] and recs[12]["bl"] == _EDGE_POISON and all(r["bl"] is None for r in recs[13:30]) and recs[30]["bl"] == recs[30]["ml"]
        assert all(r["bl"] is None for r in recs[31:])
    cases["bl_middle_range_has_none"] = (with_bl(chain, lambda k: k < 13 or k == 30, poison=(12,)), 72, (3,), chk)
    # no range has any: every rank takes part in the exchange, nobody has anything to say
    def chk(recs, rg):
        assert all(r["bl"] is None for r in recs) and len(rg) in (2, 3)
    cases["bl_nowhere"] = (with_bl(chain, lambda k: False), 72, (2, 3), chk)

    # a name first seen as a TARGET in the first range with one length, then as a query in the second with another: the first length wins
    def chk(recs, rg):
        assert rg == [(0, 19), (19, 38)]
        first = next(k for k, r in enumerate(recs) if "r05" in (r["q"], r["t"]))
        assert first < 19 and recs[first]["t"] == "r05" and recs[first]["tl"] == _EDGE_LEN
        assert all(r["q"] != "r05" for r in recs[:19]) and [r["ql"] for r in recs[19:] if r["q"] == "r05"] == [12000] * 4
    cases["name_crosses_a_border"] = ([dict(r, ql=12000) if r["q"] == "r05" else r for r in chain], 72, (2,), chk)

    # one range with names of 1..8 bytes only, the other with a name of 13: the ranks choose different local dictionary forms and the merge compares bytes
    long_name = "r11_long_name"
    def chk(recs, rg):
        assert rg == [(0, 19), (19, 38)] and all(1 <= len(x) <= 8 for x in names(recs[:19])) and long_name in names(recs[19:]) and len(names(recs[:19]) & names(recs[19:])) >= 4
    cases["mixed_name_lengths"] = ([dict(r, t=long_name) if r["t"] == "r11" else r for r in chain], 80, (2,), chk)

    # every name in every range: the gathered rows are W times the distinct names
    def chk(recs, rg):
        assert rg == [(0, 19), (19, 38)] and names(recs[:19]) == names(recs[19:]) == names(recs) and len(names(recs)) == _EDGE_READS
    cases["every_name_in_every_range"] = (chain[0::2] + chain[1::2], 72, (2,), chk)

    # nothing stored anywhere
    def chk(recs, rg):
        assert not any(stored(r) for r in recs) and all(b > a for a, b in rg)
    cases["nothing_stored"] = ([_edge_unstored(k) for k in range(6)], 72, (2, 3), chk)
    return cases


# cases on which the right answer is an empty GFA: too few lines, or (the two bl cases) so many lines dropped under the inherited bl that nothing assembles --
# a rank that inherited 0 instead would keep its lines and write a unitig
_EDGE_EMPTY_GFA = ("more_ranks_than_lines", "nothing_stored", "bl_first_range_only", "bl_middle_range_has_none")


@pytest.mark.parametrize("case", sorted(_edge_cases()))
def test_byte_range_ingest_at_its_edges(case, tmpdir_s):
    """`MA_GPUS=N miniasm text.paf` on hand-made texts of at most 57 lines that put the edges of the sharded reader (csrc/paf.hip: the cross-range counts, the stale bl
    across ranges, the merged dictionary) on chosen ranks: empty ranges, a range without names, 11-column lines in the first / the last / not the middle / no range, a
    name that crosses a border with two lengths, ranges that choose different local dictionary forms, every name in every range, nothing stored.  stdout and the
    reader's own summary (records read, hits stored, names, total length) equal the one-rank run's and, when it is built, the reference binary's; the `rank g of N:
    bytes [a, b)` lines on stderr must show the split the case was built for."""
    import re
    import subprocess
    recs, width, worlds, check = _edge_cases()[case]
    lines = _edge_text(recs, width)
    paf = os.path.join(tmpdir_s, "edge_%s.paf" % case)
    with open(paf, "wb") as fo:
        fo.write(b"".join(lines))
    size = os.path.getsize(paf)
    summary = lambda err: re.findall(r"read (\d+) hits; stored (\d+) hits and (\d+) sequences \((\d+) bp\)", err)
    env1 = dict(os.environ)
    env1.pop("MA_GPUS", None)
    r1 = subprocess.run([ma.CLI_PATH, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env1, timeout=120)
    assert r1.returncode == 0, r1.stderr.decode()[-2000:]
    one, one_sum = r1.stdout, summary(r1.stderr.decode())
    assert len(one_sum) == 1
    assert (b"\na\t" in b"\n" + one) == (case not in _EDGE_EMPTY_GFA), "the case is built to assemble (or not): it would no longer test what it says"
    if R.have_ref():
        ref, ref_err = R.run_cli(R.REF_BIN, [], paf)
        assert one == ref and one_sum == summary(ref_err), "one rank differs from the reference"
    for world in worlds:
        split = _edge_split(lines, world)
        check(recs, [(a, b) for a, b, _, _ in split])
        env = dict(os.environ, MA_GPUS=str(world), MA_COMM="shm", MA_PIPE_TIMING="1")
        r = subprocess.run([ma.CLI_PATH, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
        err = r.stderr.decode()
        assert r.returncode == 0, err[-2000:]
        spans = sorted((int(g), int(a), int(b)) for g, a, b in re.findall(r"rank (\d+) of %d: bytes \[(\d+), (\d+)\) of %d;" % (world, size), err))
        assert spans == [(g, a, b) for g, (_, _, a, b) in enumerate(split)], "the ranks did not get the lines the case puts on them: %r" % spans
        assert r.stdout == one, "%d ranks: GFA differs from the one-rank run's" % world
        assert summary(err) == one_sum, "%d ranks: %r, one rank: %r" % (world, summary(err), one_sum)


@pytest.mark.parametrize("who", ["one_gpu", "child", "parent"])
def test_cli_on_n_ranks_never_leaves_a_rank_waiting(who, tmpdir_s):
    """no rank is ever left waiting: a request the sharded head does not serve (hit dumps, early -S stages, -1 / -2) is decided before the ranks
    exist and runs on one GPU with the same output; when one rank dies in the middle, the others are not left in a collective (children die
    with the parent, the parent stops when a child ends abnormally)"""
    import subprocess
    import time
    if who != "one_gpu" and not getattr(ma, "IS_EMU", False) and os.environ.get("MA_TEST_KILL") != "1":
        pytest.skip("kills ranks in the middle of a run: host-side process handling, exercised on the CPU build; MA_TEST_KILL=1 runs it on the GPU")
    paf = R.pafgen(os.path.join(tmpdir_s, "shc_fail.paf"), 800, 12000, 7, [])
    env = dict(os.environ, MA_GPUS="3", MA_COMM="shm")
    if who == "one_gpu":
        for args in (["-p", "paf"], ["-p", "sg", "-S3"], ["-1"], ["-2", "-p", "sg"], ["-p", "bed"]):
            r = subprocess.run([ma.CLI_PATH] + args + [paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
            assert r.returncode == 0 and b"runs on one GPU" in r.stderr
            assert r.stdout == R.run_cli(ma.CLI_PATH, args, paf)[0]
    else:
        env["MA_TEST_FAIL_RANK"] = "1" if who == "child" else "0"
        t0 = time.time()
        r = subprocess.run([ma.CLI_PATH, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
        assert r.returncode != 0 and time.time() - t0 < 60
    time.sleep(0.5)
    left = subprocess.run(["pgrep", "-f", paf], stdout=subprocess.PIPE).stdout.split()
    assert not left, "ranks still alive: %r" % left


@pytest.mark.skipif(ma.lib().mahip_device_count() < 2, reason="needs two GPUs (RCCL refuses two ranks on one device)")
def test_cli_on_two_gpus_over_rccl(tmpdir_s):
    import subprocess
    paf = R.pafgen(os.path.join(tmpdir_s, "shc_rccl.paf"), 6000, 200000, 83, ["-L", "uniform", "-d", "0.3", "-x", "0.03"])
    one, _ = R.run_cli(ma.CLI_PATH, [], paf)
    env = dict(os.environ, MA_GPUS="2")
    env.pop("MA_COMM", None)
    r = subprocess.run([ma.CLI_PATH, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == one


@pytest.mark.skipif(getattr(ma, "IS_EMU", False), reason="RCCL needs a GPU")
def test_cli_on_one_rank_really_calls_rccl(tmpdir_s):
    """MA_GPUS=1 MA_RCCL_ONE_RANK=1: the sharded runner (host/sharded.c) on a ONE-rank RCCL communicator with the one-rank short cuts off -- every
    ncclAllGather / ncclAllReduce of the step is issued on the context's stream (symbol binding, datatypes, in-place reduction, ordering against the
    kernels around them), which is as much of the RCCL path as a box with one GPU can run.  Output = the plain single-GPU run's, tie-rich input included."""
    import subprocess
    for k, extra in enumerate((["-L", "uniform", "-d", "0.3", "-x", "0.03"], ["-q", "16", "-L", "uniform", "-d", "0.3", "-x", "0.03"])):
        paf = R.pafgen(os.path.join(tmpdir_s, "shc_rccl1_%d.paf" % k), 5000, 150000, 84 + k, extra)
        one, _ = R.run_cli(ma.CLI_PATH, [], paf)
        env = dict(os.environ, MA_GPUS="1", MA_RCCL_ONE_RANK="1")
        env.pop("MA_COMM", None)
        r = subprocess.run([ma.CLI_PATH, paf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == one


def test_rccl_loads_and_initialises_a_one_rank_communicator():
    """librccl is opened at run time (dlopen); a one-rank communicator comes up on this GPU and the collectives degenerate to copies"""
    L = ma.lib()
    L.mahip_comm_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    L.mahip_comm_all_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.mahip_comm_destroy.argtypes = [C.c_void_p]
    L.mahip_comm_world.argtypes = [C.c_void_p]
    ctx = ma.Ctx(0)
    idb = C.create_string_buffer(128)
    ma._chk(L.mahip_comm_unique_id(idb), "comm_unique_id")
    ma._chk(L.mahip_comm_init(ctx.h, idb.raw, 0, 1), "comm_init")
    assert L.mahip_comm_world(ctx.h) == 1
    a = torch.arange(1000, dtype=torch.uint8, device="cuda")
    b = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    ma._chk(L.mahip_comm_all_gather(ctx.h, a.data_ptr(), b.data_ptr(), 1000), "all_gather")
    ma._chk(L.mahip_sync(ctx.h), "sync")
    assert torch.equal(a, b)
    L.mahip_comm_destroy(ctx.h)
    ctx.close()


def test_a_table_of_read_ranges_describes_one_upload():
    """round-4 review, What's weak #9: a table of read ranges (mahip_set_shard_bounds / mahip_hits_balance) used to survive a new input with the same number
    of reads, so a second input of equal read count silently got the stale ranges.  Like the hints and the positions it now describes ONE upload: every
    upload / adopt forgets it, the caller installs it again behind the records (bench.py and tests/shard_step_worker.py do)."""
    L = ma.lib()
    L.mahip_set_shard_bounds.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]
    L.mahip_shard_bounds.restype = C.POINTER(C.c_uint32)
    L.mahip_shard_bounds.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    ctx = ma.Ctx(0)
    try:
        hits = np.zeros(64, dtype=ma.HIT_DT)
        hits["qns"] = (np.arange(64, dtype=np.uint64) % np.uint64(8)) << np.uint64(32)
        hits["tn"] = (np.arange(64) + 1) % 8
        ctx.hits_upload(hits, 8)
        b = (C.c_uint32 * 3)(0, 5, 8)
        ma._chk(L.mahip_set_shard_bounds(ctx.h, b, 2), "set_shard_bounds")
        w = C.c_int(-1)
        p = L.mahip_shard_bounds(ctx.h, C.byref(w))
        assert w.value == 2 and [p[0], p[1], p[2]] == [0, 5, 8]
        ctx.hits_upload(hits, 8)  # the same number of reads: until round 4 the table stayed
        p = L.mahip_shard_bounds(ctx.h, C.byref(w))
        assert w.value == 0 and not p, "a table of read ranges survived the next upload"
    finally:
        ctx.close()
