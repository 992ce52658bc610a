"""The sharded PAF ingest (csrc/paf.hip: paf_cross_counts, paf_stale_bl with its exchange, paf_dict_merged and the k_dict_merge / k_merge_* / k_name_rows
kernels), the record routing (csrc/hits.hip: mahip_hits_route, k_rec_keep / k_rec_compact / k_rec_positions / k_add_u32) and the collectives they go through
(csrc/comm.hip: the shared-memory double), rank by rank: W child processes (tests/ingest_rank_worker.py, one context each, one device) walk a list of hand-built
texts through mahip_paf_load_fd_range + mahip_paf_parse_sharded + mahip_hits_route on byte ranges the TEST cut, so that a case can put any line on any rank, and
write down what the context holds behind the parse (info, report, flags and number columns, dictionary, records) and behind the route (bounds, records,
positions, n_total, bytes_sent).

Expected values never come from the sharded code: tests/pafmodel.py on the WHOLE text (tests/test_gpu_ingest_edges.py holds that model to the one-context
reader, the host reader and the reference library) gives names, first-seen lengths, ids, the bl of every line and the records in input order; the read ranges
are stages.balance_model (the rule stated for mahip_hits_balance) of the model's query ids.  Everything is an integer: equality everywhere.  Every case asserts,
from the model, that it has the shape it was written for (shape_of).

Per case and rank r with the lines [l0, l1) (check_case): the totals and the rank's own counts of mahip_paf_info_t, the report's n_lines; the valid / stored
flags and the bl of every valid line; the dictionary byte for byte on every rank; the records of the rank's lines with global ids; the bounds; the routed
records (query id in the rank's read range, input order) and their positions in the model's record array; n_total; bytes_sent.

Worlds 2, 3, 5 and 8 (nine processes with the device open), world 3 once more with 4 KiB slots of the shared-memory segment, world 1 in this process.
World 8 takes mahip_comm_all_gather_u64 through its second chunk of 32 words (40 words of line counts, 64 of record counts).

Not reachable: W * stride_rows == 257 (a prime: no world divides it) -- the cases stand on the largest multiple of W up to 256 and on the next one above.
Left out on purpose: the RCCL path (one GPU per rank: test_cli_on_two_gpus_over_rccl), the failure branches of mahip_hits_route (they would need a rank
that fails on purpose), ingest_sharded.c's own line_start_at (the end-to-end cases of tests/test_gpu_sharded.py check its spans)."""
import json
import os
import signal
import subprocess
import sys
import time

import numpy as np
import pytest

import miniasm_amd as ma
import pafmodel as PM
import stages as ST

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MIN_SPAN, MIN_MATCH = 2000, 100
TIME_LIMIT = 600  # seconds for ALL cases of one world (a few seconds on a device; the CPU build with guard pages takes longer)


# --------------------------------------------------------------------------------------------- lines
def ln(q, t, ql=9000, tl=8000, qs=10, qe=5000, ts=20, te=5010, ml=800, bl=4990, st="+", ncol=12):
    f = [q, ql, qs, qe, st, t, tl, ts, te, ml, bl, "255"]
    f = [x if isinstance(x, bytes) else str(x).encode("latin-1") for x in f]
    return b"\t".join(f[:ncol])


def drop(q, t, **kw):
    """a valid line the filter drops (span 10 < MIN_SPAN): parsed, counted, not stored -- its names get no id"""
    return ln(q, t, qs=10, qe=20, **kw)


JUNK = b"not\ta\tpaf\tline"


def pair_lines(names, k0=0, **kw):
    """stored lines that show exactly these names, two per line (an odd one out: a line whose query and target are that name, with two lengths)"""
    out = [ln(names[i], names[i + 1], qs=(k0 + i) % 900, ql=9000 + i, tl=8000 + i, **kw) for i in range(0, len(names) - 1, 2)]
    if len(names) % 2:
        out.append(ln(names[-1], names[-1], ql=7000, tl=7001, qs=(k0 + len(names)) % 900, **kw))
    return out


def pool_lines(n, k0, n_names=40, **kw):
    """n stored lines over a pool of names shared by all ranges, query != target"""
    assert n_names % 2 == 0  # (6 k + 3 is odd: query and target never meet)
    return [ln("p%d" % ((k0 + j) % n_names), "p%d" % ((7 * (k0 + j) + 3) % n_names), qs=(k0 + j) % 977, ql=9000 + (k0 + j) % 13, tl=8000 + (k0 + j) % 7, **kw) for j in range(n)]


class Case:
    def __init__(self, ranges, bi_dir=1):
        self.ranges, self.bi_dir = ranges, bi_dir


def spread(W, per_rank):
    """per_rank: {rank or negative rank: lines}; every other rank gets an empty range"""
    out = [[] for _ in range(W)]
    for r, lines in per_rank.items():
        out[r % W] = lines
    return out


# --------------------------------------------------------------------------------------------- the cases: name -> builder(W) -> Case, or None where W is too small
SIZE_PATTERN = [0, 1, 255, 256, 257, 0, 0, 256]


def c_sizes(rot):
    def build(W):
        if (W >= 5 and rot not in (0, 3)) or (W == 3 and rot == 4):
            return None
        sizes = [SIZE_PATTERN[(rot + r) % 8] for r in range(W)]
        k, ranges = 0, []
        for n in sizes:
            ranges.append(pool_lines(n, k))
            k += n
        return Case(ranges, bi_dir=0)  # one record per line: the ranks hold 0 / 1 / 255 / 256 / 257 records in front of the route
    return build


def c_empties(which):
    def build(W):
        pat = {2: ["01", "10"], 3: ["010", "101"], 5: ["01001", "10010"], 8: ["01001100", "10010011"]}[W][which]
        k, ranges = 0, []
        for ch in pat:
            ranges.append(pool_lines(40, k) if ch == "1" else [])
            k += 40
        return Case(ranges)
    return build


def c_more_ranks_than_lines(W):
    return Case(spread(W, {r: pool_lines(1, r) for r in range(max(1, W // 2))}))


def c_one_rank_holds_all(W):
    return Case(spread(W, {W // 2: pool_lines(300, 0)}))


def c_invalid_and_unstored_ranges(W):
    """range 0: valid lines of which none is stored; range 1: lines of which none is valid; the last range stores -- its first name gets id 0"""
    ranges = [[drop("u%d" % k, "v%d" % k, bl=100 + k) for k in range(7)], [JUNK, b"", JUNK + b"\tx", b"\t" * 8]]
    ranges += [[drop("u%d" % k, "last_q", bl=200 + k) for k in range(3)] for _ in range(W - 3)]
    ranges.append([ln("last_q", "last_t", ql=4321, tl=1234), ln("last_t", "u0", ql=99, tl=98)])
    return Case(ranges[:W - 1] + [ranges[-1]])


def c_nothing_stored(W):
    return Case([[drop("a%d" % r, "b%d" % k) for k in range(r + 1)] + [JUNK] * (r % 2) for r in range(W)])


def c_sum_rows(n):
    """the ranks' tables hold n names together (gcap = pow2_at_least(2 n + 1024): 2048 up to n = 512, 4096 from 513 on); ten names are in every table"""
    def build(W):
        if n < 10 * W:  # n = 1: one line whose query and target are the same name with two lengths, on the last rank
            return Case(spread(W, {-1: pair_lines(["same"]), 0: [drop("same", "other", ql=5)]}))
        own = n - 10 * W
        per = [own // W + (1 if r < own % W else 0) for r in range(W)]
        shared = ["sh%d" % k for k in range(10)]
        return Case([pair_lines(["n%d_%d" % (r, k) for k in range(per[r] // 2)] + shared + ["n%d_%d" % (r, k) for k in range(per[r] // 2, per[r])], k0=r) for r in range(W)])
    return build


def c_stride_rows(above):
    """one rank holds the largest table, the others 0 or 1 names: W * stride_rows on the largest multiple of W up to 256 (255 at worlds 3 and 5, 256 at 2 and
    8) and on the next multiple above 256 -- the grids of k_dict_merge; the rows behind a short table are padding nobody wrote"""
    def build(W):
        stride = 256 // W + (1 if above else 0)
        big = W // 2
        per = {big: pair_lines(["big%d" % k for k in range(stride)])}
        for k, r in enumerate(x for x in range(W) if x != big):
            if k % 2 == 1:
                per[r] = pair_lines(["big%d" % (stride - 1 - r)])  # one name, known to the big table
        return Case(spread(W, per))
    return build


def c_name_bytes(nb):
    """the largest block of name bytes is 15 / 16 / 17 bytes (stride_bytes is rounded up to 16: 16, 16, 32); another range has none"""
    def build(W):
        a, b = {15: (6, 7), 16: (7, 7), 17: (7, 8)}[nb]
        per = {-1: pair_lines(["x" * a, "y" * b]), 0: [drop("x" * a, "zz")]}
        if W > 2:
            per[1] = pair_lines(["y" * b])
        return Case(spread(W, per))
    return build


def c_every_name_everywhere(W):
    names = ["e%d" % k for k in range(24)]
    return Case([pair_lines(names[r % 24:] + names[:r % 24], k0=r) for r in range(W)])


def c_no_name_shared(W):
    return Case([pair_lines(["r%d_%d" % (r, k) for k in range(9 + r)], k0=r) for r in range(W)])


def c_prefixes(W):
    """a name that is a prefix of another, across ranks, at 3 / 4 and 8 / 9 bytes (the short-key and the text form of the local tables)"""
    return Case(spread(W, {0: [ln("abc", "abcdefgh", ql=1, tl=2)], -1: [ln("abcd", "abcdefghi", ql=3, tl=4), ln("abcdefgh", "abc", ql=5, tl=6), ln("ab", "abcdefghij", ql=7, tl=8)]}))


def c_name_lengths(W):
    """names of 1, 8, 9 and 255 bytes: a range with short names only keeps its local table by key, one with a long name by text"""
    long9, long255 = "L" * 9, "M" * 255
    per = {0: [ln("a", "bbbbbbbb", ql=11, tl=12), ln("c", "a", ql=13, tl=14)], -1: [ln(long9, "bbbbbbbb", ql=15, tl=16), ln(long255, "a", ql=17, tl=18), ln(long255[:254], long9, ql=19, tl=20)]}
    if W > 2:
        per[1] = [ln("bbbbbbbb", "c", ql=21, tl=22), ln("d", "d", ql=23, tl=24)]
    return Case(spread(W, per))


def c_first_seen_across_a_border(W):
    """a name first seen as a target on the last line of range r and as a query with another length on the first line of range r + 1; and the reverse"""
    ranges = [[] for _ in range(W)]
    ranges[0] = [ln("s0", "s1", ql=100, tl=101), ln("s2", "edge_a", ql=102, tl=555)]
    ranges[1] = [ln("edge_a", "s0", ql=666, tl=103), ln("s1", "s2", ql=104, tl=105), ln("edge_b", "s1", ql=777, tl=106)]
    if W > 2:
        ranges[2] = [ln("s0", "edge_b", ql=107, tl=888)]
    else:
        ranges[1].append(ln("s0", "edge_b", ql=107, tl=888))
    return Case(ranges)


def ten(k, **kw):
    return ln("q%d" % (k % 17), "t%d" % (k % 5), qs=k % 800, ncol=10, **kw)


def c_stale(where):
    """lines with a `bl` column in the first range only / the last range only / in none; every other range has 10-column lines, which inherit"""
    def build(W):
        ranges = [[ten(10 * r + k) for k in range(4 + r)] for r in range(W)]
        if where == "first":
            ranges[0] = [ten(0), ln("q0", "t0", bl=1111), ten(1), ln("q1", "t1", bl=2222)]  # (no 10-column line behind its last bl: what it leaves is 2222)
        elif where == "last":
            ranges[-1] = [ten(90), ln("q0", "t0", bl=3333), ten(91)]
        return Case(ranges)
    return build


def c_stale_five(W):
    """`bl` columns in range 0 and range 3, none in 1 and 2, range 2 empty, range 4 (and up) 10-column lines only; a distinct bl per source"""
    if W < 5:
        return None
    ranges = [[ln("q0", "t0", bl=1000), ten(1), ln("q1", "t1", bl=1001)], [ten(2), ten(3)], [], [ten(4), ten(5), ln("q2", "t2", bl=3000), ten(6), ln("q3", "t3", bl=3001), ten(7)]]
    ranges += [[ten(10 + r), ten(20 + r)] for r in range(4, W)]
    return Case(ranges)


def c_stale_only_line(pos, kind):
    """a range's only line with a `bl` column is its first / its last line; kind: a plain one, one the byte-wise routine parses (a blank in front of the
    number), one that is not stored.  The range behind it has 10-column lines only and no line with a bl of its own; the last range has no 10-column line"""
    def build(W):
        if W < 3:
            return None
        src = {"plain": ln("q0", "t0", bl=4242), "odd": ln("q0", "t0", bl=b" 4243"), "unstored": drop("q0", "t0", bl=4244)}[kind]
        mid = [ten(1), ten(2), ten(3)]
        ranges = [[ln("q5", "t5", bl=77), ten(0)], ([src] + mid) if pos == "first" else (mid + [src]), [ten(4), ten(5)]]
        ranges += [[ten(30 + r)] for r in range(3, W - 1)]
        if W > 3:
            ranges.append([ln("q6", "t6", bl=88), ln("q7", "t7", bl=89)])
        return Case(ranges)
    return build


def c_one_read_all_hits(W):
    """every record has the same query: the ranks between the first and the last own no read"""
    return Case([[ln("hub", "s%d" % ((7 * r + k) % 23), qs=(50 * r + k) % 900) for k in range(20 + r)] for r in range(W)], bi_dir=0)


def c_all_on_their_owner(W):
    """every record already stands on the rank that owns its query read: nothing is sent"""
    return Case([[ln("own%d" % r, "tgt", qs=k) for k in range(60)] for r in range(W)], bi_dir=0)


def c_all_on_the_wrong_rank(W):
    """rank 0 has no line, rank r's records belong to rank r - 1 (ids go by first appearance, so read 0 is always rank 0's)"""
    return Case([[]] + [[ln("own%d" % r, "tgt", qs=k) for k in range(60)] for r in range(1, W)], bi_dir=0)


def c_second_chunk(W):
    """world 8 only: 5 x 8 = 40 words of line counts and 8 x 8 = 64 words of record counts -- the ranks 6 and 7 (words 30 .. 39) and the rows of the ranks 4 .. 7
    (words 32 .. 63) decide the totals, the ids, the stale bl and what is received"""
    if W != 8:
        return None
    ranges = [[ln("q%d" % (r % 3), "t%d" % r, qs=100 * r + k, bl=500 + r) for k in range(3 + r)] + [ten(100 + r, qe=5000 + r)] + [JUNK] * r for r in range(W)]
    ranges[7] = ranges[7] + [ln("late_%d" % k, "q%d" % (k % 3), qs=900 + k) for k in range(12)]
    return Case(ranges)


def c_small_slots(W):
    """4 KiB slots (128 records): three hub reads of 500 records; rank 0 sends read B 300 records (three rounds) and read C none, rank 1 sends A 100 (one
    round) and C 300, rank 2 sends A 200 and B 100 -- rounds of unequal length, rounds in which a rank has nothing to send.  256 names / 4096 name bytes /
    1024 reads per range are the limits of the all-gathers and the all-reduce behind one slot: three names here"""
    if W != 3:
        return None
    plan = [dict(A=200, B=300, C=0), dict(A=100, B=100, C=300), dict(A=200, B=100, C=200)]
    ranges, k = [], 0
    for r in range(3):
        todo = dict(plan[r])
        lines = []
        while sum(todo.values()):
            for h in "ABC":  # interleaved: the records of one destination do not stand together
                if todo[h]:
                    todo[h] -= 1
                    lines.append(ln(h, "B" if h != "B" else "A", qs=k % 4000, qe=3000 + k))
                    k += 1
        ranges.append(lines)
    return Case(ranges, bi_dir=0)


CASES = {"sizes_rot%d" % k: c_sizes(k) for k in range(5)}
CASES.update({"empties_a": c_empties(0), "empties_b": c_empties(1), "more_ranks_than_lines": c_more_ranks_than_lines, "one_rank_holds_all": c_one_rank_holds_all,
              "invalid_and_unstored_ranges": c_invalid_and_unstored_ranges, "nothing_stored": c_nothing_stored})
CASES.update({"sum_rows_%d" % n: c_sum_rows(n) for n in (1, 511, 512, 513)})
CASES.update({"stride_rows_at_256": c_stride_rows(False), "stride_rows_above_256": c_stride_rows(True)})
CASES.update({"name_bytes_%d" % n: c_name_bytes(n) for n in (15, 16, 17)})
CASES.update({"every_name_everywhere": c_every_name_everywhere, "no_name_shared": c_no_name_shared, "prefixes": c_prefixes, "name_lengths": c_name_lengths,
              "first_seen_across_a_border": c_first_seen_across_a_border})
CASES.update({"stale_%s" % w: c_stale(w) for w in ("first", "last", "none")})
CASES["stale_five"] = c_stale_five
CASES.update({"stale_only_%s_%s" % (p, k): c_stale_only_line(p, k) for p in ("first", "last") for k in ("plain", "odd", "unstored")})
CASES.update({"one_read_all_hits": c_one_read_all_hits, "all_on_their_owner": c_all_on_their_owner, "all_on_the_wrong_rank": c_all_on_the_wrong_rank, "second_chunk": c_second_chunk})
SMALL_SLOT_CASES = {"small_slots": c_small_slots}

RUNS = {"2": (2, None), "3": (3, None), "5": (5, None), "8": (8, None), "3s": (3, 12)}  # run -> (world, MA_SHM_SLOT_LOG2)
_BUILT = {}


def built_case(run, name):
    """(Case with text, line cuts, byte ranges and model M) or None; built once"""
    if (run, name) not in _BUILT:
        W = RUNS[run][0]
        c = (SMALL_SLOT_CASES if run == "3s" else CASES)[name](W)
        if c is not None:
            assert len(c.ranges) == W, (name, W, len(c.ranges))
            c.world, c.name = W, name
            c.cuts = np.r_[0, np.cumsum([len(x) for x in c.ranges])].astype(np.int64)
            blocks = [b"".join(l + b"\n" for l in x) for x in c.ranges]
            c.text = b"".join(blocks)
            off = np.r_[0, np.cumsum([len(b) for b in blocks])]
            c.bytes = [(int(off[r]), len(blocks[r])) for r in range(W)]
            c.M = None
        _BUILT[(run, name)] = c
    return _BUILT[(run, name)]


PAIRS = [(run, name) for run in RUNS for name in (SMALL_SLOT_CASES if run == "3s" else CASES) if built_case(run, name) is not None]


# --------------------------------------------------------------------------------------------- the ranks
_RANK_DIED = []  # a worker died of a signal or ran into its time limit: nothing more is started on the device


def kill_all(procs):
    for p in procs:
        if p.poll() is None:
            try:
                os.killpg(p.pid, signal.SIGKILL)  # (the process group: `timeout` and the rank under it)
            except ProcessLookupError:
                pass
    for p in procs:
        p.wait()


def run_world(run, tmp):
    """start the W ranks together, wait for all of them under one time limit, end all of them as soon as one fails (a rank that lost its peers would spin in the
    barrier of the shared-memory double for ever); -> {case name: [npz of rank 0, ...]}"""
    assert not _RANK_DIED, "a rank of %s died of a signal or hung: no further ranks are started" % _RANK_DIED[0]
    W, slot = RUNS[run]
    names = [n for r, n in PAIRS if r == run]
    out_dir = os.path.join(tmp, "ingest_ranks_%s" % run)
    os.makedirs(out_dir)
    job = []
    for n in names:
        c = built_case(run, n)
        path = os.path.join(out_dir, n + ".paf")
        with open(path, "wb") as f:
            f.write(c.text)
        job.append(dict(name=n, path=path, ranges=c.bytes, min_span=MIN_SPAN, min_match=MIN_MATCH, bi_dir=c.bi_dir))
    job_path = os.path.join(out_dir, "job.json")
    with open(job_path, "w") as f:
        json.dump(job, f)
    env = dict(os.environ, MA_WORKER_EMU="1" if getattr(ma, "IS_EMU", False) else "0")
    for k in ("MA_GPUS", "MA_SHM_SLOT_LOG2", "MA_SHM_SERIAL", "MA_PAF_TILE_K", "MA_DICT_CAP_LOG2", "MA_DICT_EXACT_TEXT"):
        env.pop(k, None)
    if slot is not None:
        env["MA_SHM_SLOT_LOG2"] = str(slot)
    seg = "ma_ingest_%d_%s" % (os.getpid(), run)
    procs, errs = [], []
    t0 = time.monotonic()
    try:
        for r in range(W):
            errs.append(open(os.path.join(out_dir, "stderr.r%d" % r), "wb"))
            procs.append(subprocess.Popen(["timeout", "-k", "10", str(TIME_LIMIT), sys.executable, os.path.join(HERE, "ingest_rank_worker.py"), str(r), str(W), seg, job_path, out_dir],
                                          env=env, stdout=subprocess.DEVNULL, stderr=errs[-1], start_new_session=True))
        bad = None
        while bad is None and any(p.poll() is None for p in procs):
            for r, p in enumerate(procs):
                try:
                    rc = p.wait(timeout=0.02)
                except subprocess.TimeoutExpired:
                    continue
                if rc != 0:
                    bad = (r, rc)
                    break
            if bad is None and time.monotonic() - t0 > TIME_LIMIT:
                bad = (-1, 124)
        if bad is not None:
            kill_all(procs)
            r, rc = bad
            if rc < 0 or rc >= 124:
                _RANK_DIED.append("world %s (rank %d, status %d)" % (run, r, rc))
            tail = b"".join(open(os.path.join(out_dir, "stderr.r%d" % k), "rb").read()[-1500:] for k in range(W)).decode("latin-1")
            pytest.fail("world %s: rank %d ended with status %d after %.1f s\n%s" % (run, r, rc, time.monotonic() - t0, tail))
    finally:
        kill_all(procs)
        for f in errs:
            f.close()
        try:
            os.unlink("/dev/shm/" + seg)  # (rank 0 removes the name once every rank has mapped it; a run that ended before that leaves it)
        except OSError:
            pass
    wall = time.monotonic() - t0
    print("world %s: %d cases on %d ranks in %.2f s" % (run, len(names), W, wall))
    return {n: [dict(np.load(os.path.join(out_dir, "%s.r%d.npz" % (n, r)))) for r in range(W)] for n in names}


_RESULTS = {}


@pytest.fixture(scope="module")
def world_run(request, tmpdir_s):
    """one run of the ranks per world, whatever its end: a world that failed is not started again"""
    run = request.param
    if run not in _RESULTS:
        try:
            _RESULTS[run] = run_world(run, tmpdir_s)
        except BaseException as e:
            _RESULTS[run] = e
            raise
    if isinstance(_RESULTS[run], BaseException):
        pytest.fail("world %s did not finish: %s" % (run, str(_RESULTS[run])[:3000]))
    return run, _RESULTS[run]


# --------------------------------------------------------------------------------------------- what is expected
def expected(c):
    """the model of the WHOLE text and what follows from it per rank; computed once per case and left unchanged"""
    if c.M is not None:
        return c.M
    M = PM.model(c.text, MIN_SPAN, MIN_MATCH, c.bi_dir)
    W = c.world
    assert M.L == c.cuts[-1]
    per_line = np.where(M.stored, 1 + ((M.qid != M.tid) & bool(c.bi_dir)), 0).astype(np.int64)
    M.roff = np.r_[0, np.cumsum(per_line)]
    assert M.roff[-1] == len(M.hits)
    M.rcuts = M.roff[c.cuts]                                     # records in front of every range
    M.rec_qid = (M.hits["qns"] >> np.uint64(32)).astype(np.int64)
    M.bounds = ST.balance_model(M.rec_qid, len(M.names), W)
    idx = np.arange(len(M.hits))
    M.src = np.searchsorted(M.rcuts, idx, side="right") - 1      # (of equal borders the last one opens the range)
    M.dst = np.searchsorted(np.asarray(M.bounds), M.rec_qid, side="right") - 1
    M.mat = np.zeros((W, W), dtype=np.int64)
    np.add.at(M.mat, (M.src, M.dst), 1)
    M.local_names = []
    for r in range(W):
        seen = []
        for i in range(c.cuts[r], c.cuts[r + 1]):
            if M.stored[i]:
                for nm in (M.qname[i], M.tname[i]):
                    if nm not in seen:
                        seen.append(nm)
        M.local_names.append(seen)
    M.rows = [len(x) for x in M.local_names]
    M.name_bytes = [sum(len(nm) + 1 for nm in x) for x in M.local_names]
    M.blob = b"".join(nm + b"\0" for nm in M.names)
    c.M = M
    return M


def check_case(c, M, got):
    W = c.world
    n_seq = len(M.names)
    for r in range(W):
        g, what = got[r], "%s, world %d, rank %d" % (c.name, W, r)
        l0, l1 = int(c.cuts[r]), int(c.cuts[r + 1])
        r0, r1 = int(M.rcuts[r]), int(M.rcuts[r + 1])
        n_lines, n_records, n_stored, n_hits, name_bytes, g_seq, max_qs, n_excl = (int(x) for x in g["info"])
        # info
        assert (n_lines, n_records, n_stored) == (M.L, int(M.valid.sum()), int(M.stored.sum())), "%s: totals %r" % (what, g["info"])
        assert n_hits == r1 - r0, "%s: n_hits %d, the model has %d records on its lines" % (what, n_hits, r1 - r0)
        assert max_qs == M.max_qs and n_excl == 0, "%s: max_qs %d, model %d" % (what, max_qs, M.max_qs)
        assert int(g["rep"][0]) == l1 - l0, "%s: the report counts %d lines, the range has %d" % (what, g["rep"][0], l1 - l0)
        # columns
        v = M.valid[l0:l1]
        assert ((g["flags"] & 1) == v).all() and ((g["flags"] >> 1 & 1) == M.stored[l0:l1]).all(), "%s: valid / stored flags" % what
        bad = np.flatnonzero(v & (g["nums"][7] != M.nums[7][l0:l1]))
        assert len(bad) == 0, "%s: bl of line %d (%d of its range): %d, model %d" % (what, l0 + bad[0], bad[0], g["nums"][7][bad[0]], M.nums[7][l0 + bad[0]])
        for k in range(7):
            assert (g["nums"][k][v] == M.nums[k][l0:l1][v]).all(), "%s: number column %d" % (what, k)
        # dictionary
        assert g_seq == n_seq and name_bytes == len(M.blob), "%s: %d names in %d bytes, model %d in %d" % (what, g_seq, name_bytes, n_seq, len(M.blob))
        assert g["names"].tobytes() == M.blob, "%s: names %r, model %r" % (what, g["names"].tobytes()[:200], M.blob[:200])
        assert g["lens"].tolist() == M.lens, "%s: first-seen lengths" % what
        # records behind the parse
        assert g["parsed"].tobytes() == M.hits[r0:r1].tobytes(), "%s: the records of its lines" % what
        # behind the route
        assert g["bounds"].tolist() == M.bounds, "%s: bounds %r, the stated rule gives %r" % (what, g["bounds"].tolist(), M.bounds)
        sel = M.dst == r
        assert len(g["routed"]) == int(sel.sum()), "%s: holds %d records behind the route, owns %d" % (what, len(g["routed"]), sel.sum())
        assert g["routed"].tobytes() == M.hits[sel].tobytes(), "%s: its records behind the route" % what
        assert g["pos"].tolist() == np.flatnonzero(sel).tolist(), "%s: positions" % what
        assert int(g["route"][0]) == len(M.hits) and (len(M.hits) == 0 or int(g["pos_total"][0]) == len(M.hits)), "%s: n_total %r / %r" % (what, g["route"], g["pos_total"])
        away = int(((M.src == r) & (M.dst != r)).sum())
        assert int(g["route"][1]) == 36 * away, "%s: bytes_sent %d, %d of its records belong to other ranks" % (what, g["route"][1], away)
        assert int(g["have_pos"][0]) == int(len(M.hits) > 0)


def shape_of(c, M, got):
    """every case has the shape it was written for -- from the model, and for what only the ranks know (the form of a local table) from their reports"""
    W, name = c.world, c.name
    sizes = np.diff(c.cuts).tolist()
    recs = np.diff(M.rcuts).tolist()
    hasbl = [int(M.hasbl[c.cuts[r]:c.cuts[r + 1]].sum()) for r in range(W)]
    nobl = [int((M.valid & ~M.hasbl)[c.cuts[r]:c.cuts[r + 1]].sum()) for r in range(W)]
    sent = [int(M.mat[r].sum() - M.mat[r, r]) for r in range(W)]
    bl = M.nums[7]
    if name.startswith("sizes_rot"):
        assert recs == sizes and set(sizes) <= {0, 1, 255, 256, 257} and len(set(sizes)) >= 2
        if W >= 5 and name == "sizes_rot0":
            assert set(sizes) == {0, 1, 255, 256, 257} and sizes[0] == 0
        if W == 8 and name == "sizes_rot0":
            assert sizes[5] == sizes[6] == 0
    elif name.startswith("empties"):
        assert 0 in sizes and 40 in sizes
    elif name == "more_ranks_than_lines":
        assert M.L < W and max(sizes) == 1
    elif name == "one_rank_holds_all":
        assert sorted(sizes)[:-1] == [0] * (W - 1) and sizes[W // 2] == 300
    elif name == "invalid_and_unstored_ranges":
        assert M.valid[:c.cuts[1]].all() and not M.stored[:c.cuts[1]].any() and (W < 3 or (sizes[1] > 0 and not M.valid[c.cuts[1]:c.cuts[2]].any()))
        assert not M.stored[:c.cuts[-2]].any() and M.names[0] == b"last_q" and M.lens[:2] == [4321, 1234] and M.names[2] == b"u0" and M.lens[2] == 98
    elif name == "nothing_stored":
        assert M.valid.any() and not M.stored.any() and len(M.names) == 0 and len(M.hits) == 0
    elif name.startswith("sum_rows_"):
        n = int(name.split("_")[-1])
        assert sum(M.rows) == n, "the tables hold %r names" % M.rows
        assert pow2_at_least(2 * n + 1024) == (2048 if n <= 512 else 4096)
        if n == 1:
            assert M.names == [b"same"] and M.lens == [7000] and len(M.hits) == 1, "one line, query == target, two lengths: the query's wins"
        else:
            assert len(M.names) == n - 10 * (W - 1), "ten names are in every table"
    elif name.startswith("stride_rows_"):
        stride = max(M.rows)
        assert sorted(M.rows)[-2] <= 1 and 0 in M.rows
        if name.endswith("at_256"):
            assert W * stride == (255 if W in (3, 5) else 256)
        else:
            assert 256 < W * stride <= 256 + W
    elif name.startswith("name_bytes_"):
        assert max(M.name_bytes) == int(name.split("_")[-1]) and 0 in M.name_bytes
    elif name == "every_name_everywhere":
        assert all(sorted(x) == sorted(M.names) for x in M.local_names) and len(M.names) == 24
        assert sent[0] > 0 and any(sent[r] > 0 and M.rcuts[r] > 0 for r in range(1, W)), "rank 0 sends (base 0) and a later rank sends (base > 0)"
    elif name == "no_name_shared":
        assert sum(M.rows) == len(M.names) and min(M.rows) >= 9
    elif name == "prefixes":
        assert {b"abc", b"abcd", b"abcdefgh", b"abcdefghi", b"ab", b"abcdefghij"} == set(M.names) and M.lens[M.names.index(b"abcdefgh")] == 2 and M.lens[M.names.index(b"abc")] == 1
    elif name == "name_lengths":
        assert {1, 8, 9, 254, 255} <= {len(x) for x in M.names}
        assert ma.PAF_DICT_FORMS[int(got[0]["rep"][2])] == "short" and ma.PAF_DICT_FORMS[int(got[W - 1]["rep"][2])] == "text", "the ranks chose different local forms"
    elif name == "first_seen_across_a_border":
        assert M.lens[M.names.index(b"edge_a")] == 555 and M.lens[M.names.index(b"edge_b")] == 777
        assert M.tname[c.cuts[1] - 1] == b"edge_a" and M.qname[c.cuts[1]] == b"edge_a"
    elif name.startswith("stale_") and name.split("_")[1] in ("first", "last", "none"):
        where = name.split("_")[1]
        assert all(n > 0 for n in nobl)
        if where == "first":
            assert hasbl[0] == 2 and sum(hasbl) == 2 and (bl[c.cuts[1]:] == 2222).all() and bl[0] == 0 and bl[2] == 1111
        elif where == "last":
            assert hasbl[-1] == 1 and sum(hasbl) == 1 and (bl[:c.cuts[-2] + 1] == 0).all() and bl[-1] == 3333
        else:
            assert sum(hasbl) == 0 and (bl == 0).all() and M.n_nobl == M.L
    elif name == "stale_five":
        assert hasbl[:4] == [2, 0, 0, 2] and sizes[2] == 0 and sum(hasbl[4:]) == 0
        assert (bl[c.cuts[1]:c.cuts[3] + 2] == 1001).all() and (bl[c.cuts[4]:] == 3001).all() and bl[c.cuts[3] + 3] == 3000
    elif name.startswith("stale_only_"):
        _, _, pos, kind = name.split("_")
        want = {"plain": 4242, "odd": 4243, "unstored": 4244}[kind]
        assert hasbl[1] == 1 and hasbl[2] == 0 and nobl[2] > 0 and (bl[c.cuts[2]:c.cuts[3]] == want).all()
        i = int(c.cuts[1]) if pos == "first" else int(c.cuts[2]) - 1
        assert M.hasbl[i] and bl[i] == want and bool(M.stored[i]) == (kind != "unstored") and M.odd[i] == (kind == "odd")
        assert (bl[c.cuts[1]:c.cuts[2]] == (want if pos == "first" else 77))[~M.hasbl[c.cuts[1]:c.cuts[2]]].all()
        if W > 3:
            assert nobl[-1] == 0 and sum(nobl) > 0, "a rank with no 10-column line of its own"
    elif name == "one_read_all_hits":
        assert len(set(M.rec_qid.tolist())) == 1 and M.bounds == [0] + [1] * (W - 1) + [len(M.names)] and (W == 2 or M.mat[:, 1].sum() == 0)
    elif name == "all_on_their_owner":
        assert sent == [0] * W and all(M.mat[r, r] == 60 for r in range(W))
    elif name == "all_on_the_wrong_rank":
        assert all(M.mat[r, r] == 0 for r in range(W)) and sum(sent) == len(M.hits) == 60 * (W - 1) and recs[0] == 0
    elif name == "second_chunk":
        assert 5 * W == 40 and W * W == 64, "both gathers go beyond one chunk of 32 words"
        for r in (6, 7):  # the words 30 .. 39: lines, valid, stored, 10-column lines, max_qs of the ranks 6 and 7
            assert sizes[r] > 0 and nobl[r] > 0 and M.stored[c.cuts[r]:c.cuts[r + 1]].sum() > 0
        assert int(M.nums[1][c.cuts[7]:].max()) == M.max_qs > int(M.nums[1][:c.cuts[6]].max()), "max_qs comes from the last rank"
        assert (M.mat[4:].sum(axis=1) > 0).all() and (M.mat[4:] > 0).sum() >= 8 and (M.mat[4:, :4] > 0).any(), "the rows 4 .. 7 of the count matrix (words 32 .. 63) hold records, for low ranks too"
    elif name == "small_slots":
        assert M.bounds == [0, 1, 2, 3] and M.names == [b"A", b"B", b"C"] and len(M.hits) == 1500
        assert M.mat.tolist() == [[200, 300, 0], [100, 100, 300], [200, 100, 200]]
        assert M.mat[0, 1] * 32 > 2 * 4096 and 0 < M.mat[2, 1] * 32 < 4096, "three rounds to rank 1: rank 2 has nothing to send in the second and third"
    else:
        raise KeyError(name)


def pow2_at_least(x):
    p = 1
    while p < x:
        p <<= 1
    return p


@pytest.mark.parametrize("world_run,name", PAIRS, indirect=["world_run"], ids=["%s-%s" % p for p in PAIRS])
def test_sharded_ingest(world_run, name):
    run, results = world_run
    c = built_case(run, name)
    M = expected(c)
    shape_of(c, M, results[name])
    check_case(c, M, results[name])


def test_every_stated_edge_has_a_case():
    """what the case list promises, over all worlds: range sizes, table sizes, name-byte sizes, both directions, every world"""
    sizes, rows, strides, nbytes, bi, recs = set(), set(), set(), set(), set(), set()
    for run, name in PAIRS:
        c = built_case(run, name)
        M = expected(c)
        sizes |= set(np.diff(c.cuts).tolist())
        recs |= set(np.diff(M.rcuts).tolist())
        rows.add(sum(M.rows))
        strides.add(c.world * max(M.rows + [1]))
        nbytes.add(max(M.name_bytes))
        bi.add(c.bi_dir)
    assert {0, 1, 255, 256, 257} <= sizes and {0, 1, 255, 256, 257} <= recs and {0, 1, 511, 512, 513} <= rows and {255, 256, 258, 260, 264} <= strides
    assert {0, 15, 16, 17} <= nbytes and bi == {0, 1} and {RUNS[r][0] for r, _ in PAIRS} == {2, 3, 5, 8}


def test_world_one_is_the_plain_parse(gpu_ctx, tmpdir_s):
    """without a communicator mahip_paf_parse_sharded is mahip_paf_parse, and mahip_hits_route leaves the records alone, sets the bounds [0, n_seq] and no positions"""
    import ingest_rank_worker as WK
    L = WK.bind(ma.lib())
    for name in ("sizes_rot1", "stale_first", "name_lengths", "nothing_stored"):
        c = CASES[name](3)
        text = b"".join(l + b"\n" for x in c.ranges for l in x)
        path = os.path.join(tmpdir_s, "world1_%s.paf" % name)
        with open(path, "wb") as f:
            f.write(text)
        M = PM.model(text, MIN_SPAN, MIN_MATCH, c.bi_dir)
        g = WK.run_case(L, gpu_ctx, path, 0, len(text), MIN_SPAN, MIN_MATCH, c.bi_dir, False)
        assert [int(x) for x in g["info"][:4]] == [M.L, int(M.valid.sum()), int(M.stored.sum()), len(M.hits)] and int(g["info"][6]) == M.max_qs
        assert int(g["rep"][1]) == int(M.n_nobl > 0), "the one-context stale-bl pass"
        assert ((g["flags"] & 1) == M.valid).all() and (g["nums"][7][M.valid] == M.nums[7][M.valid]).all()
        assert g["names"].tobytes() == b"".join(nm + b"\0" for nm in M.names) and g["lens"].tolist() == M.lens
        assert g["parsed"].tobytes() == M.hits.tobytes() and g["routed"].tobytes() == M.hits.tobytes()
        assert g["bounds"].tolist() == [0, len(M.names)] and g["route"].tolist() == [len(M.hits), 0] and int(g["have_pos"][0]) == 0
        tot = WK.C.c_uint64(7)
        assert L.mahip_hits_positions_download(gpu_ctx.h, None, WK.C.byref(tot)) == -1 and b"mahip_hits_positions_download: no positions set" in L.mahip_strerror() and tot.value == 7
