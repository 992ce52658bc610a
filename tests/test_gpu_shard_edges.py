"""The sharded head (host/sharded.c) stage by stage at every read-range edge, in ONE process: stages.sharded_stages walks the phases of
ma_pipeline_head_sharded on one context per rank, one rank after the other, and does every exchange itself through the ABI (mahip_xbuf, mahip_copy_out,
mahip_memcpy_d2h, numpy, mahip_memcpy_h2d, mahip_copy_in / import).  No threads, no communicator, no child process: nothing here can leave a rank waiting.

Expected values never come from the sharded code: tie mode 0 is held to the CPU oracle (stages.orc_stages), exactly; tie mode 2 to the fused chain on ONE
context (stages.gpu_stages_fused, which tests/test_gpu_fused_hits.py and tests/test_gpu_graph_edges.py hold to the reference library) and, where oracle/_ref is
built, to the reference library's own graph.

What is asserted per phase, for every rank r with the reads [q0, q1) (check_stages):
  sub#1, cut+flt+sub#2   the rank's slice of the interval array; the summed counters; after the exchange every rank holds the whole array
  contained flags        the OR over the ranks of r_cont / r_used is the one-context array; no rank sets a flag that array does not have
  finish                 n_seq_new, the squeeze map and the squeezed intervals: identical on all ranks, the oracle's
  sg flags               the OR of seq.del
  local arcs             the rank's rows are the oracle's sorted arcs of its reads, in that order; in rank order they are the oracle's arc list
  import rows            every rank holds the oracle's arcs, seq and CSR index; its census is the census of those arcs
  tie repair             (tie mode 2, whole input) every rank holds the one-context graph
  reduction              the rank's n_red and the del bits of its own block are those of the oracle's marking pass over its vertices
  rank 0                 after flags_in + cleanup (+ symm) the reduced graph; what the cleanup removed is the sum of the ranks' n_red
on read-range tables no end-to-end test produces (TABLES): a border on, behind and 63 reads in front of the reads with 513 / 4 097 / 9 001 hits, a read without
hits and the reads with 64 / 65 / 511 / 512 arcs (lane 0 of a shifted chunk of k_arc_group_sort, the range's last read, lane 63); ranges of 1, 63, 64, 65 and
129 reads; empty ranges first, in the middle (one, two in a row) and last; one rank owning every read; a rank whose reads have hits and no arc; a world larger
than the dictionary; equal read counts with a remainder; world 1; the tables mahip_hits_balance itself makes when one read has all the hits.  Every table
asserts that it has the shape it was written for.

Covered elsewhere, because they run collectives inside and need real ranks: mahip_paf_parse_sharded, mahip_hits_route and the shared-memory collectives of
csrc/comm.hip they go through (the word gather in chunks of 32, the personalised exchange in slot-sized rounds) are checked rank by rank, stage by stage, at
their size edges by tests/test_gpu_ingest_shard_edges.py (worlds 1, 2, 3, 5 and 8, against tests/pafmodel.py and stages.balance_model).
NOT covered stage by stage: the RCCL and caller-transport paths of csrc/comm.hip and the tie repair of own-record shards with positions -- end to end only
(tests/test_gpu_sharded.py, tests/test_dist_gloo.py)."""
import ctypes as C

import numpy as np
import pytest

import miniasm_amd as ma
import refapi as R
import stages as ST

pytestmark = pytest.mark.gpu

MAX_WORLD = 8


@pytest.fixture(scope="module")
def ranks():
    """eight contexts beside the session's (nine open at a time), closed whatever happens"""
    cs = []
    try:
        for _ in range(MAX_WORLD):
            cs.append(ma.Ctx(0))
        yield cs
    finally:
        for c in cs:
            c.close()


# --------------------------------------------------------------------------------------------- inputs and what is expected of them
def five_read_hits():
    """five reads of 20 kb in a row, every read overlapping the next two by dovetails on both strands, six copies of every hit: run with min_dp = 1"""
    lines = []
    for q in range(5):
        for t in range(5):
            if q != t:
                for k in range(3):
                    lines.append(ST.dovetail(q, t, (q + t + k) % 2, 3000 + 1000 * abs(q - t) + 10 * k, k, 20000))
    return ST.hits_from_lines(lines)


def one_read_hits(n_seq, q, n=120):
    """all hits on read q"""
    h = ST.sparse_id_hits(n_seq, n, "first")
    h["qns"] = (h["qns"] & np.uint64(0xffffffff)) | np.uint64(q) << np.uint64(32)
    h["tn"] = np.where(h["tn"] == q, (q + 1) % n_seq, h["tn"])
    return h


def opt_dp1():
    o = ma.default_opt()
    o.min_dp = 1
    return o


def make_input(name):
    if name == "edge300":  # 479 reads, group sizes 0 .. 9 001, record + mirror side by side
        h, n_seq, sizes = ST.edge_hits(300, True, 0)
        return h, n_seq, ma.default_opt(), sizes
    if name == "edge0":  # 179 reads, the records of a read together
        h, n_seq, sizes = ST.edge_hits(0, False, 10)
        return h, n_seq, ma.default_opt(), sizes
    if name in ("arcs", "ties", "arcs1021"):  # 0 .. 512 arcs per read at ARC_EDGE_IDS; ties: arc lengths from a set of eight
        h, _, sizes = ST.arc_edge_hits(few_lengths=name == "ties", n_seq=1021 if name == "arcs1021" else 1024, seed=2)
        return h, 1021 if name == "arcs1021" else 1024, opt_dp1(), sizes
    if name == "random":
        h, n_seq = ST.random_hits(4)
        assert (n_seq, len(h)) == (200, 60000)
        return h, n_seq, ma.default_opt(), {}
    if name == "five":
        return five_read_hits(), 5, opt_dp1(), {}
    if name.startswith("one_read"):  # one_read-<n_seq>-<q>
        _, n_seq, q = name.split("-")
        return one_read_hits(int(n_seq), int(q)), int(n_seq), opt_dp1(), {}
    raise KeyError(name)


_CACHE = {}


def expected(name, ctx, tie_mode):
    """(hits, n_seq, opt, sizes, X): X = what one context and the oracle make of the input, computed once per input and tie mode and left unchanged"""
    if name not in _CACHE:
        h, n_seq, opt, sizes = make_input(name)
        orc = ST.orc_stages(h, n_seq, opt)
        _CACHE[name] = dict(inp=(h, n_seq, opt, sizes), orc=orc, flags=ST.one_context_flags(ctx, h, n_seq, opt), hits_per_read=np.bincount((h["qns"] >> np.uint64(32)).astype(np.int64), minlength=n_seq))
    E = _CACHE[name]
    if ("X", tie_mode) not in E:
        h, n_seq, opt, _ = E["inp"]
        orc = E["orc"]
        fused = ST.gpu_stages_fused(ctx, h, n_seq, opt, tie_mode=tie_mode, snapshots=False)
        X = dict(orc=orc, fused=fused, flags=E["flags"], ns=orc["n_seq_new"])
        if tie_mode == 0:  # the oracle, exact
            idx = np.zeros(2 * max(X["ns"], 1), dtype="<u8")
            R.orc().orc_arc_index(X["ns"], len(orc["sg_arcs"]), orc["sg_arcs"].ctypes.data, idx.ctypes.data)
            X.update(sg_arcs=orc["sg_arcs"], sg_seq=orc["sg_seq"], sg_idx=idx[:2 * X["ns"]], tr_arcs=orc["tr_arcs"], tr_idx=orc["tr_idx"][:2 * X["ns"]])
            ST.compare(fused, orc, "%s: one context against the oracle" % name, exact_order=True)
        else:  # the reference's order of equal keys: the one-context chain
            X.update({k: fused[k] for k in ("sg_arcs", "sg_seq", "sg_idx", "tr_arcs", "tr_idx")})
            ST.compare(fused, orc, "%s: one context against the oracle" % name, exact_order=False, graph=False)  # (the order inside a tie group decides what the reduction deletes)
            assert R.canon(fused["sg_arcs"]).tobytes() == R.canon(orc["sg_arcs"]).tobytes() and fused["sg_seq"].tobytes() == orc["sg_seq"].tobytes()
        X["ref"] = ST.ref_graph(h, n_seq, opt) if R.have_ref() and tie_mode == 2 else None
        mp = orc["map"]
        u_old = np.flatnonzero(mp >= 0)[(X["sg_arcs"]["ul"] >> np.uint64(33)).astype(np.int64)] if len(X["sg_arcs"]) else np.zeros(0, np.int64)
        X["arcs_per_read"] = np.bincount(u_old, minlength=n_seq)
        X["hits_per_read"] = E["hits_per_read"]
        E[("X", tie_mode)] = X
    return E["inp"] + (E[("X", tie_mode)],)


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and len(a) == len(b), "%s: %d %s vs %d %s" % (what, len(a), a.dtype, len(b), b.dtype)
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero(a != b)
        raise AssertionError("%s: %d of %d entries differ, first at %d: %r vs %r" % (what, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]]))


def check_stages(S, n_seq, opt, X, tie_mode, full_input, what):
    """every assertion of the module's table, for every rank"""
    W, rng, orc, fused = S["world"], S["ranges"], X["orc"], X["fused"]
    ns, mp = X["ns"], orc["map"]
    sq = lambda q: int((mp[:q] >= 0).sum())  # squeezed id of the first surviving read at or behind q
    assert S["order"] == ST.shard_phase_names(), "the model walks the phases of host/sharded.c in their order"
    # sub#1 / cut+flt+sub#2
    for ph, xp, key, ctrs in (("sub#1", "x:sub0", "sub1", (("n_rem1", orc["n_rem1"]),)),
                              ("cut+flt+sub#2", "x:sub1", "sub2", (("n_cut", fused["n_cut1"]), ("n_flt", fused["n_flt"]), ("n_rem2", fused["n_rem2"]), ("n_rem2", orc["n_rem2"])))):
        for r, (q0, q1) in enumerate(rng):
            same(S[ph]["contrib"][r], orc[key][q0:q1], "%s: %s, rank %d's reads [%d, %d)" % (what, ph, r, q0, q1))
            if W > 1:
                same(S[xp]["contrib"][r], orc[key][q0:q1], "%s: %s, what rank %d sent" % (what, xp, r))
            same(S[xp]["held"][r], orc[key], "%s: %s, rank %d afterwards" % (what, xp, r))
        for k, v in ctrs:
            assert sum(S[ph][k]) == v, "%s: %s: the ranks' %s %r sum to %d, expected %d" % (what, ph, k, S[ph][k], sum(S[ph][k]), v)
    assert sum(S["cut+flt+sub#2"]["n_flt"]) == len(orc["flt"])
    # merge + contained flags
    P = S["merge+cut+contained"]
    for r in range(W):
        same(P["subm"][r], orc["subm"], "%s: merged intervals on rank %d" % (what, r))
    for k, key in enumerate(("r_cont", "r_used")):
        one = X["flags"][k]
        same(np.maximum.reduce(P[key]), one, "%s: OR of %s over the ranks" % (what, key))
        for r in range(W):
            assert not (P[key][r] & ~one).any() and P[key][r].max(initial=0) <= 1, "%s: rank %d sets a %s flag the one-context run does not have" % (what, r, key)
            same(S["x:flags"]["held"][r][k], one, "%s: %s on rank %d after the exchange" % (what, key, r))
    assert ((X["flags"][0] != 0) | (X["flags"][1] == 0)).tobytes() == (mp < 0).tobytes(), "%s: contained or untouched == dropped by the oracle" % what
    # finish
    P = S["squeeze+sg flags"]
    for r in range(W):
        assert P["n_seq_new"][r] == ns, "%s: n_seq_new on rank %d: %d, expected %d" % (what, r, P["n_seq_new"][r], ns)
        same(P["map"][r], mp, "%s: squeeze map on rank %d" % (what, r))
        same(P["sub"][r], orc["cont_sub"], "%s: squeezed intervals on rank %d" % (what, r))
    assert sum(P["n_cut"]) == fused["n_cut2"], "%s: second cut: %r, expected %d in all" % (what, P["n_cut"], fused["n_cut2"])
    # sg flags
    keep = mp >= 0
    exp_del = (X["sg_seq"] >> np.uint32(31)).astype(np.uint8)
    same(np.maximum.reduce(P["sdel"])[keep], exp_del, "%s: OR of seq.del over the ranks" % what)
    for r in range(W):
        same(S["x:seq.del"]["held"][r][keep], exp_del, "%s: seq.del on rank %d after the exchange" % (what, r))
        same(S["x:seq.del"]["held"][r], S["x:seq.del"]["held"][0], "%s: seq.del on rank %d and rank 0" % (what, r))
    # local arcs
    n_loc, Pc = S["local arcs"]["n_loc"], S["x:arc counts"]
    assert sum(n_loc) == len(X["sg_arcs"]) == Pc["tot"], "%s: local arcs %r, expected %d in all" % (what, n_loc, len(X["sg_arcs"]))
    assert sum(S["local arcs"]["n_hits"]) == len(orc["cont"]), "%s: live hits %r, expected %d in all" % (what, S["local arcs"]["n_hits"], len(orc["cont"]))
    assert Pc["stride"] == max(1, max(n_loc)) and Pc["first"] == [sum(n_loc[:r]) for r in range(W)]
    for r, (q0, q1) in enumerate(rng):  # a rank none of whose reads has more than 512 arcs: the register sort per read, on the rank's range, must do it alone (a
        # stretch it takes for longer than that, or for another read's, sends the whole sort down the radix path -- same arcs, so only the launches show it)
        if n_loc[r] > 1 and X["arcs_per_read"][q0:q1].max() <= 512 and (tie_mode == 0 or (W > 1 and (q0, q1) != (0, n_seq))):
            names = S["local arcs"]["kernels"][r]
            assert "k_arc_group_sort" in names and "k_arc_permute" not in names, "%s: rank %d sorted its arcs with %r" % (what, r, names)
    u_sq = (X["sg_arcs"]["ul"] >> np.uint64(33)).astype(np.int64)
    if W > 1:
        blocks = [ST.rows_to_arcs(b, mp) for b in S["x:arc blocks"]["contrib"]]
        for r, (q0, q1) in enumerate(rng):
            mine = X["sg_arcs"][(u_sq >= sq(q0)) & (u_sq < sq(q1))]
            assert len(blocks[r]) == n_loc[r] == len(mine), "%s: rank %d exported %d rows, sg_finish said %d, its reads have %d arcs" % (what, r, len(blocks[r]), n_loc[r], len(mine))
            if tie_mode == 0:
                same(blocks[r], mine, "%s: rank %d's rows against the oracle's arcs of its reads" % (what, r))
            else:
                same(R.canon(blocks[r]), R.canon(mine), "%s: rank %d's rows (as a set) against the arcs of its reads" % (what, r))
        if tie_mode == 0:
            same(np.concatenate(blocks), X["sg_arcs"], "%s: the blocks in rank order" % what)
    # import rows
    repaired = S["tie repair"]["repaired"]
    for r in range(W):
        arcs, seq, idx = S["x:arc blocks"]["held"][r]
        if tie_mode == 0 or W == 1:
            same(arcs, X["sg_arcs"], "%s: arcs on rank %d after the import" % (what, r))
        else:
            same(R.canon(arcs), R.canon(X["sg_arcs"]), "%s: arcs (as a set) on rank %d after the import" % (what, r))
            assert (arcs["ul"][1:] >= arcs["ul"][:-1]).all(), "%s: sorted by (u, len) on rank %d" % (what, r)
        same(seq, X["sg_seq"], "%s: seq on rank %d after the import" % (what, r))
        same(idx, X["sg_idx"], "%s: CSR index on rank %d after the import" % (what, r))
        if tie_mode != 0 and W > 1:
            t = S["x:arc blocks"]["tie"][r]
            assert (t["arc_tie_groups"], t["arc_tie_arcs"]) == ST.arc_tie_census(arcs), "%s: census on rank %d: %r" % (what, r, t)
            assert t["unrepaired"] == (t["arc_tie_groups"] > 0)
    # tie repair
    if tie_mode == 2 and (full_input or W == 1):
        assert repaired == 1 or ST.arc_tie_census(X["sg_arcs"])[0] == 0, "%s: tie groups and no repair" % what
    if tie_mode == 0 or repaired == 1 or ST.arc_tie_census(X["sg_arcs"])[0] == 0:
        for r in range(W):
            arcs, seq, idx = S["tie repair"]["held"][r]
            same(arcs, X["sg_arcs"], "%s: arcs on rank %d in front of the reduction" % (what, r))
            same(idx, X["sg_idx"], "%s: CSR index on rank %d in front of the reduction" % (what, r))
        # reduction
        first = Pc["first"]
        n_red = S["reduction (own vertices)"]["n_red"]
        all_del = np.zeros(len(X["sg_arcs"]), dtype="<u4")
        for r, (q0, q1) in enumerate(rng):
            marked, nr, _ = ST.orc_trans_only(ns, X["sg_arcs"], X["sg_idx"], X["sg_seq"], opt.gap_fuzz, 2 * sq(q0), 2 * sq(q1))
            assert n_red[r] == nr, "%s: rank %d reduced %d arcs among its vertices, the oracle %d" % (what, r, n_red[r], nr)
            blk = slice(first[r], first[r] + n_loc[r])
            if W > 1:
                same(S["x:del flags"]["contrib"][r], marked["oldel"][blk], "%s: del bits of rank %d's block" % (what, r))
            all_del[blk] = marked["oldel"][blk]
        for r in range(W):
            same(S["x:del flags"]["held"][r], all_del, "%s: ol|del column on rank %d after the exchange" % (what, r))
        # rank 0
        P = S["rank 0: cleanup+symm"]
        assert P["n_red"] == sum(n_red), "%s: rank 0's cleanup removed %d arcs, the ranks reduced %r" % (what, P["n_red"], n_red)
        assert P["n_red"] == fused["n_red"] and (tie_mode != 0 or P["n_red"] == orc["n_red"])
        arcs, seq, idx = P["graph"]
        same(arcs, X["tr_arcs"], "%s: rank 0's reduced graph" % what)
        same(idx, X["tr_idx"], "%s: rank 0's reduced index" % what)
        if X["ref"] is not None and tie_mode == 2:
            same(arcs, X["ref"]["tr_arcs"], "%s: rank 0's reduced graph against the reference library's" % what)
            same(idx, X["ref"]["tr_idx"], "%s: rank 0's reduced index against the reference library's" % what)
            assert P["n_red"] == X["ref"]["n_red"]


def equal(a, b):
    """nested lists / tuples / dicts of arrays and numbers, bit for bit"""
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(equal(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b or (isinstance(a, float) and ST.same_f32(a, b))


def run_case(ranks, gpu_ctx, name, bounds, full_input, tie_mode, what=None):
    h, n_seq, opt, sizes, X = expected(name, gpu_ctx, tie_mode)
    S = ST.sharded_stages(ranks, h, n_seq, opt, bounds, full_input, tie_mode)
    check_stages(S, n_seq, opt, X, tie_mode, full_input, what or "%s %r" % (name, bounds))
    return S, X


# --------------------------------------------------------------------------------------------- the tables
def read_with(per_read, n):
    x = np.flatnonzero(per_read == n)
    assert len(x) >= 1, "the generator no longer makes a read with %d" % n
    return int(x[0])


def borders(n_seq, inner):
    b = [0] + sorted(inner) + [n_seq]
    assert len(b) - 1 <= MAX_WORLD and all(0 <= x <= n_seq for x in b)
    return b


def range_from(b, q):
    """the range of table b that starts at border q -> (q0, q1)"""
    r = max(i for i in range(len(b) - 1) if b[i] == q)  # (of equal borders the last one opens the range)
    return b[r], b[r + 1]


def lane63_tables(n_seq, xs):
    """tables with a border 63 reads in front of every x, and no other border up to x: as few tables as that allows"""
    groups = []
    for x in sorted(xs):
        if groups and x - 63 > groups[-1][-1]:
            groups[-1].append(x)
        else:
            groups.append([x])
    out = []
    for g in groups:
        b = borders(n_seq, [x - 63 for x in g])
        for x in g:
            q0, q1 = range_from(b, x - 63)
            assert q0 + 63 == x < q1, "read %d on lane 63 of the first chunk of its range" % x
        out.append(b)
    assert sorted(x for g in groups for x in g) == sorted(xs)
    return out


@pytest.mark.parametrize("mode", ["whole_input", "own_records"])
@pytest.mark.parametrize("which", ["lane63", "first_and_last_a", "first_and_last_b"])
def test_borders_at_the_deep_reads(which, mode, ranks, gpu_ctx):
    """a border on x, behind x and 63 reads in front of x for the reads x with 513 hits (the first of tier 2), 4 097 and 9 001 hits (tier B) and a read without
    hits: x on lane 0 of a chunk that starts at the range's first read, x the range's last read (q_hi cuts the chunk behind it), x on lane 63"""
    name, full = ("edge300", 1) if mode == "whole_input" else ("edge0", 0)
    h, n_seq, opt, sizes, X = expected(name, gpu_ctx, 0)
    per = X["hits_per_read"]
    xs = [read_with(per, n) for n in (513, 4097, 9001)] + [int(np.flatnonzero(per == 0)[0]) if name == "edge0" else next(int(q) for q in np.flatnonzero(per == 0) if q >= 63)]
    assert [int(per[x]) for x in xs] == [513, 4097, 9001, 0] and min(xs) >= 63
    if which == "lane63":
        tables = lane63_tables(n_seq, xs)
    else:
        pick = xs[:2] if which == "first_and_last_a" else xs[2:]
        tables = [borders(n_seq, [x for x in pick] + [x + 1 for x in pick])]
        for x in pick:
            assert range_from(tables[0], x) == (x, x + 1), "read %d opens and closes a range of its own" % x
    for b in tables:
        run_case(ranks, gpu_ctx, name, b, full, 0)


@pytest.mark.parametrize("tie_mode", [0, 2])
@pytest.mark.parametrize("which", ["lane63", "first_and_last_a", "first_and_last_b"])
def test_borders_at_the_many_arc_reads(which, tie_mode, ranks, gpu_ctx):
    """the same three borders for the reads with 64 / 65 arcs (one and two register rows of k_arc_group_sort<true>) and 511 / 512 arcs (eight rows of <false>, AG_MAX):
    the 64-read chunks of the arc sort start at q_lo, the `last` lane is cut by q_hi"""
    name = "ties" if tie_mode else "arcs"
    h, n_seq, opt, sizes, X = expected(name, gpu_ctx, tie_mode)
    xs = [read_with(X["arcs_per_read"], n) for n in (64, 65, 511, 512)]
    assert [int(X["arcs_per_read"][x]) for x in xs] == [64, 65, 511, 512] and min(xs) >= 63 and set(xs) <= set(i % n_seq for i in ST.ARC_EDGE_IDS)
    if tie_mode:
        assert ST.arc_tie_census(X["sg_arcs"])[0] > 100, "a tie-rich input"
    if which == "lane63":
        tables = lane63_tables(n_seq, xs)
    else:
        pick = xs[:2] if which == "first_and_last_a" else xs[2:]
        tables = [borders(n_seq, pick + [x + 1 for x in pick])]
        for x in pick:
            assert range_from(tables[0], x) == (x, x + 1)
    for b in tables:
        S, _ = run_case(ranks, gpu_ctx, name, b, 1, tie_mode)
        if tie_mode:
            assert S["tie repair"]["repaired"] == 1 and S["x:arc blocks"]["tie"][0]["unrepaired"] == 1


RANGE_TABLES = {
    "sizes_1_63_64_65_129": lambda n: [0, 0, 1, 64, 128, 193, 322, n, n],  # an empty range first and last, too
    "empty_in_the_middle": lambda n: [0, 300, 300, 500, 500, 500, n],      # two equal borders; three in a row
    "empty_first_two": lambda n: [0, 0, 0, 640, n],
    "no_arcs_and_longest": lambda n: [0, 1, 384, 385, n],                  # read 0: a hit and no arc; read 384: 512 arcs
}


@pytest.mark.parametrize("mode", ["whole_input", "own_records"])
@pytest.mark.parametrize("table", sorted(RANGE_TABLES))
def test_range_sizes_and_empty_ranges(table, mode, ranks, gpu_ctx):
    """ranges of 1, 63, 64, 65 and 129 reads (the grids of the coverage sweeps and of the arc sort are sized by the range: Rr); empty ranges first, in the
    middle, last (Rr = 1, a grid of one block that finds nothing; counts[r] == 0 under stride >= 1 in the imports); a rank whose reads have hits and no arc"""
    name = "arcs"
    h, n_seq, opt, sizes, X = expected(name, gpu_ctx, 0)
    b = RANGE_TABLES[table](n_seq)
    assert b[0] == 0 and b[-1] == n_seq and all(x <= y for x, y in zip(b, b[1:])) and len(b) - 1 <= MAX_WORLD
    ln = [y - x for x, y in zip(b, b[1:])]
    if table == "sizes_1_63_64_65_129":
        assert set(ln) >= {0, 1, 63, 64, 65, 129} and ln[0] == 0 and ln[-1] == 0
    elif table == "empty_in_the_middle":
        assert ln[1] == 0 and ln[3] == ln[4] == 0 and ln[0] and ln[2] and ln[5]
    elif table == "empty_first_two":
        assert ln[0] == ln[1] == 0
    S, _ = run_case(ranks, gpu_ctx, name, b, 1 if mode == "whole_input" else 0, 0)
    counts = S["x:arc counts"]["counts"]
    for r in range(len(ln)):
        if ln[r] == 0:
            assert counts[r] == 0 and S["local arcs"]["n_hits"][r] == 0
    if table == "no_arcs_and_longest":
        assert X["hits_per_read"][0] > 0 and counts[0] == 0 and S["x:arc counts"]["stride"] >= 1, "rank 0: hits and no arc"
        assert X["arcs_per_read"][384] == 512 and counts[2] == 512
        assert int(counts.max()) == S["x:arc counts"]["stride"] and S["x:arc counts"]["stride"] > 512, "the longest block fills its slot"


@pytest.mark.parametrize("tie_mode", [0, 2])
@pytest.mark.parametrize("owner", [0, 1])
def test_one_rank_owns_every_read(owner, tie_mode, ranks, gpu_ctx):
    """[0, n, n] and [0, 0, n]: the owner's context is NO shard ((q_beg, q_end) == (0, n_seq)): its ma_sg_gen takes the census and walks itself and keeps no
    push rows (n_push == 0), the other rank yields nothing.  The census behind mahip_asg_import_rows still says `unrepaired` (it cannot know), so the repair of
    host/sharded.c runs: mahip_asg_export_rows_push copies zero rows, and mahip_asg_import_push_rows walks over what exchange buffer 0 still holds -- the rows of
    the exchange before, the owner's graph in the order its own walk left.  That is safe, and this test is what says so: those rows are sorted by (u, len), and on
    a sequence that is sorted by its keys the reference's sort moves nothing (every record already stands in its radix bucket, the insertion sort of the small
    buckets is stable), so every rank ends with the owner's graph again.  On the tie-rich input, both tie modes"""
    h, n_seq, opt, sizes, X = expected("ties", gpu_ctx, tie_mode)
    b = [0, n_seq, n_seq] if owner == 0 else [0, 0, n_seq]
    assert ST.arc_tie_census(X["sg_arcs"])[0] > 100
    S, _ = run_case(ranks, gpu_ctx, "ties", b, 1, tie_mode)
    assert S["ranges"][owner] == (0, n_seq) and S["sort"]["path"][owner] != "records_plain", "the owner sorts as an unsharded context does"
    assert list(S["x:arc counts"]["counts"]) == ([len(X["sg_arcs"]), 0] if owner == 0 else [0, len(X["sg_arcs"])])
    if tie_mode == 2:
        for r in range(2):
            same(S["x:arc blocks"]["held"][r][0], X["sg_arcs"], "rank %d holds the owner's walked order right after the import" % r)
        assert S["x:arc blocks"]["tie"][0]["unrepaired"] == 1 and S["tie repair"]["conflicts"] == [0, 0] and S["tie repair"]["repaired"] == 1
        same(S["tie repair"]["contrib"][owner], S["x:arc blocks"]["contrib"][owner], "the rows the repair gathered from the owner: those of the exchange before")
    else:
        assert S["tie repair"]["repaired"] == 0 and "contrib" not in S["tie repair"]


def test_world_larger_than_the_dictionary(ranks, gpu_ctx):
    """five reads at world 8, no table: the equal-count rule gives the ranks 5 .. 7 the empty range [5, 5)"""
    for tie_mode, full in ((0, 1), (0, 0), (2, 1)):
        S, X = run_case(ranks, gpu_ctx, "five", 8, full, tie_mode)
        assert S["table"] is None and S["per"] == 1 and S["ranges"] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 5), (5, 5), (5, 5)]
        assert len(X["sg_arcs"]) > 0


@pytest.mark.parametrize("name", ["arcs", "ties", "five", "edge0"])
def test_world_one_is_the_unsharded_run(name, ranks, gpu_ctx):
    """world 1 through the same walk: no exchange, the context's own census and walk; every stage equals the unsharded run"""
    for tie_mode in (0, 2):
        h, n_seq, opt, sizes, X = expected(name, gpu_ctx, tie_mode)
        S, _ = run_case(ranks, gpu_ctx, name, [0, n_seq], 1, tie_mode)
        assert S["ranges"] == [(0, n_seq)] and "contrib" not in S["x:sub0"]
        S1, _ = run_case(ranks, gpu_ctx, name, 1, 0, tie_mode)  # (no table)
        assert S1["table"] is None


@pytest.mark.parametrize("world", [2, 3, 5])
def test_equal_read_counts_with_a_remainder(world, ranks, gpu_ctx):
    """no table, n_seq % world != 0: ceil(n_seq / world) reads a rank, the last rank the rest; the gathered slots ARE the array (one mahip_copy_in of n_seq entries)"""
    h, n_seq, opt, sizes, X = expected("arcs1021", gpu_ctx, 0)
    assert n_seq % world != 0
    for full in (1, 0):
        S, _ = run_case(ranks, gpu_ctx, "arcs1021", world, full, 0)
        cc = -(-n_seq // world)
        assert S["table"] is None and S["per"] == cc and S["ranges"][-1] == (cc * (world - 1), n_seq) and S["ranges"][-1][1] - S["ranges"][-1][0] < cc


def test_random_hit_block(ranks, gpu_ctx):
    """hit records no overlapper writes (start > end, self hits, ml > bl ...) on the table mahip_hits_balance makes of them, world 3"""
    h, n_seq, opt, sizes, X = expected("random", gpu_ctx, 0)
    b = balance_of(gpu_ctx, h, n_seq, 3)
    assert b == ST.balance_model((h["qns"] >> np.uint64(32)).astype(np.int64), n_seq, 3)
    for full in (1, 0):
        run_case(ranks, gpu_ctx, "random", b, full, 0)


def test_the_same_table_twice_on_the_same_contexts(ranks, gpu_ctx):
    """upload, head, upload, head: bounds, positions and the push order describe ONE upload -- the second pass equals the first, stage by stage"""
    h, n_seq, opt, sizes, X = expected("ties", gpu_ctx, 2)
    b = [0, 100, 128, 128, 700, n_seq]
    passes = [run_case(ranks, gpu_ctx, "ties", b, 1, 2)[0] for _ in range(2)]
    run_case(ranks, gpu_ctx, "arcs", [0, 64, 900, 1024], 0, 0)  # another input, another world in between
    passes.append(run_case(ranks, gpu_ctx, "ties", b, 1, 2)[0])
    for S in passes[1:]:
        assert S["order"] == passes[0]["order"]
        for ph in S["order"]:
            assert sorted(S[ph]) == sorted(passes[0][ph])
            for k, v in S[ph].items():
                assert equal(v, passes[0][ph][k]), "%s / %s differs between the passes" % (ph, k)


def test_model_walks_the_phases_of_sharded_c(ranks, gpu_ctx):
    """the drift guard: the model names its phases with the strings of ma_shard_phase_name[] (read from the library) and walks exactly that list, in that order"""
    names = ST.shard_phase_names()
    assert len(names) == ma.SHARD_N_PHASES == len(set(names)) and names == ma.SHARD_PHASE_NAMES
    h, n_seq, opt, _ = make_input("five")
    S = ST.sharded_stages(ranks, h, n_seq, opt, [0, 2, 5], 1, 2)
    assert S["order"] == names
    assert all(isinstance(S[n], dict) for n in names)


# --------------------------------------------------------------------------------------------- mahip_hits_balance
def balance_of(ctx, h, n_seq, world):
    ctx.hits_upload(h, n_seq)
    out = np.zeros(world + 1, dtype="<u4")
    ma._chk(ST.shard_api().mahip_hits_balance(ctx.h, world, out.ctypes.data), "hits_balance")
    bw = C.c_int(0)
    p = ST.shard_api().mahip_shard_bounds(ctx.h, C.byref(bw))
    assert bw.value == world and [int(p[r]) for r in range(world + 1)] == out.tolist(), "the table is kept in the context"
    return out.tolist()


def qid_hits(qid):
    return ST.sort_hits(np.asarray(qid, dtype=np.int64))


BALANCE_CASES = {
    "all_on_first": (40, np.zeros(100, int), (2, 4, 7)),
    "all_on_middle": (40, np.full(100, 17), (2, 4, 7)),
    "all_on_last": (40, np.full(100, 39), (2, 4, 7)),
    "three_of_four": (4, np.array([2] * 100), (4,)),  # counts [0, 0, 100, 0] -> [0, 3, 3, 3, 4]
    "fewer_hits_than_ranks": (40, np.array([3, 3, 20]), (5, 8)),
    "world_above_n_seq": (5, np.array([0, 1, 1, 2, 4, 4, 4, 3, 0, 2, 2]), (8, 64, 1024)),
    "world_one": (40, np.arange(200) % 40, (1,)),
    "uniform": (40, np.arange(2000) % 40, (2, 3, 5, 8)),
    "skewed": (300, np.minimum(np.random.default_rng(5).geometric(0.03, 5000) - 1, 299), (2, 3, 5, 8)),
    "ids_outside_the_dictionary": (10, np.r_[np.arange(50) % 10, np.full(150, 10), np.full(3, 4000000000)], (2, 4, 8)),
}


@pytest.mark.parametrize("case", sorted(BALANCE_CASES))
def test_hits_balance_against_the_stated_rule(case, gpu_ctx):
    """rank r starts at the smallest q + 1 with cum[q] * world >= n_hits * r (stages.balance_model); records whose query id is not in the dictionary count
    as hits and lie in no read, so the ranks that would start behind them get nothing"""
    n_seq, qid, worlds = BALANCE_CASES[case]
    h = qid_hits(qid)
    for world in worlds:
        b = balance_of(gpu_ctx, h, n_seq, world)
        assert b == ST.balance_model(qid, n_seq, world), "%s, world %d: %r" % (case, world, b)
        assert b[0] == 0 and b[world] == n_seq and all(x <= y for x, y in zip(b, b[1:]))
    if case == "three_of_four":
        assert b == [0, 3, 3, 3, 4]
    if case == "ids_outside_the_dictionary":
        assert b[-2] == n_seq, "three quarters of the hits lie in no read: the last ranks start at n_seq"


def test_hits_balance_without_hits_falls_back_to_equal_counts(gpu_ctx):
    for n_seq, world in ((10, 3), (5, 8), (7, 1), (0, 4)):
        b = balance_of(gpu_ctx, np.zeros(0, dtype=ma.HIT_DT), n_seq, world)
        per = -(-n_seq // world)
        assert b == [min(r * per, n_seq) for r in range(world)] + [n_seq] == ST.balance_model([], n_seq, world)


@pytest.mark.parametrize("world", [0, 1025, -1])
def test_hits_balance_refuses_a_bad_world(world, gpu_ctx):
    gpu_ctx.hits_upload(qid_hits(np.arange(20) % 5), 5)
    out = np.full(1030, 77, dtype="<u4")
    assert ST.shard_api().mahip_hits_balance(gpu_ctx.h, world, out.ctypes.data) == -1
    assert b"bad world size" in ma.lib().mahip_strerror() and (out == 77).all()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("world", [2, 4, 7])
def test_tables_of_one_read_with_all_hits_through_the_head(world, where, ranks, gpu_ctx):
    """the empty-range tables the product itself makes: every hit on the first, a middle or the last read, balanced over 2, 4 and 7 ranks"""
    n_seq = 40
    q = {"first": 0, "middle": 17, "last": n_seq - 1}[where]
    name = "one_read-%d-%d" % (n_seq, q)
    h, _, opt, _, X = expected(name, gpu_ctx, 0)
    b = balance_of(gpu_ctx, h, n_seq, world)
    assert b == [0] + [q + 1] * (world - 1) + [n_seq], "ranks 1 .. world - 2 are empty, the last one owns the reads behind q"
    for tie_mode, full in ((0, 1), (0, 0), (2, 1)):
        run_case(ranks, gpu_ctx, name, b, full, tie_mode)


# --------------------------------------------------------------------------------------------- the slice copies at their ends
def test_copy_out_and_in_at_the_ends_of_the_arrays(ranks, gpu_ctx):
    """mahip_copy_out / mahip_copy_in: count 0 at first == n, the last element, and one past the end -- refused with the "bad range" message, nothing changed"""
    L = ST.shard_api()
    c = ranks[0]
    h, n_seq, opt, _ = make_input("five")
    ST.sharded_stages(ranks, h, n_seq, opt, [0, n_seq], 1, 0)  # every array is there
    for which, dt in sorted(ST.BUF_ELEM.items()):
        es = dt.itemsize
        before = ST.buf_get(c, which, 0, n_seq)
        p = ST.xbuf(c, 0, 4 * es)
        ST.dev_write(c, p, np.full(4 * es, 0xA5, np.uint8))
        assert L.mahip_copy_out(c.h, which, p, n_seq, 0) == 0 and L.mahip_copy_in(c.h, which, p, n_seq, 0) == 0
        assert (ST.dev_read(c, p, 4 * es) == 0xA5).all()
        assert L.mahip_copy_out(c.h, which, p, n_seq - 1, 1) == 0
        got = ST.dev_read(c, p, 4 * es)
        assert got[:es].tobytes() == before[n_seq - 1:].tobytes() and (got[es:] == 0xA5).all(), "the last element, and nothing behind it"
        for first, count in ((n_seq, 1), (n_seq - 1, 2), (0, n_seq + 1)):
            assert L.mahip_copy_out(c.h, which, p, first, count) == -1 and b"bad buffer/range" in ma.lib().mahip_strerror()
            assert L.mahip_copy_in(c.h, which, p, first, count) == -1 and b"bad buffer/range" in ma.lib().mahip_strerror()
        assert L.mahip_copy_out(c.h, 5, p, 0, 1) == -1 and L.mahip_copy_in(c.h, -1, p, 0, 1) == -1
        assert (ST.dev_read(c, p, 4 * es)[es:] == 0xA5).all()
        same(ST.buf_get(c, which, 0, n_seq), before, "array %d after the refused calls" % which)
        last = np.frombuffer(bytes([0x01] * es), dtype=dt)
        ST.dev_write(c, p, last)
        assert L.mahip_copy_in(c.h, which, p, n_seq - 1, 1) == 0
        after = ST.buf_get(c, which, 0, n_seq)
        same(after[:n_seq - 1], before[:n_seq - 1], "array %d in front of its last element" % which)
        assert after[n_seq - 1:].tobytes() == last.tobytes()


def test_arc_flags_out_and_in_at_the_ends_of_the_graph(ranks, gpu_ctx):
    """mahip_asg_flags_out / _in: count 0 at first == n_arc, the last arc, one past the end refused ("bad range") with the column unchanged"""
    L = ST.shard_api()
    c = ranks[0]
    h, n_seq, opt, _ = make_input("five")
    S = ST.sharded_stages(ranks, h, n_seq, opt, [0, n_seq], 1, 0)
    col = c.asg_download()[0]["oldel"].copy()
    n = len(col)
    assert n > 4
    p = ST.xbuf(c, 0, 16)
    ST.dev_write(c, p, np.full(16, 0xA5, np.uint8))
    assert L.mahip_asg_flags_out(c.h, p, n, 0) == 0 and L.mahip_asg_flags_in(c.h, p, n, 0) == 0
    assert (ST.dev_read(c, p, 16) == 0xA5).all()
    assert L.mahip_asg_flags_out(c.h, p, n - 1, 1) == 0
    got = ST.dev_read(c, p, 16)
    assert got[:4].view("<u4")[0] == col[-1] and (got[4:] == 0xA5).all()
    for first, count in ((n, 1), (n - 1, 2), (0, n + 1)):
        assert L.mahip_asg_flags_out(c.h, p, first, count) == -1 and b"mahip_asg_flags_out: bad range" in ma.lib().mahip_strerror()
        assert L.mahip_asg_flags_in(c.h, p, first, count) == -1 and b"mahip_asg_flags_in: bad range" in ma.lib().mahip_strerror()
    assert (ST.dev_read(c, p, 16)[4:] == 0xA5).all()
    same(c.asg_download()[0]["oldel"], col, "the column after the refused calls")
    ST.dev_write(c, p, np.array([col[-1] | 0x80000000], dtype="<u4"))
    assert L.mahip_asg_flags_in(c.h, p, n - 1, 1) == 0
    after = c.asg_download()[0]["oldel"]
    same(after[:-1], col[:-1], "the column in front of the last arc")
    assert after[-1] == col[-1] | 0x80000000
