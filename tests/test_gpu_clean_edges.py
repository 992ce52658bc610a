"""GPU: the tail of the pipeline -- the four order-dependent cleaners (miniasm_amd/csrc/clean.hip over clean_core.h), the unitig construction (ug.hip over
ug_core.h) and the scan both lean on (scan.hip) -- at every size they branch on, through the C ABI (mahip_asg_upload -> cleaner or mahip_ug_gen -> download),
every case against the unmodified reference library on the same graph: the graph after every call, the call's return value, and for unitigs the members,
lengths, ends, circular flags, unitig arcs and the ma_ug_print text.  The graphs come from the builders in stages.py (Gb, ladder_bubble, fan_bubble,
hub_bubble, tip_comb, internal_comb, tip_piece, biloop_piece, chain_graph): symmetric, sorted, indexed, no multi-arcs.

A. bubble tables tier by tier at the product's default sizes: ladders whose probe holds 11 / 12 / 13, 767 / 768 / 769, 12 287 / 12 288 / 12 289 and
   196 608 / 196 609 vertices, fans at the first three borders, tips inside; the tier (0, 0, 1 / 1, 1, 2 / 2, 2, 3 / 3, 4), the kernel form (thread / wave
   with the table in LDS / in HBM) and the sources per tier from mahip_clean_last; at every border a probe that overflows the tier and three that fill it and
   then fail (too far, a cycle through the source, no sink), each followed on the same table by a bubble over the same vertices that must pop.
B. the wave form's staging (64 arcs of the expanded vertex at a time), inside a probe that has already overflowed tier 0: expanded vertices of 1, 2, 63, 64,
   65, 127, 128, 129 and 200 arcs; at list positions 0, 63 and 64 an arc flagged deleted, an arc back to the source that is flagged deleted too, and the arc
   on which d + l is max_dist / max_dist + 1; and arcs at those positions that are dead only by the stamp of a smaller source, met in the second sweep.
   (A target met twice in one vertex's list would be a multi-arc: the builders' contract has none.)
C. strides: 8 193 bubbles of 13 entries -- 16 386 overflowing sources on the LDS form's 8 192 blocks; sources in lanes 0 and 63 of a 64-vertex chunk and as
   the graph's last vertex; and the cases named *_in_child_too once more in a fresh process each under MA_BUBBLE_THREADS0=64 (64 / 4 / 1 / 1 / 1 tables: every
   stride loops), MA_BUBBLE_THREAD_TIERS=1 (the thread form in the upper tiers) and MA_BUBBLE_LDS_CAP=16 (the wave form with its table in HBM from tier 1 on).
D. the fixpoint: chains of dependent actions of depth 1, 2, 3, 8 and 40 for asg_cut_tip, asg_cut_internal and asg_pop_bubble (a pop that makes the next source
   a bubble, the later ones in tier 1), ids ascending (D + 1 sweeps) and descending (2).
E. rule parameters: tips of max_ext - 1 / max_ext / max_ext + 1 reads ending in each end kind, max_ext 1, 2, 4; asg_cut_internal with 1, 2, 3;
   asg_cut_biloop with ov > / == / < ox and the fork on the walk's last step and one behind it.
F. shapes: R = 1, 63, 64, 65, 257, 1000 without any arc; A < R with the acting reads last; V = 2048 x 256 (k_clean_rule's grid) and one read less / more, acting
   vertices at both ends.
G. unitigs: chains and rings of 1, 2, 3 and 2^k - 1 / 2^k / 2^k + 1 reads (k = 5 .. 17) as the whole graph, the discovery vertex at head, middle and tail,
   mixed strands, the same inside a larger graph; 255 / 256 / 257 unitigs; U = 2047 / 2048 / 2049, V = 2048, A = 2048 (one tile of the scan and the first
   chained launch) and V = 524 288 / 524 290 (256 tiles: still chained; 257: reduce / scan / downsweep); the form every scan of every case took is asserted
   from mahip_scan_forms (k_scan_down alone / k_scan_chain / k_scan_reduce).

Every size a case claims is asserted present, from the input graph or from mahip_clean_last.  All integers: equality everywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import miniasm_amd as ma
import refapi as R
import stages as ST
from test_host_vs_ref import libc, product_graph_api

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not built")]

IS_EMU = getattr(ma, "IS_EMU", False)
THREAD_TIERS = "MA_BUBBLE_THREAD_TIERS" in os.environ
LDS_CAP = min(int(os.environ.get("MA_BUBBLE_LDS_CAP", "1024")), 1024)
CAPS = (16, 1024, 16384, 262144, 4194304)  # the product's default table sizes (clean.hip: bub_cap); a probe fits while it holds at most 3/4 of them
BORDERS = tuple(c * 3 // 4 for c in CAPS)  # 12, 768, 12 288, 196 608, (3 145 728: the "visits more than" error, not built)
CLEANERS = {"cut_tip": "asg_cut_tip", "cut_internal": "asg_cut_internal", "cut_biloop": "asg_cut_biloop", "pop_bubble": "asg_pop_bubble"}


def tier_of(entries):
    return next(t for t, b in enumerate(BORDERS) if entries <= b)


def form_of(tier):
    return ST.FORM_THREAD if tier == 0 or THREAD_TIERS else ST.FORM_LDS if CAPS[tier] <= LDS_CAP else ST.FORM_HBM


def test_default_table_sizes():
    assert "MA_BUBBLE_CAP0" not in os.environ and "MA_BUBBLE_CAP1" not in os.environ and "MA_BUBBLE_SEQ" not in os.environ, "this module is about the default sizes"
    assert BORDERS[:4] == (12, 768, 12288, 196608) and [tier_of(e) for e in (11, 12, 13, 768, 769, 12288, 12289, 196608, 196609)] == [0, 0, 1, 1, 2, 2, 3, 3, 4]


class RefGraph:
    """the graph in malloc'ed memory, as the reference library wants it (is_srt and is_symm set: taken as it is)"""

    def __init__(self, arcs, seq, idx):
        self.g = g = ma.Asg()
        for field, arr in (("arc", arcs), ("seq", seq), ("idx", idx)):
            p = libc.malloc(max(arr.nbytes, 16))
            C.memmove(p, arr.ctypes.data, arr.nbytes)
            setattr(g, field, p)
        g.m_arc, g.n_arc_srt, g.m_seq, g.n_seq_symm = max(len(arcs), 1), len(arcs) | 1 << 31, max(len(seq), 1), len(seq) | 1 << 31

    def arrays(self):
        return R.asg_arrays(C.pointer(self.g))

    def free(self):
        for f in ("arc", "seq", "idx"):
            R.ref().free_buf(getattr(self.g, f))


def same_graph(got, want, what):
    for k, name in enumerate(("arcs", "seq", "index")):
        assert len(got[k]) == len(want[k]), "%s: %d vs %d %s" % (what, len(got[k]), len(want[k]), name)
        assert got[k].tobytes() == want[k].tobytes(), "%s: %s differ from the reference's" % (what, name)


def run_script(ctx, graph, script, what):
    """upload, then every (cleaner, argument) of the script on the device and in the reference library, the graph compared after every call
    -> [(return value, n_tips or None, mahip_clean_last)]"""
    L, LR = ST.clean_api(), R.ref()
    n_seq, arcs, seq, idx = graph
    ST.asg_upload(ctx, arcs, seq, idx)
    ref = RefGraph(arcs, seq, idx)
    out = []
    try:
        for fn, arg in script:
            a, b = C.c_uint32(0), C.c_uint32(0)
            if fn == "del_short":
                ma._chk(L.mahip_asg_del_short(ctx.h, arg, C.byref(a)), fn)
                if a.value:
                    ctx.symm()  # asg.c:95-98
                want = LR.asg_arc_del_short(C.byref(ref.g), arg)
            else:
                if fn == "pop_bubble":
                    ma._chk(L.mahip_asg_pop_bubble(ctx.h, arg, C.byref(a), C.byref(b)), fn)
                else:
                    ma._chk(getattr(L, "mahip_asg_" + fn)(ctx.h, arg, C.byref(a)), fn)
                want = getattr(LR, CLEANERS[fn])(C.byref(ref.g), arg)
            assert a.value == want, "%s: %s(%r) returned %d, the reference %d" % (what, fn, arg, a.value, want)
            same_graph(ctx.asg_download(), ref.arrays(), "%s after %s(%r)" % (what, fn, arg))
            out.append((a.value, b.value if fn == "pop_bubble" else None, ST.clean_last(ctx) if fn != "del_short" else None))
    finally:
        ref.free()
    return out


def check_bubble(ctx, graph, max_dist, what, pops, n_tips, tier, exact_src=None):
    (n, tips, info), = run_script(ctx, graph, [("pop_bubble", max_dist)], what)
    print("%s: %d pops, %d tips, %r" % (what, n, tips, info))
    assert (n, tips) == (pops, n_tips), "%s: %d pops / %d tips, the construction has %d / %d" % (what, n, tips, pops, n_tips)
    assert info["max_tier"] == tier and not info["seq_sweep"], "%s: meant tier %d: %r" % (what, tier, info)
    assert info["form"][:tier + 1] == [form_of(t) for t in range(tier + 1)] and not any(info["form"][tier + 1:]), "%s: kernel forms %r" % (what, info["form"])
    if exact_src is not None:
        assert info["n_src"] == exact_src, "%s: sources per tier %r, the construction gives %r" % (what, info["n_src"], exact_src)
    return info


def lone_bubble_src(tier, n_bubbles=1):
    """one bubble = two sources, s and the sink's complement; sweep 1 probes both through every tier up to the one that holds it, sweep 2 (the one that finds
    nothing new) probes s again, while the sink's complement now sees one live arc and is turned away in tier 0: 4 sources in tier 0, 3 in every tier above"""
    return [n_bubbles * (4 if t == 0 else 3 if t <= tier else 0) for t in range(5)]


# ------------------------------------------------------------------------------------------------------------- A
def ladder(entries, broken=None, tips=0, pad=3, mixed=False):
    gb = ST.Gb(mixed)
    gb.reads(pad)
    m1, m2 = ST.ladder_of(entries - tips)
    info = ST.ladder_bubble(gb, m1, m2, broken=broken if broken != "far" else None, tips=tips)
    assert info["entries"] == entries and (tips or info["far_is_last"])
    return gb.finish(d_len=0), info


@pytest.mark.parametrize("tier", [0, 1, 2, 3])
def test_ladders_on_both_sides_of_every_table_border(tier, gpu_ctx):
    """in this order on one context, so that every probe finds the table as the one before left it: one entry too many (the tier overflows: the table is handed
    back through the overflow path), three probes that fill the tier to the border and then give up on their LAST arc, then the bubbles that fit"""
    B = BORDERS[tier]
    g, info = ladder(B + 1)
    check_bubble(gpu_ctx, g, info["far"], "ladder of %d entries" % (B + 1), 1, 0, tier + 1, lone_bubble_src(tier + 1) if tier + 1 > 0 else None)
    for broken in ("far", "cycle", "nosink"):
        g, info = ladder(B, broken)
        i = check_bubble(gpu_ctx, g, info["far"] - (1 if broken == "far" else 0), "ladder of %d entries, %s" % (B, broken), 0, 0, tier)
        assert i["n_iter"] == 1
        g, info = ladder(B)  # the same vertices on the same table (block 0 / thread 0 of the tier): a slot left behind makes this one fail
        i = check_bubble(gpu_ctx, g, info["far"], "ladder of %d entries after the %s one" % (B, broken), 1, 0, tier, lone_bubble_src(tier))
        assert i["n_iter"] == 2
    for e in ((B - 1, B) if tier < 3 else (B,)):
        for mixed in (False, True):
            g, info = ladder(e, mixed=mixed)
            check_bubble(gpu_ctx, g, info["far"], "ladder of %d entries" % e, 1, 0, tier, lone_bubble_src(tier))
            check_bubble(gpu_ctx, g, info["far"] - 1, "ladder of %d entries, one too far" % e, 0, 0, tier)


@pytest.mark.parametrize("entries", [11, 12, 13, 767, 768, 769])
def test_fans_and_tips_on_both_sides_of_the_first_two_borders_in_child_too(entries, gpu_ctx):
    tier = tier_of(entries)
    for tips in (0, 3):
        gb = ST.Gb(mixed=bool(tips))
        gb.reads(5)
        info = ST.fan_bubble(gb, entries - 1 - tips, tips)
        g = gb.finish()
        assert info["entries"] == entries
        cnt = (g[3] & np.uint64(0xffffffff)).astype(np.int64)
        assert cnt[info["s"]] == cnt[info["t1"]] == entries - 1 - tips and info["s"] < info["t1"]
        i = check_bubble(gpu_ctx, g, 50000, "fan of %d entries, %d tips" % (entries, tips), 1, tips, tier, None if tips else lone_bubble_src(tier))
        assert i["n_iter"] == 2
        check_bubble(gpu_ctx, g, info["far"] - 1, "fan of %d entries, too far" % entries, 0, 0, tier_of(entries - tips - 1) if tier_of(entries - tips - 1) < tier else tier)
        g2, info2 = ladder(entries, tips=tips)
        check_bubble(gpu_ctx, g2, 50000, "ladder of %d entries, %d tips" % (entries, tips), 1, tips, tier)


@pytest.mark.parametrize("entries", [12287, 12288, 12289])
def test_fans_on_both_sides_of_the_third_border(entries, gpu_ctx):
    """one expanded vertex of 12 286 .. 12 288 arcs: 192 batches of the wave form against a table in HBM.  (No fan at the fourth border: a pop deletes the
    mirror of every walked arc by a search of the sink's list, k^2 / 2 steps on one lane -- and in the reference -- for a fan of k: half a minute per case on the
    device already here; the ladders cover that border.)"""
    tier = tier_of(entries)
    gb = ST.Gb()
    gb.reads(7)
    info = ST.fan_bubble(gb, entries - 1)
    g = gb.finish()
    cnt = (g[3] & np.uint64(0xffffffff)).astype(np.int64)
    assert info["entries"] == entries and cnt[info["s"]] == cnt[info["t1"]] == entries - 1
    i = check_bubble(gpu_ctx, g, 50000, "fan of %d entries" % entries, 1, 0, tier, lone_bubble_src(tier))
    assert i["n_iter"] == 2


# ------------------------------------------------------------------------------------------------------------- B
HUB_ARCS = (1, 2, 63, 64, 65, 127, 128, 129, 200)


@pytest.mark.parametrize("nv", HUB_ARCS)
def test_wave_form_expanded_vertices_in_child_too(nv, gpu_ctx):
    gb = ST.Gb()
    gb.reads(2)
    info = ST.hub_bubble(gb, nv)
    g = gb.finish()
    assert 13 < info["entries"] <= 768 and nv in set((g[3] & np.uint64(0xffffffff)).tolist())
    n_cand = int(((g[3] & np.uint64(0xffffffff)) >= 2).sum())  # s, F and (from two arcs on) X are handed to tier 0 in both sweeps; s overflows it in both, X -- all its
    src = [2 * n_cand, 2 + (nv > 12), 0, 0, 0]                  # targets are arc-less: no bubble -- only in the first (in the second its read is dead) and only above 12 arcs
    i = check_bubble(gpu_ctx, g, 50000, "hub of %d arcs" % nv, 1, info["n_tips"], 1, src)
    assert i["n_iter"] == 2


@pytest.mark.parametrize("pos", [0, 63, 64])
@pytest.mark.parametrize("special", ["dead", "v0_dead", "far"])
def test_wave_form_decisions_at_batch_positions_in_child_too(special, pos, gpu_ctx):
    for nv in sorted({pos + 1, 64, 65, 130} - set(range(pos + 1))):
        gb = ST.Gb()
        gb.reads(2)
        info = ST.hub_bubble(gb, nv, special, pos)
        g = gb.finish()
        n_seq, arcs, seq, idx = g
        st = [int(idx[v] >> np.uint64(32)) for v in range(2 * n_seq) if int(idx[v] & np.uint64(0xffffffff)) == nv]
        x0 = next(s for s in st if (arcs["ul"][s] & np.uint64(0xffffffff)) == 100)  # X's list: presence of what the case is about, at the position it claims
        if special == "far":
            ln = (arcs["ul"][x0:x0 + nv] & np.uint64(0xffffffff)).astype(np.int64)
            assert ln[pos] == 100 + pos and (ln[pos:] == ln[pos]).all() and (pos == 0 or ln[pos - 1] < ln[pos])
            check_bubble(gpu_ctx, g, info["far"], "hub of %d arcs, d + l == max_dist at %d" % (nv, pos), 1, info["n_tips"], 1)
            check_bubble(gpu_ctx, g, info["far"] - 1, "hub of %d arcs, d + l == max_dist + 1 at %d" % (nv, pos), 0, 0, 1)
        else:
            assert arcs["oldel"][x0 + pos] >> 31 and (arcs["oldel"][x0:x0 + nv] >> 31).sum() == 1
            assert (arcs["v"][x0 + pos] == info["s"]) == (special == "v0_dead")
            check_bubble(gpu_ctx, g, 50000, "hub of %d arcs, %s at %d" % (nv, special, pos), int(info["pops"]), info["n_tips"], 1)


@pytest.mark.parametrize("nv", [70, 130, 200])
def test_wave_form_arcs_stamped_dead_by_a_smaller_source_in_child_too(nv, gpu_ctx):
    """X's arcs at batch positions 0, 63 and 64 (and everywhere but nv - 2) carry no base flag: they are dead for s only because S0 < s stamped them.  s expands
    X in the second sweep, in the wave form, after tier 0 has overflowed: cl_arc_dead and cl_live_out compare the stamp with the source there"""
    gb = ST.Gb()
    gb.reads(2)
    fan = ST.stamped_hub(gb, nv, outer=False)
    g = gb.finish()
    ref = RefGraph(*g[1:])  # presence, from the reference alone: S0's pop leaves X exactly its arc at position nv - 2
    try:
        assert R.ref().asg_pop_bubble(C.byref(ref.g), 50000) == 1
        arcs, _, idx = ref.arrays()
        st, cnt = int(idx[fan["X"]] >> np.uint64(32)), int(idx[fan["X"]] & np.uint64(0xffffffff))
        assert cnt == 1 and int(arcs["ul"][st] & np.uint64(0xffffffff)) == 10 + (nv - 2) + 3 and nv - 2 not in (0, 63, 64)
    finally:
        ref.free()
    gb = ST.Gb()
    gb.reads(2)
    info = ST.stamped_hub(gb, nv)
    g = gb.finish()
    n_seq, arcs, seq, idx = g
    assert info["S0"] < info["s"] and int(idx[info["X"]] & np.uint64(0xffffffff)) == nv
    st = int(idx[info["X"]] >> np.uint64(32))
    assert not (arcs["oldel"][st:st + nv] >> 31).any() and (np.diff((arcs["ul"][st:st + nv] & np.uint64(0xffffffff)).astype(np.int64)) == 1).all()
    i = check_bubble(gpu_ctx, g, 50000, "hub of %d arcs, all but one stamped by a smaller source" % nv, 2, info["n_tips"], 1)
    assert i["n_iter"] >= 2 and i["n_src"][1] >= 2, "s overflows tier 0 in the sweep that sees the stamps too"


# ------------------------------------------------------------------------------------------------------------- C
def many_ladders(sizes, broken_every=0):
    gb = ST.Gb()
    pops = 0
    for k, e in enumerate(sizes):
        b = "cycle" if broken_every and k % broken_every == 1 else None
        ST.ladder_bubble(gb, *ST.ladder_of(e), broken=b)
        pops += b is None
        if k % 5 == 0:
            gb.reads(1 + k % 3)  # arc-less reads in between
    return gb.finish(), pops


def test_more_overflowing_sources_than_the_lds_form_has_blocks(gpu_ctx):
    n = 8193
    g, pops = many_ladders([13] * n)
    assert pops == n
    i = check_bubble(gpu_ctx, g, 50000, "%d ladders of 13 entries" % n, n, 0, 1, lone_bubble_src(1, n))
    assert i["n_iter"] == 2 and i["n_src"][1] == 3 * n and 2 * n > 8192


def test_a_few_hundred_sources_of_every_tier_in_child_too(gpu_ctx):
    """with MA_BUBBLE_THREADS0=64 every tier has fewer tables than this graph has sources for it: a table serves source after source, behind a pop, behind a
    probe that failed and behind one that overflowed"""
    sizes = [13] * 150 + [769] * 3 + [5, 12, 13, 40] * 40 + [769] * 4 + [12289, 12289]
    g, pops = many_ladders(sizes, broken_every=7)
    n_big = sum(1 for k, e in enumerate(sizes) if e > 768)
    i = check_bubble(gpu_ctx, g, 50000, "%d ladders, every seventh broken" % len(sizes), pops, 0, 3)
    assert i["n_iter"] == 2 and i["n_src"][0] > 2 * 64 and i["n_src"][1] > 2 * 190 and i["n_src"][2] >= 2 * n_big and i["n_src"][3] >= 4


def test_sources_in_lanes_0_and_63_and_as_the_last_vertex(gpu_ctx):
    gb = ST.Gb(mixed=True)
    want = []
    for first in (31, 96, 400):  # read 31 on its reverse strand = vertex 63; read 96 = vertex 192; more than 64 arc-less reads in front of read 400
        gb.reads(first - gb.n)
        want.append(ST.ladder_bubble(gb, 6, 6)["s"])
    assert [w % 64 for w in want[:2]] == [63, 0]
    gb.reads((3 - (gb.n + 14) % 3) % 3 + (3 if (gb.n + 14) % 3 == 1 else 0))
    last = ST.ladder_bubble(gb, 6, 6)
    g = gb.finish()
    assert last["t1"] == 2 * g[0] - 1, "the last bubble's second source is the graph's last vertex"
    cnt = (g[3] & np.uint64(0xffffffff)).astype(np.int64)
    assert all(cnt[w] == 2 for w in want) and cnt[last["t1"]] == 2 and cnt[256:640].sum() == 0
    check_bubble(gpu_ctx, g, 50000, "bubbles at chunk edges", 4, 0, 1, lone_bubble_src(1, 4))


CHILD_ENVS = [{"MA_BUBBLE_THREADS0": "64"}, {"MA_BUBBLE_THREAD_TIERS": "1"}, {"MA_BUBBLE_LDS_CAP": "16"}]


@pytest.mark.parametrize("env", CHILD_ENVS, ids=["%s=%s" % kv for e in CHILD_ENVS for kv in e.items()])
def test_named_subset_again_in_a_fresh_process(env):
    """the width and form switches are read once per process: the *_in_child_too cases once more, one child at a time, each under its own time limit;
    a child that fails, aborts or runs out of time ends the test there"""
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"] + (["-p", "emu_plugin"] if IS_EMU else [])
    cmd += [os.path.abspath(__file__), "-k", "in_child_too"]
    r = subprocess.run(cmd, cwd=ma.ROOT, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    tail = r.stdout[-4000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail and " skipped" not in tail, tail


# ------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("depth", [1, 2, 3, 8, 40])
@pytest.mark.parametrize("rule", ["cut_tip", "cut_internal"])
def test_fixpoint_needs_as_many_sweeps_as_the_chain_is_deep(rule, depth, order, gpu_ctx):
    for mixed in (False, True):
        g, actions, sweeps = (ST.tip_comb if rule == "cut_tip" else ST.internal_comb)(depth, order, mixed)
        (n, _, info), = run_script(gpu_ctx, g, [(rule, 4 if rule == "cut_tip" else 1)], "%s comb, depth %d, %s" % (rule, depth, order))
        assert n == actions, "the construction has %d actions, the reference found %d" % (actions, n)
        assert info["n_iter"] == sweeps, "%s comb, depth %d, %s: %d sweeps, the construction needs %d" % (rule, depth, order, info["n_iter"], sweeps)


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("depth,inner", [(1, 1), (2, 1), (3, 1), (8, 1), (40, 1), (3, 14)])
def test_fixpoint_of_dependent_bubble_pops(depth, inner, order, gpu_ctx):
    """a pop that makes the next source a bubble; the bubble sweeps run the overflow tiers and the second comparison of the stamps inside every sweep"""
    g, pops, sweeps, max_dist = ST.bubble_comb(depth, order, inner)
    (n, tips, info), = run_script(gpu_ctx, g, [("pop_bubble", max_dist)], "bubble comb, depth %d, %s" % (depth, order))
    print(info)
    assert (n, tips) == (pops, 0), "the construction has %d pops, the reference found %d" % (pops, n)
    assert info["n_iter"] == sweeps and not info["seq_sweep"], "bubble comb, depth %d, %s: %d sweeps, the construction needs %d" % (depth, order, info["n_iter"], sweeps)
    if order == "ascending" and (depth >= 8 or inner > 12):  # the dependent sources hold more than 12 vertices: they pop in tier 1, in a sweep later than the first
        assert info["max_tier"] == 1 and info["n_src"][1] > 0 and info["form"][1] == form_of(1), info


# ------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("max_ext", [1, 2, 4])
def test_tips_around_max_ext_ending_in_every_kind(max_ext, gpu_ctx):
    for mixed in (False, True):
        gb = ST.Gb(mixed)
        ring = gb.ring(40)
        cut = 0
        for n in (max_ext - 1, max_ext, max_ext + 1):
            for end in ST.END_KINDS:
                if n >= 1:
                    ST.tip_piece(gb, n, end, gb.ring(6) if end != "TIP" else ring)
                    cut += n <= max_ext
        g = gb.finish()
        (n, _, info), = run_script(gpu_ctx, g, [("cut_tip", max_ext)], "tips around max_ext %d" % max_ext)
        assert n == cut, "tips of up to %d reads go, one read more stays: %d cut, the construction has %d" % (max_ext, n, cut)


@pytest.mark.parametrize("max_ext", [1, 2, 3])
def test_cut_internal_around_max_ext(max_ext, gpu_ctx):
    gb = ST.Gb()
    cut, pieces = 0, []
    for n in (max_ext - 1, max_ext, max_ext + 1):
        if n >= 1:  # h -> c_1 .. c_n -> another ring: wedged between two forks
            h, g2 = gb.ring(6), gb.ring(6)
            c = gb.reads(n)
            gb.arc(gb.v(h[1]), gb.v(c[0]), 20)
            gb.path(c, 10)
            gb.arc(gb.v(c[-1]), gb.v(g2[1]), 30)
            cut += n <= max_ext
            pieces.append((c, n <= max_ext))
    g = gb.finish()
    (n, _, info), = run_script(gpu_ctx, g, [("cut_internal", max_ext)], "internal pieces around max_ext %d" % max_ext)
    assert n >= cut > 0, (n, cut)  # (with max_ext > 1 the reference also takes ring stretches between two forks; its count, compared exactly in run_script, is the yardstick)
    seq = gpu_ctx.asg_download()[1]
    for c, goes in pieces:  # the built pieces themselves: gone up to max_ext reads, whole beyond
        assert ((seq[c] >> 31) == goes).all(), "piece of %d reads, max_ext %d" % (len(c), max_ext)


@pytest.mark.parametrize("max_ext", [1, 2, 4])
def test_biloops_by_overlap_and_walk_length(max_ext, gpu_ctx):
    gb = ST.Gb()
    cut = 0
    for n in (max_ext, max_ext + 1):
        for ov, ox in ((900, 800), (800, 800), (700, 800)):
            ST.biloop_piece(gb, n, ov, ox, gb.ring(6))
            cut += ov > ox and n <= max_ext
    g = gb.finish()
    script = [("cut_biloop", max_ext), ("del_short", 0.7), ("cut_tip", max_ext), ("cut_biloop", max_ext)]
    res = run_script(gpu_ctx, g, script, "bi-loops, max_ext %d" % max_ext)
    assert res[0][0] == cut == 1, "only ov > ox with the fork within max_ext steps is cut: %d, the construction has %d" % (res[0][0], cut)


# ------------------------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("R_", [1, 63, 64, 65, 257, 1000])  # (k_clean_apply runs over max(A, R) in blocks of 256: above 256 reads a launch sized by A alone stops short)
def test_reads_without_any_arc_are_all_tips(R_, gpu_ctx):
    gb = ST.Gb()
    gb.reads(R_)
    g = gb.finish()
    assert len(g[1]) == 0
    res = run_script(gpu_ctx, g, [("cut_internal", 1), ("cut_biloop", 4), ("pop_bubble", 50000), ("cut_tip", 4)], "%d reads, no arcs" % R_)
    assert [r[0] for r in res] == [0, 0, 0, R_] and res[2][2]["n_iter"] == 0
    assert (gpu_ctx.asg_download()[1] >> 31).all()


@pytest.mark.parametrize("R_", [63, 64, 65, 200, 600])
def test_fewer_arcs_than_reads_with_the_actions_on_the_last_reads(R_, gpu_ctx):
    gb = ST.Gb()
    gb.reads(R_ - 9)
    ring = gb.ring(6)
    ST.tip_piece(gb, 3, "MULTI_NEI", ring)
    g = gb.finish()
    assert g[0] == R_ and 0 < len(g[1]) < R_
    (n, _, _), = run_script(gpu_ctx, g, [("cut_tip", 4)], "%d reads, %d arcs" % (R_, len(g[1])))
    assert n == R_ - 9 + 1
    seq = gpu_ctx.asg_download()[1]
    assert (seq >> 31).sum() == R_ - 6 and (seq[-3:] >> 31).all()


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_vertex_count_around_one_pass_of_the_rule_kernels_grid(d, gpu_ctx):
    R_ = 2048 * 256 // 2 + d
    gb = ST.Gb()
    first = ST.tip_piece(gb, 2, "MULTI_NEI", gb.ring(6))  # acting vertices at the front ...
    ST.biloop_piece(gb, 1, 900, 800, gb.ring(6))
    lone = gb.reads(R_ - gb.n - 16)
    ST.biloop_piece(gb, 1, 900, 800, gb.ring(6))
    last = ST.tip_piece(gb, 2, "MULTI_NEI", gb.ring(6))  # ... and as the last reads
    g = gb.finish()
    assert 2 * g[0] == 2048 * 256 + 2 * d
    res = run_script(gpu_ctx, g, [("cut_biloop", 4), ("cut_internal", 1), ("cut_tip", 4)], "V = %d" % (2 * R_))
    assert res[0][0] == 2 and res[2][0] >= len(lone) + 2
    seq = gpu_ctx.asg_download()[1]
    assert (seq[first] >> 31).all() and (seq[last] >> 31).all() and (seq[lone] >> 31).all() and last[-1] == R_ - 1


# ------------------------------------------------------------------------------------------------------------- G
class Utg(C.Structure):  # miniasm.h: ma_utg_t
    _fields_ = [("len_circ", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("m", C.c_uint32), ("n", C.c_uint32), ("a", C.POINTER(C.c_uint64)), ("s", C.c_void_p)]


class Ug(C.Structure):  # miniasm.h: ma_ug_t
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.POINTER(Utg)), ("g", C.POINTER(ma.Asg))]


def scan_form(n):
    """the scan's form by size (scan.hip): one tile of 2048 (k_scan_down alone), up to 256 tiles the chained launch (k_scan_chain), above reduce / scan / downsweep"""
    return 0 if n <= 2048 else 1 if n <= 256 * 2048 else 2


def test_scan_form_borders():
    assert [scan_form(n) for n in (2047, 2048, 2049, 524288, 524289)] == [0, 0, 1, 1, 2]


def check_unitigs(ctx, graph, what, tmpdir, n_utg=None, text=True):
    """mahip_ug_gen + mahip_ug_download against the reference's ma_ug_t, field by field; then the text of both libraries' ma_ug_print"""
    L, LR, LP = ST.clean_api(), R.ref(), product_graph_api()
    n_seq, arcs, seq, idx = graph
    ST.asg_upload(ctx, arcs, seq, idx)
    nu, nm, na = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    before = ST.scan_forms(ctx)
    ma._chk(L.mahip_ug_gen(ctx.h, C.byref(nu), C.byref(nm), C.byref(na)), "ug_gen")
    U = nu.value
    # the pass scans V flags, then (if there is a unitig) U counts and A arc flags: each size must have taken the form its size calls for
    want = [0, 0, 0]
    for n in [2 * n_seq] + ([U, len(arcs)] if U else []):
        if n:
            want[scan_form(n)] += 1
    got = [a - b for a, b in zip(ST.scan_forms(ctx), before)]
    assert got == want, "%s: scans of %r elements took the forms %r (one tile, chained, three-phase), their sizes call for %r" % (what, (2 * n_seq, U, len(arcs)), got, want)
    u = [np.zeros(U + 1, dtype="<u4") for _ in range(5)]
    mem, ua = np.zeros(nm.value + 1, dtype="<u8"), np.zeros(na.value + 1, dtype=ma.ARC_DT)
    ma._chk(L.mahip_ug_download(ctx.h, *[x.ctypes.data for x in u], mem.ctypes.data, ua.ctypes.data), "ug_download")
    u_n, u_len, u_start, u_end, u_off = [x[:U] for x in u]
    ref = RefGraph(arcs, seq, idx)
    LR.ma_ug_gen.restype = C.POINTER(Ug)
    ug = LR.ma_ug_gen(C.byref(ref.g))
    try:
        r = ug.contents
        assert U == r.n, "%s: %d unitigs, the reference has %d" % (what, U, r.n)
        if n_utg is not None:
            assert U == n_utg, "%s: meant %d unitigs, has %d" % (what, n_utg, U)
        for k in range(U):
            t = r.a[k]
            circ = t.len_circ >> 31
            assert (int(u_n[k]), int(u_len[k])) == (t.n, t.len_circ & 0x7fffffff), "%s: unitig %d: reads / length %r vs %r" % (what, k, (u_n[k], u_len[k]), (t.n, t.len_circ & 0x7fffffff))
            assert circ == (u_start[k] == 0xffffffff) == (u_end[k] == 0xffffffff), "%s: unitig %d: circular flag" % (what, k)
            assert circ or (int(u_start[k]), int(u_end[k])) == (t.start, t.end), "%s: unitig %d: ends" % (what, k)
            want = np.ctypeslib.as_array(t.a, shape=(t.n,))
            assert mem[int(u_off[k]):int(u_off[k]) + t.n].tobytes() == want.tobytes(), "%s: unitig %d: members differ" % (what, k)
        assert nm.value == int(u_n.sum())
        ra = R.asg_arrays(r.g)[0]
        assert na.value == len(ra) and R.canon(ua[:na.value]).tobytes() == R.canon(ra).tobytes(), "%s: unitig arcs differ" % what
        if text:
            outs = []
            g2 = RefGraph(arcs, seq, idx)
            LP.ma_ug_gen.restype = C.c_void_p
            for tag, Lx, h in (("ref", LR, ug), ("mine", LP, None)):
                d = Lx.sd_init()
                for i in range(n_seq):
                    Lx.sd_put(d, b"r%d" % i, 0)
                h = h if h is not None else LP.ma_ug_gen(C.byref(g2.g))
                path = os.path.join(tmpdir, "ce_%s.gfa" % tag)
                fp = libc.fopen(path.encode(), b"w")
                Lx.ma_ug_print(h, d, None, fp)
                libc.fclose(fp)
                outs.append(open(path, "rb").read())
                if tag == "mine":
                    LP.ma_ug_destroy(h)
                Lx.sd_destroy(d)
            g2.free()
            assert outs[0] == outs[1], "%s: ma_ug_print text differs" % what
    finally:
        LR.ma_ug_destroy.argtypes = [C.c_void_p]
        LR.ma_ug_destroy(C.cast(ug, C.c_void_p))
        ref.free()
    return U, nm.value, na.value


def _ug_argtypes():
    LR, LP = R.ref(), product_graph_api()
    for Lx in (LR, LP):
        Lx.sd_init.restype = C.POINTER(ma.Sdict)
        Lx.sd_put.restype = C.c_int32
        Lx.sd_put.argtypes = [C.POINTER(ma.Sdict), C.c_char_p, C.c_uint32]
        Lx.sd_destroy.argtypes = [C.POINTER(ma.Sdict)]
        Lx.ma_ug_gen.argtypes = [C.POINTER(ma.Asg)]
        Lx.ma_ug_print.argtypes = [C.c_void_p, C.POINTER(ma.Sdict), C.c_void_p, C.c_void_p]
    LP.ma_ug_destroy.argtypes = [C.c_void_p]


CHAIN_LENGTHS = (2, 3) + tuple(2 ** k + d for k in range(5, 18) for d in (-1, 0, 1))


@pytest.mark.parametrize("L_", CHAIN_LENGTHS)
def test_one_chain_or_ring_that_is_the_whole_graph(L_, gpu_ctx, tmpdir_s):
    """pointer jumping runs bitlen_u64(V) + 1 rounds: the whole vertex set in ONE chain (V == 2L), lengths on both sides of every power of two"""
    _ug_argtypes()
    small = L_ <= 4097
    for ring in (False, True):
        for first in ((0, L_ // 2, 1) if small else (L_ // 2,)):  # the discovery vertex at the head, in the middle, at the tail
            for mixed in ((False, True) if small else (ring,)):
                g = ST.chain_graph(L_, ring, first, mixed)
                assert g[0] == L_ and len(g[1]) == 2 * (L_ - 1 + ring)
                U, n_mem, _ = check_unitigs(gpu_ctx, g, "%s of %d reads, read 0 at %d" % ("ring" if ring else "chain", L_, (L_ - first) % L_), tmpdir_s, n_utg=1, text=small or ring)
                assert n_mem == L_


def test_a_single_read_without_arcs_is_no_unitig(gpu_ctx, tmpdir_s):
    _ug_argtypes()
    gb = ST.Gb()
    gb.reads(1)
    assert check_unitigs(gpu_ctx, gb.finish(), "one read", tmpdir_s, n_utg=0) == (0, 0, 0)


@pytest.mark.parametrize("U_", [255, 256, 257, 2047, 2048, 2049])
def test_unitig_counts_around_the_mark_kernels_grid_and_the_scans_tile(U_, gpu_ctx, tmpdir_s):
    """U unitigs: chains of 2 and 3 reads, rings of 3, mixed strands, arc-less reads in between; joined by forks so that there are unitig arcs"""
    _ug_argtypes()
    gb = ST.Gb(mixed=True)
    for k in range(U_):
        if k % 3 == 2:
            ST.chain_graph(3, ring=True, first=k % 3, gb=gb)
        else:
            ST.chain_graph(2 + k % 2, gb=gb)
        if k % 7 == 0:
            gb.reads(1)
    g = gb.finish(d_len=7)
    check_unitigs(gpu_ctx, g, "%d unitigs" % U_, tmpdir_s, n_utg=U_, text=U_ < 300)


@pytest.mark.parametrize("L_", [1024, 1025, 1026])
def test_chains_inside_a_larger_graph_with_v_and_a_around_the_scans_tile(L_, gpu_ctx, tmpdir_s):
    """V = 2048 with L = 1024 (alone), A = 2048 with L = 1025; and the same chain beside forks, rings and bubbles, whose ends make unitig arcs"""
    _ug_argtypes()
    g = ST.chain_graph(L_, first=L_ // 3)
    assert 2 * g[0] == 2 * L_ and len(g[1]) == 2 * L_ - 2 and 2048 in (2 * L_, 2 * L_ - 2, 2 * L_ - 4)
    check_unitigs(gpu_ctx, g, "chain of %d reads" % L_, tmpdir_s, n_utg=1)
    gb = ST.Gb(mixed=True)
    ST.ladder_bubble(gb, 3, 4)
    ST.chain_graph(L_, first=5, gb=gb)
    ST.tip_piece(gb, 3, "MULTI_OUT", gb.ring(9))
    ST.chain_graph(33, ring=True, first=7, gb=gb)
    ST.fan_bubble(gb, 5)
    U, _, n_ua = check_unitigs(gpu_ctx, gb.finish(d_len=7), "chain of %d reads in a larger graph" % L_, tmpdir_s)
    assert U > 10 and n_ua > 10


@pytest.mark.parametrize("R_", [262144, 262145])
def test_vertex_counts_on_both_sides_of_the_chained_scans_limit(R_, gpu_ctx, tmpdir_s):
    """V = 524 288 = 256 tiles of the scan (the chained launch still) and V = 524 290 (257 tiles: reduce / scan / downsweep), one chain of 2^18 reads
    (19 + 1 jumping rounds) and a second short one"""
    _ug_argtypes()
    gb = ST.Gb()
    ST.chain_graph(262144 - 3, first=1000, gb=gb)
    ST.chain_graph(3, gb=gb)
    gb.reads(R_ - gb.n)
    g = gb.finish(d_len=7)
    assert 2 * g[0] in (524288, 524290) and 2048 < len(g[1]) <= 524288
    before = ST.scan_forms(gpu_ctx)
    check_unitigs(gpu_ctx, g, "V = %d" % (2 * g[0]), tmpdir_s, n_utg=2, text=False)
    got = [a - b for a, b in zip(ST.scan_forms(gpu_ctx), before)]
    assert got == ([1, 2, 0] if R_ == 262144 else [1, 1, 1]), "V = %d: 256 tiles are still one chained launch, 257 are not: %r" % (2 * g[0], got)
