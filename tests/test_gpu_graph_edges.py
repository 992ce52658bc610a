"""GPU: the graph kernels (miniasm_amd/csrc/graph.hip) stage by stage at every size edge they branch on, through the C ABI, against the C oracle
(order included; tie mode 0 is the stable order the oracle computes) and, where it is built, the unmodified reference library (tie mode 2).

A. arcs per READ (ma_sg_gen against given read lengths -> arc sort per read -> index -> census): reads of exactly 0, 1, 2, 63/64/65, 127/128/129,
   255/256/257, 511/512 arcs (register rows 1 / 2 / 4 / 8 of k_arc_group_sort), plus one of 513 (the whole sort takes the radix path), arcs of 21 and
   22 bits, all arcs on one strand, runs of equal keys, the edge reads in lanes 0 / 63 of a 64-read chunk and as the dictionary's last read; hit arrays
   on both sides of k_sg_emit's tile with 64-slot words of 0 / 1 / 5 / 6 / 64 candidates.
B. arcs per VERTEX (asg_arc_del_trans): hand-made graphs in which the lists of the expanded NEIGHBOURS are chosen too (stages.trans_gadget_graph), hubs
   of 1 .. 1300 arcs in every tier (alive, on a deleted read, with multi-arcs), chunks of 64 vertices with 1 .. 9 active ones, vertex ranges cut at
   odd borders; mahip_asg_trans_inner against the oracle's count on every one of them.
C. arc COUNTS (asg_arc_rm, both forms of the cleanup) on both sides of the tile and group sizes, every residue mod 8, eight deletion patterns.

Every size a test claims to cover is asserted to be present, from the oracle's output or the input graph.  All integers: equality everywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import miniasm_amd as ma
import refapi as R
import stages as ST

pytestmark = pytest.mark.gpu


def prof_names(ctx, fn):
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = fn()
        return out, {r["name"] for r in ctx.prof_get()}
    finally:
        ctx.prof_enable(False)


# ------------------------------------------------------------------------------------------------------------- A
def check_sg(ctx, hits, seq_len, opt, what, radix=None, sizes=None, reduce=True):
    """ma_sg_gen on `hits` against read lengths, then del_trans + symm.  radix: None = the register sort must have run alone; "arcs" = it ran, met a read
    of more than 512 arcs and the radix path took over; "bits" / "switch" = the radix path alone"""
    n_seq = len(seq_len)
    arcs, seq, idx, srt = ST.orc_sg(hits, seq_len, opt)
    per_read = np.bincount((arcs["ul"] >> np.uint64(33)).astype(np.int64), minlength=n_seq)
    if sizes is not None:  # presence: the oracle's graph has the stretches the case is about
        assert all(per_read[r] == n for r, n in sizes.items()), [(r, n, int(per_read[r])) for r, n in sizes.items() if per_read[r] != n]
    assert len(arcs) > 0, what
    # tie mode 0: sorted here, the stable order
    ctx.set_exact_ties(0)
    ctx.hits_upload(hits, n_seq)
    ctx.set_run_stride(0)
    ctx.sort()
    n_arc, names = prof_names(ctx, lambda: ctx.sg_gen(opt, use_sub=False, seq_len=seq_len))
    g = ctx.asg_download()
    assert n_arc == len(arcs), "%s: %d arcs vs %d" % (what, n_arc, len(arcs))
    assert g[0].tobytes() == arcs.tobytes(), "%s: arcs differ from the oracle's (order included)" % what
    assert g[1].tobytes() == seq.tobytes() and g[2].tobytes() == idx.tobytes(), "%s: seq / index differ" % what
    if radix is None:
        assert "k_arc_group_sort" in names and "k_arc_permute" not in names, (what, sorted(names))
    else:
        assert "k_arc_permute" in names and ("k_arc_group_sort" in names) == (radix == "arcs"), (what, radix, sorted(names))
    if reduce:
        sdel = (seq >> 31).astype(np.uint8)
        tr, tr_idx, cnt = ST.orc_reduce(n_seq, arcs, sdel, opt.gap_fuzz)
        n_red = ctx.del_trans(opt.gap_fuzz)  # (clean form of the cleanup: ma_sg_gen left arcs between live reads only and says so)
        assert (n_red, ST.trans_inner(ctx)) == (cnt["n_red"], cnt["n_inner"]), "%s: reduced / inner %r vs %r" % (what, (n_red, ST.trans_inner(ctx)), cnt)
        if n_red:
            assert ctx.symm() == (cnt["n_multi"], cnt["n_asymm"]), what
        g2 = ctx.asg_download()
        assert g2[0].tobytes() == tr.tobytes() and g2[2].tobytes() == tr_idx.tobytes(), "%s: graph after del_trans + symm differs" % what
    # tie mode 2: the hits as the oracle sorted them, indexed as they stand; the census, and the reference library's ma_sg_gen on the same array
    ctx.set_exact_ties(2)
    ctx.hits_upload(srt, n_seq)
    ctx.index()
    _, names2 = prof_names(ctx, lambda: ctx.sg_gen(opt, use_sub=False, seq_len=seq_len))
    g = ctx.asg_download()
    tie = ctx.tie_stats()
    want = ST.arc_tie_census(arcs)
    assert (tie["arc_tie_groups"], tie["arc_tie_arcs"]) == want, "%s: census %r vs %r" % (what, (tie["arc_tie_groups"], tie["arc_tie_arcs"]), want)
    assert ("k_arc_group_sort" in names2) == (radix in (None, "arcs")), (what, sorted(names2))
    assert R.canon(g[0]).tobytes() == R.canon(arcs).tobytes() and g[1].tobytes() == seq.tobytes() and g[2].tobytes() == idx.tobytes(), what
    if want[0] == 0:
        assert g[0].tobytes() == arcs.tobytes(), what
    if R.have_ref():
        r = ST.ref_sg(srt, seq_len, opt)
        assert g[0].tobytes() == r[0].tobytes(), "%s: arcs differ from the reference library's (order included)" % what
        assert g[1].tobytes() == r[1].tobytes() and g[2].tobytes() == r[2].tobytes(), "%s: seq / index differ from the reference library's" % what
    return per_read


SG_INPUTS = [  # (name, arguments of stages.arc_edge_hits, why the radix path runs)
    ("strand0", dict(strands="0", seed=0), None),
    ("strand1", dict(strands="1", seed=1), None),
    ("split", dict(strands="split", seed=2), None),
    ("few_lengths", dict(few_lengths=True, seed=3), None),
    ("few_lengths_strand0_1023_reads", dict(few_lengths=True, strands="0", n_seq=1023, seed=4), None),
    ("split_1025_reads", dict(n_seq=1025, seed=5), None),
    ("plus_513_arcs", dict(extra=(513,), few_lengths=True, seed=6), "arcs"),
    ("longest_21_bits", dict(longest=2 ** 21 - 1, seed=7), None),
    ("longest_22_bits", dict(longest=2 ** 21, seed=8), "bits"),
]


@pytest.mark.parametrize("switch", [False, True], ids=["default", "MA_ARC_RADIX"])
@pytest.mark.parametrize("name,kw,radix", SG_INPUTS, ids=[c[0] for c in SG_INPUTS])
def test_arcs_per_read_on_every_size_edge_of_the_arc_sort(name, kw, radix, switch, gpu_ctx):
    h, seq_len, sizes = ST.arc_edge_hits(**kw)
    assert sorted(sizes.values()) == sorted(ST.ARC_EDGE_SIZES + tuple(kw.get("extra", ())))
    assert len(seq_len) - 1 in sizes and 0 in sizes and 63 in sizes and sizes[len(seq_len) - 1] > 0
    opt = ma.default_opt()
    old = os.environ.get("MA_ARC_RADIX")
    if switch:
        os.environ["MA_ARC_RADIX"] = "1"  # read with getenv at every call
    try:
        per = check_sg(gpu_ctx, h, seq_len, opt, name, radix="switch" if switch and radix != "bits" else radix, sizes=sizes)
    finally:
        if switch:
            os.environ.pop("MA_ARC_RADIX")
            if old is not None:
                os.environ["MA_ARC_RADIX"] = old
    assert per[192:300].sum() == 0, "more than 64 reads without arcs between two edge reads"
    arcs = ST.orc_sg(h, seq_len, opt)[0]
    ln = (arcs["ul"] & np.uint64(0xffffffff)).astype(np.int64)
    if "longest" in kw:
        assert ln.max() == kw["longest"]
    if kw.get("strands", "split") != "split":  # every edge read's arcs on one vertex
        assert set(((arcs["ul"] >> np.uint64(32)) & np.uint64(1))[np.isin(arcs["ul"] >> np.uint64(33), list(sizes))].tolist()) == {int(kw["strands"])}
    if kw.get("few_lengths"):  # a run of equal (u, len) longer than a register row of 64 lanes: it crosses lane and row borders
        run = np.diff(np.flatnonzero(np.r_[True, arcs["ul"][1:] != arcs["ul"][:-1], True]))
        assert run.max() > 16 and ST.arc_tie_census(arcs)[0] > 50


@pytest.mark.parametrize("n_slots", [16383, 16384, 16385, 2 * 16384 + 1])
def test_sg_emit_tiles_and_words(n_slots, gpu_ctx):
    """k_sg_emit: hit arrays on both sides of its tile of 16384 slots, a last word that is not full, words of 0 / 1 / 5 / 6 / 64 candidates (lane walk below
    SG_DENSE = 6, the whole wave from there on), candidates dropped because another hit deleted one of their reads (asm.c:27-34)"""
    h, seq_len = ST.sg_emit_hits(n_slots)
    opt = ST.sg_emit_opt()
    assert len(h) == n_slots
    words = ST.sg_candidate_words(h, seq_len, opt)
    assert {0, 1, 5, 6, 64} <= set(words.tolist()), sorted(set(words.tolist()))
    arcs, seq, _, srt = ST.orc_sg(h, seq_len, opt)
    assert srt.tobytes() == h.tobytes(), "the builder's records are in sorted order: a slot's word is what the builder chose"
    assert (seq >> 31).sum() >= 2 and 0 < len(arcs) < words.sum(), "some candidates lose an endpoint to another hit's side effect"
    check_sg(gpu_ctx, h, seq_len, opt, "sg_emit %d slots" % n_slots)


# ------------------------------------------------------------------------------------------------------------- B
def check_trans(ctx, n_seq, arcs, seq, idx, fuzz, what, big=None):
    """marking alone (mahip_asg_del_trans_range over everything: the del bits are still there to look at), then the whole call with its cleanup"""
    L = ST.graph_api()
    marked, n_red, n_inner = ST.orc_trans_only(n_seq, arcs, idx, seq, fuzz)
    ST.asg_upload(ctx, arcs, seq, idx)
    got = C.c_uint32(0)
    _, names = prof_names(ctx, lambda: ma._chk(L.mahip_asg_del_trans_range(ctx.h, fuzz, 0, 2 * n_seq, C.byref(got)), "del_trans_range"))
    g = ctx.asg_download()
    assert (got.value, ST.trans_inner(ctx)) == (n_red, n_inner), "%s: reduced / inner iterations %r vs the oracle's %r" % (what, (got.value, ST.trans_inner(ctx)), (n_red, n_inner))
    assert g[0].tobytes() == marked.tobytes(), "%s: del bits differ from the oracle's" % what
    if big is not None:
        assert ("k_asg_trans_big" in names) == big, (what, sorted(names))
    ST.asg_upload(ctx, arcs, seq, idx)
    assert ctx.del_trans(fuzz) == n_red and ST.trans_inner(ctx) == n_inner, what
    g = ctx.asg_download()
    want, want_idx = ST.orc_rm_index(n_seq, marked, seq) if n_red else (arcs, idx)  # (chained form of the cleanup: an uploaded graph is not known to be clean)
    assert g[0].tobytes() == want.tobytes() and g[1].tobytes() == seq.tobytes() and g[2].tobytes() == want_idx.tobytes(), "%s: graph after the call differs from the oracle's" % what
    tr, tr_idx, cnt = ST.orc_reduce(n_seq, arcs, (seq >> 31).astype(np.uint8), fuzz)  # asg.c:187-191: the reference's call goes on with asg_symm when it reduced something
    if n_red:
        assert ctx.symm() == (cnt["n_multi"], cnt["n_asymm"]), what
        g = ctx.asg_download()
    assert (cnt["n_red"], cnt["n_inner"]) == (n_red, n_inner)
    assert g[0].tobytes() == tr.tobytes() and g[2].tobytes() == tr_idx.tobytes(), "%s: graph after asg_symm differs from the oracle's" % what
    if R.have_ref():
        from test_host_vs_ref import libc
        LR = R.ref()
        gr = ma.Asg()
        for field, arr in (("arc", arcs), ("seq", seq), ("idx", idx)):
            p = libc.malloc(max(arr.nbytes, 16))
            C.memmove(p, arr.ctypes.data, arr.nbytes)
            setattr(gr, field, p)
        gr.m_arc, gr.n_arc_srt, gr.m_seq, gr.n_seq_symm = max(len(arcs), 1), len(arcs) | 1 << 31, n_seq, n_seq
        assert LR.asg_arc_del_trans(C.byref(gr), fuzz) == n_red, what
        r = R.asg_arrays(C.pointer(gr))
        assert g[0].tobytes() == r[0].tobytes() and g[1].tobytes() == r[1].tobytes() and g[2].tobytes() == r[2].tobytes(), "%s: graph differs from the reference library's" % what
        for p in (gr.arc, gr.seq, gr.idx):
            libc.free(C.c_void_p(p))
    return marked, n_red, n_inner


HUB_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1300)


@pytest.mark.parametrize("n", HUB_SIZES)
def test_reduction_of_vertices_on_every_tier_edge(n, gpu_ctx):
    """a vertex of exactly n arcs alive, on a deleted read and with a tenth of its targets twice: 1 .. 128 the pipelined tier, 129 .. 512 the wave tier,
    more the block tier (which must run from 513 on and not before)"""
    n_seq, rows, deleted = ST.hub_graph(n)
    arcs, seq, idx = ST.graph_from_rows(n_seq, rows, deleted)
    cnt = (idx & np.uint64(0xffffffff)).astype(np.int64)
    assert cnt[0] == cnt[2] == cnt[4] == n and seq[1] >> 31 and not seq[0] >> 31 and not seq[2] >> 31
    hub2 = arcs["v"][int(idx[4] >> np.uint64(32)):][:n]
    assert n < 10 or len(set(hub2.tolist())) == n - n // 10, "multi-arcs to one target"
    for fuzz in (1000, 0):
        marked, n_red, _ = check_trans(gpu_ctx, n_seq, arcs, seq, idx, fuzz, "hub of %d arcs, fuzz %d" % (n, fuzz), big=n > 512)
        assert n_red >= n, "the deleted read's arcs all go"
        if n >= 63 and fuzz:
            st = int(idx[4] >> np.uint64(32))
            d = marked["oldel"][st:st + n] >> 31
            tgt = marked["v"][st:st + n]
            first = np.array([t not in set(tgt[:i].tolist()) for i, t in enumerate(tgt)])
            assert d[first].sum() > 0 and d[~first].sum() == 0, "of several arcs to one reduced target only the first is deleted"


@pytest.mark.parametrize("fuzz", [0, 1000])
def test_reduction_when_the_neighbours_lists_sit_on_the_edges(fuzz, gpu_ctx):
    n_seq, rows, deleted = ST.trans_gadget_graph(fuzz)
    arcs, seq, idx = ST.graph_from_rows(n_seq, rows, deleted)
    P = ST.trans_profile(arcs, idx, seq, fuzz)
    # presence, from the input graph: the first neighbour's list (length, prefix inside L) around entries 64 and 128 ...
    assert {(63, 63), (64, 64), (65, 64), (65, 65), (127, 65), (127, 127), (128, 128), (129, 127), (129, 129), (300, 63), (300, 128), (300, 129), (300, 200)} <= P["first"], sorted(P["first"])
    # ... later candidates' lists around entry 16 and one behind 64 ...
    assert {(15, 14), (15, 15), (16, 15), (16, 16), (17, 15), (17, 16), (17, 17), (40, 16), (40, 17), (40, 40), (80, 65), (80, 70)} <= P["later"], sorted(P["later"])
    # ... candidates in lane 63 and in the second row's first lane, two batches of candidates, a candidate marked by its own batch, lx + li == L, both row counts
    assert {63, 64} <= P["cand_at"] and P["pending"] >= 6 and P["skipped_in_batch"] >= 10 and P["exact"] >= 20 and P["rows1"] > 0 and P["rows2"] > 0
    assert {1, 2, 63, 64, 65, 127, 128, 129} <= P["nv"]
    check_trans(gpu_ctx, n_seq, arcs, seq, idx, fuzz, "gadgets, fuzz %d" % fuzz)


def test_reduction_with_few_active_vertices_in_a_chunk(gpu_ctx):
    """the four-stage pipeline of the first tier starts and drains: chunks of 64 vertices with 1, 2, 3, 4 and 9 vertices that have arcs"""
    n_seq, rows = ST.chunk_graph()
    arcs, seq, idx = ST.graph_from_rows(n_seq, rows)
    act = ((idx & np.uint64(0xffffffff)) > 0).reshape(-1, 64)
    assert tuple(act.sum(axis=1)) == ST.CHUNK_FILL and act[0, 63] and act[-1, 63] and len(idx) == 64 * len(ST.CHUNK_FILL)
    _, n_red, _ = check_trans(gpu_ctx, n_seq, arcs, seq, idx, 1000, "chunks")
    assert n_red > 0


@pytest.mark.parametrize("which", ["gadgets", "hub513"])
def test_reduction_over_vertex_ranges_cut_at_odd_borders(which, gpu_ctx):
    """mahip_asg_del_trans_range (the sharded mode's call) piece by piece: borders that are no multiple of 64, pieces of 1, 63, 64 and 65 vertices"""
    L = ST.graph_api()
    fuzz = 1000
    if which == "gadgets":
        n_seq, rows, deleted = ST.trans_gadget_graph(fuzz)
    else:
        n_seq, rows, deleted = ST.hub_graph(513)
    arcs, seq, idx = ST.graph_from_rows(n_seq, rows, deleted)
    V = 2 * n_seq
    cuts = [0, 1, 64, 129, 192, 257, 321, 640, 641, 704, 769, 833, 1000, V - 1, V]
    cuts = [c for c in cuts if c <= V]
    assert {1, 63, 64, 65} <= {b - a for a, b in zip(cuts, cuts[1:])} and any(c % 64 for c in cuts)
    whole, n_red, n_inner = ST.orc_trans_only(n_seq, arcs, idx, seq, fuzz)
    ST.asg_upload(gpu_ctx, arcs, seq, idx)
    red_sum = inner_sum = 0
    for a, b in zip(cuts, cuts[1:]):
        _, o_red, o_inner = ST.orc_trans_only(n_seq, arcs, idx, seq, fuzz, a, b)
        got = C.c_uint32(0)
        ma._chk(L.mahip_asg_del_trans_range(gpu_ctx.h, fuzz, a, b, C.byref(got)), "del_trans_range")
        assert (got.value, ST.trans_inner(gpu_ctx)) == (o_red, o_inner), "vertices [%d, %d): %r vs the oracle's %r" % (a, b, (got.value, ST.trans_inner(gpu_ctx)), (o_red, o_inner))
        red_sum += got.value
        inner_sum += ST.trans_inner(gpu_ctx)
    assert (red_sum, inner_sum) == (n_red, n_inner)
    assert gpu_ctx.asg_download()[0].tobytes() == whole.tobytes(), "del bits after the pieces differ from one whole run's"
    ST.asg_upload(gpu_ctx, arcs, seq, idx)
    got = C.c_uint32(0)
    ma._chk(L.mahip_asg_del_trans_range(gpu_ctx.h, fuzz, 0, V, C.byref(got)), "del_trans_range")
    assert got.value == n_red and gpu_ctx.asg_download()[0].tobytes() == whole.tobytes()


# ------------------------------------------------------------------------------------------------------------- C
def test_arc_count_residues():
    assert {n % 8 for n in ST.RM_SIZES} == set(range(8)) and {n % 4 for n in ST.RM_SIZES} == set(range(4))


@pytest.mark.parametrize("n", ST.RM_SIZES)
def test_arc_rm_on_every_count_edge_both_forms(n, gpu_ctx):
    L = ST.graph_api()
    O = R.orc()
    for pat in ST.RM_PATTERNS:
        keep = ST.rm_pattern(n, pat)
        assert len(keep) == n
        # CHAINED form (k_arc_rm_chain): the first cleanup of an uploaded graph -- mahip_asg_upload clears the context's arcs_clean flag; arcs go by their own
        # bit, by a deleted target and by a deleted source read
        n_seq, arcs, seq, idx = ST.rm_graph(keep, chained=True)
        want, want_idx = ST.orc_rm_index(n_seq, arcs, seq)
        assert len(want) == keep.sum(), (n, pat)
        ST.asg_upload(gpu_ctx, arcs, seq, idx)
        m = C.c_uint32(0)
        ma._chk(L.mahip_asg_cleanup(gpu_ctx.h, C.byref(m)), "asg_cleanup")
        g = gpu_ctx.asg_download()
        assert m.value == len(want) and g[0].tobytes() == want.tobytes(), "chained form, %d arcs, %s: arcs differ" % (n, pat)
        assert g[2].tobytes() == (want_idx if len(want) != n else idx).tobytes(), "chained form, %d arcs, %s: index differs" % (n, pat)
        # CLEAN form (k_arc_rm_count / _write): a first cleanup (which removes nothing here) sets arcs_clean; asg_arc_del_asymm then marks the arcs
        # without a mirror and the cleanup behind it looks at the arcs' bits alone.  With nothing marked that cleanup is asked for directly.
        n_seq, arcs, seq, idx = ST.rm_graph(keep, chained=False)
        marked = arcs.copy()
        n_asymm = O.orc_arc_del_asymm(n_seq, n, marked.ctypes.data, idx.ctypes.data)
        assert n_asymm == n - keep.sum() and ((marked["oldel"] >> 31) == ~keep).all(), (n, pat)
        want, want_idx = ST.orc_rm_index(n_seq, marked, seq)
        ST.asg_upload(gpu_ctx, arcs, seq, idx)
        ma._chk(L.mahip_asg_cleanup(gpu_ctx.h, C.byref(m)), "asg_cleanup")
        assert m.value == n
        got = C.c_uint32(0)
        ma._chk(L.mahip_asg_del_asymm(gpu_ctx.h, C.byref(got)), "asg_del_asymm")
        assert got.value == n_asymm, (n, pat)
        if n_asymm == 0:
            ma._chk(L.mahip_asg_cleanup(gpu_ctx.h, C.byref(m)), "asg_cleanup")
            assert m.value == n
        g = gpu_ctx.asg_download()
        assert len(g[0]) == len(want) and g[0].tobytes() == want.tobytes(), "clean form, %d arcs, %s: arcs differ" % (n, pat)
        assert g[2].tobytes() == want_idx.tobytes(), "clean form, %d arcs, %s: index differs" % (n, pat)
