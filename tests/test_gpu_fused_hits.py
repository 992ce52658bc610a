"""GPU: the FUSED hit passes the resident pipeline runs (host/pipeline.c, fused branch: graph output, -S >= 5, neither -1 nor -2), stage by
stage.  mahip_hits_cutflt_sub runs the first ma_hit_cut + ma_hit_flt inside the second coverage pass; mahip_hits_cut_contained runs the second
cut with the flag pass of ma_hit_contained and leaves the squeeze of the hits to the next reader.  Every stage is compared with the C oracle
(tie mode 0, order included; the coverage estimate bit for bit), on the stage-parity inputs, on garbage hit arrays and on reads whose hit
counts sit on every size edge of the coverage kernel (register classes, tier B, tier B's global scratch) under every form of the first pass
(no gather, gather from keys, gather from runs).  The unmodified reference library checks the oracle on the same arrays."""
import os

import numpy as np
import pytest

import miniasm_amd as ma
import refapi as R
import stages as ST

pytestmark = pytest.mark.gpu


def check_fused_vs_oracle(ctx, h, n_seq, opt, what, orc=None, stride=None):
    orc = orc or ST.orc_stages(h, n_seq, opt)
    fus = ST.gpu_stages_fused(ctx, h, n_seq, opt, stride=stride)
    ST.compare(orc, fus, "oracle vs fused [%s]" % what, exact_order=True, graph=True)
    assert fus["n_cut1"] == len(orc["cut1"]) and fus["n_flt"] == len(orc["flt"]) and fus["n_cut2"] == len(orc["cut2"]), what
    return orc, fus


@pytest.mark.parametrize("name,reads,lines,seed,extra", ST.PAF_CASES, ids=[c[0] for c in ST.PAF_CASES])
def test_fused_stages_match_oracle_and_reference(name, reads, lines, seed, extra, tmpdir_s, gpu_ctx):
    paf = R.pafgen(os.path.join(tmpdir_s, "f_%s.paf" % name), reads, lines, seed, extra)
    opt = ma.default_opt()
    ing = ma.Ingest(paf, opt)
    orc, fus = check_fused_vs_oracle(gpu_ctx, ing.hits, ing.n_seq, opt, name)
    idx = np.zeros(2 * fus["n_seq_new"], dtype="<u8")
    R.orc().orc_arc_index(fus["n_seq_new"], len(fus["tr_arcs"]), fus["tr_arcs"].ctypes.data, idx.ctypes.data)
    assert idx.tobytes() == fus["tr_idx"].tobytes(), "CSR index differs"
    # the pipeline's own sequence: nothing downloaded between the fused calls, ma_sg_gen performs the deferred squeeze
    bare = ST.gpu_stages_fused(gpu_ctx, ing.hits, ing.n_seq, opt, snapshots=False)
    ST.compare(orc, bare, "oracle vs fused, no snapshots [%s]" % name, exact_order=True, graph=True)
    assert bare["tr_idx"].tobytes() == fus["tr_idx"].tobytes()
    if R.have_ref():
        ref = ST.ref_stages(paf, opt)
        auto = ST.gpu_stages_fused(gpu_ctx, ing.hits, ing.n_seq, opt, tie_mode=2)
        ST.compare(ref, auto, "reference vs fused, default tie mode [%s]" % name, exact_order=True, graph=True)
        assert ref["tr_idx"].tobytes() == auto["tr_idx"].tobytes()
        assert auto["n_cut1"] == len(ref["cut1"]) and auto["n_cut2"] == len(ref["cut2"])
        R.ref().asg_destroy(ref["g"])
    ing.close()


@pytest.mark.parametrize("block", range(4))
def test_fused_random_hit_arrays(block, gpu_ctx):
    """garbage in (start > end, bl = 0, ml > bl, self hits, 31-bit wrap in ma_sub_merge): the oracle's garbage out, and the oracle's is the reference's"""
    opt = ma.default_opt()
    for seed in range(block * 8, block * 8 + 8):
        h, n_seq = ST.random_hits(seed)
        orc, _ = check_fused_vs_oracle(gpu_ctx, h, n_seq, opt, "random hits, seed %d" % seed)
        if R.have_ref():
            ST.compare(orc, ST.ref_hit_stages(h, n_seq, opt), "oracle vs reference library, random hits seed %d" % seed, exact_order=False, graph=False)


EDGE_INPUTS = [(0, True), (3000, True), (70000, True), (3000, False)]  # (reads without hits, mirrored records)


@pytest.mark.parametrize("pad,mirrored", EDGE_INPUTS, ids=["pad%d-%s" % (p, "mirrored" if m else "grouped") for p, m in EDGE_INPUTS])
def test_group_size_edges_every_form_of_the_coverage_pass(pad, mirrored, gpu_ctx):
    """reads of exactly 0, 1, 2, 63/64/65, 127/128/129, 255/256/257, 511/512/513, 4095/4096/4097 and 9001 hits: one slot per lane or two, CLS 0 / 1 / 2,
    the register tiers / tier B, tier B in LDS / in global scratch.  Per-symbol and fused chains under run stride 0 (gather from keys), 1 and 2 (gather
    from runs where the layout has them)"""
    h, n_seq, sizes = ST.edge_hits(pad, mirrored)
    cnt = np.bincount((h["qns"] >> np.uint64(32)).astype(np.int64), minlength=n_seq)
    assert sorted(sizes.values()) == sorted(ST.EDGE_SIZES)
    assert all(cnt[r] == n for r, n in sizes.items()), [(n, int(cnt[r])) for r, n in sizes.items() if cnt[r] != n]
    runs_stride = 2 if mirrored else 1
    for min_dp in (3, 1):  # (min_dp 1: the run a read's last event closes is a candidate too, and the reads of 1 and 2 hits keep an interval)
        opt = ma.default_opt()
        opt.min_dp = min_dp
        orc = ST.orc_stages(h, n_seq, opt)
        flt_q = np.bincount((orc["flt"]["qns"] >> np.uint64(32)).astype(np.int64), minlength=n_seq)
        assert all(flt_q[r] * 3 > n for r, n in sizes.items() if n >= 63), "a real share of every larger read survives the first cut and filter"
        assert orc["n_seq_new"] > 0 and len(orc["tr_arcs"]) > 0
        if R.have_ref():
            ST.compare(orc, ST.ref_hit_stages(h, n_seq, opt), "oracle vs reference library, edges pad %d min_dp %d" % (pad, min_dp), exact_order=False, graph=False)
        for stride in (0, 1, 2):
            what = "edges pad %d %s min_dp %d stride %d" % (pad, "mirrored" if mirrored else "grouped", min_dp, stride)
            gpu = ST.gpu_stages(gpu_ctx, h, n_seq, opt, stride=stride)
            ST.compare(orc, gpu, "oracle vs per-symbol [%s]" % what, exact_order=True, graph=True)
            _, fus = check_fused_vs_oracle(gpu_ctx, h, n_seq, opt, what, orc=orc, stride=stride)
            # the runs path (gather from runs) where the layout has runs at that stride; elsewhere too few runs (mirrors under stride 1) or two interleaved runs of one read (stride 2 on grouped records)
            assert (gpu["runs"] > 0) == (fus["runs"] > 0) == (stride == runs_stride), "%s: runs %d / %d" % (what, gpu["runs"], fus["runs"])


def test_fused_custom_thresholds(gpu_ctx, tmpdir_s):
    paf = R.pafgen(os.path.join(tmpdir_s, "thr.paf"), 2000, 50000, 52, ["-L", "uniform", "-d", "0.2", "-x", "0.05", "-i", "0.1"])
    for t in ST.THRESHOLD_SETS:
        opt = ST.threshold_opt(*t)
        ing = ma.Ingest(paf, opt)
        check_fused_vs_oracle(gpu_ctx, ing.hits, ing.n_seq, opt, "thresholds %r" % (t,))
        ing.close()


@pytest.mark.parametrize("n_seq,n,where", ST.SPARSE_ID_SHAPES)
def test_fused_group_offsets_when_most_reads_have_no_hits(n_seq, n, where, gpu_ctx):
    opt = ma.default_opt()
    opt.min_dp = 1
    check_fused_vs_oracle(gpu_ctx, ST.sparse_id_hits(n_seq, n, where), n_seq, opt, "sparse ids: %d reads, %d hits, %s" % (n_seq, n, where))


def test_fused_ragged_groups_without_mirrored_hits(gpu_ctx, tmpdir_s):
    """-b style input: no record has its mirror"""
    paf = R.pafgen(os.path.join(tmpdir_s, "rag.paf"), 900, 120000, 51, ["-S", "0.9"])
    opt = ma.default_opt()
    ing = ma.Ingest(paf, opt, bi_dir=False)
    check_fused_vs_oracle(gpu_ctx, ing.hits, ing.n_seq, opt, "ragged bi_dir=False", stride=1)
    ing.close()
