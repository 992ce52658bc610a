"""Run the hit/graph passes stage by stage through (a) the unmodified reference library, (b) the C oracle,
(c) the HIP library, returning comparable snapshots after every pass."""
import ctypes as C
import os

import numpy as np

import miniasm_amd as ma
import refapi as R

HIT_DT, SUB_DT, ARC_DT = ma.HIT_DT, ma.SUB_DT, ma.ARC_DT


def flt_params(opt):
    return int(opt.max_hang * 1.5), int(opt.min_ovlp * .5)  # reference main.c:125


# --------------------------------------------------------------------------------------------- inputs
def random_hits(seed):
    """hit arrays no overlapper writes: a few very deep reads, coordinates on a coarse grid (ties everywhere, zero-length and full-length overlaps),
    start > end, self hits, ml > bl, bl = 0 -- the passes are integer arithmetic with C's wrap-around rules, so garbage in must give the oracle's
    garbage out, bit for bit"""
    rng = np.random.default_rng(seed)
    R_ = int(rng.choice([1, 3, 20, 200, 2000]))
    n = int(rng.choice([1, 2, 50, 3000, 60000]))
    mode = int(rng.integers(0, 4))
    rl = rng.integers(500, 20000, R_)
    q = rng.integers(0, R_, n) if mode != 3 else np.minimum(rng.geometric(0.05, n) - 1, R_ - 1)
    t = rng.integers(0, R_, n)
    ql, tl = rl[q], rl[t]
    if mode == 0:
        qs = (rng.random(n) * ql * 0.8).astype(np.int64); qe = qs + 1 + (rng.random(n) * (ql - qs - 1)).astype(np.int64)
        ts = (rng.random(n) * tl * 0.8).astype(np.int64); te = ts + 1 + (rng.random(n) * (tl - ts - 1)).astype(np.int64)
    elif mode == 1:
        g = 250
        qs = rng.integers(0, 8, n) * g; qe = np.minimum(qs + rng.integers(0, 40, n) * g, ql)
        ts = rng.integers(0, 8, n) * g; te = np.minimum(ts + rng.integers(0, 40, n) * g, tl)
    else:
        qs = rng.integers(0, ql + 1); qe = rng.integers(0, ql + 1)
        ts = rng.integers(0, tl + 1); te = rng.integers(0, tl + 1)
    bl = rng.integers(0, 30000, n)
    ml = (bl * rng.random(n) * 1.2).astype(np.int64)
    h = np.zeros(n, dtype=HIT_DT)
    h["qns"] = (q.astype(np.uint64) << np.uint64(32)) | (qs.astype(np.uint64) & np.uint64(0xffffffff))
    h["qe"] = qe.astype(np.uint32); h["tn"] = t.astype(np.uint32); h["ts"] = ts.astype(np.uint32); h["te"] = te.astype(np.uint32)
    h["mlrev"] = (ml.astype(np.uint32) & np.uint32(0x7fffffff)) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))
    h["bldel"] = bl.astype(np.uint32) & np.uint32(0x7fffffff)
    return h, R_


PAF_CASES = [  # pafgen inputs of the stage-parity tests: (name, reads, lines, seed, extra arguments)
    ("lognormal", 3000, 80000, 41, []),
    ("fixed", 2500, 70000, 42, ["-L", "fixed"]),
    ("lowid", 2000, 50000, 43, ["-i", "0.2"]),
    ("genome_order", 2000, 50000, 44, ["-g"]),
    ("noisy", 4000, 90000, 45, ["-L", "uniform", "-d", "0.35", "-x", "0.03"]),
    ("deep_groups", 400, 300000, 46, []),                 # ~1500 hits per read: second tier of the coverage kernel
    ("deep_vertices", 1500, 1200000, 47, ["-L", "fixed"]),  # ~800 arcs per vertex: second tier of the reduction kernel
]

THRESHOLD_SETS = ((2, .05, 1500, 500, .7, 500), (5, .1, 2500, 2000, .9, 0), (3, .2, 2000, 1000, .8, 3000))  # (min_dp, min_iden, min_span, max_hang, int_frac, gap_fuzz)


def threshold_opt(dp, iden, span, hang, frac, fuzz):
    opt = ma.default_opt()
    opt.min_dp, opt.min_iden, opt.min_span, opt.max_hang, opt.int_frac, opt.gap_fuzz = dp, iden, span, hang, frac, fuzz
    opt.min_ovlp = span
    return opt


SPARSE_ID_SHAPES = [(2048, 1, "last"), (2049, 100, "first"), (6000, 300, "middle"), (6000, 5000, "ends"), (70000, 20000, "sparse"), (70000, 3, "last")]


def sparse_id_hits(n_seq, n, where):
    """hits of a few reads among many that have none (run with min_dp = 1): ids in use only at one end, in one tile of 2048 ids of several, or thinly spread"""
    rng = np.random.default_rng(n_seq + n)
    if where == "last":
        q = np.full(n, n_seq - 1)
    elif where == "first":
        q = np.zeros(n, dtype=np.int64)
    elif where == "middle":
        q = rng.integers(2500, 2600, n)
    elif where == "ends":
        q = np.where(rng.integers(0, 2, n) == 0, rng.integers(0, 3, n), n_seq - 1 - rng.integers(0, 3, n))
    else:
        q = rng.choice(n_seq, 40, replace=False)[rng.integers(0, 40, n)]
    t = rng.integers(0, n_seq, n)
    qs = rng.integers(0, 5000, n); qe = qs + rng.integers(1, 5000, n)
    ts = rng.integers(0, 5000, n); te = ts + rng.integers(1, 5000, n)
    bl = rng.integers(1, 6000, n)
    h = np.zeros(n, dtype=HIT_DT)
    h["qns"] = (q.astype(np.uint64) << np.uint64(32)) | qs.astype(np.uint64)
    h["qe"] = qe.astype(np.uint32); h["tn"] = t.astype(np.uint32); h["ts"] = ts.astype(np.uint32); h["te"] = te.astype(np.uint32)
    h["mlrev"] = (bl * 9 // 10).astype(np.uint32); h["bldel"] = bl.astype(np.uint32)
    return h


EDGE_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 9001)  # hits per read around every size edge of the coverage kernel


def edge_hits(pad, mirrored=True, seed=0):
    """reads with exactly EDGE_SIZES hits (and "partner" reads they overlap), placed at random among `pad` reads without hits.
    Every read is 10 kb long; coordinates lie on a 500 bp grid, so equal events and runs of equal length are common.  A hit is a
    dovetail or containment at offset d (a grid step) between the read and a partner, both strands; some hits are shortened
    (internal: dropped by the filter), some have a low identity (no coverage event), a few are self hits.  Every other read
    leaves out the hits that cross its middle: two windows of (nearly always) equal length -- the "first longest run" rule
    decides.  mirrored: every record is followed by its mirror (ma_hit_read's layout, run stride 2), else the records of one
    read stand together (run stride 1).  -> (hits, n_seq, {read id: intended group size})"""
    rng = np.random.default_rng(1000 + seed)
    L, g, n_part = 10000, 500, 160
    n_used = len(EDGE_SIZES) + n_part
    ids = np.sort(rng.choice(n_used + pad, n_used, replace=False)) if pad else np.arange(n_used)
    ids = rng.permutation(ids)
    edge, part = ids[:len(EDGE_SIZES)], ids[len(EDGE_SIZES):]
    lines = []  # (q, t, d, rev, kind)

    def add(q, tgts, n, gap, self_hits):
        if gap:  # both windows: the span of q [max(0, d), min(L, d + L)) stays clear of [4500, 5500)
            dd = np.concatenate([np.arange(-7000, -5499, g), np.arange(5500, 7001, g)])
        else:
            dd = np.concatenate([np.arange(-7500, 0, g), np.arange(g, 7501, g)])  # (d = 0: two copies of one read, each contains the other)
        t = tgts[rng.integers(0, len(tgts), n)]
        d = rng.choice(dd, n)
        rev = rng.integers(0, 2, n)
        kind = rng.choice(4, n, p=[.8, .12, .05, .03] if self_hits else [.82, .13, .05, 0])  # 0 clean, 1 shortened, 2 low identity, 3 self hit (partners only: its mirror is the read's too)
        kind[1:][(kind[1:] == 3) & (kind[:-1] == 3)] = 0  # (two self hits in a row leave two interleaved runs of one read: the sort would not take runs)
        for k in range(n):
            lines.append((q, q if kind[k] == 3 else int(t[k]), int(d[k]), int(rev[k]), int(kind[k])))

    for k, (q, n) in enumerate(zip(edge, EDGE_SIZES)):
        add(int(q), part, n, k % 2 == 1, False)
    for q in part:  # the partners' own coverage: overlaps among themselves
        add(int(q), part[part != q], 24, False, True)
    m = len(lines)
    q = np.array([x[0] for x in lines], dtype=np.int64); t = np.array([x[1] for x in lines], dtype=np.int64)
    d = np.array([x[2] for x in lines], dtype=np.int64); rev = np.array([x[3] for x in lines], dtype=np.int64)
    kind = np.array([x[4] for x in lines], dtype=np.int64)
    qs, qe = np.maximum(0, d), np.minimum(L, d + L)
    ts, te = np.maximum(0, -d), np.minimum(L, L - d)
    sh = np.where(kind == 1, np.minimum(rng.integers(4, 9, m) * g, qe - qs), 0)  # shortened at one end on both reads: an overhang on each side
    left = rng.integers(0, 2, m).astype(bool)
    qs, ts = np.where(left, qs + sh, qs), np.where(left, ts + sh, ts)
    qe, te = np.where(left, qe, qe - sh), np.where(left, te, te - sh)
    ts, te = np.where(rev == 1, L - te, ts), np.where(rev == 1, L - ts, te)  # the target's coordinates on the other strand
    bl = (qe - qs) + rng.integers(0, 3, m) * g
    ml = np.where(kind == 2, bl // 50, (bl * rng.integers(3, 9, m)) // 10)
    rec = np.zeros(m, dtype=HIT_DT)
    rec["qns"] = (q.astype(np.uint64) << np.uint64(32)) | qs.astype(np.uint64)
    rec["qe"], rec["tn"], rec["ts"], rec["te"] = qe, t, ts, te
    rec["mlrev"] = ml.astype(np.uint32) | (rev.astype(np.uint32) << np.uint32(31))
    rec["bldel"] = bl.astype(np.uint32)
    if mirrored:  # hit.c:87-98: the mirror of a line right behind it, query and target swapped (a self hit has none)
        mir = rec.copy()
        mir["qns"] = (t.astype(np.uint64) << np.uint64(32)) | ts.astype(np.uint64)
        mir["qe"], mir["tn"], mir["ts"], mir["te"] = te, q, qs, qe
        out = np.empty((m, 2), dtype=HIT_DT)
        out[:, 0], out[:, 1] = rec, mir
        rec = out.reshape(-1)[np.repeat(q != t, 2) | (np.arange(2 * m) % 2 == 0)]
    sizes = {int(r): n for r, n in zip(edge, EDGE_SIZES)}
    return rec, n_used + pad, sizes


# --------------------------------------------------------------------------------------------- reference
def ref_stages(paf, opt, upto="trans"):
    L = R.ref()
    d = L.sd_init()
    n = C.c_size_t(0)
    p = L.ma_hit_read(paf.encode(), opt.min_span, opt.min_match, d, C.byref(n), 1, None)
    S = {"n_seq": d.contents.n_seq}
    n = n.value
    def snap(m):
        a = R.np_from(p, m, HIT_DT)
        a["bldel"] &= 0x7FFFFFFF  # the reference never initialises ma_hit_t.del (hit.c:87-91): heap garbage, unused everywhere
        return a
    S["sorted"] = snap(n)
    sub = L.ma_hit_sub(opt.min_dp, opt.min_iden, 0, n, p, S["n_seq"])
    S["sub1"] = R.np_from(sub, S["n_seq"], SUB_DT)
    n = L.ma_hit_cut(sub, opt.min_span, n, p)
    S["cut1"] = snap(n)
    cov = C.c_float(0)
    mh, mo = flt_params(opt)
    n = L.ma_hit_flt(sub, mh, mo, n, p, C.byref(cov))
    S["flt"], S["cov"] = snap(n), cov.value
    sub2 = L.ma_hit_sub(opt.min_dp, opt.min_iden, opt.min_span // 2, n, p, S["n_seq"])
    S["sub2"] = R.np_from(sub2, S["n_seq"], SUB_DT)
    n = L.ma_hit_cut(sub2, opt.min_span, n, p)
    S["cut2"] = snap(n)
    L.ma_sub_merge(S["n_seq"], sub, sub2)
    S["subm"] = R.np_from(sub, S["n_seq"], SUB_DT)
    L.free_buf(sub2)
    n = L.ma_hit_contained(C.byref(opt), d, sub, n, p)
    S["n_seq_new"] = d.contents.n_seq
    S["cont"] = snap(n)
    S["cont_sub"] = R.np_from(sub, S["n_seq_new"], SUB_DT)
    S["names"] = [d.contents.seq[i].name.decode() for i in range(S["n_seq_new"])]
    if upto != "hits":
        g = L.ma_sg_gen(C.byref(opt), d, sub, n, p)
        S["sg_arcs"], S["sg_seq"], S["sg_idx"] = R.asg_arrays(g)
        S["n_red"] = L.asg_arc_del_trans(g, opt.gap_fuzz)
        S["tr_arcs"], S["tr_seq"], S["tr_idx"] = R.asg_arrays(g)
        S["g"] = g  # caller may keep cleaning; caller frees with asg_destroy
    L.free_buf(sub)
    L.free_buf(p)
    L.sd_destroy(d)
    return S


# --------------------------------------------------------------------------------------------- oracle
def _ptr(a):
    return a.ctypes.data


def orc_reduce(n_seq, arcs, seq_del, fuzz):
    """asg_arc_del_trans + cleanup + symm exactly as reference asg.c:148-193 strings them together"""
    O = R.orc()
    arcs = arcs.copy()
    idx = np.zeros(2 * n_seq, dtype="<u8")
    O.orc_arc_index(n_seq, len(arcs), _ptr(arcs), _ptr(idx))
    inner = C.c_uint64(0)
    n_red = O.orc_arc_del_trans(n_seq, len(arcs), _ptr(arcs), _ptr(idx), _ptr(seq_del), fuzz, C.byref(inner))
    n_multi = n_asymm = 0
    if n_red:
        m = O.orc_arc_rm(len(arcs), _ptr(arcs), _ptr(seq_del)); arcs = arcs[:m].copy()
        O.orc_arc_index(n_seq, len(arcs), _ptr(arcs), _ptr(idx))
        n_multi = O.orc_arc_del_multi(n_seq, len(arcs), _ptr(arcs), _ptr(idx))
        if n_multi:
            m = O.orc_arc_rm(len(arcs), _ptr(arcs), _ptr(seq_del)); arcs = arcs[:m].copy()
            O.orc_arc_index(n_seq, len(arcs), _ptr(arcs), _ptr(idx))
        n_asymm = O.orc_arc_del_asymm(n_seq, len(arcs), _ptr(arcs), _ptr(idx))
        if n_asymm:
            m = O.orc_arc_rm(len(arcs), _ptr(arcs), _ptr(seq_del)); arcs = arcs[:m].copy()
            O.orc_arc_index(n_seq, len(arcs), _ptr(arcs), _ptr(idx))
    return arcs, idx, dict(n_red=n_red, n_multi=n_multi, n_asymm=n_asymm, n_inner=inner.value)


def orc_stages(hits, n_seq, opt, upto="trans"):
    O = R.orc()
    a = np.ascontiguousarray(hits, dtype=HIT_DT).copy()
    S = {"n_seq": n_seq}
    O.orc_hit_sort(len(a), _ptr(a))
    S["sorted"] = a.copy()
    sub = np.zeros(n_seq, dtype=SUB_DT)
    S["n_rem1"] = O.orc_hit_sub(opt.min_dp, opt.min_iden, 0, len(a), _ptr(a), n_seq, _ptr(sub))
    S["sub1"] = sub.copy()
    n = O.orc_hit_cut(_ptr(sub), opt.min_span, len(a), _ptr(a)); a = a[:n].copy()
    S["cut1"] = a.copy()
    cov = C.c_float(0)
    mh, mo = flt_params(opt)
    n = O.orc_hit_flt(_ptr(sub), mh, mo, len(a), _ptr(a), C.byref(cov)); a = a[:n].copy()
    S["flt"], S["cov"] = a.copy(), cov.value
    sub2 = np.zeros(n_seq, dtype=SUB_DT)
    S["n_rem2"] = O.orc_hit_sub(opt.min_dp, opt.min_iden, opt.min_span // 2, len(a), _ptr(a), n_seq, _ptr(sub2))
    S["sub2"] = sub2.copy()
    n = O.orc_hit_cut(_ptr(sub2), opt.min_span, len(a), _ptr(a)); a = a[:n].copy()
    S["cut2"] = a.copy()
    O.orc_sub_merge(n_seq, _ptr(sub), _ptr(sub2))
    S["subm"] = sub.copy()
    seq_del = np.zeros(max(n_seq, 1), dtype=np.uint8)
    mp = np.zeros(max(n_seq, 1), dtype=np.int32)
    nn = C.c_uint32(0)
    n = O.orc_hit_contained(C.byref(opt), n_seq, _ptr(seq_del), _ptr(sub), len(a), _ptr(a), _ptr(mp), C.byref(nn)); a = a[:n].copy()
    S["n_seq_new"], S["cont"], S["cont_sub"], S["map"] = nn.value, a.copy(), sub[:nn.value].copy(), mp[:n_seq].copy()
    if upto != "hits":
        ns = nn.value
        arcs = np.zeros(max(len(a), 1), dtype=ARC_DT)
        slen = np.zeros(max(ns, 1), dtype="<u4")
        sdel = np.zeros(max(ns, 1), dtype=np.uint8)
        m = O.orc_sg_gen(C.byref(opt), ns, _ptr(S["cont_sub"]) if ns else None, None, None, len(a), _ptr(a), _ptr(arcs), _ptr(slen), _ptr(sdel))
        arcs = arcs[:m].copy()
        S["sg_arcs"], S["sg_seq"] = arcs.copy(), (slen[:ns] | (sdel[:ns].astype("<u4") << 31))
        tr, idx, cnt = orc_reduce(ns, arcs, sdel, opt.gap_fuzz)
        S["tr_arcs"], S["tr_idx"], S["tr_cnt"] = tr, idx, cnt
        S["n_red"] = cnt["n_red"]
    return S


# --------------------------------------------------------------------------------------------- HIP
def run_stride(stride=None):
    # the sort may take RUNS of records as its elements when told how a query's own records stand in the array (mahip_set_run_stride); the hint may be wrong for
    # the data (random hit arrays of the parity tests are not mirrored): the result must not depend on it.  MA_TEST_RUN_STRIDE=0|1|2 (default 2: ma_hit_read's layout)
    return int(os.environ.get("MA_TEST_RUN_STRIDE", "2")) if stride is None else stride


def gpu_stages(ctx, hits, n_seq, opt, upto="trans", tie_mode=0, stride=None):
    """tie_mode 0: the stable total order (what the oracle computes); 2: the default -- the reference's order of equal keys.
    The per-symbol entry points, each pass on its own; the sorted hits are downloaded first, so the first coverage pass finds the columns written"""
    S = {"n_seq": n_seq}
    ctx.set_exact_ties(tie_mode)
    ctx.hits_upload(hits, n_seq)
    ctx.set_run_stride(run_stride(stride))
    ctx.sort()
    S["runs"] = ctx.sorted_runs()
    S["sorted"] = ctx.hits_download()
    S["n_rem1"] = ctx.sub(opt.min_dp, opt.min_iden, 0, 0)
    S["sub1"] = ctx.sub_download(0, n_seq)
    ctx.cut(0, opt.min_span)
    S["cut1"] = ctx.hits_download()
    mh, mo = flt_params(opt)
    _, S["cov"] = ctx.flt(0, mh, mo)
    S["flt"] = ctx.hits_download()
    S["n_rem2"] = ctx.sub(opt.min_dp, opt.min_iden, opt.min_span // 2, 1)
    S["sub2"] = ctx.sub_download(1, n_seq)
    ctx.cut(1, opt.min_span)
    S["cut2"] = ctx.hits_download()
    ctx.sub_merge()
    S["subm"] = ctx.sub_download(0, n_seq)
    S["n_seq_new"], _ = ctx.contained(opt)
    S["cont"] = ctx.hits_download()
    S["cont_sub"] = ctx.sub_download(0, n_seq, squeezed=True)[:S["n_seq_new"]]
    S["map"] = ctx.map_download(n_seq)
    if upto != "hits":
        ctx.sg_gen(opt, True)
        S["sg_arcs"], S["sg_seq"], S["sg_idx"] = ctx.asg_download()
        S["n_red"] = ctx.del_trans(opt.gap_fuzz)
        if S["n_red"]:
            ctx.symm()
        S["tr_arcs"], S["tr_seq"], S["tr_idx"] = ctx.asg_download()
    S["tie"] = ctx.tie_stats()
    ctx.set_exact_ties(2)
    return S


def gpu_stages_fused(ctx, hits, n_seq, opt, tie_mode=0, stride=None, snapshots=True):
    """The fused branch of ma_pipeline_head (host/pipeline.c), call for call and with the same derived arguments: sort, the first coverage pass (which
    gathers the records itself: nothing is downloaded between the sort and it), cut + filter inside the second coverage pass, merge, cut + the flag pass
    of contained with the squeeze of the hits deferred; then the graph as gpu_stages builds it.  snapshots: also download the hits after the fused
    calls ("flt"; "cont" performs the deferred squeeze) -- without them ma_sg_gen does that squeeze, as in the pipeline.  There is no "sorted",
    "cut1" or "cut2" array: the fused calls report their counts instead (n_cut1, n_flt, n_cut2)."""
    S = {"n_seq": n_seq, "fused": True}
    ctx.set_exact_ties(tie_mode)
    ctx.hits_upload(hits, n_seq)
    ctx.set_run_stride(run_stride(stride))
    ctx.sort()
    S["runs"] = ctx.sorted_runs()
    S["n_rem1"] = ctx.sub(opt.min_dp, opt.min_iden, 0, 0)
    S["sub1"] = ctx.sub_download(0, n_seq)
    mh, mo = flt_params(opt)
    S["n_cut1"], S["n_flt"], S["cov"], S["n_rem2"] = ctx.cutflt_sub(0, opt.min_span, mh, mo, opt.min_dp, opt.min_iden, opt.min_span // 2, 1)
    if snapshots:
        S["flt"] = ctx.hits_download()
    S["sub2"] = ctx.sub_download(1, n_seq)
    ctx.sub_merge()
    S["subm"] = ctx.sub_download(0, n_seq)
    S["n_cut2"], S["n_seq_new"] = ctx.cut_contained(1, opt.min_span, opt)
    if snapshots:
        S["cont"] = ctx.hits_download()
    S["cont_sub"] = ctx.sub_download(0, n_seq, squeezed=True)[:S["n_seq_new"]]
    S["map"] = ctx.map_download(n_seq)
    ctx.sg_gen(opt, True)
    S["sg_arcs"], S["sg_seq"], S["sg_idx"] = ctx.asg_download()
    S["n_red"] = ctx.del_trans(opt.gap_fuzz)
    if S["n_red"]:
        ctx.symm()
    S["tr_arcs"], S["tr_seq"], S["tr_idx"] = ctx.asg_download()
    S["tie"] = ctx.tie_stats()
    ctx.set_exact_ties(2)
    return S


# --------------------------------------------------------------------------------------------- reference on a hit array
def ref_hit_stages(hits, n_seq, opt):
    """the unmodified reference library's hit passes on an array (no PAF text): radix_sort_hit, ma_hit_sub, ma_hit_cut, ma_hit_flt, the second
    ma_hit_sub + ma_hit_cut, ma_sub_merge, ma_hit_contained with a dictionary of n_seq generated names (sd_put).  Ties are left as the reference's
    sort leaves them: compare in canonical order"""
    L = R.ref()
    L.radix_sort_hit.argtypes = [C.c_void_p, C.c_void_p]
    L.radix_sort_hit.restype = None
    a = np.ascontiguousarray(hits, dtype=HIT_DT)
    n = len(a)
    p = L.malloc_buf(max(n, 1) * HIT_DT.itemsize)
    C.memmove(p, a.ctypes.data, n * HIT_DT.itemsize)
    d = L.sd_init()
    for i in range(n_seq):
        L.sd_put(d, b"r%d" % i, 10000)
    S = {"n_seq": n_seq}
    L.radix_sort_hit(p, p + n * HIT_DT.itemsize)
    S["sorted"] = R.np_from(p, n, HIT_DT)
    sub = L.ma_hit_sub(opt.min_dp, opt.min_iden, 0, n, p, n_seq)
    S["sub1"] = R.np_from(sub, n_seq, SUB_DT)
    n = L.ma_hit_cut(sub, opt.min_span, n, p)
    S["cut1"] = R.np_from(p, n, HIT_DT)
    cov = C.c_float(0)
    mh, mo = flt_params(opt)
    n = L.ma_hit_flt(sub, mh, mo, n, p, C.byref(cov))
    S["flt"], S["cov"] = R.np_from(p, n, HIT_DT), cov.value
    sub2 = L.ma_hit_sub(opt.min_dp, opt.min_iden, opt.min_span // 2, n, p, n_seq)
    S["sub2"] = R.np_from(sub2, n_seq, SUB_DT)
    n = L.ma_hit_cut(sub2, opt.min_span, n, p)
    S["cut2"] = R.np_from(p, n, HIT_DT)
    L.ma_sub_merge(n_seq, sub, sub2)
    S["subm"] = R.np_from(sub, n_seq, SUB_DT)
    L.free_buf(sub2)
    n = L.ma_hit_contained(C.byref(opt), d, sub, n, p)
    S["n_seq_new"] = d.contents.n_seq
    S["cont"] = R.np_from(p, n, HIT_DT)
    S["cont_sub"] = R.np_from(sub, S["n_seq_new"], SUB_DT)
    L.free_buf(sub)
    L.free_buf(p)
    L.sd_destroy(d)
    return S


HIT_KEYS = ["sorted", "cut1", "flt", "cut2", "cont"]
SUB_KEYS = ["sub1", "sub2", "subm", "cont_sub"]
FUSED_ABSENT = {"sorted": None, "cut1": "n_cut1", "cut2": "n_cut2"}  # arrays the fused chain never materialises -> the count it reports instead


def same_f32(a, b):
    """bit for bit as a float32; two NaNs are equal (both sides divide two integer sums once: hit.c:212)"""
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def compare(A, B, what, exact_order=False, graph=True):
    """assert two stage dicts agree; hit arrays are compared in canonical order unless exact_order"""
    assert A["n_seq"] == B["n_seq"], what
    for k in HIT_KEYS:
        if k not in A or k not in B:  # only a fused chain may lack an array, and only one it never builds (or a snapshot it was told to skip)
            for X, Y in ((A, B), (B, A)):
                if k not in X:
                    assert X.get("fused") and (k in FUSED_ABSENT or k in ("flt", "cont")), "%s: %s missing" % (what, k)
                    cnt = FUSED_ABSENT.get(k)
                    if cnt and k in Y:
                        assert X[cnt] == len(Y[k]), "%s: %s %d vs %d records in %s" % (what, cnt, X[cnt], len(Y[k]), k)
            continue
        a, b = A[k], B[k]
        assert len(a) == len(b), "%s: %s count %d vs %d" % (what, k, len(a), len(b))
        if not exact_order:
            a, b = R.canon(a), R.canon(b)
        if a.tobytes() != b.tobytes():
            diff = {f: int((a[f] != b[f]).sum()) for f in a.dtype.names}
            raise AssertionError("%s: %s records differ: per-field mismatches %r" % (what, k, diff))
    for k in SUB_KEYS:
        assert A[k].tobytes() == B[k].tobytes(), "%s: %s differs" % (what, k)
    assert A["n_seq_new"] == B["n_seq_new"], what
    assert same_f32(A["cov"], B["cov"]), "%s: cov %r vs %r" % (what, A["cov"], B["cov"])
    for k in ("n_rem1", "n_rem2", "n_cut1", "n_flt", "n_cut2"):
        if k in A and k in B:
            assert A[k] == B[k], "%s: %s %d vs %d" % (what, k, A[k], B[k])
    for X, Y in ((A, B), (B, A)):
        if "n_flt" in X and "flt" in Y:
            assert X["n_flt"] == len(Y["flt"]), "%s: n_flt %d vs %d records in flt" % (what, X["n_flt"], len(Y["flt"]))
    if "map" in A and "map" in B:
        assert A["map"].tobytes() == B["map"].tobytes(), "%s: map differs" % what
    if graph and "sg_arcs" in A and "sg_arcs" in B:
        for k in ("sg_arcs", "tr_arcs"):
            a, b = A[k], B[k]
            assert len(a) == len(b), "%s: %s count %d vs %d" % (what, k, len(a), len(b))
            if not exact_order:
                a, b = R.canon(a), R.canon(b)
            assert a.tobytes() == b.tobytes(), "%s: %s differ" % (what, k)
        assert A["sg_seq"].tobytes() == B["sg_seq"].tobytes(), "%s: seq differ" % what
        assert A["n_red"] == B["n_red"], what
