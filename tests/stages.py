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
        S["n_inner"] = trans_inner(ctx)
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
    S["n_inner"] = trans_inner(ctx)
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
        for X, Y in ((A, B), (B, A)):  # the oracle's count of asg.c:169's loop bodies against mahip_asg_trans_inner (the reference library keeps no such count)
            if "tr_cnt" in X and "n_inner" in Y:
                assert X["tr_cnt"]["n_inner"] == Y["n_inner"], "%s: inner iterations of the reduction %d vs %d" % (what, X["tr_cnt"]["n_inner"], Y["n_inner"])


# --------------------------------------------------------------------------------------------- graph size edges (tests/test_gpu_graph_edges.py)
def graph_api():
    """the C ABI entry points of the graph passes the thin harness does not wrap"""
    L = ma.lib()
    vp, u32 = C.c_void_p, C.c_uint32
    L.mahip_asg_trans_inner.restype = C.c_uint64
    L.mahip_asg_trans_inner.argtypes = [vp]
    L.mahip_asg_del_trans_range.argtypes = [vp, C.c_int, u32, u32, C.POINTER(u32)]
    L.mahip_asg_cleanup.argtypes = [vp, C.POINTER(u32)]
    L.mahip_asg_del_asymm.argtypes = [vp, C.POINTER(u32)]
    return L


def trans_inner(ctx):
    return int(graph_api().mahip_asg_trans_inner(ctx.h))


def asg_upload(ctx, arcs, seq, idx):
    """a hand-made graph (arcs sorted by (u, len), seq = len | del << 31, CSR index) onto the device: mahip_asg_upload"""
    arcs, seq, idx = np.ascontiguousarray(arcs, dtype=ARC_DT), np.ascontiguousarray(seq, dtype="<u4"), np.ascontiguousarray(idx, dtype="<u8")
    g = ma.Asg()
    g.arc, g.seq, g.idx = arcs.ctypes.data, seq.ctypes.data, idx.ctypes.data
    g.m_arc, g.n_arc_srt, g.m_seq, g.n_seq_symm = max(len(arcs), 1), len(arcs) | 1 << 31, max(len(seq), 1), len(seq)
    ma._chk(ma.lib().mahip_asg_upload(ctx.h, C.byref(g)), "asg_upload")
    ma._chk(ma.lib().mahip_sync(ctx.h), "sync")  # (the copies are asynchronous: the arrays must outlive them)


def graph_from_rows(n_seq, rows, deleted=(), seq_len=9000):
    """rows of (u, v, len, ol) -> (arcs stably sorted by (u, len), seq words, index by orc_arc_index)"""
    r = np.asarray(rows, dtype=np.uint64).reshape(-1, 4)
    a = np.zeros(len(r), dtype=ARC_DT)
    a["ul"], a["v"], a["oldel"] = r[:, 0] << np.uint64(32) | r[:, 2], r[:, 1], r[:, 3]
    a = a[np.argsort(a["ul"], kind="stable")]
    seq = np.full(n_seq, seq_len, dtype="<u4")
    seq[np.asarray(deleted, dtype=np.int64)] |= np.uint32(1 << 31)
    idx = np.zeros(2 * n_seq, dtype="<u8")
    R.orc().orc_arc_index(n_seq, len(a), _ptr(a), _ptr(idx))
    return a, seq, idx


def with_mirrors(rows, d_len=3):
    """every arc u -> v and its mirror v^1 -> u^1 (asg.c:104-145 expects both); the mirror is d_len longer"""
    out = []
    for (u, v, ln, ol) in rows:
        out.append((u, v, ln, ol))
        out.append((v ^ 1, u ^ 1, ln + d_len, ol))
    return out


def orc_trans_only(n_seq, arcs, idx, seq, fuzz, v_beg=0, v_end=None):
    """the marking pass alone (asg.c:148-186) on a copy -> (arcs with del bits, n_reduced, n_inner)"""
    O = R.orc()
    a = arcs.copy()
    sdel = (seq >> 31).astype(np.uint8)
    inner = C.c_uint64(0)
    n_red = O.orc_arc_del_trans_range(n_seq, len(a), _ptr(a), _ptr(idx), _ptr(sdel), fuzz, v_beg, 2 * n_seq if v_end is None else v_end, C.byref(inner))
    return a, n_red, inner.value


def orc_rm_index(n_seq, arcs, seq):
    """asg_cleanup (asg.c:72-80) on a copy: orc_arc_rm + orc_arc_index"""
    O = R.orc()
    a = arcs.copy()
    sdel = (seq >> 31).astype(np.uint8)
    m = O.orc_arc_rm(len(a), _ptr(a), _ptr(sdel))
    a = a[:m].copy()
    idx = np.zeros(2 * n_seq, dtype="<u8")
    O.orc_arc_index(n_seq, len(a), _ptr(a), _ptr(idx))
    return a, idx


ARC_EDGE_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)  # arcs per read around every size edge of the arc sort per read
ARC_EDGE_IDS = (0, 63, 64, 127, 128, 191, 300, 383, 384, 500, 640, 703, 800, -1)  # lanes 0 and 63 of 64-read chunks, > 64 arcless reads in between (192 .. 299), the dictionary's last read


def dovetail(q, t, strand, ln, jit, rl):
    """one hit between two reads of length rl that ma_hit2arc (miniasm.h:86-104) turns into the arc (q << 1 | strand) -> (t << 1 | strand) of length ln;
    jit: the overhang in front of the overlap (<= max_hang), which makes the query start distinct without touching the arc"""
    if strand == 0:
        qs, qe, ts, te = ln + jit, rl, jit, rl - ln
    else:
        qs, qe, ts, te = jit, rl - ln, ln + jit, rl
    return (q, qs, qe, t, ts, te)


def hits_from_lines(lines, bl_of=None):
    """(q, qs, qe, t, ts, te) forward-strand lines -> hit records"""
    x = np.asarray(lines, dtype=np.uint64).reshape(-1, 6)
    h = np.zeros(len(x), dtype=HIT_DT)
    h["qns"] = x[:, 0] << np.uint64(32) | x[:, 1]
    h["qe"], h["tn"], h["ts"], h["te"] = x[:, 2], x[:, 3], x[:, 4], x[:, 5]
    bl = (x[:, 2] - x[:, 1]).astype(np.uint32)
    h["bldel"], h["mlrev"] = bl, bl // np.uint32(2)
    return h


def arc_edge_hits(strands="split", few_lengths=False, n_seq=1024, extra=(), longest=0, seed=0):
    """hits in which the reads ARC_EDGE_IDS get exactly ARC_EDGE_SIZES arcs (a permutation of them chosen by the seed; `extra`: more sizes, e.g. 513, on reads of
    their own), all reads equally long so that no read contains another: every hit is a dovetail (see dovetail()) to one of 40 partner reads, which overlap among
    themselves with short arcs (so the reduction finds transitive arcs); every other read has no hit.  strands: "0" / "1" / "split" -- which of the read's two
    vertices its arcs leave.  few_lengths: arc lengths from a set of eight, so runs of equal (u, len) cross lane and register-row borders of the sort.
    longest: if set, one arc of that length (the register sort holds lengths of up to 21 bits).  The records of a read stand together, in random order.
    -> (hits, seq_len[n_seq], {read: arcs})"""
    rng = np.random.default_rng(4200 + seed)
    rl = max(longest, 20000) + 6000
    sizes = list(rng.permutation(ARC_EDGE_SIZES))
    if sizes[-1] == 0:  # the dictionary's last read must have arcs
        sizes[-1], sizes[0] = sizes[0], sizes[-1]
    ids = [i if i >= 0 else n_seq - 1 for i in ARC_EDGE_IDS] + [420 + 10 * k for k in range(len(extra))]
    sizes = [int(s) for s in sizes] + [int(s) for s in extra]
    part = np.arange(820, 860)
    assert n_seq > 900 and not set(ids) & set(part.tolist())
    lines = []
    for q, n in zip(ids, sizes):
        t = part[rng.integers(0, len(part), n)]
        st = {"0": np.zeros(n, int), "1": np.ones(n, int), "split": np.arange(n) % 2}[strands]
        ln = rng.choice(np.arange(1, 9) * 700, n) if few_lengths else rng.integers(1, 20000, n)
        if longest and n == 64:
            ln[0] = longest
        for k in rng.permutation(n):
            lines.append(dovetail(q, int(t[k]), int(st[k]), int(ln[k]), int(k), rl))
    for p in part:
        for k, t in enumerate(rng.choice(part[part != p], 4, replace=False)):
            lines.append(dovetail(int(p), int(t), k % 2, int(rng.integers(1, 600)), k, rl))
    return hits_from_lines(lines), np.full(n_seq, rl, dtype="<u4"), dict(zip(ids, sizes))


SG_WORD_FILL = (0, 1, 5, 6, 64, 3, 7, 0, 64, 6, 5, 1, 20)  # arc-yielding slots per 64-slot word of the hit array, repeated (SG_DENSE = 6: lane walk below, whole wave from there on)


def sg_emit_opt():
    opt = ma.default_opt()
    opt.max_hang, opt.int_frac, opt.min_ovlp = 1500, .5, 2000
    return opt


def sg_emit_hits(n_slots, seed=0):
    """a hit array of exactly n_slots records, sorted by (query, start), in which 64-slot word w holds SG_WORD_FILL[w % 13] hits that yield an arc; the rest are
    internal matches (no arc).  40 records per read, so reads cross word borders; run with sg_emit_opt().  A few reads carry a full-length hit (the query is
    contained: asm.c:34 deletes it, and with it the arcs that other reads have to it), one a palindromic self hit (asm.c:27-31).  -> (hits, seq_len)"""
    rng = np.random.default_rng(5200 + seed)
    rl, per = 30000, 40
    n_seq = (n_slots + per - 1) // per
    lines, rev = [], []
    killers = set(rng.choice(np.arange(3, n_seq - 1), max(n_seq // 60, 1), replace=False).tolist())
    for s in range(n_slots):
        q, k, w = s // per, s % per, s // 64
        fill = SG_WORD_FILL[w % len(SG_WORD_FILL)]
        order = np.random.default_rng(w).permutation(64)  # which slots of the word yield: fixed per word
        t = int(rng.integers(0, n_seq - 1))
        t += t >= q
        qs = 1000 + 10 * k
        r = 0
        if k == 0 and q in killers:
            ln = (q, 0, rl, t, 0, rl)  # query contained
            if q % 2:
                ln, r = (q, 500, rl - 200, q, 500, rl - 200), 1  # self hit on the other strand with an arc verdict
        elif order[s % 64] < fill:
            ln = (q, qs, rl, t, 1, 1 + rl - qs) if s % 2 == 0 else (q, qs, rl - (1 + 7 * (s % 1000)), t, 1 + 7 * (s % 1000) + qs, rl)
        else:
            ln = (q, qs, qs + 4000, t, 6000, 10000)  # ends in the middle of both reads: internal
        lines.append(ln)
        rev.append(r)
    h = hits_from_lines(lines)
    h["mlrev"] |= np.asarray(rev, dtype=np.uint32) << np.uint32(31)
    return h, np.full(n_seq, rl, dtype="<u4")


def sg_candidate_words(hits, seq_len, opt):
    """per 64-slot word of a hit array the number of slots ma_hit2arc answers with an arc between two different reads (the oracle's verdict per hit)"""
    O = R.orc()
    arc = np.zeros(1, dtype=ARC_DT)
    cand = np.zeros((len(hits) + 63) // 64 * 64, dtype=np.int64)
    for i in range(len(hits)):
        q, t = int(hits["qns"][i] >> np.uint64(32)), int(hits["tn"][i])
        r = O.orc_hit2arc(_ptr(hits[i:i + 1]), int(seq_len[q]), int(seq_len[t]), opt.max_hang, opt.int_frac, opt.min_ovlp, _ptr(arc))
        cand[i] = r >= 0 and q != t
    return cand.reshape(-1, 64).sum(axis=1)


def orc_sg(hits, seq_len, opt, presorted=False):
    """ma_sg_gen against given read lengths (no intervals) -> (arcs, seq words, index); the hits are sorted by the oracle first unless presorted"""
    O = R.orc()
    a = np.ascontiguousarray(hits, dtype=HIT_DT).copy()
    n_seq = len(seq_len)
    if not presorted:
        O.orc_hit_sort(len(a), _ptr(a))
    arcs = np.zeros(max(len(a), 1), dtype=ARC_DT)
    slen, sdel = np.zeros(n_seq, dtype="<u4"), np.zeros(n_seq, dtype=np.uint8)
    m = O.orc_sg_gen(C.byref(opt), n_seq, None, _ptr(seq_len), None, len(a), _ptr(a), _ptr(arcs), _ptr(slen), _ptr(sdel))
    arcs = arcs[:m].copy()
    idx = np.zeros(2 * n_seq, dtype="<u8")
    O.orc_arc_index(n_seq, m, _ptr(arcs), _ptr(idx))
    return arcs, slen | (sdel.astype("<u4") << 31), idx, a


def ref_sg(hits_sorted, seq_len, opt):
    """the unmodified reference library's ma_sg_gen on a hit array as it stands (asm.c:9-39, no intervals: the dictionary's lengths)"""
    L = R.ref()
    d = L.sd_init()
    for i, n in enumerate(seq_len):
        L.sd_put(d, b"r%d" % i, int(n))
    a = np.ascontiguousarray(hits_sorted, dtype=HIT_DT)
    g = L.ma_sg_gen(C.byref(opt), d, None, len(a), _ptr(a))
    out = R.asg_arrays(g)
    L.asg_destroy(g)
    L.sd_destroy(d)
    return out


def arc_tie_census(arcs):
    """(groups, arcs) of equal (u, len) keys among sorted arcs: what mahip_tie_stats reports in tie mode 2"""
    ul = arcs["ul"]
    if len(ul) < 2:
        return 0, 0
    eq = ul[1:] == ul[:-1]
    tied = np.r_[eq, False] | np.r_[False, eq]
    return int((eq & ~np.r_[False, eq[:-1]]).sum()), int(tied.sum())


# (k = arcs of the centre, (length, prefix inside L) of the first neighbour's list, [(arc index, list length, prefix inside L) of later candidates], centre on a deleted read)
TRANS_GADGETS = [
    (1, (2, 1), [], False), (2, (3, 2), [], False),
    (40, (63, 63), [(5, 15, 15), (9, 16, 16), (13, 17, 17)], False),
    (64, (64, 64), [(20, 40, 16), (24, 40, 17), (28, 80, 70), (58, 17, 15)], False),
    (64, (65, 65), [(30, 16, 15)], False),
    (100, (65, 64), [(56, 16, 15), (60, 17, 16), (63, 40, 40)], False),
    (100, (127, 127), [(64, 17, 17), (70, 80, 65)], False),
    (128, (128, 128), [(100, 15, 15), (120, 17, 17)], False),
    (128, (129, 129), [(5, 40, 40), (66, 16, 16)], False),
    (127, (300, 128), [(66, 16, 16)], False),
    (65, (300, 129), [(10, 15, 14)], False),
    (63, (300, 200), [(10, 17, 17)], False),
    (30, (300, 63), [], False), (30, (127, 65), [], False), (30, (129, 127), [], False),
    (129, (129, 64), [(3, 17, 17), (70, 80, 65)], False),  # (a centre of the wave tier behind the first one)
    (50, (64, 64), [(5, 17, 17)], True), (3, (2, 2), [], True),
]


def trans_gadget_graph(fuzz, gadgets=TRANS_GADGETS):
    """a graph made of one gadget per entry of TRANS_GADGETS.  A gadget is a centre vertex with k arcs (lengths 1000, 1010, ...; the last one 4000 longer, so
    L = longest + fuzz leaves room) whose neighbours' lists are chosen: the first neighbour's list has the given length and prefix inside L; the entry that
    ends the prefix has lx + li == L exactly and is the ONLY arc that reaches one neighbour of the centre (its "witness"), the entry behind it is the only
    arc to another witness that therefore stays marked 1; the rest of the prefix reaches the centre's other neighbours ("covered") and filler reads.  A later
    candidate stands at a chosen arc index and has a list of its own with two witnesses, which are the centre's next two arcs: the first is marked by its
    own batch of four and must be skipped, the second is expanded after it.  Arcs are mirrored.  -> (n_seq, rows)"""
    rows, n_read = [], 0
    fill0, n_fill = 0, 320
    n_read += n_fill  # filler reads: targets that are no neighbour of any centre
    for (k, (n0, p0), cands, dead) in gadgets:
        c = n_read
        nb = [n_read + 1 + i for i in range(k)]
        n_read += 1 + k
        d = [1000 + 10 * i for i in range(k)]
        d[-1] += 4000
        L = d[-1] + fuzz
        for i in range(k):
            rows.append((2 * c, 2 * nb[i], d[i], 5000))
        role = {0: (n0, p0)}
        wit = set()
        for (i, nw, p) in cands:
            assert i + 2 < k - 1 and not {i, i + 1, i + 2} & (set(role) | wit)
            role[i] = (nw, p)
            wit |= {i + 1, i + 2}
        if k > 3:
            assert not {k - 3, k - 2} & (set(role) | wit)
            wit |= {k - 3, k - 2}  # the first neighbour's witnesses
        covered = [i for i in range(1, k - 1) if i not in role and i not in wit]
        for i in range(k):
            if i in role:
                nw, p = role[i]
                w_in, w_out = (i + 1, i + 2) if i else (k - 3, k - 2)
                tg = ([2 * nb[x] for x in covered] if i == 0 else [])[:max(p - 1, 0)]
            elif i == k - 1:
                nw, p, tg, w_in, w_out = 1, 0, [], -1, -1
            else:
                nw, p, tg, w_in, w_out = 1, 1, [], -1, -1  # a witness or a covered neighbour the prefix had no room for: one arc to a filler
            if i == k - 1:
                p = min(p, fuzz)
            for j in range(nw):
                ln = L - d[i] - (p - 1 - j) if j < p else L - d[i] + 1 + (j - p)
                if j < len(tg):
                    v = tg[j]
                elif j == p - 1 and w_in > 0 and k > 3:
                    v = 2 * nb[w_in]
                elif j == p and w_out > 0 and k > 3:
                    v = 2 * nb[w_out]
                else:
                    v = 2 * (fill0 + j % n_fill)
                rows.append((2 * nb[i], v, ln, 4000))
        if dead:
            rows.append(("dead", c, 0, 0))
    deleted = [r[1] for r in rows if r[0] == "dead"]
    rows = with_mirrors([r for r in rows if r[0] != "dead"])
    return n_read, rows, deleted


def trans_profile(arcs, idx, seq, fuzz):
    """replay of asg.c:148-186 for the live vertices of 1 .. 128 arcs, as the first tier of the device walks them (candidates taken four at a time inside a
    row of 64 arcs), to say WHAT the input contains: -> dict of sets / counts the size-edge test asserts to be present"""
    P = dict(nv=set(), first=set(), later=set(), cand_at=set(), pending=0, skipped_in_batch=0, exact=0, rows1=0, rows2=0)
    ul, av = arcs["ul"], arcs["v"]
    ln_all = (ul & np.uint64(0xffffffff)).astype(np.int64)
    for v in range(len(idx)):
        st, nv = int(idx[v] >> np.uint64(32)), int(idx[v] & np.uint64(0xffffffff))
        P["nv"].add(nv)
        if nv == 0 or nv > 128 or seq[v >> 1] >> 31:
            continue
        tg, ln = av[st:st + nv].tolist(), ln_all[st:st + nv].tolist()
        L = ln[-1] + fuzz
        mark = {t: 1 for t in tg}

        def expand(i):
            ws, nw = int(idx[tg[i]] >> np.uint64(32)), int(idx[tg[i]] & np.uint64(0xffffffff))
            p = 0
            while p < nw and ln_all[ws + p] + ln[i] <= L:
                if av[ws + p] in mark:
                    mark[av[ws + p]] = 2
                p += 1
            P["exact"] += p > 0 and ln_all[ws + p - 1] + ln[i] == L
            return nw, p
        f = expand(0)
        P["first"].add(f)
        P["rows1" if nv <= 64 and f[0] <= 64 else "rows2"] += 1
        P["pending"] = max(P["pending"], sum(1 for i in range(1, nv) if mark[tg[i]] == 1))
        for base in (0, 64):
            passed = 0 if base else 1
            while True:
                cand = [i for i in range(base + passed, min(base + 64, nv)) if mark[tg[i]] == 1]
                if not cand:
                    break
                for i in cand[:4]:
                    passed = i - base + 1
                    if mark[tg[i]] != 1:
                        P["skipped_in_batch"] += 1
                        continue
                    P["later"].add(expand(i))
                    P["cand_at"].add(i)
    return P


def hub_graph(n, seed=0):
    """reads on a line, an arc u -> v of length pos[v] - pos[u] to the next 2 .. 6 reads (transitive by construction), and three hubs of exactly n arcs each:
    read 0 (alive), read 1 (flagged deleted: asg.c:158-161, all its arcs go), read 2 (alive, a tenth of its targets twice: of several arcs to one reduced
    target only the first is deleted, asg.c:181-184).  Mirrored.  -> (n_seq, rows, deleted reads)"""
    rng = np.random.default_rng(7700 + seed + n)
    n_seq = n + 60
    pos = np.sort(rng.choice(np.arange(1, 400000), n_seq, replace=False))
    rows = []
    for u in range(3, n_seq):
        for v in range(u + 1, min(n_seq, u + 1 + int(rng.integers(2, 7)))):
            rows.append((2 * u, 2 * v, int(pos[v] - pos[u]), 5000))
    for hub in (0, 1, 2):
        n_dup = n // 10 if hub == 2 else 0
        tg = rng.choice(np.arange(3, n_seq), n - n_dup, replace=False)
        for v in tg:
            rows.append((2 * hub, 2 * int(v), int(pos[v] - pos[hub]), 4000))
        for v in tg[:n_dup]:
            rows.append((2 * hub, 2 * int(v), int(pos[v] - pos[hub]) + int(rng.integers(0, 3)), 3999))
    return n_seq, with_mirrors(rows), [1]


CHUNK_FILL = (1, 2, 3, 4, 9, 1)  # vertices with arcs per chunk of 64 consecutive vertices


def chunk_graph():
    """64-vertex chunks that hold exactly CHUNK_FILL vertices with arcs: the first chunk's is its last vertex (63), the last chunk's the graph's last vertex.
    Not mirrored (a mirror would give a second vertex its arcs).  -> (n_seq, rows)"""
    rng = np.random.default_rng(7800)
    n_seq = 32 * len(CHUNK_FILL)
    act = []
    for c, n in enumerate(CHUNK_FILL):
        if c == 0:
            act += [63]
        elif c == len(CHUNK_FILL) - 1:
            act += [64 * c + 63]
        else:
            act += sorted((64 * c + rng.choice(64, n, replace=False)).tolist())
    rows = []
    for k, v in enumerate(act):
        w = [act[(k + j) % len(act)] for j in (1, 2, 3)]
        for j, t in enumerate(w):
            rows.append((v, t, 100 * (j + 1), 3000))
    return n_seq, rows


RM_SIZES = (1, 7, 2047, 2048, 2049, 2050, 2051, 8191, 8192, 8193, 8196, 32767, 32768, 32769, 32773, 32774, 65536 + 3)  # arc counts around RM_TILE = 2048 and RMC_GROUP = 32768, every residue mod 8
RM_PATTERNS = ("none", "all", "first_block", "all_but_last", "tail_deleted", "tail_survives", "random10", "random90")


def rm_pattern(n, name):
    """which of n arcs stay"""
    keep = np.ones(n, dtype=bool)
    rng = np.random.default_rng(n)
    if name == "all":
        keep[:] = False
    elif name == "first_block":  # everything in the first group of 32768 / tile of 2048 (or the first half of a graph smaller than that)
        keep[:32768 if n > 32768 else 2048 if n > 2048 else max(n // 2, 1)] = False
    elif name == "all_but_last":
        keep[:-1] = False
    elif name == "tail_deleted":  # only behind the last multiple of 4 before the end
        keep[(n - 1) // 4 * 4:] = False
    elif name == "tail_survives":  # nothing but the last tile's / group's tail: behind the last multiple of 8 before the end
        keep[:(n - 1) // 8 * 8] = False
    elif name.startswith("random"):
        keep = rng.random(n) >= int(name[6:]) / 100.
    return keep


def rm_graph(keep, chained):
    """n arcs, arc p the only arc of vertex p (so it stands at position p).
    chained = False: an arc that stays is p -> p^1, its own mirror; one that goes is p -> a read without arcs and has no mirror: asg_arc_del_asymm marks exactly those.
    chained = True: an arc that goes has its del bit set already (even p), or its target is a read flagged deleted (odd p), or -- both arcs of a read going -- now and then
    the read itself is flagged: asg_arc_rm decides by the arc's bit AND both seq.del look-ups.  -> (n_seq, arcs, seq, idx)"""
    n = len(keep)
    p = np.arange(n, dtype=np.int64)
    R_ = (n + 1) // 2
    z, dd = R_, R_ + 1
    v = np.where(keep, p ^ 1, 2 * z)
    ol = np.full(n, 3000, dtype=np.int64)
    deleted = []
    if chained:
        both = np.flatnonzero(~keep[:n // 2 * 2:2] & ~keep[1:n // 2 * 2:2])
        src = both[both % 3 == 0]  # reads deleted as a whole: their two arcs look like arcs that stay
        by_read = np.zeros(n, dtype=bool)
        by_read[2 * src], by_read[2 * src + 1] = True, True
        v = np.where(by_read, p ^ 1, v)
        ol = np.where(~keep & ~by_read & (p % 2 == 0), ol | (1 << 31), ol)
        v = np.where(~keep & ~by_read & (p % 2 == 1), 2 * dd, v)
        deleted = src.tolist() + [dd]
    a = np.zeros(n, dtype=ARC_DT)
    a["ul"], a["v"], a["oldel"] = (p.astype(np.uint64) << np.uint64(32)) | np.uint64(100), v, ol
    seq = np.full(R_ + 2, 9000, dtype="<u4")
    seq[np.asarray(deleted, dtype=np.int64)] |= np.uint32(1 << 31)
    idx = np.zeros(2 * (R_ + 2), dtype="<u8")
    R.orc().orc_arc_index(R_ + 2, n, _ptr(a), _ptr(idx))
    return R_ + 2, a, seq, idx


# --------------------------------------------------------------------------------------------- cleaners and unitigs at their size edges (tests/test_gpu_clean_edges.py)
class CleanInfo(C.Structure):  # include/mahip.h: mahip_clean_info_t
    _fields_ = [("n_iter", C.c_uint32), ("max_tier", C.c_uint32), ("seq_sweep", C.c_uint32), ("form", C.c_uint32 * 5), ("n_src", C.c_uint64 * 5)]


FORM_THREAD, FORM_LDS, FORM_HBM = 1, 2, 3  # MAHIP_BUBBLE_THREAD / _WAVE_LDS / _WAVE_HBM


def clean_api():
    """the C ABI entry points of the cleaners and the unitig pass, and the view of what the last cleaner call did"""
    L = graph_api()
    vp, u32 = C.c_void_p, C.c_uint32
    for name in ("mahip_asg_cut_tip", "mahip_asg_cut_internal", "mahip_asg_cut_biloop"):
        getattr(L, name).argtypes = [vp, C.c_int, C.POINTER(u32)]
    L.mahip_asg_pop_bubble.argtypes = [vp, C.c_int, C.POINTER(u32), C.POINTER(u32)]
    L.mahip_asg_del_short.argtypes = [vp, C.c_float, C.POINTER(u32)]
    L.mahip_clean_last.argtypes = [vp, C.POINTER(CleanInfo)]
    L.mahip_ug_gen.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.mahip_ug_download.argtypes = [vp] + [vp] * 7
    L.mahip_scan_forms.restype = None
    L.mahip_scan_forms.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
    return L


def clean_last(ctx):
    """mahip_clean_last as a dict: n_iter, max_tier, seq_sweep, form[5], n_src[5]"""
    info = CleanInfo()
    ma._chk(clean_api().mahip_clean_last(ctx.h, C.byref(info)), "clean_last")
    return dict(n_iter=info.n_iter, max_tier=info.max_tier, seq_sweep=info.seq_sweep, form=list(info.form), n_src=[int(x) for x in info.n_src])


def scan_forms(ctx):
    """mahip_scan_forms: scans of this context so far that took [one tile, the chained launch, reduce / scan / downsweep]"""
    out = (C.c_uint64 * 3)()
    clean_api().mahip_scan_forms(ctx.h, C.byref(out))
    return [int(x) for x in out]


def mirror_rows(rows, d_len=3):
    """with_mirrors on an (n, 4) array: row k and its mirror stand at 2k and 2k + 1"""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    out = np.empty((2 * len(r), 4), dtype=np.int64)
    out[0::2] = r
    out[1::2, 0], out[1::2, 1], out[1::2, 2], out[1::2, 3] = r[:, 1] ^ 1, r[:, 0] ^ 1, r[:, 2] + d_len, r[:, 3]
    return out


class Gb:
    """a graph under construction: reads are handed out in id order, arcs are given between VERTICES (Gb.v(read), ^ 1 for the other strand);
    finish() adds the mirrors and returns what asg_symm + asg_cleanup leave: symmetric, sorted, indexed, no multi-arcs (asserted).
    mixed: every third read is used on its reverse strand."""
    DEL = 1 << 31

    def __init__(self, mixed=False):
        self.n, self.rows, self.raw, self.mixed = 0, [], [], mixed

    def reads(self, k):
        self.n += k
        return np.arange(self.n - k, self.n, dtype=np.int64)

    def read(self):
        return int(self.reads(1)[0])

    def v(self, r):
        r = np.asarray(r, dtype=np.int64)
        return 2 * r + (r % 3 == 1 if self.mixed else 0)

    def arc(self, u, v, ln, ol=3000, dead=False):
        u, v, ln, ol = np.broadcast_arrays(np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64), np.asarray(ln, dtype=np.int64), np.asarray(ol, dtype=np.int64))
        if u.size:
            self.rows.append(np.stack([u.ravel(), v.ravel(), ln.ravel(), ol.ravel() | (self.DEL if dead else 0)], axis=1))

    def arc2(self, u, v, ln, ln_mirror, ol=3000):
        """an arc and its mirror with lengths of their own (finish() adds no mirror for these)"""
        self.raw.append(np.array([[u, v, ln, ol], [v ^ 1, u ^ 1, ln_mirror, ol]], dtype=np.int64))

    def path(self, reads, ln=1, ol=3000):
        self.arc(self.v(reads[:-1]), self.v(reads[1:]), ln, ol)

    def ring(self, k):
        """k reads in a ring: nothing about it is a tip, a fork or a bubble"""
        h = self.reads(k)
        self.path(np.r_[h, h[:1]], 50)
        return h

    def finish(self, d_len=3, pad_to=None):
        if pad_to is not None:
            assert pad_to >= self.n
            self.n = pad_to
        rows = mirror_rows(np.concatenate(self.rows), d_len) if self.rows else np.zeros((0, 4), dtype=np.int64)
        rows = np.concatenate([rows] + self.raw) if self.raw else rows
        uv = rows[:, 0] << 32 | rows[:, 1]
        assert len(np.unique(uv)) == len(uv), "multi-arcs"
        assert len(rows) == 0 or rows[:, :2].max() < 2 * self.n
        return (self.n,) + graph_from_rows(self.n, rows)


def ladder_bubble(gb, m1, m2, broken=None, tips=0):
    """source s -> two parallel paths p (m1 reads) and q (m2 reads) -> sink t -> one more read (a sink without arcs would be a tip: asg.c:393-395).
    The probe from s expands q first (arcs are taken in list order, the work list is LIFO), meets t, then p: its table holds m1 + m2 + 1 + tips entries
    when it walks its LAST arc, p's last read -> t, and that arc also has the largest d + l of the probe, `far` (p's inner arcs are 3 long, q's 1:
    asserted) -- so max_dist = far pops with d + l == max_dist on the last arc, max_dist = far - 1 gives up there with the table full.
    t^1 is a bubble source too (the mirror image, same distances with finish(d_len=0)); s is the smaller vertex and pops, t^1 must see it popped.
    tips: reads without arcs hanging off q's first reads; the pop trims them (n_tips), and the mirror probe fails (an arc comes in from outside).
    broken: "cycle": p's last read goes back to s instead of t; "nosink": it goes nowhere (the work list runs empty) -- neither is a bubble, both fill
    the table first.
    -> dict(s, t1 = t^1, entries, far)"""
    assert m1 >= 1 and m2 >= 1 and tips <= m2
    s, p, q, z, t = gb.read(), gb.reads(m1), gb.reads(m2), gb.read(), gb.read()  # (t last: without tips t^1 can be the graph's last vertex)
    gb.arc(gb.v(s), gb.v(p[0]), 1)
    gb.arc(gb.v(s), gb.v(q[0]), 2)
    gb.path(p, 3)
    gb.path(q, 1)
    gb.arc(gb.v(q[-1]), gb.v(t), 2)
    if broken is None:
        gb.arc(gb.v(p[-1]), gb.v(t), 1)
    else:  # t keeps waiting for an arc from a ring the probe never reaches (else t, expanded, would leave p as the last open end: a bubble)
        assert broken in ("cycle", "nosink")
        gb.arc(gb.v(gb.ring(4)[1]), gb.v(t), 1)
        if broken == "cycle":
            gb.arc(gb.v(p[-1]), gb.v(s), 1)
    gb.arc(gb.v(t), gb.v(z), 5)
    if tips:
        w = gb.reads(tips)
        gb.arc(gb.v(q[:tips]), gb.v(w), 7)
    far_p, far_q = 3 * (m1 - 1) + 2, m2 + 3 + (6 if tips else 0)
    return dict(s=int(gb.v(s)), t1=int(gb.v(t)) ^ 1, entries=m1 + m2 + 1 + tips, far=far_p, far_is_last=far_p > far_q)


def ladder_of(entries):
    """(m1, m2) of the ladder whose probe holds `entries` vertices"""
    return entries // 2, (entries - 1) // 2


def fan_bubble(gb, k, tips=0):
    """source s -> k middle reads -> sink t -> one more read: the probe's table holds k + 1 + tips entries, s and t^1 have k arcs each (the wave form stages
    them 64 at a time).  tips: reads without arcs hanging off the first middles.  -> dict(s, t1, entries, far)"""
    s, m, z, t = gb.read(), gb.reads(k), gb.read(), gb.read()
    i = np.arange(k)
    gb.arc(gb.v(s), gb.v(m), 10 + i)
    gb.arc(gb.v(m), gb.v(t), 10 + i)
    gb.arc(gb.v(t), gb.v(z), 5)
    if tips:
        gb.arc(gb.v(m[:tips]), gb.v(gb.reads(tips)), 4000)
    return dict(s=int(gb.v(s)), t1=int(gb.v(t)) ^ 1, entries=k + 1 + tips, far=20 + 2 * (k - 1))


def hub_bubble(gb, nv, special=None, pos=0, pre=12):
    """the wave form's staging: source s -> c (a short chain), X, F.  F is expanded first and finds `pre` reads without arcs (13 .. 15 entries: tier 0 is
    full), then X with exactly nv arcs, then only c is left on the work list: a bubble whose sink is c and whose pop trims the arc-less reads (n_tips).
    X's arc at list position j is 100 + j long, d(X) = 2.  special at position pos of X's list:
      "dead"     the arc is flagged deleted (to a read of its own): skipped, one tip fewer;
      "v0_dead"  the arc goes back to s AND is flagged deleted: the check for the source comes first (asg.c:377-378), no bubble;
      "far"      the arcs from pos on are all 100 + pos long: max_dist = far pops (d + l == max_dist at pos), far - 1 gives up exactly at pos.
    -> dict(s, entries, n_tips, far)"""
    assert nv >= 1 and 0 <= pos < nv
    s, c, X, F = gb.read(), gb.reads(3), gb.read(), gb.read()
    gb.arc(gb.v(s), gb.v([c[0], X, F]), [1, 2, 3])
    gb.path(c, 1)
    gb.arc(gb.v(F), gb.v(gb.reads(pre)), 1 + np.arange(pre) // 4)
    j = np.arange(nv)
    ln = 100 + (np.minimum(j, pos) if special == "far" else j)
    y = gb.reads(nv)
    keep = np.ones(nv, dtype=bool)
    if special in ("dead", "v0_dead"):
        keep[pos] = False
        gb.arc(gb.v(X), gb.v(y[pos]) if special == "dead" else gb.v(s), int(ln[pos]), dead=True)
    gb.arc(gb.v(X), gb.v(y[keep]), ln[keep])
    n_tips = pre + int(keep.sum())
    return dict(s=int(gb.v(s)), entries=3 + n_tips, n_tips=0 if special == "v0_dead" else n_tips, far=102 + pos, pops=special != "v0_dead")


def tip_comb(depth, order="ascending", mixed=False):
    """asg_cut_tip, a chain of dependent actions: a_1 -> a_2 -> ... -> a_D, every a_k with a second arc into a ring (so each is a fork: MULTI_OUT ends
    the walk at once, whatever max_ext).  Only a_1 has nothing coming in; a_k becomes a tip when a_{k-1} is cut.  ascending: a_k's ids grow with k, the
    reference's one sweep cuts all D, and the fixpoint needs D + 1 sweeps: sweep k is the first whose view holds the stamps of a_1 .. a_{k-1}, so it is the
    first in which a_k acts, and sweep D + 1 is the first that changes nothing.  descending: the ids fall with k, a_2 never sees a dead a_1 (its stamp is
    not smaller than a_2), one tip is cut, and the second sweep already changes nothing: 2 sweeps.  -> (graph, actions, sweeps)"""
    gb = Gb(mixed)
    h = gb.ring(depth + 3)
    a = gb.reads(depth)
    if order == "descending":
        a = a[::-1]
    gb.path(a, 10)
    gb.arc(gb.v(a), gb.v(h[1:depth + 1]), 20)
    gb.arc(gb.v(a[-1]), gb.v(h[depth + 1]), 30)
    return gb.finish(), (depth if order == "ascending" else 1), (depth + 1 if order == "ascending" else 2)


def internal_comb(depth, order="ascending", mixed=False):
    """asg_cut_internal(max_ext = 1), the same dependency: v_1 -> v_2 -> ... -> v_D -> a ring, every v_k also entered from a ring vertex h_k (which has two
    arcs out).  v_k is "internal" when h_k is its only way in (MULTI_NEI behind it) and its one arc leads to a vertex with other ways in (MULTI_NEI ahead):
    true for v_1 from the start, for v_k once v_{k-1} is gone.  Sweeps as in tip_comb: D + 1 ascending, 2 descending.  -> (graph, actions, sweeps)"""
    gb = Gb(mixed)
    h = gb.ring(depth + 3)
    g2 = gb.ring(4)
    a = gb.reads(depth)
    if order == "descending":
        a = a[::-1]
    gb.path(a, 10)
    gb.arc(gb.v(h[1:depth + 1]), gb.v(a), 20)
    gb.arc(gb.v(a[-1]), gb.v(g2[1]), 30)
    return gb.finish(), (depth if order == "ascending" else 1), (depth + 1 if order == "ascending" else 2)


def bubble_comb(depth, order="ascending", inner=1, big=100000):
    """asg_pop_bubble, a chain of dependent pops: bubble k is S_k -> {A_k, L_k} -> T_k.  L_k is one read; the arc L_k -> T_k is short, but its mirror T_k^1 -> L_k^1
    is `big`, longer than any max_dist.  A_1 is a chain of `inner` reads; A_k (k > 1) is a_k -> T_{k-1}^1 -> (the whole of bubble k-1, backwards) -> S_{k-1}^1:
    while L_{k-1} lives, the probe from S_k meets the big arc out of T_{k-1}^1 and gives up (too far).  The pop from S_{k-1} keeps A (visited second: the shorter
    arc out of S) and deletes L_{k-1} with the big arc, its mirror; from then on the way through bubble k-1 is a plain path and S_k is a bubble.  Ascending ids:
    the reference pops all D in one sweep; in the fixpoint S_k pops first in sweep k (the first whose view holds S_{k-1}'s stamps), sweep D + 1 is the first that
    changes nothing: D + 1 sweeps.  Descending (S_1 has the largest id): S_2 never sees S_1's stamps, one pop, 2 sweeps.  The probe from S_k holds about
    4k + inner vertices: from some k on it overflows tier 0.  No T_k^1 ever pops (big arc, or one live arc).  -> (graph, pops, sweeps, max_dist)"""
    gb = Gb()
    n = inner + 3 + 4 * (depth - 1) + 1
    ids = iter(np.arange(n) if order == "ascending" else np.arange(n)[::-1])
    gb.reads(n)
    rd = lambda: 2 * int(next(ids))
    prev_s = prev_t = None
    for k in range(depth):
        S, L, T = rd(), rd(), rd()
        if k == 0:
            A = [rd() for _ in range(inner)]
            gb.arc(S, A[0], 1)
            gb.arc(A[:-1], A[1:], 1)
            gb.arc(A[-1], T, 1)
        else:
            a = rd()
            gb.arc(S, a, 1)
            gb.arc(a, prev_t ^ 1, 1)
            gb.arc(prev_s ^ 1, T, 1)
        gb.arc(S, L, 2)
        gb.arc2(L, T, 2, big)
        prev_s, prev_t = S, T
    gb.arc(prev_t, rd(), 1)
    return gb.finish(d_len=0), (depth if order == "ascending" else 1), (depth + 1 if order == "ascending" else 2), 1000


def stamped_hub(gb, nv, outer=True):
    """the wave form against arcs that a SMALLER source's pop has stamped dead.  A fan S0 -> nv middles -> X^1; the pop from S0 keeps the way through ONE middle
    (the second one visited: position nv - 2 of the lists, asserted by the test from the reference's result) and deletes every other arc into X^1 together with
    its mirror, an arc out of X: X's list then holds nv - 1 arcs that are dead by their stamp alone, at every position but nv - 2.  Then (outer) a larger source s
    as in hub_bubble: s -> c (a chain), X, F; F's 12 arc-less reads fill tier 0 first, then X is expanded, and its one live arc leads through S0^1 into c's third
    read, the sink.  -> dict(S0, s, X, n_tips)"""
    S0, m, Xr = gb.read(), gb.reads(nv), gb.read()
    i = np.arange(nv)
    gb.arc(gb.v(S0), gb.v(m), 10 + i)
    gb.arc(gb.v(m), gb.v(Xr), 10 + i)
    X = int(gb.v(Xr)) ^ 1
    if not outer:
        gb.arc(gb.v(Xr), gb.v(gb.read()), 1)  # (a sink needs an arc out)
        return dict(S0=int(gb.v(S0)), X=X)
    s, c, F = gb.read(), gb.reads(4), gb.read()
    gb.arc(gb.v(s), [int(gb.v(c[0])), X, int(gb.v(F))], [1, 2, 3])
    gb.path(c, 1)
    gb.arc(gb.v(F), gb.v(gb.reads(12)), 1 + np.arange(12) // 4)
    gb.arc(int(gb.v(S0)) ^ 1, gb.v(c[2]), 1)
    return dict(S0=int(gb.v(S0)), s=int(gb.v(s)), X=X, n_tips=12)


END_KINDS = ("TIP", "MULTI_OUT", "MULTI_NEI")


def tip_piece(gb, n, end, ring):
    """a chain of exactly n reads that starts at a dead end and ends in `end`: nothing at all (the whole piece is linear, both ends are tips), a fork
    (two arcs into the ring) or one arc to a ring vertex, which has another way in.  asg_extend (asg.c:223-236) looks at the ends of at most max_ext
    reads: the piece goes iff n <= max_ext."""
    c = gb.reads(n)
    gb.path(c, 10)
    if end == "MULTI_OUT":
        gb.arc(gb.v(c[-1]), gb.v(ring[[1, 3]]), [20, 30])
    elif end == "MULTI_NEI":
        gb.arc(gb.v(c[-1]), gb.v(ring[1]), 20)
    return c


def biloop_piece(gb, n, ov, ox, ring):
    """asg.c:274-306: w -> c_1 -> ... -> c_n, c_n a fork (to w^1 and into the ring), and w -> c_n^1: the walk from v = c_1 ends MULTI_OUT at c_n within
    max_ext iff n <= max_ext, x = c_n^1, and the arc w -> x goes iff ov (overlap of w -> v) > ox (overlap of w -> x)."""
    w, c = gb.read(), gb.reads(n)
    gb.arc(gb.v(w), gb.v(c[0]), 10, ov)
    gb.path(c, 10)
    gb.arc(gb.v(w), gb.v(c[-1]) ^ 1, 15, ox)
    gb.arc(gb.v(c[-1]), gb.v(ring[1]), 20)
    return w, c


def chain_graph(L, ring=False, first=0, mixed=False, gb=None):
    """L reads in one chain (or ring); position k of the chain holds read (k + first) mod L of the piece, so read 0 -- whose vertex is the smallest with an
    arc, where the reference discovers the unitig -- stands at position L - first.  With gb=None the chain is the WHOLE graph (V == 2L)."""
    own = gb is None
    gb = Gb(mixed) if own else gb
    r = gb.reads(L)
    r = np.r_[r[first:], r[:first]] if first else r
    gb.path(np.r_[r, r[:1]] if ring else r, 700 + np.arange(L - 1 + (1 if ring else 0)) % 50)
    return gb.finish(d_len=7) if own else r


# --------------------------------------------------------------------------------------------- the hit sort at its size edges (tests/test_gpu_sort_edges.py)
class SortInfo(C.Structure):  # include/mahip.h: mahip_sort_info_t
    _fields_ = [("path", C.c_int), ("fallback", C.c_int), ("n_elem", C.c_uint64), ("n_runs_seen", C.c_uint64), ("n_pass", C.c_int), ("bits", C.c_int * 8),
                ("shift", C.c_int * 8), ("fixed7", C.c_uint32), ("groups", C.c_int)]


SORT_PATHS = {0: None, 1: "runs", 2: "records_fused_hist", 3: "records_plain"}  # MAHIP_SORT_*
RUNS_FALLBACKS = {0: None, 1: "not_tried", 2: "few_runs", 3: "id_range", 4: "interleaved", 5: "field_width"}  # MAHIP_RUNS_*
RUN_SLAB = 1024  # csrc/hits.hip: a run never crosses a border of 1024 records


def sort_api():
    L = ma.lib()
    vp = C.c_void_p
    L.mahip_sort_last.argtypes = [vp, C.POINTER(SortInfo)]
    L.mahip_hits_layout_download.argtypes = [vp, vp, vp]
    L.mahip_set_hints.argtypes = [vp, C.c_uint32]
    L.mahip_set_shard.argtypes = [vp, C.c_uint32, C.c_uint32]
    return L


def sort_last(ctx):
    """mahip_sort_last as a dict: path and fallback as names, n_elem, n_runs_seen, bits / shift per pass, fixed7 per pass, groups"""
    s = SortInfo()
    ma._chk(sort_api().mahip_sort_last(ctx.h, C.byref(s)), "sort_last")
    return dict(path=SORT_PATHS[s.path], fallback=RUNS_FALLBACKS[s.fallback], n_elem=int(s.n_elem), n_runs_seen=int(s.n_runs_seen), bits=list(s.bits)[:s.n_pass],
                shift=list(s.shift)[:s.n_pass], fixed7=[bool(s.fixed7 >> p & 1) for p in range(s.n_pass)], groups=bool(s.groups))


def layout_download(ctx, n_hits, n_seq):
    """mahip_hits_layout_download -> (sidx[n_hits], goff[n_seq + 1]): the layout the sort itself made"""
    sidx, goff = np.zeros(max(n_hits, 1), dtype="<u4"), np.zeros(n_seq + 1, dtype="<u4")
    ma._chk(sort_api().mahip_hits_layout_download(ctx.h, sidx.ctypes.data, goff.ctypes.data), "hits_layout_download")
    return sidx[:n_hits], goff


def sort_hits(qid, qs=None, seed=0):
    """records with the given query ids; qe = input position, so no two records are equal and every slot says which record it holds.
    qs None: every record of a read has the same start (the order inside a group that a dump shows is then the resident order); else the starts given"""
    qid = np.asarray(qid, dtype=np.uint64)
    n = len(qid)
    rng = np.random.default_rng(77 + seed)
    qs = (qid * np.uint64(7919)) % np.uint64(5000) if qs is None else np.asarray(qs, dtype=np.uint64)
    h = np.zeros(n, dtype=HIT_DT)
    h["qns"] = qid << np.uint64(32) | qs
    h["qe"] = np.arange(n, dtype=np.uint32)
    h["tn"] = (qid + np.uint64(1)) % (qid.max() + np.uint64(1)) if n else 0  # some id of the input: in the dictionary wherever the query ids are
    h["ts"] = rng.integers(0, 5000, n); h["te"] = h["ts"] + rng.integers(1, 5000, n).astype(np.uint32)
    h["bldel"] = 1000; h["mlrev"] = 900
    return h


def run_hits(runs, stride, mirror_ids=None):
    """[(qid, run length)] -> query ids of a stride-1 array (the runs one behind the other) or a stride-2 array (every record of a run followed by a
    mirrored single: an id out of mirror_ids, taken in turn -- at least two ids, none a run's id, so that every odd position is a run of one)"""
    r = np.asarray(runs, dtype=np.int64).reshape(-1, 2)
    own = np.repeat(r[:, 0], r[:, 1])
    if stride == 1:
        return own
    assert stride == 2 and len(mirror_ids) >= 2 and not set(np.asarray(mirror_ids).tolist()) & set(r[:, 0].tolist())
    out = np.empty(2 * len(own), dtype=np.int64)
    out[0::2] = own
    out[1::2] = np.asarray(mirror_ids, dtype=np.int64)[np.arange(len(own)) % len(mirror_ids)]
    return out


def run_list(qid, stride):
    """the run model (csrc/hits.hip: k_hit_keys_runs): record p is a head if it stands less than `stride` records behind the start of its slab of 1024, or
    qid[p - stride] != qid[p]; a run goes on at this stride until the next head of its parity class or the slab's end.  -> (id, first position, length) per run,
    in input order of the first positions"""
    qid = np.asarray(qid, dtype=np.int64)
    n = len(qid)
    head = (np.arange(n) % RUN_SLAB) < stride
    head[stride:] |= qid[stride:] != qid[:-stride]
    pos, ln = [], []
    for cls in range(stride):
        sub = head[cls::stride]
        i = np.flatnonzero(sub)
        pos.append(i * stride + cls)
        ln.append(np.diff(np.r_[i, len(sub)]))
    pos, ln = np.concatenate(pos), np.concatenate(ln)
    o = np.argsort(pos, kind="stable")
    assert len(pos) == int(head.sum()) and int(ln.sum()) == n
    return qid[pos[o]], pos[o], ln[o]


def bit_length(x):
    return max(int(x).bit_length(), 1)


def digit_plan(lo, nbits, max_bits=9):
    """csrc/radix.hip plan_digits: as few passes as possible, each at most 9 bits, widths balanced -> (shift, bits) per pass"""
    np_ = (nbits + max_bits - 1) // max_bits
    out, s = [], lo
    for i in range(np_):
        w = (nbits - (s - lo) + (np_ - i) - 1) // (np_ - i)
        out.append((s, w)); s += w
    return out


def sort_model(qid, stride, n_seq):
    """what mahip_hits_sort must report for an unsharded context: dict(path, fallback, n_elem, bits, shift, groups).  The runs path is taken when a stride is
    set, the dictionary size is known, id | position | length fit one word with at least 10 length bits, every id is < n_seq, there are at most three runs per
    four records and no two runs of one read interleave (the later one starts at or in front of the earlier one's last record)"""
    qid = np.asarray(qid, dtype=np.int64)
    n = len(qid)
    bi = bit_length(n - 1)
    bq = bit_length(n_seq - 1) if n_seq else bit_length(qid.max())
    M = dict(path="records_fused_hist", fallback=None, n_elem=n, n_runs=0, groups=bool(n_seq))
    lo = bi
    if stride:
        if not n_seq:
            M["fallback"] = "not_tried"
        elif 64 - bq - bi < 10:
            M["fallback"] = "field_width"
        else:
            rid, rpos, rlen = run_list(qid, stride)
            M["n_runs"] = len(rid)
            o = np.argsort(rid, kind="stable")
            sid, spos, slen = rid[o], rpos[o], rlen[o]
            inter = (sid[1:] == sid[:-1]) & (spos[1:] <= spos[:-1] + stride * (slen[:-1] - 1))
            if (qid >= n_seq).any():
                M["fallback"] = "id_range"
            elif len(rid) * 4 > n * 3:
                M["fallback"] = "few_runs"
            elif inter.any():
                M["fallback"] = "interleaved"
            else:
                M.update(path="runs", n_elem=len(rid), groups=False)
                lo = bi + min(16, 64 - bq - bi)
    plan = digit_plan(lo, bq)
    M["shift"], M["bits"] = [p[0] for p in plan], [p[1] for p in plan]
    return M


# --------------------------------------------------------------------------------------------- the sharded head in one process (tests/test_gpu_shard_edges.py)
ROW_DT = np.dtype([("u", "<u4"), ("v", "<u4"), ("len", "<u4"), ("oldel", "<u4")])  # include/mahip.h: the packed rows of mahip_asg_export_rows
BUF_SUB0, BUF_SUB1, BUF_RCONT, BUF_RUSED, BUF_SDEL = range(5)  # MAHIP_BUF_*


def shard_api():
    """the C ABI building blocks of the sharded mode (include/mahip.h) that the thin harness does not wrap"""
    L = graph_api()
    vp, sz, u32, i32, u64 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_uint64
    L.mahip_set_shard.argtypes = [vp, u32, u32]
    L.mahip_set_full_input.argtypes = [vp, i32]
    L.mahip_set_shard_bounds.argtypes = [vp, vp, i32]
    L.mahip_shard_bounds.restype = C.POINTER(u32)
    L.mahip_shard_bounds.argtypes = [vp, C.POINTER(i32)]
    L.mahip_hits_balance.argtypes = [vp, i32, vp]
    L.mahip_hits_set_positions.argtypes = [vp, vp, i32, u64]
    L.mahip_hits_have_positions.argtypes = [vp]
    L.mahip_xbuf.argtypes = [vp, i32, sz, C.POINTER(vp)]
    L.mahip_copy_out.argtypes = [vp, i32, vp, sz, sz]
    L.mahip_copy_in.argtypes = [vp, i32, vp, sz, sz]
    L.mahip_hits_cut_contained_flags.argtypes = [vp, i32, i32, C.POINTER(ma.MaOpt)]
    L.mahip_hits_cut_contained_finish.argtypes = [vp, C.POINTER(sz), C.POINTER(u32)]
    L.mahip_sg_flags.argtypes = [vp, C.POINTER(ma.MaOpt), i32, vp, vp]
    L.mahip_sg_finish.argtypes = [vp, C.POINTER(u32)]
    L.mahip_asg_export_rows.argtypes = [vp, vp]
    L.mahip_asg_import_rows.argtypes = [vp, vp, vp, i32, sz]
    L.mahip_sg_push_conflicts.argtypes = [vp, C.POINTER(u64)]
    L.mahip_sg_push_fix.argtypes = [vp]
    L.mahip_asg_export_rows_push.argtypes = [vp, vp]
    L.mahip_asg_import_push_rows.argtypes = [vp, vp, vp, i32, sz]
    L.mahip_asg_flags_out.argtypes = [vp, vp, sz, sz]
    L.mahip_asg_flags_in.argtypes = [vp, vp, sz, sz]
    return L


def shard_phase_names():
    """host/sharded.c: ma_shard_phase_name[], read from the library"""
    return [s.decode() for s in (C.c_char_p * ma.SHARD_N_PHASES).in_dll(ma.lib(), "ma_shard_phase_name")]


def xbuf(ctx, slot, nbytes):
    p = C.c_void_p(0)
    ma._chk(shard_api().mahip_xbuf(ctx.h, slot, nbytes, C.byref(p)), "xbuf")
    return p.value


def dev_read(ctx, dptr, nbytes):
    """mahip_memcpy_d2h -> bytes as a u8 array"""
    out = np.zeros(max(nbytes, 1), dtype=np.uint8)
    if nbytes:
        ma._chk(ma.lib().mahip_memcpy_d2h(ctx.h, out.ctypes.data, dptr, nbytes), "memcpy_d2h")
    return out[:nbytes]


def dev_write(ctx, dptr, arr):
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    if len(a):
        ma._chk(ma.lib().mahip_memcpy_h2d(ctx.h, dptr, a.ctypes.data, len(a)), "memcpy_h2d")


BUF_ELEM = {BUF_SUB0: SUB_DT, BUF_SUB1: SUB_DT, BUF_RCONT: np.dtype(np.uint8), BUF_RUSED: np.dtype(np.uint8), BUF_SDEL: np.dtype(np.uint8)}


def buf_get(ctx, which, first, count):
    """elements [first, first + count) of one of the read-indexed arrays: mahip_copy_out into exchange buffer 1, then down (buffer 0 is left alone: the
    orchestrator's send side, whose contents between two exchanges are part of what the stage tests look at)"""
    dt = BUF_ELEM[which]
    p = xbuf(ctx, 1, count * dt.itemsize)
    ma._chk(shard_api().mahip_copy_out(ctx.h, which, p, first, count), "copy_out")
    return dev_read(ctx, p, count * dt.itemsize).view(dt).copy()


def shard_range(ctx, n_seq, world, rank):
    """host/sharded.c shard_range: the context's table when it has one for this world size and dictionary, else equal read counts
    -> (per, q0, q1, bounds or None)"""
    bw = C.c_int(0)
    p = shard_api().mahip_shard_bounds(ctx.h, C.byref(bw))
    if p and bw.value == world and p[world] == n_seq:
        b = [int(p[r]) for r in range(world + 1)]
        return max([1] + [b[r + 1] - b[r] for r in range(world)]), b[rank], b[rank + 1], b
    cc = (n_seq + world - 1) // world if world > 0 else n_seq
    return cc, min(rank * cc, n_seq), min(rank * cc + cc, n_seq), None


def rows_to_arcs(rows, mp=None):
    """packed rows (ids of the dictionary before the squeeze) -> asg_arc_t records, renumbered by the squeeze map when given"""
    u, v = rows["u"].astype(np.int64), rows["v"].astype(np.int64)
    if mp is not None and len(rows):
        u, v = mp[u >> 1].astype(np.int64) << 1 | (u & 1), mp[v >> 1].astype(np.int64) << 1 | (v & 1)
    a = np.zeros(len(rows), dtype=ARC_DT)
    a["ul"], a["v"], a["oldel"] = u.astype(np.uint64) << np.uint64(32) | rows["len"].astype(np.uint64), v, rows["oldel"]
    return a


def sharded_stages(ctxs, hits, n_seq, opt, bounds, full_input, tie_mode, positions=None, stride=None):
    """ma_pipeline_head_sharded (host/sharded.c) walked on len(bounds) - 1 contexts in ONE process, rank after rank, phase by phase: every ABI call with the
    arguments sharded.c derives, every exchange done here -- mahip_xbuf + mahip_copy_out / export, mahip_memcpy_d2h, the combine in numpy (rank-major gather
    with the slot of the longest range, element-wise max, sums), mahip_memcpy_h2d, mahip_copy_in / import.  A test model of the ORDER, not a second orchestrator:
    the phases carry the names of ma_shard_phase_name[] (read from the library; S["order"] is what was walked).
    bounds: the table of read ranges (installed with mahip_set_shard_bounds after the upload), or an int = the world size with NO table (equal read counts).
    full_input 0: every context is uploaded only the records whose query lies in its range, in input order; positions (True): and told where they stood.
    -> S[phase] = dict(contrib = what every rank contributed, held = what every rank held afterwards, ...)"""
    L = shard_api()
    names = shard_phase_names()
    table = not isinstance(bounds, (int, np.integer))
    W = len(bounds) - 1 if table else int(bounds)
    assert 1 <= W <= len(ctxs)
    ctxs = list(ctxs[:W])
    active = W > 1
    hits = np.ascontiguousarray(hits, dtype=HIT_DT)
    qid = (hits["qns"] >> np.uint64(32)).astype(np.int64)
    S = {"order": [], "world": W}

    def phase(name):
        assert name in names, "host/sharded.c has no phase %r" % name
        S["order"].append(name)
        S[name] = {}
        return S[name]

    def each(f):
        return [f(r, c) for r, c in enumerate(ctxs)]

    def x_slices(which):  # exchange_slices
        es = BUF_ELEM[which].itemsize
        loc = []
        for r, c in enumerate(ctxs):
            p = xbuf(c, 0, per * es)
            xbuf(c, 1, per * es * W)
            ma._chk(L.mahip_copy_out(c.h, which, p, rng[r][0], rng[r][1] - rng[r][0]), "copy_out")
            loc.append(dev_read(c, p, per * es))
        gathered = np.concatenate(loc)
        for c in ctxs:
            p = xbuf(c, 1, per * es * W)
            dev_write(c, p, gathered)
            if tab is None:
                ma._chk(L.mahip_copy_in(c.h, which, p, 0, n_seq), "copy_in")
            else:
                for r in range(W):
                    ma._chk(L.mahip_copy_in(c.h, which, p + r * per * es, tab[r], tab[r + 1] - tab[r]), "copy_in")
        return [loc[r][:(rng[r][1] - rng[r][0]) * es].view(BUF_ELEM[which]).copy() for r in range(W)]

    def x_flags(which):  # exchange_flags
        nw = len(which)
        loc = []
        for c in ctxs:
            p = xbuf(c, 0, n_seq * nw)
            for k, w in enumerate(which):
                ma._chk(L.mahip_copy_out(c.h, w, p + k * n_seq, 0, n_seq), "copy_out")
            loc.append(dev_read(c, p, n_seq * nw))
        red = np.maximum.reduce(loc) if loc else np.zeros(0, np.uint8)
        for c in ctxs:
            p = xbuf(c, 0, n_seq * nw)
            dev_write(c, p, red)
            for k, w in enumerate(which):
                ma._chk(L.mahip_copy_in(c.h, w, p + k * n_seq, 0, n_seq), "copy_in")
        return [[l[k * n_seq:(k + 1) * n_seq].copy() for k in range(nw)] for l in loc]

    def x_rows(export, imp):  # the arc blocks, padded to the largest: export -> all-gather -> import
        loc = []
        for c in ctxs:
            p = xbuf(c, 0, stride_a * 16)
            xbuf(c, 1, stride_a * 16 * W)
            ma._chk(export(c.h, p), "export rows")
            loc.append(dev_read(c, p, stride_a * 16))
        gathered = np.concatenate(loc)
        for c in ctxs:
            p = xbuf(c, 1, stride_a * 16 * W)
            dev_write(c, p, gathered)
            ma._chk(imp(c.h, p, counts.ctypes.data, W, stride_a), "import rows")
        return [loc[r][:int(counts[r]) * 16].view(ROW_DT).copy() for r in range(W)]

    try:
        for r, c in enumerate(ctxs):
            c.set_exact_ties(tie_mode)
            if full_input or not active:
                own = hits
            else:  # (before the upload: the rank's range by sharded.c's rule, stated here)
                cc = (n_seq + W - 1) // W
                lo, hi = (int(bounds[r]), int(bounds[r + 1])) if table else (min(r * cc, n_seq), min(r * cc + cc, n_seq))
                own = hits[(qid >= lo) & (qid < hi)]
            c.hits_upload(own, n_seq)
            c.set_run_stride(run_stride(stride))
            if table:  # a table describes one upload: after the records
                b = np.ascontiguousarray(bounds, dtype="<u4")
                ma._chk(L.mahip_set_shard_bounds(c.h, b.ctypes.data, W), "set_shard_bounds")
            if positions and not full_input and active:
                pos = np.ascontiguousarray(np.flatnonzero((qid >= lo) & (qid < hi)), dtype="<u4")
                ma._chk(L.mahip_hits_set_positions(c.h, pos.ctypes.data, 0, len(hits)), "hits_set_positions")
        got = each(lambda r, c: shard_range(c, n_seq, W, r))
        per, tab = got[0][0], got[0][3]
        rng = [(g[1], g[2]) for g in got]
        S["per"], S["ranges"], S["table"] = per, rng, tab
        mh, mo = flt_params(opt)

        P = phase("sort")
        for r, c in enumerate(ctxs):
            ma._chk(L.mahip_set_full_input(c.h, 1 if full_input or W == 1 else 0), "set_full_input")
            ma._chk(L.mahip_set_shard(c.h, rng[r][0] if active else 0, rng[r][1] if active else 0xffffffff), "set_shard")
            c.sort()
        P["path"] = each(lambda r, c: sort_last(c)["path"])

        P = phase("sub#1")
        P["n_rem1"] = each(lambda r, c: c.sub(opt.min_dp, opt.min_iden, 0, 0))
        P["contrib"] = each(lambda r, c: c.sub_download(0, n_seq)[rng[r][0]:rng[r][1]])  # (the rest of the array is not the rank's to say)
        P = phase("x:sub0")
        if active:
            P["contrib"] = x_slices(BUF_SUB0)
        P["held"] = each(lambda r, c: c.sub_download(0, n_seq))

        P = phase("cut+flt+sub#2")
        res = each(lambda r, c: c.cutflt_sub(0, opt.min_span, mh, mo, opt.min_dp, opt.min_iden, opt.min_span // 2, 1))
        P["n_cut"], P["n_flt"], P["cov"], P["n_rem2"] = [x[0] for x in res], [x[1] for x in res], [x[2] for x in res], [x[3] for x in res]
        P["contrib"] = each(lambda r, c: c.sub_download(1, n_seq)[rng[r][0]:rng[r][1]])
        P = phase("x:sub1")
        if active:
            P["contrib"] = x_slices(BUF_SUB1)
        P["held"] = each(lambda r, c: c.sub_download(1, n_seq))

        P = phase("merge+cut+contained")
        for c in ctxs:
            c.sub_merge()
            ma._chk(L.mahip_hits_cut_contained_flags(c.h, 1, opt.min_span, C.byref(opt)), "hits_cut_contained_flags")
        P["subm"] = each(lambda r, c: c.sub_download(0, n_seq))
        P["r_cont"] = each(lambda r, c: buf_get(c, BUF_RCONT, 0, n_seq))
        P["r_used"] = each(lambda r, c: buf_get(c, BUF_RUSED, 0, n_seq))
        P = phase("x:flags")
        if active:
            P["contrib"] = x_flags([BUF_RCONT, BUF_RUSED])
        P["held"] = each(lambda r, c: (buf_get(c, BUF_RCONT, 0, n_seq), buf_get(c, BUF_RUSED, 0, n_seq)))

        P = phase("squeeze+sg flags")
        P["n_cut"], P["n_seq_new"] = [], []
        for c in ctxs:
            nc, nn = C.c_size_t(0), C.c_uint32(0)
            ma._chk(L.mahip_hits_cut_contained_finish(c.h, C.byref(nc), C.byref(nn)), "hits_cut_contained_finish")
            P["n_cut"].append(nc.value); P["n_seq_new"].append(nn.value)
        P["map"] = each(lambda r, c: c.map_download(n_seq))
        P["sub"] = each(lambda r, c: c.sub_download(0, n_seq, squeezed=True)[:P["n_seq_new"][r]])
        for c in ctxs:
            ma._chk(L.mahip_sg_flags(c.h, C.byref(opt), 1, None, None), "sg_flags")
        P["sdel"] = each(lambda r, c: buf_get(c, BUF_SDEL, 0, n_seq))
        P = phase("x:seq.del")
        if active:
            P["contrib"] = [x[0] for x in x_flags([BUF_SDEL])]
        P["held"] = each(lambda r, c: buf_get(c, BUF_SDEL, 0, n_seq))

        P = phase("local arcs")
        P["n_loc"], P["kernels"] = [], []  # kernels: the profiled launches of the call -- which arc sort ran (tests/test_gpu_graph_edges.py reads it the same way)
        for c in ctxs:
            n = C.c_uint32(0)
            c.prof_enable(True)
            c.prof_reset()
            try:
                ma._chk(L.mahip_sg_finish(c.h, C.byref(n)), "sg_finish")
                P["kernels"].append(sorted({k["name"] for k in c.prof_get()}))
            finally:
                c.prof_enable(False)
            P["n_loc"].append(n.value)
        P["n_hits"] = each(lambda r, c: int(L.mahip_hits_live(c.h)))
        n_loc = P["n_loc"]

        P = phase("x:arc counts")  # one counter per rank, summed
        counts = np.asarray(n_loc, dtype="<u4")
        stride_a = max(1, int(counts.max()))
        first = [int(counts[:r].sum()) for r in range(W)]
        tot = int(counts.sum())
        P["counts"], P["stride"], P["first"], P["tot"] = counts.copy(), stride_a, first, tot

        P = phase("x:arc blocks")
        if active:
            P["contrib"] = x_rows(L.mahip_asg_export_rows, L.mahip_asg_import_rows)
        P["held"] = each(lambda r, c: c.asg_download())
        P["tie"] = each(lambda r, c: c.tie_stats())

        P = phase("tie repair")
        P["repaired"], P["conflicts"] = 0, None
        if active:
            unrep = [t["unrepaired"] for t in S["x:arc blocks"]["tie"]]
            assert len(set(unrep)) == 1, "the ranks hold one graph and must take one decision: unrepaired %r" % unrep
            if unrep[0]:
                conf = []
                for c in ctxs:
                    n = C.c_uint64(0)
                    ma._chk(L.mahip_sg_push_conflicts(c.h, C.byref(n)), "sg_push_conflicts")
                    conf.append(n.value)
                have_pos = sum(1 for c in ctxs if L.mahip_hits_have_positions(c.h))
                P["conflicts"] = conf
                if sum(conf) == 0 or full_input or have_pos == W:
                    if sum(conf) and not full_input:
                        P["repaired"] = None  # own records with positions: hits_reference_rank gathers the keys of all ranks through a live communicator -- the multi-process tests
                    else:
                        if sum(conf):
                            for c in ctxs:
                                ma._chk(L.mahip_sg_push_fix(c.h), "sg_push_fix")
                        P["contrib"] = x_rows(L.mahip_asg_export_rows_push, L.mahip_asg_import_push_rows)
                        P["repaired"] = 1
        else:
            P["repaired"] = ctxs[0].tie_stats()["arc_walk"]
        P["held"] = each(lambda r, c: c.asg_download())

        P = phase("reduction (own vertices)")
        P["n_red"] = []
        for r, c in enumerate(ctxs):
            n = C.c_uint32(0)
            ma._chk(L.mahip_asg_del_trans_range(c.h, opt.gap_fuzz, 2 * rng[r][0], 2 * rng[r][1] if active else 2 * n_seq, C.byref(n)), "asg_del_trans_range")
            P["n_red"].append(n.value)
        n_red = P["n_red"]

        P = phase("x:del flags")
        if active:
            loc = []
            for r, c in enumerate(ctxs):
                p = xbuf(c, 0, stride_a * 4)
                xbuf(c, 1, stride_a * 4 * W)
                ma._chk(L.mahip_asg_flags_out(c.h, p, first[r], n_loc[r]), "asg_flags_out")
                loc.append(dev_read(c, p, stride_a * 4))
            gathered = np.concatenate(loc)
            for r, c in enumerate(ctxs):
                p = xbuf(c, 1, stride_a * 4 * W)
                dev_write(c, p, gathered)
                off = 0
                for i in range(W):
                    if i != r and counts[i]:
                        ma._chk(L.mahip_asg_flags_in(c.h, p + i * stride_a * 4, off, int(counts[i])), "asg_flags_in")
                    off += int(counts[i])
            P["contrib"] = [loc[r][:n_loc[r] * 4].view("<u4").copy() for r in range(W)]
        P["held"] = each(lambda r, c: c.asg_download()[0]["oldel"].copy())

        P = phase("rank 0: cleanup+symm")
        c = ctxs[0]
        n_arc, P["n_multi"], P["n_asymm"] = C.c_uint32(0), 0, 0
        if active:
            ma._chk(L.mahip_asg_cleanup(c.h, C.byref(n_arc)), "asg_cleanup")
            P["n_red"] = tot - n_arc.value
            if P["n_red"]:
                P["n_multi"], P["n_asymm"] = c.symm()
        else:
            P["n_red"] = n_red[0]
            if n_red[0]:
                ma._chk(L.mahip_asg_cleanup(c.h, C.byref(n_arc)), "asg_cleanup")
                P["n_multi"], P["n_asymm"] = c.symm()
        P["graph"] = c.asg_download()
    finally:
        for c in ctxs:
            L.mahip_set_shard(c.h, 0, 0xffffffff)
            L.mahip_set_full_input(c.h, 1)
            c.set_exact_ties(2)
    return S


def one_context_flags(ctx, hits, n_seq, opt):
    """the contained / touched-by-a-hit flags (hit.c:234-235, 24-36) of an unsharded run, read between the two halves of mahip_hits_cut_contained"""
    L = shard_api()
    ctx.hits_upload(hits, n_seq)
    ctx.set_run_stride(run_stride())
    ctx.sort()
    ctx.sub(opt.min_dp, opt.min_iden, 0, 0)
    mh, mo = flt_params(opt)
    ctx.cutflt_sub(0, opt.min_span, mh, mo, opt.min_dp, opt.min_iden, opt.min_span // 2, 1)
    ctx.sub_merge()
    ma._chk(L.mahip_hits_cut_contained_flags(ctx.h, 1, opt.min_span, C.byref(opt)), "hits_cut_contained_flags")
    out = buf_get(ctx, BUF_RCONT, 0, n_seq), buf_get(ctx, BUF_RUSED, 0, n_seq)
    nc, nn = C.c_size_t(0), C.c_uint32(0)
    ma._chk(L.mahip_hits_cut_contained_finish(ctx.h, C.byref(nc), C.byref(nn)), "hits_cut_contained_finish")
    return out


def ref_graph(hits, n_seq, opt):
    """the unmodified reference library from a hit array to the reduced graph: the passes of ref_hit_stages, then ma_sg_gen against the merged intervals and
    asg_arc_del_trans (with the cleanup and asg_symm it runs itself when something was reduced) -> dict(sg_arcs, sg_seq, n_red, tr_arcs, tr_idx)"""
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
    L.radix_sort_hit(p, p + n * HIT_DT.itemsize)
    sub = L.ma_hit_sub(opt.min_dp, opt.min_iden, 0, n, p, n_seq)
    n = L.ma_hit_cut(sub, opt.min_span, n, p)
    cov = C.c_float(0)
    mh, mo = flt_params(opt)
    n = L.ma_hit_flt(sub, mh, mo, n, p, C.byref(cov))
    sub2 = L.ma_hit_sub(opt.min_dp, opt.min_iden, opt.min_span // 2, n, p, n_seq)
    n = L.ma_hit_cut(sub2, opt.min_span, n, p)
    L.ma_sub_merge(n_seq, sub, sub2)
    L.free_buf(sub2)
    n = L.ma_hit_contained(C.byref(opt), d, sub, n, p)
    g = L.ma_sg_gen(C.byref(opt), d, sub, n, p)
    S = {}
    S["sg_arcs"], S["sg_seq"], _ = R.asg_arrays(g)
    S["n_red"] = L.asg_arc_del_trans(g, opt.gap_fuzz)
    S["tr_arcs"], _, S["tr_idx"] = R.asg_arrays(g)
    L.asg_destroy(g)
    L.free_buf(sub)
    L.free_buf(p)
    L.sd_destroy(d)
    return S


def balance_model(qid, n_seq, world):
    """include/mahip.h mahip_hits_balance: rank r starts at the first read behind which r / world of the hits lie -- the smallest q + 1 with
    cum[q] * world >= n_hits * r (records with an id outside the dictionary count as hits of no read); entries no rank reaches are n_seq; without reads or hits:
    equal read counts"""
    qid = np.asarray(qid, dtype=np.int64)
    n_hits = len(qid)
    b = [0] + [n_seq] * world
    if n_seq and n_hits and world > 1:
        cum = np.cumsum(np.bincount(qid[qid < n_seq], minlength=n_seq)[:n_seq]).tolist()
        for r in range(1, world):
            b[r] = next((q + 1 for q in range(n_seq) if cum[q] * world >= n_hits * r), n_seq)
    elif world > 1:
        per = (n_seq + world - 1) // world
        for r in range(1, world):
            b[r] = min(r * per, n_seq)
    return b
