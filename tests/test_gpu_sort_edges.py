"""mahip_hits_sort at every size it branches on, path by path: the layout the sort itself leaves -- sidx (input position of the record in every slot) and
goff (first slot of every read), read back with mahip_hits_layout_download -- against a plain reference written here,

    sidx == argsort(qid, stable)        goff == searchsorted(qid[sidx], arange(n_seq + 1))

and what the sort says it did (mahip_sort_last: path, fallback reason, elements, digit plan, group starts) against a model of the run rule in Python
(stages.run_list / stages.sort_model).  Every case also compares mahip_hits_download in tie mode 0 with the oracle's sort and, where oracle/_ref is built,
in tie mode 2 with the reference's radix_sort_hit.  qe = input position in every array, so no two records are equal; unless a case says otherwise all
records of a read have one qs, so the order a dump shows inside a group is the resident order and the on-demand order sort cannot cover for a wrong sidx.

What the cases reach (csrc/hits.hip, csrc/radix.hip):
 * k_hit_keys_runs: run lengths 1 .. 1025 (stride 1) and 1 .. 513 (stride 2) starting on, ending on and crossing a 1024-record slab border; the carry across
   a 64-lane round; both parity classes; partly filled last slabs and tiles, odd record counts at stride 2; two and three RUN_TILEs (the look-back); *d_total.
 * the worth-it rule on both sides of equality (40000 records in 30000 / 30001 runs).
 * k_runs_count / k_runs_expand: RX_LONG (15 / 16 / 17), a whole wave on one run (63 / 64 / 65), 1023 .. 1025 and 16383 .. 16385 runs, kfirst and the
   interleave check across a tile and a group border, the slot sum.
 * the radix passes: RS_TILE (4095 / 4096 / 4097 keys), 1 .. 9 and 15 .. 17 tiles (rs_tile_id), RS_CHUNK (64 x 4096 - 1, + 0, + 1 keys), as records and as runs;
   digit plans for id widths 1, 2, 7, 8, 9, 10, 14, 18, 19, 21, 23 and -- without a dictionary size (n_seq = 0: k_hit_bounds, k_hit_goff) -- 32 bits in four
   passes; the 7-bit form at compile time; with GROUPS (records), without (runs, shard), with a value array (the order sort behind every download).
 * group starts out of the last pass: n_seq + 1 around GS_TILE, records for the first / last / one middle id only, whole empty tiles, 526337 ids
   (k_group_close's loop over the tile minima takes a second round).
 * k_hit_keys_tiled against k_hit_keys + k_radix_hist; the shard form (keep, scan, k_key_compact, k_goff_outside, k_hit_goff).
 * the on-demand order sort: qs maxima 0, 127, 511, 65535, 2^32 - 1, with and without mahip_set_hints, 4097 and 262145 records.
 * production form (real GPU only): 256 * 64 * 4096 + 4097 records, the smallest input at which k_radix_colscan_top has per = 2; layout only.
   Measured on an MI355X: 2.2 s (the whole module: 218 cases in 5.7 s).

NOT covered: the `64 - bq - bi < 10` fallback of the runs path ("field_width") needs billions of ids or records."""
import ctypes as C

import numpy as np
import pytest

import miniasm_amd as ma
import refapi as R
import stages as ST

pytestmark = pytest.mark.gpu

IS_EMU = getattr(ma, "IS_EMU", False)


def reference_layout(qid, n_seq):
    sidx = np.argsort(np.asarray(qid, dtype=np.int64), kind="stable")
    return sidx, np.searchsorted(np.asarray(qid, dtype=np.int64)[sidx], np.arange(n_seq + 1))


def assert_layout(ctx, qid, n_seq, what):
    sidx, goff = ST.layout_download(ctx, len(qid), n_seq)
    exp_sidx, exp_goff = reference_layout(qid, n_seq)
    bad = np.flatnonzero(sidx != exp_sidx)
    assert len(bad) == 0, "%s: sidx differs in %d slots, first slot %d: position %d, expected %d" % (what, len(bad), bad[0], sidx[bad[0]], exp_sidx[bad[0]])
    bad = np.flatnonzero(goff != exp_goff)
    assert len(bad) == 0, "%s: goff differs for %d reads, first read %d: %d, expected %d" % (what, len(bad), bad[0], goff[bad[0]], exp_goff[bad[0]])


def assert_downloads(ctx, h, n_seq, stride, what, hint=0):
    """mahip_hits_download in tie mode 0 against the oracle (the context holds the sorted input), then tie mode 2 against the reference's sort"""
    got = ctx.hits_download()
    exp = h.copy()
    R.orc().orc_hit_sort(len(exp), exp.ctypes.data)
    assert got.tobytes() == exp.tobytes(), "%s: download differs from the oracle's sort" % what
    if R.have_ref():
        ctx.set_exact_ties(2)
        ctx.hits_upload(h, n_seq)
        ctx.set_run_stride(stride)
        if hint:
            ST.sort_api().mahip_set_hints(ctx.h, hint)
        ctx.sort()
        got = ctx.hits_download()
        LR = R.ref()
        LR.radix_sort_hit.argtypes = [C.c_void_p, C.c_void_p]
        LR.radix_sort_hit.restype = None
        exp = h.copy()
        LR.radix_sort_hit(exp.ctypes.data, exp.ctypes.data + len(exp) * 32)
        ctx.set_exact_ties(0)
        assert got.tobytes() == exp.tobytes(), "%s: download differs from the reference's sort (tie mode 2)" % what


def check_sort(ctx, qid, n_seq, stride, what, qs=None, hint=0, downloads=True):
    """upload, sort, and check layout, report and downloads -> (mahip_sort_last, the model)"""
    qid = np.asarray(qid, dtype=np.int64)
    h = ST.sort_hits(qid, qs)
    ctx.set_exact_ties(0)
    try:
        ctx.hits_upload(h, n_seq)
        ctx.set_run_stride(stride)
        if hint:
            ST.sort_api().mahip_set_hints(ctx.h, hint)
        ctx.sort()
        info, M = ST.sort_last(ctx), ST.sort_model(qid, stride, n_seq)
        assert_layout(ctx, qid, n_seq, what)
        assert (info["path"], info["fallback"]) == (M["path"], M["fallback"]), "%s: sorted as %r (fallback %r), the model says %r (%r)" % (what, info["path"], info["fallback"], M["path"], M["fallback"])
        assert info["n_elem"] == M["n_elem"], "%s: %d elements sorted, the model says %d" % (what, info["n_elem"], M["n_elem"])
        assert ctx.sorted_runs() == (M["n_elem"] if M["path"] == "runs" else 0), what
        if M["n_runs"]:
            assert info["n_runs_seen"] == M["n_runs"], "%s: k_hit_keys_runs counted %d runs, the model %d" % (what, info["n_runs_seen"], M["n_runs"])
        assert (info["shift"], info["bits"]) == (M["shift"], M["bits"]), "%s: digit plan %r / %r, expected %r / %r" % (what, info["shift"], info["bits"], M["shift"], M["bits"])
        assert info["fixed7"] == [b == 7 for b in M["bits"]] and info["groups"] == M["groups"], "%s: %r" % (what, info)
        if downloads:
            assert_downloads(ctx, h, n_seq, stride, what, hint)
    finally:
        ctx.set_exact_ties(2)
    return info, M


MIRRORS = lambda n_seq: np.arange(n_seq - 5, n_seq)  # ids of the mirrored singles of a stride-2 array: the dictionary's last five


def filler(own_from, own_to, ids, k0):
    """runs of (at most) four records with ids out of `ids` in turn, covering own-record offsets [own_from, own_to)"""
    out, k, at = [], k0, own_from
    while at < own_to:
        ln = min(4, own_to - at)
        out.append((int(ids[k % len(ids)]), ln)); k += 1; at += ln
    return out, k


def placed_runs(lengths, where, stride):
    """every length as a run of an id of its own (100 + k), each behind at least one slab of filler runs: `start` -- on a slab's first record, `end` -- ending
    on a slab's last record, `across` -- over a slab border, half on either side"""
    per = ST.RUN_SLAB // stride  # own records per slab
    fill_ids = np.arange(10, 17)
    runs, cur, k = [], 0, 0
    for j, L in enumerate(lengths):
        base = ((cur + per - 1) // per + 1) * per
        at = base if where == "start" else base + (-L) % per if where == "end" else base + per - (L + 1) // 2
        f, k = filler(cur, at, fill_ids, k)
        runs += f + [(100 + j, L)]
        cur = at + L
    f, k = filler(cur, (cur + per - 1) // per * per, fill_ids, k)
    return runs + f


RUN_LENGTHS = {1: (1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025), 2: (1, 2, 15, 16, 17, 63, 64, 65, 511, 512, 513)}


@pytest.mark.parametrize("where", ["start", "end", "across"])
@pytest.mark.parametrize("stride", [1, 2])
def test_run_lengths_at_the_slab_border(stride, where, gpu_ctx):
    """every run length at which k_hit_keys_runs or k_runs_expand takes another turn, placed on, against and across a slab border; a run longer than a slab's share,
    or one across a border, comes out cut, its pieces touch (the next starts one stride behind the previous one's last record) and the runs path is kept"""
    n_seq = 400
    runs = placed_runs(RUN_LENGTHS[stride], where, stride)
    qid = ST.run_hits(runs, stride, MIRRORS(n_seq))
    rid, rpos, rlen = ST.run_list(qid, stride)
    per = ST.RUN_SLAB // stride
    for j, L in enumerate(RUN_LENGTHS[stride]):  # the model itself: a run is cut exactly where it crosses slab borders
        at = int(rpos[rid == 100 + j][0]) // stride
        pieces = (at + L - 1) // per - at // per + 1
        assert (rid == 100 + j).sum() == pieces and rlen[rid == 100 + j].sum() == L, (L, where)
        assert pieces == (2 if L > per or (where == "across" and L > 1) else 1), (L, where, pieces)
    info, M = check_sort(gpu_ctx, qid, n_seq, stride, "run lengths, stride %d, %s" % (stride, where))
    assert info["path"] == "runs" and info["fallback"] is None


@pytest.mark.parametrize("stride", [1, 2])
def test_all_run_lengths_side_by_side(stride, gpu_ctx):
    """long and short runs as neighbours, ids ascending with position: they are neighbours in the sorted run sequence too and share waves of k_runs_expand"""
    n_seq = 3000
    lens = [L for _ in range(6) for L in RUN_LENGTHS[stride] + (3, 40, 1, 20)]
    runs = [(20 + j, L) for j, L in enumerate(lens)]
    qid = ST.run_hits(runs, stride, MIRRORS(n_seq))
    info, _ = check_sort(gpu_ctx, qid, n_seq, stride, "all run lengths, stride %d" % stride)
    assert info["path"] == "runs"


@pytest.mark.parametrize("n", [b + d for b in (1024, 4096, 8192, 12288) for d in (-1, 0, 1)])
@pytest.mark.parametrize("stride", [1, 2])
def test_record_counts_around_slab_and_tile(stride, n, gpu_ctx):
    """partly filled last slabs and RUN_TILEs (one to four tiles: the chained look-back, *d_total from the last one), odd record counts at stride 2"""
    n_seq = 60
    own = [(j % 41, 3) for j in range(n // 3 + 2)]
    qid = ST.run_hits(own, stride, MIRRORS(n_seq))[:n]
    info, _ = check_sort(gpu_ctx, qid, n_seq, stride, "%d records, stride %d" % (n, stride))
    assert info["path"] == "runs"


def ascending_runs(n_ids, second=(), first_len=2):
    """runs of `first_len` records for the ids 0 .. n_ids - 1 in turn, then further runs [(id, length)]: in the sorted run sequence they stand right behind the
    id's first run"""
    return [(j, first_len) for j in range(n_ids)] + list(second)


RUN_COUNT_CASES = [(T, T + d, "new", ()) for T in (1024, 16384) for d in (-1, 0, 1)]
RUN_COUNT_CASES += [(T, T + 6, "continues", ((T - 1, 2),)) for T in (1024, 16384)]       # sorted run T is the second run of read T - 1
RUN_COUNT_CASES += [(T, T + 6, "continues_long", ((T - 1, 40),)) for T in (1024, 16384)]  # ... and a whole wave writes it
RUN_COUNT_CASES += [(T, T + 6, "far", ((T - 2, 2), (T + 1, 1), (T - 2, 17), (T + 2, 1), (T - 2, 3))) for T in (1024, 16384)]  # runs T - 2 .. T + 1 are one read's: the border run's predecessors lie in the tile before


@pytest.mark.parametrize("border,n_ids,kind,second", RUN_COUNT_CASES, ids=["%d-%d-%s" % c[:3] for c in RUN_COUNT_CASES])
def test_run_counts_at_the_expand_tile_and_group_border(border, n_ids, kind, second, gpu_ctx):
    """RX_TILE (1024 runs) and RX_GROUP * RX_TILE (16384 runs): run counts on either side, and the run that opens a tile / a group once starting a new read,
    once continuing the read of the run in front of it (kfirst = rkey[r00 - 1])"""
    runs = ascending_runs(n_ids, second)
    qid = ST.run_hits(runs, 1)
    n_seq = n_ids
    rid = np.sort(ST.run_list(qid, 1)[0], kind="stable")
    assert len(rid) == n_ids + len(second)
    if kind != "new":
        assert rid[border] == rid[border - 1], "the border run continues a read"
    else:
        assert len(rid) <= border or rid[border] != rid[border - 1]
    info, _ = check_sort(gpu_ctx, qid, n_seq, 1, "%d runs, %s" % (len(rid), kind))
    assert info["path"] == "runs" and info["n_elem"] == len(rid)


def test_worth_it_rule_on_both_sides(gpu_ctx):
    """n_runs * 4 <= n * 3: 40000 records in exactly 30000 runs are sorted as runs, in 30001 as records"""
    unit = np.array([0, 0, 1, 2])
    qid = (unit[None, :] + 3 * np.arange(10000)[:, None]).reshape(-1)  # a pair and two singles, 256 times a slab: no pair crosses a border
    n_seq = 30000
    assert len(qid) == 40000 and len(ST.run_list(qid, 1)[0]) == 30000
    info, _ = check_sort(gpu_ctx, qid, n_seq, 1, "30000 runs")
    assert info["path"] == "runs"
    q2 = qid.copy()
    q2[4 * 7001 + 1] = 5  # one pair less
    assert len(ST.run_list(q2, 1)[0]) == 30001
    info, _ = check_sort(gpu_ctx, q2, n_seq, 1, "30001 runs")
    assert info["path"] == "records_fused_hist" and info["fallback"] == "few_runs" and info["n_runs_seen"] == 30001


@pytest.mark.parametrize("x", [500, 1023, 16383])
def test_interleaved_runs_fall_back(x, gpu_ctx):
    """four records in a row with one id under stride 2 (a row of self hits) are two runs of one read over the same stretch: the sort must notice and sort
    records.  The two runs are neighbours x and x + 1 of the sorted run sequence: inside a tile, across a 1024-run tile border, across a 16384-run group border"""
    n_ids = x + 10
    n_seq = n_ids + 5
    qid = ST.run_hits(ascending_runs(n_ids), 2, MIRRORS(n_seq))
    qid[4 * x:4 * x + 4] = x
    rid, rpos, _ = ST.run_list(qid, 2)
    o = np.argsort(rid, kind="stable")
    assert rid[o][x] == x and rid[o][x + 1] == x and rpos[o][x + 1] == rpos[o][x] + 1
    info, _ = check_sort(gpu_ctx, qid, n_seq, 2, "self row at run %d" % x)
    assert info["fallback"] == "interleaved" and info["path"] == "records_fused_hist"


@pytest.mark.parametrize("at", ["first", "last"])
def test_id_n_seq_itself_is_out_of_the_dictionary(at, gpu_ctx):
    """the smallest id that is not in the dictionary, in the first and in the last record: no runs path; the record path files it in front of the sentinel"""
    n_seq = 3000
    qid = ST.run_hits([(j * 7 % n_seq, 40) for j in range(200)], 1)
    qid[0 if at == "first" else -1] = n_seq
    info, _ = check_sort(gpu_ctx, qid, n_seq, 1, "id n_seq in the %s record" % at)
    assert info["fallback"] == "id_range" and gpu_ctx.sorted_runs() == 0


TILE_COUNTS = [4095, 4096] + [k * 4096 + 1 for k in list(range(1, 10)) + [15, 16, 17]] + [64 * 4096 - 1, 64 * 4096, 64 * 4096 + 1]


@pytest.mark.parametrize("n", TILE_COUNTS)
@pytest.mark.parametrize("ids", ["few", "ascending"])
def test_radix_tiles_records(ids, n, gpu_ctx):
    """RS_TILE, every tile count rs_tile_id remaps differently, RS_CHUNK: sorted as records.  few: three ids, a digit's run spans many tiles; ascending: the ids
    rise with the position, so a tile's first key continues the id of the tile in front (the atomicMin of the group starts)"""
    if ids == "few":
        n_seq, qid = 5, np.random.default_rng(n).integers(1, 4, n)
    else:
        n_seq = n // 700 + 2
        qid = np.arange(n, dtype=np.int64) * (n_seq - 1) // n
    info, _ = check_sort(gpu_ctx, qid, n_seq, 0, "%d records, %s ids" % (n, ids))
    assert info["path"] == "records_fused_hist" and info["groups"]


@pytest.mark.parametrize("n", TILE_COUNTS)
@pytest.mark.parametrize("ids", ["few", "ascending"])
def test_radix_tiles_runs(ids, n, gpu_ctx):
    """the same element counts as RUNS under stride 1 (pairs of records)"""
    rid = np.arange(n) % 3 + 1 if ids == "few" else np.arange(n)
    n_seq = 5 if ids == "few" else n
    qid = np.repeat(rid, 2)
    info, _ = check_sort(gpu_ctx, qid, n_seq, 1, "%d runs, %s ids" % (n, ids))
    assert info["path"] == "runs" and info["n_elem"] == n


@pytest.mark.parametrize("bq", [1, 2, 7, 8, 9, 10, 14, 18, 19, 21, 23])
@pytest.mark.parametrize("stride", [0, 1])
def test_digit_plans(stride, bq, gpu_ctx):
    """one to three passes of 1 .. 9 bits over the id; 7, 14 and 21 id bits take the scatter with the width at compile time (asserted in check_sort from
    mahip_sort_last); stride 0: the last pass writes the group starts, stride 1: runs, no group starts; every download adds the pair sort (value array)"""
    n_seq = (1 << (bq - 1)) + 1 if bq > 1 else 2
    rng = np.random.default_rng(bq)
    qid = np.repeat(rng.integers(0, n_seq, 2500), 2)
    qid[:2], qid[-2:] = n_seq - 1, 0
    info, M = check_sort(gpu_ctx, qid, n_seq, stride, "%d id bits, stride %d" % (bq, stride))
    assert sum(info["bits"]) == bq and len(info["bits"]) == (bq + 8) // 9 and max(info["bits"]) - min(info["bits"]) <= 1
    assert info["path"] == ("runs" if stride else "records_fused_hist")
    if bq % 7 == 0:
        assert info["fixed7"] == [True] * (bq // 7)


@pytest.mark.parametrize("stride", [0, 1])
def test_no_dictionary_size_32_bit_ids(stride, gpu_ctx):
    """n_seq = 0: the id width comes from a sweep (k_hit_bounds), four passes of 8 bits, the one group offset from k_hit_goff; a run stride is not tried"""
    rng = np.random.default_rng(5)
    qid = np.repeat(rng.integers(0, (1 << 32) - 1, 2100), 2)
    qid[7] = (1 << 32) - 2
    info, _ = check_sort(gpu_ctx, qid, 0, stride, "32-bit ids, stride %d" % stride, qs=rng.integers(0, 9000, len(qid)))
    assert info["bits"] == [8, 8, 8, 8] and not info["groups"] and info["fallback"] == ("not_tried" if stride else None)


GROUP_CASES = [(n1 - 1, w) for n1 in (2047, 2048, 2049, 4096, 4097) for w in ("first", "last", "middle")]
GROUP_CASES += [(5 * 2048 + 3, "tiles_0_and_4"), (524288 + 2049, "first_and_last_tile")]


@pytest.mark.parametrize("n_seq,where", GROUP_CASES, ids=["%d-%s" % c for c in GROUP_CASES])
@pytest.mark.parametrize("stride", [0, 1])
def test_group_starts_of_reads_without_records(stride, n_seq, where, gpu_ctx):
    """the group starts of reads without records are closed tile by tile of 2048 entries (k_group_tile_min, k_group_close): records for the first id only, the
    last only, one id in the middle of a tile, none in whole tiles in a row, and more than 256 tiles of entries"""
    pick = {"first": [0], "last": [n_seq - 1], "middle": [n_seq - 1000], "tiles_0_and_4": [3, 2047, 4 * 2048, n_seq - 1],
            "first_and_last_tile": [0, 2047, n_seq - 2048, n_seq - 1]}[where]
    qid = np.repeat(np.asarray(pick)[np.arange(150) % len(pick)], 2)
    check_sort(gpu_ctx, qid, n_seq, stride, "%d reads, records of %s" % (n_seq, where))


def shard_sort(ctx, h, n_seq, lo, hi):
    ctx.set_exact_ties(0)
    ctx.hits_upload(h, n_seq)
    ST.sort_api().mahip_set_shard(ctx.h, lo, hi)
    ctx.set_run_stride(2)
    ctx.sort()


@pytest.mark.parametrize("n", [4095, 4097, 8193])
def test_fused_and_plain_first_histogram_agree(n, gpu_ctx):
    """an unsharded context counts the first digit while it writes the keys (k_hit_keys_tiled); a shard writes keys and flags (k_hit_keys) and the first pass
    counts for itself (k_radix_hist).  A shard [1, n_seq) of an input without records of read 0 keeps every record: both forms on one input, one layout"""
    n_seq = 300
    qid = np.random.default_rng(n).integers(1, n_seq, n)
    h = ST.sort_hits(qid)
    try:
        info, _ = check_sort(gpu_ctx, qid, n_seq, 0, "fused, %d records" % n)
        fused = ST.layout_download(gpu_ctx, n, n_seq)  # (check_sort's last sort: the same input, the same path)
        assert info["path"] == "records_fused_hist"
        shard_sort(gpu_ctx, h, n_seq, 1, n_seq)
        info = ST.sort_last(gpu_ctx)
        assert info["path"] == "records_plain" and info["fallback"] == "not_tried" and info["n_elem"] == n and not info["groups"]
        plain = ST.layout_download(gpu_ctx, n, n_seq)
        assert_layout(gpu_ctx, qid, n_seq, "plain, %d records" % n)
        assert fused[0].tobytes() == plain[0].tobytes() and fused[1].tobytes() == plain[1].tobytes()
    finally:
        ST.sort_api().mahip_set_shard(gpu_ctx.h, 0, 0xffffffff)
        gpu_ctx.set_exact_ties(2)


SHARD_RANGES = [("head", 0, 77), ("tail", 77, 200), ("middle", 50, 120), ("empty", 77, 77), ("no_records", 120, 130), ("whole", 0, 200)]


@pytest.mark.parametrize("name,lo,hi", SHARD_RANGES, ids=[r[0] for r in SHARD_RANGES])
@pytest.mark.parametrize("n", [4095, 4097, 8193])
def test_shard_keeps_its_reads_records_in_order(n, name, lo, hi, gpu_ctx):
    """mahip_set_shard: the context keeps the records of the reads [lo, hi) -- the oracle's records of those reads in its order --, sidx still counts positions
    in the whole input, the groups of the reads outside are empty (in front: 0, behind: the record count), and the coverage pass on the shard gives the
    oracle's intervals for the reads in range"""
    n_seq = 200
    rng = np.random.default_rng(n + lo)
    qid = rng.integers(0, n_seq, n)
    qid[(qid >= 120) & (qid < 130)] = 131
    h = ST.sort_hits(qid)
    opt = ma.default_opt()
    try:
        shard_sort(gpu_ctx, h, n_seq, lo, hi)
        info = ST.sort_last(gpu_ctx)
        keep = np.flatnonzero((qid >= lo) & (qid < hi))
        m = len(keep)
        if m:
            assert info["path"] == ("records_fused_hist" if name == "whole" else "records_plain") and info["n_elem"] == m
        sidx, goff = ST.layout_download(gpu_ctx, m, n_seq)
        exp_sidx = keep[np.argsort(qid[keep], kind="stable")]
        assert sidx.tobytes() == exp_sidx.astype("<u4").tobytes(), "shard %s: sidx" % name
        exp_goff = np.searchsorted(qid[exp_sidx], np.arange(n_seq + 1))
        assert (exp_goff[:lo + 1] == 0).all() and (exp_goff[hi:] == m).all()
        assert goff.tobytes() == exp_goff.astype("<u4").tobytes(), "shard %s: goff" % name
        exp = h.copy()
        R.orc().orc_hit_sort(n, exp.ctypes.data)
        eq = (exp["qns"] >> np.uint64(32)).astype(np.int64)
        exp = exp[(eq >= lo) & (eq < hi)]
        assert gpu_ctx.hits_download().tobytes() == exp.tobytes(), "shard %s: records" % name
        gpu_ctx.sub(1, opt.min_iden, 0, 0)
        full = h.copy()
        R.orc().orc_hit_sort(n, full.ctypes.data)
        sub = np.zeros(n_seq, dtype=ma.SUB_DT)
        R.orc().orc_hit_sub(1, opt.min_iden, 0, n, full.ctypes.data, n_seq, sub.ctypes.data)  # (the oracle's coverage pass over the whole input)
        assert gpu_ctx.sub_download(0, n_seq)[lo:hi].tobytes() == sub[lo:hi].tobytes(), "shard %s: sub" % name
    finally:
        ST.sort_api().mahip_set_shard(gpu_ctx.h, 0, 0xffffffff)
        gpu_ctx.set_exact_ties(2)


@pytest.mark.parametrize("n", [4097, 262145])
@pytest.mark.parametrize("hinted", [False, True], ids=["swept", "hinted"])
@pytest.mark.parametrize("max_qs", [0, 127, 511, 65535, (1 << 32) - 1])
def test_order_sort_behind_a_download(max_qs, hinted, n, gpu_ctx):
    """a download orders the slots by (qid, qs, input position) with a pair sort over the qs bits (from mahip_set_hints, or a sweep) and the id bits: qs of 1,
    7, 9, 16 and 32 bits, distinct starts inside a read"""
    n_seq = 300
    rng = np.random.default_rng(n % 1000 + (max_qs & 0xffff))
    qid = rng.integers(0, n_seq, n)
    qs = rng.integers(0, max_qs + 1, n)
    qs[n // 2] = max_qs
    check_sort(gpu_ctx, qid, n_seq, 0, "qs up to %d, %s, %d records" % (max_qs, "hinted" if hinted else "swept", n), qs=qs, hint=max_qs if hinted else 0)


@pytest.mark.skipif(IS_EMU, reason="production-sized input: real GPU only")
def test_production_form_colscan_top_two_chunks_per_thread(gpu_ctx):
    """256 * 64 * 4096 + 4097 records under stride 0: 16386 radix tiles in 257 chunks, the smallest input at which every thread of k_radix_colscan_top scans two
    chunk sums (per = 2).  Layout only.  Measured on an MI355X: 2.2 s for the whole case, 1.8 s of it building the input and the reference in numpy; every
    other case of the module takes 0.13 s or less there"""
    import time
    n, n_seq = 256 * 64 * 4096 + 4097, 5000
    rng = np.random.default_rng(1)
    qid = rng.integers(0, n_seq, n, dtype=np.int64).astype(np.uint16)
    t0 = time.time()
    h = np.zeros(n, dtype=ma.HIT_DT)
    h["qns"] = qid.astype(np.uint64) << np.uint64(32)
    h["qe"] = np.arange(n, dtype=np.uint32)
    exp_sidx = np.argsort(qid, kind="stable")
    exp_goff = np.searchsorted(qid[exp_sidx], np.arange(n_seq + 1))
    t1 = time.time()
    gpu_ctx.hits_upload(h, n_seq)
    gpu_ctx.set_run_stride(0)
    gpu_ctx.sort()
    info = ST.sort_last(gpu_ctx)
    sidx, goff = ST.layout_download(gpu_ctx, n, n_seq)
    t2 = time.time()
    print("production form: reference %.1f s, upload + sort + layout download %.1f s" % (t1 - t0, t2 - t1))
    assert info["path"] == "records_fused_hist" and info["n_elem"] == n and info["bits"] == [7, 6] and info["groups"]
    assert (n + 4095) // 4096 > 256 * 64, "more than 256 chunks of 64 tiles"
    assert np.array_equal(goff, exp_goff.astype("<u4")), "goff"
    assert np.array_equal(sidx, exp_sidx.astype("<u4")), "sidx"
    gpu_ctx.hits_upload(np.zeros(1, dtype=ma.HIT_DT), 1)  # give the 2 GB of records back
