"""A plain model of the PAF reader, pure Python on `bytes` (tests/test_gpu_ingest_edges.py).  Written from the reader semantics DESIGN 3.10 and the header of
csrc/paf.hip state -- kseq lines, paf.c columns, strtol numbers, hit.c:85, sdict.c ids, hit.c:87-98 records, hit.c:38-68 for -R -- and, for what the kernels
should have DECIDED, from the comment block above k_paf_parse_tile: which tile a line belongs to, where a tile's first line starts, and whether the
straight-line parser covers a line.  It is not trusted alone: the tests hold it against the host reader and the reference library as well."""
import numpy as np

LONG_MAX, LONG_MIN = (1 << 63) - 1, -(1 << 63)
M32 = 0xFFFFFFFF
GRAN = 1024          # a granule of the newline census
OVER = 960           # bytes in front of a tile in which its first line may start
GROUP = 4096         # granules per group of the "last newline" look-up
BATCH = 256          # lines of a tile that are parsed together, one per lane
NUM_COLS = (1, 2, 3, 6, 7, 8, 9, 10)  # ql qs qe tl ts te ml bl
BLANKS = b" \x0b\x0c\r"  # what strtol skips and a column can hold (TAB and LF cannot occur inside one)


def strtol(col):
    """strtol(col, 0, 10) of a column: leading blanks, one sign, digits; junk (a NUL too) ends it; saturates"""
    p = 0
    while p < len(col) and col[p] in BLANKS:
        p += 1
    neg = False
    if p < len(col) and col[p] in b"+-":
        neg = col[p] == 0x2D
        p += 1
    q = p
    while q < len(col) and 0x30 <= col[q] <= 0x39:
        q += 1
    v = int(col[p:q]) if q > p else 0
    v = -v if neg else v
    return min(max(v, LONG_MIN), LONG_MAX)


def split_lines(text):
    """kseq lines: -> (starts[L + 1], ends[L]); a line is [start, end), `end` the position of its newline; an open last line gets a virtual newline at len(text)"""
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10).astype(np.int64)
    if len(text) and text[-1] != 10:
        nl = np.r_[nl, len(text)]
    starts = np.r_[0, nl + 1]
    return starts, nl


def host_tile_k(n, L):
    """the tile size the host chooses: about 240 lines a tile, 1..31 KiB"""
    k = 240.0 * (n / L) / GRAN
    return 1 if k < 1.0 else 31 if k > 31.0 else int(k)


def covered_by_straight_line(body, cols):
    """does the straight-line code cover this line (CR already dropped)?  True / False, or None where the design leaves it open: a line with fewer than 10
    columns whose LAST column runs past a number window -- whether the window still reaches the line end depends on where the column starts, and nothing of
    such a line is ever used.  The rules: every number column is 1..8 digits and nothing else; a name is at most 63 bytes without a NUL; a column that is
    followed by a TAB fits its window (names 64 bits of TAB flags, the others 33)."""
    ncol = len(cols)
    look = cols[:11]
    for k, c in enumerate(look):
        last = k == ncol - 1
        if k in (0, 5):
            if len(c) >= (65 if last else 64):
                return False
        elif not last and len(c) >= 33:
            return False
    if ncol < 10:
        k = ncol - 1
        if k <= 10 and k not in (0, 5) and 33 <= len(cols[k]) <= 64:
            return None
        if k <= 10 and k not in (0, 5) and len(cols[k]) > 64:
            return False
        return True
    for k in NUM_COLS:
        if k < ncol and not (1 <= len(cols[k]) <= 8 and cols[k].isdigit()):
            return False
    for k in (0, 5):
        if len(cols[k]) >= 64 or b"\0" in cols[k]:
            return False
    return True


def no_cont_verdict(ql, qs, qe, tl, ts, te, rev, max_hang, int_frac):
    """hit.c:52-64: 0 nothing, 1 the target read is clearly contained, 2 the query read is (uint32 fields, int hangs, float products)"""
    def i32(x):
        x &= M32
        return x - (1 << 32) if x >> 31 else x
    f = np.float32
    l5, l3 = (i32(tl - te), i32(ts)) if rev else (i32(ts), i32(tl - te))
    if ql >> 1 > tl:
        if l5 > max_hang >> 2 or l3 > max_hang >> 2 or f((te - ts) & M32) < f(tl) * f(int_frac):
            return 0
        if i32(qs) - l5 > max_hang << 1 and i32(ql - qe) - l3 > max_hang << 1:
            return 1
    elif ql < tl >> 1:
        if qs > (max_hang >> 2) & M32 or (ql - qe) & M32 > (max_hang >> 2) & M32 or f((qe - qs) & M32) < f(ql) * f(int_frac):
            return 0
        if l5 - i32(qs) > max_hang << 1 and l3 - i32(ql - qe) > max_hang << 1:
            return 2
    return 0


class Model:
    pass


def model(text, min_span, min_match, bi_dir, K=None, no_cont=None):
    """no_cont: None, or (max_hang, int_frac) for -R.  K: the tile size in KiB (None: the host's choice)"""
    m = Model()
    n = len(text)
    starts, ends = split_lines(text)
    L = len(ends)
    m.n, m.L, m.lstart = n, L, starts.astype(np.uint64)
    m.open_line = int(n > 0 and text[-1] != 10)
    m.valid, m.stored, m.hasbl, m.rev = (np.zeros(L, dtype=bool) for _ in range(4))
    m.nums = np.zeros((8, L), dtype=np.uint32)
    m.tnoff, m.qlen, m.tlen = (np.zeros(L, dtype=np.uint32) for _ in range(3))
    m.qname, m.tname = [None] * L, [None] * L
    m.covered = [True] * L  # by the straight-line rules on the line's own bytes (the tile rule comes below)
    m.n_nobl = 0
    last_bl = 0
    u_span = min_span & M32
    for i in range(L):
        body = text[starts[i]:ends[i]]
        if len(body) > 1 and body[-1] == 13:
            body = body[:-1]
        cols = body.split(b"\t")
        m.covered[i] = covered_by_straight_line(body, cols)
        if len(cols) < 10:
            continue
        m.valid[i] = True
        m.hasbl[i] = len(cols) >= 11
        v = [strtol(cols[k]) & M32 for k in NUM_COLS[:7]]
        v[6] &= 0x7FFFFFFF
        if m.hasbl[i]:
            last_bl = strtol(cols[10]) & M32
        else:
            m.n_nobl += 1
        v.append(last_bl)  # paf.c leaves the field alone: a 10-column line keeps the last one written
        m.nums[:, i] = v
        m.rev[i] = cols[4][:1] == b"-"
        m.qname[i], m.tname[i] = cols[0].split(b"\0")[0], cols[5].split(b"\0")[0]
        m.qlen[i], m.tlen[i] = len(m.qname[i]), len(m.tname[i])
        m.tnoff[i] = sum(len(c) + 1 for c in cols[:5])
        ql, qs, qe, tl, ts, te, ml = v[:7]
        m.stored[i] = not ((qe - qs) & M32 < u_span or (te - ts) & M32 < u_span or ml < min_match)  # hit.c:85 (ml has 31 bits: never negative as an int)
    m.passed = m.stored.copy()  # hit.c:85 alone: what the parser and the dictionary insert see
    m.n_long = sum(1 for i in np.flatnonzero(m.passed) if not (1 <= m.qlen[i] <= 8 and 1 <= m.tlen[i] <= 8))
    # -R: names some stored line shows to be clearly contained; lines that touch one are dropped before ids are given out
    m.excl = set()
    if no_cont is not None:
        for i in np.flatnonzero(m.passed):
            ql, qs, qe, tl, ts, te = (int(x) for x in m.nums[:6, i])
            w = no_cont_verdict(ql, qs, qe, tl, ts, te, bool(m.rev[i]), no_cont[0], no_cont[1])
            if w == 1:
                m.excl.add(m.tname[i])
            elif w == 2:
                m.excl.add(m.qname[i])
        for i in np.flatnonzero(m.passed):
            if m.qname[i] in m.excl or m.tname[i] in m.excl:
                m.stored[i] = False
    m.names_before_excl = len({nm for i in np.flatnonzero(m.passed) for nm in (m.qname[i], m.tname[i])})
    # dictionary: ids by first appearance (query, then target), the first length seen wins; records + mirrors
    ids, m.names, m.lens = {}, [], []
    recs = []
    m.qid, m.tid = np.full(L, -1, dtype=np.int64), np.full(L, -1, dtype=np.int64)
    for i in np.flatnonzero(m.stored):
        for nm, ln in ((m.qname[i], m.nums[0, i]), (m.tname[i], m.nums[3, i])):
            if nm not in ids:
                ids[nm] = len(m.names); m.names.append(nm); m.lens.append(int(ln))
        q, t = ids[m.qname[i]], ids[m.tname[i]]
        m.qid[i], m.tid[i] = q, t
        ql, qs, qe, tl, ts, te, ml, bl = (int(x) for x in m.nums[:, i])
        mlrev, b31 = ml | int(m.rev[i]) << 31, bl & 0x7FFFFFFF
        recs.append((q << 32 | qs, qe, t, ts, te, mlrev, b31))
        if bi_dir and q != t:
            recs.append((t << 32 | ts, te, q, qs, qe, mlrev, b31))
    m.hits = np.array(recs, dtype=[("qns", "<u8"), ("qe", "<u4"), ("tn", "<u4"), ("ts", "<u4"), ("te", "<u4"), ("mlrev", "<u4"), ("bldel", "<u4")]) if recs else \
        np.zeros(0, dtype=[("qns", "<u8"), ("qe", "<u4"), ("tn", "<u4"), ("ts", "<u4"), ("te", "<u4"), ("mlrev", "<u4"), ("bldel", "<u4")])
    m.max_qs = max([max(int(m.nums[1, i]), int(m.nums[4, i])) for i in np.flatnonzero(m.passed)] or [0])
    # ---- what the kernels should have decided
    m.n_eff = n + m.open_line
    m.n_gran = (m.n_eff + GRAN - 1) // GRAN
    if L == 0:
        m.K, m.n_tiles, m.odd, m.qcont = 1, 0, [], np.zeros(0, dtype=bool)
        return m
    m.K = host_tile_k(n, L) if K is None else K
    m.form = 1 if m.K <= 15 else 2
    T = m.K * GRAN
    m.n_tiles = (m.n_gran + m.K - 1) // m.K
    m.tile_of = (ends // T).astype(np.int64)  # a tile owns the lines that END in it
    tb0 = np.arange(m.n_tiles, dtype=np.int64) * T
    k_before = np.searchsorted(ends, tb0, side="left")  # newlines in front of every tile
    m.tfirst = np.where(k_before > 0, ends[np.maximum(k_before, 1) - 1] + 1, 0).astype(np.uint64)
    m.line0 = k_before  # the first line that ends in tile t (if any does)
    # the look-up of tfirst scans back to the start of the group of the granule in front of the tile; beyond that the per-group table has to answer
    g = tb0 // GRAN - 1
    scan_lo = np.where(g >= 0, (g // GROUP) * GROUP, 0) * GRAN
    m.needs_group_table = (m.tfirst > 0) & (m.tfirst.astype(np.int64) <= scan_lo) & (g >= 0)
    m.groups_back = np.where(m.needs_group_table, g // GROUP - (m.tfirst.astype(np.int64) - 1) // (GROUP * GRAN), 0)
    m.rank_in_tile = np.arange(L) - m.line0[m.tile_of]
    m.long_first = (m.rank_in_tile == 0) & (tb0[m.tile_of] - starts[:-1] > OVER)
    m.odd = [True if m.long_first[i] else (None if m.covered[i] is None else not m.covered[i]) for i in range(L)]
    # PF_QCONT: the line's query name is that of the stored, non-odd line directly in front of it in the same tile -- and it is not on lane 0 of its wave
    m.qcont = np.zeros(L, dtype=bool)
    for i in range(1, L):
        if m.passed[i] and m.passed[i - 1] and m.odd[i] is False and m.odd[i - 1] is False and m.tile_of[i] == m.tile_of[i - 1] and m.rank_in_tile[i] % 64 != 0:
            m.qcont[i] = m.qname[i] == m.qname[i - 1]
    return m
