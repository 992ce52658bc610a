"""The device-wide exclusive scan (csrc/scan.hip) on its own, through mahip_scan_u32, against numpy's prefix sum: graph passes, the reads-file index and the
sort's histograms all lean on it, mahip_scan_forms proves which form a size took, and until now nothing compared a scan's OUTPUT with a plain prefix sum.

Reference: numpy.cumsum in uint64, masked to 32 bits, shifted to exclusive; the total is the sum mod 2^32.  Equality is exact.

Sizes: around one tile (2048 elements), around a tile's look-back of exactly one wave step (64 predecessors), around the border between the chained launch
and the three-phase form (256 tiles), and the first sizes whose tile sums need more than one tile themselves (2048 x 2048 elements: the second recursion
level) -- each with tails of n mod 8 != 0.  Values: ones, 0xffffffff, random u32 (the prefix wraps 2^32 many times), 0..3, and a single non-zero element on
the first and last position of a tile, of a thread's eight items and of the array.  Per size and value: out of place and in place, d_total given and NULL;
the output buffer is filled with a sentinel first (nothing at or behind element n may change), the input stands at the end of its buffer (the guard-page
run of the CPU build faults on a read behind it).

The launch bookkeeping of the chained form (scan_chain_begin: epoch, running ticket base, regrow-and-clear) is walked on contexts of the test's own."""
import ctypes as C

import numpy as np
import pytest

import miniasm_amd as ma
import stages as ST

pytestmark = pytest.mark.gpu

TILE = 2048
CHAIN_MAX = 256
PAD = 64           # sentinel elements behind the output
SENT = 0xDEADBEEF
BIG = 0xFFFFFFF1   # the single non-zero element


def reference(a):
    """-> (exclusive prefix sums mod 2^32, total mod 2^32)"""
    if len(a) == 0:
        return np.zeros(0, dtype=np.uint32), 0
    incl = np.cumsum(a, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    ex = np.empty(len(a), dtype=np.uint32)
    ex[0] = 0
    ex[1:] = incl[:-1]
    return ex, int(incl[-1])


def form_of(n):
    return None if n == 0 else 0 if n <= TILE else 1 if n <= CHAIN_MAX * TILE else 2


def own_ctx():
    c = ma.Ctx(0)
    c._xcap = [0, 0]
    return c


@pytest.fixture(scope="module")
def sc():
    """a context of this module's own: it knows where its exchange buffers end (see region)"""
    c = own_ctx()
    yield c
    c.close()


def region(ctx, slot, nbytes, at_end):
    """nbytes of exchange buffer `slot`, 16-byte aligned: at its start, or as close to its end as the alignment allows"""
    need = nbytes + 256
    if need + 256 > ctx._xcap[slot]:  # mahip_xbuf reserves bytes + 256 rounded up to 256; the buffer is at least this long
        ctx._xcap[slot] = (need + 256 + 255) & ~255
    base = ST.xbuf(ctx, slot, need)
    return base + ((ctx._xcap[slot] - nbytes) & ~15) if at_end else base


def h2d(ctx, d, a):
    if a.nbytes:
        assert ctx.memcpy_h2d(d, a.ctypes.data, a.nbytes) == 0, ma.lib().mahip_strerror()


def d2h(ctx, d, n, dtype=np.uint32):
    out = np.zeros(n, dtype=dtype)
    if out.nbytes:
        assert ctx.memcpy_d2h(out.ctypes.data, d, out.nbytes) == 0, ma.lib().mahip_strerror()
    return out


def first_diff(got, want):
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    return "%d of %d differ, the first at element %d = tile %d, thread %d, item %d: got %#x, want %#x" % (len(bad), len(want), i, i // TILE, i % TILE // 8, i % 8, got[i], want[i])


def check_scan(ctx, a, in_place, with_total, what, ref=None):
    """one scan of `a` through the ABI, everything about it asserted"""
    n = len(a)
    ex, total = ref if ref is not None else reference(a)
    image = np.full(n + PAD + 1, SENT, dtype=np.uint32)  # the output buffer: n elements, the sentinels, the total's word
    d_out = region(ctx, 1, image.nbytes, at_end=False)
    d_tot = d_out + 4 * (n + PAD)
    if in_place:
        image[:n] = a
        d_in = d_out
    else:
        d_in = region(ctx, 0, 4 * n, at_end=True)
        h2d(ctx, d_in, a)
    h2d(ctx, d_out, image)
    before = ctx.scan_forms()
    ctx.scan_u32(d_in, d_out, n, d_tot if with_total else None)
    after = ctx.scan_forms()
    got = d2h(ctx, d_out, n + PAD + 1)
    want_forms = list(before)
    if n:
        want_forms[form_of(n)] += 1
    assert list(after) == want_forms, (what, n, before, after)
    assert np.array_equal(got[:n], ex), "%s, n = %d: %s" % (what, n, first_diff(got[:n], ex))
    assert (got[n:n + PAD] == SENT).all(), "%s, n = %d: element %d behind the output was written" % (what, n, n + int(np.flatnonzero(got[n:n + PAD] != SENT)[0]))
    assert int(got[n + PAD]) == (total if with_total else SENT), "%s, n = %d: d_total holds %#x, the sum is %#x" % (what, n, got[n + PAD], total)
    if not in_place:
        assert np.array_equal(d2h(ctx, d_in, n), a), "%s, n = %d: the input changed" % (what, n)


VARIANTS = [(False, True), (False, False), (True, True), (True, False)]  # (in place, d_total given)


def single_positions(n):
    """first and last position of a tile, of a thread's eight items and of the array"""
    last_tile = (n - 1) // TILE * TILE
    ps = {0, 7, 8, TILE - 1, TILE, last_tile - 1, last_tile, last_tile + 7, (n - 1) // 8 * 8, n - 1}
    return sorted(p for p in ps if 0 <= p < n)


SIZES = [0, 1, 7, 8, 9, 2047, 2048, 2049, 2055, 4096, 4097,
         64 * TILE - 1, 64 * TILE + 1, 65 * TILE + 3,
         256 * TILE - 1, 256 * TILE, 256 * TILE + 1, 257 * TILE + 9,
         TILE * TILE, TILE * TILE + 1, TILE * TILE + 2049]


@pytest.mark.parametrize("n", SIZES, ids=[("twolevel-%d" if n >= TILE * TILE else "n%d") % n for n in SIZES])
def test_scan_against_prefix_sum(n, sc):
    rng = np.random.default_rng(n + 1)
    kinds = [("ones", np.ones(n, dtype=np.uint32)),
             ("all 0xffffffff", np.full(n, 0xFFFFFFFF, dtype=np.uint32)),
             ("random u32", rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)),
             ("0..3", rng.integers(0, 4, n, dtype=np.uint64).astype(np.uint32))]
    for name, a in kinds:
        ref = reference(a)
        for in_place, with_total in VARIANTS:
            check_scan(sc, a, in_place, with_total, "%s, %s, d_total %s" % (name, "in place" if in_place else "out of place", "given" if with_total else "NULL"), ref)
    for k, p in enumerate(single_positions(n) if n else []):
        a = np.zeros(n, dtype=np.uint32)
        a[p] = BIG
        ex = np.zeros(n, dtype=np.uint32)
        ex[p + 1:] = BIG
        in_place, with_total = VARIANTS[k % 4]
        check_scan(sc, a, in_place, with_total, "one element at %d, %s" % (p, "in place" if in_place else "out of place"), (ex, BIG))


def test_empty_scan_zeroes_the_total(sc):
    """n = 0 launches nothing and counts under no form, but a given d_total comes back 0"""
    before = sc.scan_forms()
    for in_place in (False, True):
        check_scan(sc, np.zeros(0, dtype=np.uint32), in_place, True, "empty")
        check_scan(sc, np.zeros(0, dtype=np.uint32), in_place, False, "empty")
    assert sc.scan_forms() == before


# ---------------------------------------------------------------------------------------------------------------- bookkeeping across launches
def tiles_n(tiles, k=0):
    """an element count of `tiles` tiles whose tail is k mod 8 elements short of the tile (k = 0: full tiles)"""
    return tiles * TILE - (k % 8)


def test_chain_bookkeeping_across_sizes():
    """on a fresh context: 2 tiles (the first words), 256 tiles (more words than there are: regrow, clear, ticket and epoch start again), 3 tiles over the
    words the 256 left behind, a one-tile and a three-phase scan in between (they draw no ticket), 2 tiles again"""
    c = own_ctx()
    try:
        rng = np.random.default_rng(7)
        for step, tiles in enumerate((2, 256, 3, 1, 300, 2, 5, 256, 2)):
            n = tiles_n(tiles, step)
            a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            check_scan(c, a, step % 2 == 1, True, "step %d: %d tiles" % (step, tiles))
        assert c.scan_forms() == (1, 7, 1)
    finally:
        c.close()


def queue_many(ctx, launches, a, d_in, d_out, d_tot):
    """queue one chained scan of a[:n] per launch into its own output range; nothing is downloaded.  Returns [(n, element offset)]."""
    plan, off = [], 0
    for k, n in enumerate(launches):
        ctx.scan_u32(d_in, d_out + 4 * off, n, d_tot + 4 * k)
        plan.append((n, off))
        off += (n + 3) & ~3  # 16-byte aligned ranges
    return plan


def check_many(ctx, plan, ex, incl, d_out, d_tot, what):
    total_elems = plan[-1][1] + plan[-1][0]
    out = d2h(ctx, d_out, total_elems)
    tot = d2h(ctx, d_tot, len(plan))
    for k, (n, off) in enumerate(plan):
        got = out[off:off + n]
        assert np.array_equal(got, ex[:n]), "%s, launch %d (n = %d): %s" % (what, k, n, first_diff(got, ex[:n]))
        assert int(tot[k]) == int(incl[n - 1]), "%s, launch %d (n = %d): total" % (what, k, n)
        if ((n + 3) & ~3) != n:
            assert (out[off + n:off + ((n + 3) & ~3)] == SENT).all(), "%s, launch %d: written behind n" % (what, k)


def many_setup(ctx, launches, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 32, max(launches), dtype=np.uint64).astype(np.uint32)
    incl = (np.cumsum(a, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ex = np.concatenate([np.zeros(1, dtype=np.uint32), incl[:-1]])
    total_elems = sum((n + 3) & ~3 for n in launches)
    d_in = region(ctx, 0, 4 * len(a), at_end=True)
    d_out = region(ctx, 1, 4 * (total_elems + len(launches) + 4), at_end=False)
    d_tot = d_out + 4 * total_elems
    h2d(ctx, d_in, a)
    h2d(ctx, d_out, np.full(total_elems + len(launches), SENT, dtype=np.uint32))
    return a, ex, incl, d_in, d_out, d_tot


def test_three_hundred_chained_launches_back_to_back():
    """2 / 5 / 64 / 65 tiles in turn, 300 launches queued without a download in between: every launch reads words that older launches of other sizes left
    (the epoch tells them apart) and draws tickets behind theirs (the running base)"""
    c = own_ctx()
    try:
        launches = [tiles_n((2, 5, 64, 65)[k % 4], k // 4) for k in range(300)]
        a, ex, incl, d_in, d_out, d_tot = many_setup(c, launches, 11)
        plan = queue_many(c, launches, a, d_in, d_out, d_tot)
        check_many(c, plan, ex, incl, d_out, d_tot, "300 launches")
        assert c.scan_forms() == (0, 300, 0)
    finally:
        c.close()


def test_two_contexts_interleaved():
    """two fresh contexts take turns: each keeps its own words, epoch and ticket"""
    c1, c2 = own_ctx(), own_ctx()
    try:
        l1 = [tiles_n((3, 64, 2, 65, 7)[k % 5], k) for k in range(40)]
        l2 = [tiles_n((65, 2, 9, 3)[k % 4], k + 3) for k in range(40)]
        s1, s2 = many_setup(c1, l1, 21), many_setup(c2, l2, 22)
        p1, p2, o1, o2 = [], [], 0, 0
        for k in range(40):
            c1.scan_u32(s1[3], s1[4] + 4 * o1, l1[k], s1[5] + 4 * k)
            p1.append((l1[k], o1))
            o1 += (l1[k] + 3) & ~3
            c2.scan_u32(s2[3], s2[4] + 4 * o2, l2[k], s2[5] + 4 * k)
            p2.append((l2[k], o2))
            o2 += (l2[k] + 3) & ~3
        check_many(c1, p1, s1[1], s1[2], s1[4], s1[5], "context 1")
        check_many(c2, p2, s2[1], s2[2], s2[4], s2[5], "context 2")
        assert c1.scan_forms() == (0, 40, 0) and c2.scan_forms() == (0, 40, 0)
    finally:
        c1.close()
        c2.close()
