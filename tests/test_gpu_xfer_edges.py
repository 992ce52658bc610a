"""The staged copy (csrc/xfer.hip: xfer_run / xfer_worker) on its own: every byte that enters or leaves HBM in a real run goes through it, and the stage tests'
inputs are small enough that nearly all of them take the runtime's own hipMemcpyAsync instead.  Here the copy is driven through the ABI (mahip_memcpy_h2d /
_d2h / _fd2d on a region of mahip_xbuf) at every size it branches on: the 8 MiB threshold between the two roads, worker counts above, at and below the
number of 4 MiB slices, the second use of each of a worker's two pinned slots, a last slice of one byte, unaligned pointers, a file offset that is a multiple
of nothing, a file that ends early.  mahip_xfer_last says which road a copy took, in how many slices, dealt by how many workers.

The data of a case is a 64-bit mix of the byte offset and the case's seed, so a slice that is swapped, shifted, duplicated, skipped or left over from the
case before changes bytes; the comparison is exact and names the first wrong offset, its slice and the worker that dealt it.  A 64-byte sentinel stands
directly behind the device region, the region itself stands at the end of the exchange buffer (the guard-page run of the CPU build faults on a read or write
behind it), and the host destination has a sentinel margin on both sides.

Not visible here, by construction: the wait on a slot's event before the slot is refilled (`k >= 2`).  The CPU build's copies are synchronous, and on the
device leaving the wait out is a timing race that a test could only try to lose; the MI355X run of the cases with 2 W + 1 and 3 W + 1 slices is what covers
it."""
import ctypes as C
import os

import numpy as np
import pytest

import miniasm_amd as ma
import stages as ST

pytestmark = pytest.mark.gpu

S = 4 << 20  # a slice
T = 8 << 20  # memory-to-memory copies below this take the runtime's road
SENT = 64
MARGIN = 4096
_M64 = (1 << 64) - 1


def pattern(seed, n, start=0):
    """bytes [start, start + n) of the stream whose 8-byte word k is splitmix64(seed + k)"""
    k0, k1 = start // 8, (start + n + 7) // 8
    with np.errstate(over="ignore"):
        z = np.arange(k0, max(k1, k0 + 1), dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & _M64)
        z *= np.uint64(0x9E3779B97F4A7C15)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z.view(np.uint8)[start - 8 * k0:start - 8 * k0 + n]


def assert_same(got, want, workers, what):
    if np.array_equal(got, want):
        return
    assert len(got) == len(want), (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    o = int(bad[0])
    sl = o // S
    raise AssertionError("%s: %d of %d bytes differ, the first at offset %d = slice %d + %d, slice %% workers = %d (got %d, want %d; the last at offset %d)"
                         % (what, len(bad), len(want), o, sl, o - sl * S, sl % max(workers, 1), got[o], want[o], int(bad[-1])))


class threads:
    """MA_XFER_THREADS for the copies inside the block (the library reads it per call); None: unset"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("MA_XFER_THREADS")
        if self.value is None:
            os.environ.pop("MA_XFER_THREADS", None)
        else:
            os.environ["MA_XFER_THREADS"] = str(self.value)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("MA_XFER_THREADS", None)
        else:
            os.environ["MA_XFER_THREADS"] = self.old


@pytest.fixture(scope="module")
def xc():
    """a context of this module's own: its exchange buffers grow only when a case asks for more than any case before, so the case knows where they end"""
    c = ma.Ctx(0)
    c._xcap = [0, 0]
    yield c
    c.close()


def region(ctx, slot, n, dev_off=0):
    """device address of n bytes + the sentinel, as close to the end of exchange buffer `slot` as a 256-byte boundary allows (+ dev_off < 256)"""
    need = n + SENT + 256
    if need + 256 > ctx._xcap[slot]:  # mahip_xbuf reserves bytes + 256 rounded up to 256: the buffer is at least this long (the pool may hand out more)
        ctx._xcap[slot] = (need + 256 + 255) & ~255
    base = ST.xbuf(ctx, slot, need)
    return base + ((ctx._xcap[slot] - 256 - n - SENT) & ~255) + dev_off


def host_buf(n, off=0):
    """(array, view of n bytes at a 64-byte boundary + off) with MARGIN bytes of 0xC3 in front and behind"""
    raw = np.full(n + 2 * MARGIN + 128, 0xC3, dtype=np.uint8)
    a = (-raw.ctypes.data) % 64 + MARGIN + off
    return raw, raw[a:a + n], a


def margins_intact(raw, a, n):
    return bool((raw[:a] == 0xC3).all() and (raw[a + n:] == 0xC3).all())


def expect_last(ctx, to_device, n, w, file=False):
    """mahip_xfer_last after a copy of n bytes under MA_XFER_THREADS = w"""
    x = ctx.xfer_last()
    staged = file or n >= T
    slices = (n + S - 1) // S if staged else 0
    want = dict(road=("staged_file" if file else "staged_mem") if staged else "runtime", to_device=to_device, bytes=n, slices=slices, workers=min(w, slices) if staged else 0)
    assert x == want, (x, want)


def put_sentinel(ctx, d, n, seed):
    s = pattern(seed ^ 0x5E47, SENT)
    assert ctx.memcpy_h2d(d + n, s.ctypes.data, SENT) == 0, ma.lib().mahip_strerror()
    return s


def sentinel_intact(ctx, d, n, s):
    got = np.zeros(SENT, dtype=np.uint8)
    assert ctx.memcpy_d2h(got.ctypes.data, d + n, SENT) == 0, ma.lib().mahip_strerror()
    return np.array_equal(got, s)


def round_trip(ctx, n, w, seed, host_off=0, dev_off=0, workers_exact=True):
    """upload n patterned bytes, download them again; both copies exact, both reports as expected, every sentinel intact.  Returns the two reports."""
    d = region(ctx, 0, n, dev_off)
    src_raw, src, _ = host_buf(n, host_off)
    src[:] = pattern(seed, n)
    want = src.copy()
    raw, dst, a = host_buf(n, host_off)
    sent = put_sentinel(ctx, d, n, seed)
    with threads(w):
        assert ctx.memcpy_h2d(d, src.ctypes.data, n) == 0, ma.lib().mahip_strerror()
        up = ctx.xfer_last()
        if workers_exact:
            expect_last(ctx, True, n, w)
        assert ctx.memcpy_d2h(dst.ctypes.data, d, n) == 0, ma.lib().mahip_strerror()
        down = ctx.xfer_last()
        if workers_exact:
            expect_last(ctx, False, n, w)
    assert np.array_equal(src, want), "the upload changed its source"
    assert_same(dst, want, down["workers"], "%d bytes up (%d workers) and down (%d workers)" % (n, up["workers"], down["workers"]))
    assert margins_intact(raw, a, n), "the download wrote outside its destination"
    assert sentinel_intact(ctx, d, n, sent), "the upload wrote behind its destination"
    return up, down


def one_way(ctx, n, w, seed, to_device):
    """the other direction goes the runtime's road in pieces below T, so that a fault of the staged road cannot hide behind its own inverse"""
    d = region(ctx, 0, n)
    want = pattern(seed, n).copy()
    sent = put_sentinel(ctx, d, n, seed)
    piece = T - S // 2
    if to_device:
        with threads(w):
            assert ctx.memcpy_h2d(d, want.ctypes.data, n) == 0, ma.lib().mahip_strerror()
            expect_last(ctx, True, n, w)
        got = np.zeros(n, dtype=np.uint8)
        for o in range(0, n, piece):
            m = min(piece, n - o)
            assert ctx.memcpy_d2h(got.ctypes.data + o, d + o, m) == 0
            assert ctx.xfer_last()["road"] == "runtime"
        assert_same(got, want, min(w, (n + S - 1) // S), "%d bytes up with %d workers, down the runtime's road" % (n, w))
    else:
        for o in range(0, n, piece):
            m = min(piece, n - o)
            assert ctx.memcpy_h2d(d + o, want.ctypes.data + o, m) == 0
            assert ctx.xfer_last()["road"] == "runtime"
        raw, dst, a = host_buf(n)
        with threads(w):
            assert ctx.memcpy_d2h(dst.ctypes.data, d, n) == 0, ma.lib().mahip_strerror()
            expect_last(ctx, False, n, w)
        assert_same(dst, want, min(w, (n + S - 1) // S), "%d bytes up the runtime's road, down with %d workers" % (n, w))
        assert margins_intact(raw, a, n)
    assert sentinel_intact(ctx, d, n, sent)


# ---------------------------------------------------------------------------------------------------------------- the threshold between the two roads
@pytest.mark.parametrize("n", [T - 1, T, T + 1, 3 * S - 1, 3 * S, 3 * S + 1], ids=["T-1", "T", "T+1", "3S-1", "3S", "3S+1"])
def test_threshold(n, xc):
    """T - 1 bytes take the runtime's road, T and more the staged one; T + 1 and 3 S + 1 end in a slice of one byte.  Four workers are asked for: two or three
    slices get two or three"""
    up, down = round_trip(xc, n, 4, seed=n)
    assert (up["road"] == "runtime") == (n < T) and up["slices"] == (0 if n < T else (n + S - 1) // S)
    one_way(xc, n, 4, seed=n + 1, to_device=True)
    one_way(xc, n, 4, seed=n + 2, to_device=False)


# ---------------------------------------------------------------------------------------------------------------- workers against slices
def slice_counts(w):
    return sorted({c for c in (w - 1, w, w + 1, 2 * w, 2 * w + 1, 3 * w + 1) if c >= 2 or c == w})


EDGE_CASES = [(w, c, extra) for w in (1, 2, 3) for c in slice_counts(w) for extra in (0, 1)]


@pytest.mark.parametrize("w,count,extra", EDGE_CASES, ids=["W%d-%dS+%d" % t for t in EDGE_CASES])
def test_worker_and_slice_edges(w, count, extra, xc):
    """count x S bytes (+ 1: one more slice, of one byte) under W workers: W - 1, W and W + 1 slices (a worker without a slice cannot be; one with a second),
    2 W + 1 (worker 0 uses its slot 0 a second time) and 3 W + 1 (its slot 1).  S and S + 1 bytes are below the threshold: one worker's "W slices" is the
    runtime's road."""
    n = count * S + extra
    round_trip(xc, n, w, seed=n * 4 + w)
    if n >= T:
        one_way(xc, n, w, seed=n * 4 + w + 1, to_device=True)
        one_way(xc, n, w, seed=n * 4 + w + 2, to_device=False)


WIDE = [(c, extra) for c in (15, 16, 17, 33) for extra in (0, 1)]


@pytest.mark.parametrize("count,extra", WIDE, ids=["wide-%dS+%d" % t for t in WIDE])
def test_sixteen_workers(count, extra, xc):
    """the most workers there are: one slice fewer, as many, one more, and 33 slices (132 MiB + 1: every worker's third slice, worker 0's fourth of one byte)"""
    n = count * S + extra
    round_trip(xc, n, 16, seed=n)


@pytest.mark.parametrize("value,want", [("0", 1), ("-3", 1), ("abc", 1), ("99", 16)])
def test_worker_count_parsing(value, want, xc):
    """MA_XFER_THREADS as atol reads it: nothing below one worker, nothing above sixteen -- in both directions, although uploads default to at most eight"""
    n = 17 * S + 1 if want > 1 else 3 * S + 1
    d = region(xc, 0, n)
    src = pattern(77 + want, n).copy()
    raw, dst, a = host_buf(n)
    with threads(value):
        assert xc.memcpy_h2d(d, src.ctypes.data, n) == 0
        expect_last(xc, True, n, want)
        assert xc.memcpy_d2h(dst.ctypes.data, d, n) == 0
        expect_last(xc, False, n, want)
    assert_same(dst, src, want, "MA_XFER_THREADS=%s" % value)
    assert margins_intact(raw, a, n)


def test_default_worker_count(xc):
    """no MA_XFER_THREADS: the CPU quota decides, so the count is a range -- at most 8 workers up, 16 down, and never more than there are slices"""
    n = 17 * S + 1
    up, down = round_trip(xc, n, None, seed=4242, workers_exact=False)
    assert up["road"] == down["road"] == "staged_mem" and up["slices"] == down["slices"] == 18 and up["bytes"] == down["bytes"] == n
    assert up["to_device"] and not down["to_device"]
    assert 1 <= up["workers"] <= 8 and 1 <= down["workers"] <= 16, (up, down)


@pytest.mark.parametrize("n", [T + 1, 3 * S + 1], ids=["T+1", "3S+1"])
@pytest.mark.parametrize("host_off,dev_off", [(1, 0), (15, 0), (0, 1), (0, 15), (15, 1)])
def test_unaligned_pointers(host_off, dev_off, n, xc):
    round_trip(xc, n, 2, seed=n + 16 * host_off + dev_off, host_off=host_off, dev_off=dev_off)


# ---------------------------------------------------------------------------------------------------------------- order on the stream
def test_order_on_the_stream_and_reuse_of_the_workers(xc):
    """a staged copy and a small copy on the runtime's road right behind it, without a sync in between by the test, see each other's bytes; then the same
    on the same context with other worker counts, whose slots and events were created by the copies before"""
    n = 5 * S + 1
    tail = 4096
    for rnd, w in enumerate((3, 2, 5, 1)):
        d = region(xc, 0, n)
        src = pattern(900 + rnd, n).copy()
        got_tail = np.zeros(tail, dtype=np.uint8)
        with threads(w):
            assert xc.memcpy_h2d(d, src.ctypes.data, n) == 0
            expect_last(xc, True, n, w)
            assert xc.memcpy_d2h(got_tail.ctypes.data, d + n - tail, tail) == 0  # the runtime's road, behind the staged upload
            expect_last(xc, False, tail, w)
        assert_same(got_tail, src[n - tail:], w, "round %d: the last 4 KiB right after a staged upload" % rnd)
        new_tail = pattern(950 + rnd, tail).copy()
        raw, dst, a = host_buf(n)
        with threads(w):
            assert xc.memcpy_h2d(d + n - tail, new_tail.ctypes.data, tail) == 0  # the runtime's road, in front of the staged download
            assert xc.memcpy_d2h(dst.ctypes.data, d, n) == 0
            expect_last(xc, False, n, w)
        src[n - tail:] = new_tail
        assert_same(dst, src, w, "round %d: a staged download right after a small upload" % rnd)
        assert margins_intact(raw, a, n)


# ---------------------------------------------------------------------------------------------------------------- the file road
FILE_SIZES = [1, S, S + 1, T + 1, 2 * 3 * S + 1]
FILE_OFFS = [0, 1, S - 1, S + 1]
FILE_SEED = 31337
FILE_LEN = max(FILE_OFFS) + max(FILE_SIZES) + 12345


@pytest.fixture(scope="module")
def long_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("xfer") / "long.bin"
    with open(p, "wb") as f:
        f.write(pattern(FILE_SEED, FILE_LEN).tobytes())
    return str(p)


def file_case(ctx, fd, off, n, w):
    d = region(ctx, 1, n)
    sent = put_sentinel(ctx, d, n, off + n)
    with threads(w):
        rc = ctx.memcpy_fd2d(d, fd, off, n)
    assert rc == 0, (off, n, w, ma.lib().mahip_strerror())
    expect_last(ctx, True, n, w, file=True)
    with threads(2):
        got = np.zeros(n, dtype=np.uint8)
        assert ctx.memcpy_d2h(got.ctypes.data, d, n) == 0
    assert_same(got, pattern(FILE_SEED, n, off), min(w, (n + S - 1) // S), "file bytes [%d, %d + %d) with %d workers" % (off, off, n, w))
    assert sentinel_intact(ctx, d, n, sent), (off, n, w)


@pytest.mark.parametrize("w", [1, 3])
def test_file_road_in_a_longer_file(w, long_file, xc):
    """mahip_memcpy_fd2d: one byte is staged already; offsets that are multiples of nothing; the file goes on behind off + nbytes"""
    fd = os.open(long_file, os.O_RDONLY)
    try:
        for n in FILE_SIZES:
            for off in FILE_OFFS:
                file_case(xc, fd, off, n, w)
    finally:
        os.close(fd)


@pytest.mark.parametrize("w", [1, 3])
def test_file_road_to_the_end_of_the_file(w, long_file, xc, tmp_path):
    """the same with the file ending exactly at off + nbytes: a copy of the long file, cut back from case to case"""
    p = str(tmp_path / "cut.bin")
    with open(long_file, "rb") as f, open(p, "wb") as g:
        g.write(f.read())
    fd = os.open(p, os.O_RDWR)
    try:
        for end, off, n in sorted(((off + n, off, n) for n in FILE_SIZES for off in FILE_OFFS), reverse=True):
            os.ftruncate(fd, end)
            file_case(xc, fd, off, n, w)
    finally:
        os.close(fd)


@pytest.mark.parametrize("missing", [1, S, 2 * S + 5], ids=["1", "S", "2S+5"])
@pytest.mark.parametrize("w", [1, 3])
def test_file_shorter_than_promised(w, missing, long_file, xc, tmp_path):
    """the file ends `missing` bytes early (inside the last slice, at a slice border, three slices early): -1 and a message, nothing behind the region is
    written, and the next staged copies on the same context -- whose workers refill their slots without looking at the events the failed copy left -- are
    exact"""
    off, n = S + 1, 5 * S + 1
    p = str(tmp_path / "short.bin")
    with open(long_file, "rb") as f, open(p, "wb") as g:
        g.write(f.read(off + n - missing))
    d = region(xc, 1, n)
    sent = put_sentinel(xc, d, n, 555 + missing)
    fd = os.open(p, os.O_RDONLY)
    try:
        with threads(w):
            rc = xc.memcpy_fd2d(d, fd, off, n)
        assert rc == -1 and len(ma.lib().mahip_strerror()) > 0
        x = xc.xfer_last()
        assert (x["road"], x["bytes"], x["slices"], x["workers"]) == ("staged_file", n, 6, w)
        assert sentinel_intact(xc, d, n, sent)
        m = n - missing  # what the file does hold goes through right after, by the same workers
        file_case(xc, fd, off, m, w)
    finally:
        os.close(fd)
    round_trip(xc, 2 * w * S + S + 1, w, seed=8000 + missing + w)
