"""Plain gzip input inflated on the device (csrc/xfer.hip: k_gz_sync_count / k_gz_decode / k_gz_windows / k_gz_resolve / k_gz_crc, csrc/gzip_core.h; header and
trailer: host/ingest_gpu.c).

Stage: Ctx.gzip_inflate against tests/gzipmodel.py -- the text, the reason, the item the reason is about, and EVERY chunk's row (sync_bit, end_bit, out_len,
status, saw_final, on_chain) are EQUAL to the model's, which computes them from the parsed blocks.  chunk = 1024 unless a test says otherwise, images of a few
KB to a few hundred KB.

Sizes the design branches on: the chunk border (a dynamic header at a chunk's first bit, its last bit, one bit behind the border); GZ_SPAN_MAX = 16 whole chunks
between an item's chunk and the chunk it ends in; 4 chunks a workgroup in k_gz_sync_count and 2 items a workgroup in k_gz_decode; the 32768-cell window; the 64
lanes of an overlapping copy; inherited from inflate_core.h the 8 KiB flush, the 512 B fetch and the 10 / 8-bit fast tables (zlib's own streams at several
levels reach those).

The model knows true block starts only, so every generated image was checked on the CPU build to hold no false candidate; the two false-candidate tests state
their rows by hand.  Not covered at test size: texts above 4 GiB (64-bit offsets, the ISIZE wrap) -- DESIGN 5."""
import gzip
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import bgzfmodel as B
import gzipmodel as G
import miniasm_amd as ma
import refapi as R

pytestmark = pytest.mark.gpu

C = 1024
CB = 8 * C
WIN = 32768


def _rand(seed, n):
    return np.random.RandomState(seed).bytes(n)


def _texty(seed, n):
    rs = np.random.RandomState(seed)
    words = [b"read%d" % k for k in range(50)] + [b"\t", b"\n", b"+", b"-", b"12345", b"255"]
    out = b"".join(words[i] for i in rs.randint(0, len(words), n // 3))
    return (out * (n // len(out) + 1))[:n]


def _check(ctx, image, chunk=C, reason="OK", bad=None, skip_rows=(), text=None):
    """the device's answer EQUALS the model's; `reason` is what the test expects both to say"""
    m = G.model(image, chunk)
    assert m["reason"] == reason, ("the image is not what the test thinks", m["reason"])
    got, info = ctx.gzip_inflate(image, chunk)
    rows = ctx.gzip_items()
    assert (info["reason"], info["first_bad_item"]) == (m["reason"], m["first_bad_item"] if bad is None else bad), info
    assert info["reader"] == ("device" if reason == "OK" else "host") and info["comp_bytes"] == len(image) and info["chunk"] == chunk
    assert ctx.gzip_last() == info
    assert len(rows) == len(m["rows"]) == info["n_chunks"]
    if reason == "MULTI_MEMBER":  # the model reads the first member only: what the chunks behind its last one find is theirs
        skip_rows = range(m["blocks"][-1]["end"] // (8 * chunk) + 1, len(rows))
    for k, (a, b) in enumerate(zip(rows, m["rows"])):
        if k in skip_rows:
            continue
        assert a["sync_bit"] == b["sync_bit"], (k, a, b)
        if b["sync_bit"] is not None:
            assert a == b, (k, a, b)
    if not skip_rows:
        assert info["n_synced"] == m["n_synced"]
    assert info["n_items"] == m["n_items"]
    if reason == "OK":
        assert got == m["text"] and info["text_bytes"] == len(got)
        assert gzip.decompress(image) == got, "zlib reads something else"
        assert text is None or got == text
        for t, key in enumerate(("n_stored", "n_fixed", "n_dynamic")):
            assert info[key] == sum(1 for b in m["blocks"] if b["type"] == t), (key, info)
    else:
        assert got is None
    return info, m


class S:
    """a deflate stream under assembly, and the text it inflates to"""

    def __init__(self, seed=0):
        self.w, self.text, self.rs = B.Bits(), bytearray(), np.random.RandomState(seed)

    def bit(self):
        return 8 * len(self.w.out) + self.w.n

    def dyn(self, tokens, final=0, **kw):
        G.dynamic_block(self.w, final, tokens, self.text, **kw)
        return self

    def fix(self, tokens, final=0):
        G.fixed_block(self.w, final, tokens, self.text)
        return self

    def sto(self, data, final=0):
        G.stored(self.w, final, data, self.text)
        return self

    def pad_to_byte(self, target, final=0):
        """a stored block of random bytes after which the writer stands at byte `target`"""
        n = target - ((self.bit() + 3 + 7) // 8 + 4)
        assert 0 <= n <= 65535, n
        return self.sto(self.rs.bytes(n), final)

    def pad_to_bit(self, target):
        """a stored block, then a fixed block of as many 9-bit literals as bring the next block start to bit `target`"""
        b = (target - 10) % 8
        self.pad_to_byte((target - 10 - 9 * b) // 8)
        self.fix([200] * b)
        assert self.bit() == target
        return self

    def lits(self, n):
        return [int(x) for x in self.rs.randint(32, 127, n)]

    def image(self, head=None, **kw):
        return G.wrap(self.w.bytes(), bytes(self.text), head, **kw)


# ------------------------------------------------------------------------------------------------ sizes
def test_empty_text_is_one_final_block(gpu_ctx):
    info, _ = _check(gpu_ctx, G.gz(b""))
    assert info["n_chunks"] == 1 and info["n_items"] == 1 and info["text_bytes"] == 0


def test_one_byte(gpu_ctx):
    _check(gpu_ctx, G.gz(b"x"), text=b"x")


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_payload_of_a_chunk_less_one_exactly_and_plus_one(d, gpu_ctx):
    s = S(1)
    s.dyn(s.lits(300) + [(100, 7), (258, 300)])
    s.pad_to_byte(C + d, final=1)
    img = s.image()
    assert len(img) - 18 == C + d
    info, _ = _check(gpu_ctx, img)
    assert info["n_chunks"] == (2 if d == 1 else 1)


def _n_items(n, seed):
    """n items: a dynamic block a chunk, stored padding between them"""
    s = S(seed)
    for k in range(n):
        if k:
            s.pad_to_byte(k * C + 16 * k)
        s.dyn(s.lits(40) + [(30, 11), (258, 40)] + s.lits(5))
    s.fix([10], final=1)
    return s.image()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9, 17])
def test_item_counts_at_the_workgroup_edges(n, gpu_ctx):
    """2 items a workgroup in k_gz_decode (1, 2, 3, 9), 4 chunks a workgroup in k_gz_sync_count (3, 4, 5, 17)"""
    info, _ = _check(gpu_ctx, _n_items(n, n))
    assert info["n_items"] == n and info["n_chunks"] in (n, n + 1)


def test_memlevel_1_syncs_in_almost_every_chunk(gpu_ctx):
    data = _texty(3, 200000)
    info, m = _check(gpu_ctx, G.gz(data, 1, 1, head=G.header(fname=b"reads.paf")), text=data)
    assert info["n_dynamic"] > 200 and info["n_items"] >= 0.9 * info["n_chunks"] > 40


@pytest.mark.parametrize("level,memlevel,strategy,chunk", [(1, 8, zlib.Z_DEFAULT_STRATEGY, 4096), (6, 8, zlib.Z_DEFAULT_STRATEGY, 2048), (9, 8, zlib.Z_DEFAULT_STRATEGY, 4096), (6, 8, zlib.Z_RLE, 2048),
                                                          (6, 2, zlib.Z_HUFFMAN_ONLY, 1024), (9, 1, zlib.Z_FILTERED, 1024)])
def test_zlibs_own_streams(level, memlevel, strategy, chunk, gpu_ctx):
    data = _texty(level * 16 + memlevel, 250000)
    info, _ = _check(gpu_ctx, G.gz(data, level, memlevel, strategy), chunk, text=data)
    assert info["n_items"] >= 2


def test_flush_points_leave_empty_stored_blocks_at_any_bit(gpu_ctx):
    data = _texty(5, 120000)
    for mode in (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH):
        info, _ = _check(gpu_ctx, G.gz(data, 6, 4, flush_at=range(1500, len(data), 2503), flush_mode=mode), text=data)
        assert info["n_stored"] >= 40


# ------------------------------------------------------------------------------------------------ block starts against chunk borders
@pytest.mark.parametrize("where", ["first_bit", "last_bit", "one_bit_behind"])
def test_dynamic_header_at_a_chunk_border(where, gpu_ctx):
    at = {"first_bit": 3 * CB, "last_bit": 3 * CB - 1, "one_bit_behind": 3 * CB + 1}[where]
    s = S(7)
    s.dyn(s.lits(100) + [(50, 9)])
    s.pad_to_bit(at)
    s.dyn(s.lits(60) + [(258, 1000), (40, 3)])
    s.pad_to_byte(5 * C + 100)
    s.dyn(s.lits(10), final=1)
    info, m = _check(gpu_ctx, s.image())
    k = 2 if where == "last_bit" else 3
    assert m["rows"][k]["sync_bit"] == at and m["rows"][5 - k]["sync_bit"] is None and info["n_items"] == 3


def test_chunk_whose_only_block_start_is_the_final_block(gpu_ctx):
    s = S(8)
    s.dyn(s.lits(200))
    s.pad_to_byte(2 * C + 10)
    s.dyn(s.lits(30) + [(100, 20)], final=1)
    info, m = _check(gpu_ctx, s.image())
    assert info["n_items"] == 2 and m["rows"][2]["saw_final"] and m["rows"][2]["end_bit"] > m["rows"][2]["sync_bit"]


@pytest.mark.parametrize("what", ["fixed", "level_0"])
def test_streams_without_a_sync_anywhere(what, gpu_ctx):
    data = _texty(9, 40000) if what == "fixed" else _rand(9, 12000)
    info, _ = _check(gpu_ctx, G.gz(data, 6, 8, zlib.Z_FIXED) if what == "fixed" else G.gz(data, 0), text=data)
    assert info["n_dynamic"] == 0 and info["n_synced"] == 1 and info["n_items"] == 1 and info["n_chunks"] > 8


# ------------------------------------------------------------------------------------------------ spans
@pytest.mark.parametrize("unsynced", [G.SPAN_MAX, G.SPAN_MAX + 1])
def test_run_of_unsynced_chunks_at_the_span_limit(unsynced, gpu_ctx):
    s = S(10)
    s.dyn(s.lits(100))
    s.pad_to_byte(C + 50)
    s.dyn(s.lits(100))            # the item of chunk 1 ...
    s.pad_to_byte((2 + unsynced) * C + 30)
    s.dyn(s.lits(50), final=1)    # ... ends here, `unsynced` whole chunks further on
    ok = unsynced == G.SPAN_MAX
    info, m = _check(gpu_ctx, s.image(), reason="OK" if ok else "NO_SYNC")
    assert [r["sync_bit"] is not None for r in m["rows"]] == [True, True] + [False] * unsynced + [True]
    assert info["first_bad_item"] == (-1 if ok else 1) and m["rows"][-1]["on_chain"] == ok


@pytest.mark.parametrize("flush_at,reason", [((), "OK"), ((17 * C - 100,), "OK"), ((19 * C,), "NO_SYNC")], ids=["one_block", "second_block_inside_the_span", "second_block_behind_the_span"])
def test_level_0_stream_on_both_sides_of_the_span(flush_at, reason, gpu_ctx):
    """one stored block is one item however long (the limit is looked at at block starts); a second one must start within the span"""
    data = _rand(11, 30000)
    img = G.gz(data, 0, flush_at=flush_at)
    blk = G.blocks(img[10:-8])[0]
    assert all(b["type"] == 0 for b in blk) and (len(blk) == 1) == (not flush_at)
    _check(gpu_ctx, img, reason=reason)


# ------------------------------------------------------------------------------------------------ windows
def _item_of(s, n_out):
    """tokens of exactly n_out bytes of output in a few hundred bytes of input: 300 literals, then matches at distance 300"""
    toks = s.lits(min(n_out, 300))
    left = n_out - len(toks)
    while left:
        n = min(left, 258)
        if left - n in (1, 2):
            n -= 3
        toks.append((n, 300))
        left -= n
    return toks


def _first_item(seed, before):
    """a stream whose item 0 -- a dynamic block, then stored padding to the next chunk border -- inflates to exactly `before` bytes; the writer stands at the border"""
    n_pad = 500
    for _ in range(8):
        s = S(seed)
        s.dyn(_item_of(s, before - n_pad))
        at = (s.bit() + 3 + 7) // 8 + 4
        border = (at // C + 1) * C
        if border - at == n_pad:
            s.pad_to_byte(border)
            assert len(s.text) == before and s.bit() == 8 * border
            return s
        n_pad = border - at
    raise AssertionError("the padding does not settle")


@pytest.mark.parametrize("before,first,reason", [(WIN, (258, WIN), "OK"), (WIN + 5000, (258, WIN), "OK"), (WIN, (9, 1), "OK"), (WIN - 1, (258, WIN), "DIST_TOO_FAR"), (1500, (3, 1501), "DIST_TOO_FAR")],
                         ids=["first_cell_is_the_first_byte_of_the_stream", "first_cell", "one_byte_in_front", "one_byte_in_front_of_the_stream", "short_first_item"])
def test_match_into_the_window_in_front_of_an_item(before, first, reason, gpu_ctx):
    s = _first_item(12, before)
    s.dyn([first, 65, (20, 5)] + s.lits(20), final=1)
    info, m = _check(gpu_ctx, s.image(), reason=reason, text=bytes(s.text) if reason == "OK" else None)
    assert info["n_items"] == 2 and info["first_bad_item"] == (-1 if reason == "OK" else 1)
    assert m["rows"][0]["out_len"] == before


@pytest.mark.parametrize("dist", [1, 63, 64, 65])
def test_overlapping_copy_that_starts_in_the_window_and_runs_into_the_item(dist, gpu_ctx):
    s = _first_item(13 + dist, 3000)
    own = 0 if dist == 1 else 30  # bytes of the item's own output in front of the match: its source starts dist - own bytes in front of the item
    s.dyn(s.lits(own) + [(258, dist), (200, dist)] + s.lits(3), final=1)
    _check(gpu_ctx, s.image(), text=bytes(s.text))


@pytest.mark.parametrize("middle", ["short", "no_output"])
def test_references_resolve_two_items_back(middle, gpu_ctx):
    s = _first_item(14, 40000)
    if middle == "short":
        s.dyn(s.lits(20) + [(100, 30000)])
        s.pad_to_byte(((s.bit() >> 3) // C + 1) * C + 5)
    else:  # an empty dynamic block that starts 20 bytes in front of a border, a flush's empty stored block behind it, and the next item's block right there
        s.dyn(s.lits(20))
        s.pad_to_byte(((s.bit() >> 3) // C + 2) * C - 20)
        s.dyn([])
        s.sto(b"")
    k = len(s.text)
    s.dyn([(258, WIN), (258, 5000), (258, 1)] + s.lits(10), final=1)
    info, m = _check(gpu_ctx, s.image(), text=bytes(s.text))
    chain = [r for r in m["rows"] if r["on_chain"]]
    assert len(chain) == (3 if middle == "short" else 4) and chain[-2]["out_len"] == (k - 40000 if middle == "short" else 0) and chain[-2]["out_len"] < 5000


# ------------------------------------------------------------------------------------------------ false candidates
def _false_candidate(same_chunk):
    """a real dynamic block's bits, byte-aligned, at the first byte of chunk 2 inside a stored block's payload; the next true dynamic start in chunk 2 or in chunk 3"""
    f = S(20)
    f.dyn(f.lits(30) + [(40, 9)])
    fake = f.w.bytes() + b"\0"  # behind its end-of-block: zero bits, BTYPE 0
    s = S(21)
    s.dyn(s.lits(100))
    at = (s.bit() + 3 + 7) // 8 + 4  # where the stored payload starts
    end = 2 * C + (400 if same_chunk else C)
    pay = bytearray(s.rs.bytes(end - at))
    pay[2 * C - at:2 * C - at + len(fake)] = fake
    s.sto(bytes(pay))
    assert s.bit() == 8 * end
    s.dyn(s.lits(50), final=1)
    return s


def test_false_candidate_in_front_of_the_true_start_is_a_mismatch(gpu_ctx):
    s = _false_candidate(True)
    text, info = gpu_ctx.gzip_inflate(s.image(), C)
    rows = gpu_ctx.gzip_items()
    assert text is None and (info["reason"], info["first_bad_item"], info["reader"]) == ("SYNC_MISMATCH", 1, "host"), info
    assert rows[2]["sync_bit"] == 2 * CB and rows[0]["end_bit"] == 8 * (2 * C + 400) and rows[0]["on_chain"] and not rows[2]["on_chain"]
    assert G.model(s.image(), C)["reason"] == "OK"  # the stream itself is fine: the refusal costs the zlib road, nothing else


def test_false_candidate_in_a_chunk_the_chain_jumps_over(gpu_ctx):
    s = _false_candidate(False)
    info, m = _check(gpu_ctx, s.image(), skip_rows=(2,), text=bytes(s.text))
    rows = gpu_ctx.gzip_items()
    assert m["rows"][2]["sync_bit"] is None and rows[2]["sync_bit"] == 2 * CB and not rows[2]["on_chain"]
    assert info["n_items"] == 2 and info["n_synced"] == 3


# ------------------------------------------------------------------------------------------------ headers and refusals
HEADS = dict(fname=G.header(fname=b"reads.paf"), extra=G.header(extra=B.subfield(b"XY", b"abcde") + B.subfield(b"BC", b"three")), comment=G.header(comment=b"a comment"),
             hcrc=G.header(hcrc=True), mtime=G.header(mtime=1700000000), everything=G.header(fname=b"n", comment=b"c", extra=b"", hcrc=True, mtime=7, ftext=True))


@pytest.mark.parametrize("what", list(HEADS))
def test_header_fields_are_skipped(what, gpu_ctx):
    data = _texty(30, 30000)
    img = G.gz(data, 1, 1, head=HEADS[what])
    assert G.parse_header(img) == len(HEADS[what])
    _check(gpu_ctx, img, text=data)


def _refusals():
    data = _texty(31, 30000)
    good = G.gz(data, 1, 1)
    out = {}
    out["reserved_flag"] = (G.gz(data, 1, 1, head=G.header(reserved=0x20)), "BAD_HEADER", -1)
    out["not_deflate"] = (b"\x1f\x8b\x07" + good[3:], "BAD_HEADER", -1)
    out["bc_subfield"] = (G.gz(data, 1, 1, head=G.header(extra=B.subfield(b"BC", b"ab"))), "BAD_HEADER", -1)
    out["too_short"] = (good[:17], "BAD_HEADER", -1)
    n = G.model(good, C)["n_items"]
    out["two_members"] = (good + good, "MULTI_MEMBER", n - 1)
    out["trailing_bytes"] = (good + b"trailing", "MULTI_MEMBER", n - 1)
    out["wrong_crc"] = (B.set_u32(good, len(good) - 8, zlib.crc32(data) ^ 0x10), "CRC", -1)
    out["wrong_isize"] = (B.set_u32(good, len(good) - 4, len(data) + 1), "ISIZE", -1)
    return out


REFUSALS = _refusals()


def _in_use(ctx):
    L = ma.lib()
    L.mahip_mem_pool_bytes.restype = ma.C.c_size_t
    L.mahip_mem_pool_bytes.argtypes = [ma.C.c_void_p]
    return ctx.mem_bytes() - L.mahip_mem_pool_bytes(ctx.h)


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusal_by_name_and_nothing_stays_loaded(what, gpu_ctx):
    image, reason, bad = REFUSALS[what]
    before = _in_use(gpu_ctx)
    if what in ("two_members", "trailing_bytes"):  # the model reads the first member only
        _check(gpu_ctx, image, reason=reason)
    text, info = gpu_ctx.gzip_inflate(image, C)
    assert text is None and (info["reason"], info["first_bad_item"], info["reader"]) == (reason, bad, "host"), info
    for target in ("paf", "fastx"):
        assert gpu_ctx.gzip_load(image, target, C)["reason"] == reason
    pi = ma.PafInfo()
    assert ma.lib().mahip_paf_parse_excl(gpu_ctx.h, 2000, 100, 1, 0, 0, 0.0, ma.C.byref(pi)) != 0 and b"no text loaded" in ma.lib().mahip_strerror()
    fi = ma.FastxInfo()
    assert ma.lib().mahip_fastx_index(gpu_ctx.h, ma.C.byref(fi)) != 0
    assert _in_use(gpu_ctx) == before, "device memory of the refused load is still held"
    data = _texty(32, 5000)  # a plain load works afterwards
    ma._chk(ma.lib().mahip_paf_load_mem(gpu_ctx.h, data, len(data)), "paf_load_mem")
    ma._chk(ma.lib().mahip_paf_release(gpu_ctx.h), "paf_release")
    assert _in_use(gpu_ctx) == before


def test_one_flipped_payload_bit_is_never_a_wrong_text(gpu_ctx):
    data = _texty(33, 60000)
    good = G.gz(data, 1, 2)
    rs = np.random.RandomState(34)
    seen = set()
    for _ in range(24):
        byte, bit = int(rs.randint(10, len(good) - 8)), int(rs.randint(0, 8))
        text, info = gpu_ctx.gzip_inflate(B.flip_bit(good, byte, bit), C)
        assert info["reason"] != "OK" or text == data, (byte, bit, info)
        assert (text is None) == (info["reason"] != "OK")
        seen.add(info["reason"])
    assert seen - {"OK"}, seen


def test_empty_reads_file_is_left_to_the_host(gpu_ctx):
    assert gpu_ctx.gzip_load(G.gz(b""), "fastx", C)["reason"] == "EMPTY"
    assert gpu_ctx.gzip_load(G.gz(b""), "paf", C)["reason"] == "OK"
    ma._chk(ma.lib().mahip_paf_release(gpu_ctx.h), "paf_release")


# ------------------------------------------------------------------------------------------------ targets
@pytest.fixture(scope="module")
def paf(tmpdir_s):
    return R.pafgen(os.path.join(tmpdir_s, "gzip.paf"), 400, 12000, 23, ["-L", "uniform"])


def test_load_for_the_paf_reader_gives_the_plain_files_hits_and_names(paf, gpu_ctx, tmpdir_s):
    data = open(paf, "rb").read()
    a = ma.GpuIngest(gpu_ctx, paf)
    hits, names = a.hits.copy(), a.names()
    a.close()
    L = ma.lib()
    infos = []
    for load in (lambda: ma._chk(L.mahip_paf_load_mem(gpu_ctx.h, data, len(data)), "paf_load_mem"), lambda: gpu_ctx.gzip_load(G.gz(data, 1, 4, head=G.header(fname=b"gzip.paf")), "paf", 4096)):
        r = load()
        assert r is None or (r["reason"] == "OK" and r["reader"] == "device" and r["n_items"] >= 8), r
        pi = ma.PafInfo()
        ma._chk(L.mahip_paf_parse_excl(gpu_ctx.h, 2000, 100, 1, 0, 0, 0.0, ma.C.byref(pi)), "paf_parse")
        infos.append((pi.n_lines, pi.n_records, pi.n_hits, pi.n_seq, pi.name_bytes))
        ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")
    assert infos[0] == infos[1] and infos[0][0] == data.count(b"\n") and infos[0][2] == len(hits) and infos[0][3] == len(names)
    gzf = os.path.join(tmpdir_s, "gzip_target.paf.gz")
    with open(gzf, "wb") as f:
        f.write(G.gz(data, 1, 4, head=G.header(fname=b"gzip.paf")))
    old = {k: os.environ.get(k) for k in ("MA_GZIP_DEVICE", "MA_GZIP_CHUNK")}
    os.environ.update(MA_GZIP_DEVICE="1", MA_GZIP_CHUNK="4096")
    try:
        b = ma.GpuIngest(gpu_ctx, gzf)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    last = gpu_ctx.gzip_last()
    assert last["reader"] == "device" and last["reason"] == "OK" and last["text_bytes"] == len(data) and last["chunk"] == 4096
    assert b.names() == names and np.array_equal(b.hits, hits)
    b.close()


def test_load_for_the_reads_file_reader_gives_the_plain_loads_index(gpu_ctx):
    fq = b"".join(b"@r%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % k for k in range(3000))
    L = ma.lib()
    ma._chk(L.mahip_fastx_load_mem(gpu_ctx.h, fq, len(fq)), "fastx_load_mem")
    want = gpu_ctx.fastx_index()
    gpu_ctx.fastx_release()
    r = gpu_ctx.gzip_load(G.gz(fq, 6, 1), "fastx", C)
    assert r["reason"] == "OK" and r["n_items"] >= 3, r
    fi = gpu_ctx.fastx_index()
    gpu_ctx.fastx_release()
    assert fi == want and fi["n_records"] == 3000 and fi["format"] == "fastq"


# ------------------------------------------------------------------------------------------------ end to end
def _cli(binary, args, device, chunk=4096):
    env = dict(os.environ, MA_PIPE_TIMING="1", MA_GZIP_DEVICE="1" if device else "0", MA_GZIP_CHUNK=str(chunk))
    env.pop("MA_BGZF_HOST", None)
    r = subprocess.run([binary] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    log = r.stderr.decode(errors="replace")
    return r.returncode, r.stdout, log, re.findall(r"^\[T::gzip\] reader=(\w+) reason=(\d+) \(.*\) item=(-?\d+) chunks=(\d+) .*items=(\d+)", log, re.M)


@pytest.fixture(scope="module")
def e2e(paf, tmpdir_s):
    data = open(paf, "rb").read()
    img = G.gz(data, 1, 8, head=G.header(fname=b"gzip.paf", mtime=1700000000))
    out = dict(paf=paf, gz=os.path.join(tmpdir_s, "gzip_e2e.paf.gz"), flip=os.path.join(tmpdir_s, "gzip_flip.paf.gz"))
    with open(out["gz"], "wb") as f:
        f.write(img)
    with open(out["flip"], "wb") as f:
        f.write(B.flip_bit(img, len(img) // 2, 2))
    return out


def test_cli_on_a_gzipped_paf(e2e):
    """fails without the feature: no `[T::gzip]` line"""
    rc, want, log, lines = _cli(ma.CLI_PATH, [e2e["paf"]], True)
    assert rc == 0 and lines == [] and b"\nS\t" in b"\n" + want
    for binary in [ma.CLI_PATH] + ([R.DROPIN_BIN] if os.path.exists(R.DROPIN_BIN) else []):
        rc, out, log, lines = _cli(binary, [e2e["gz"]], True)
        assert rc == 0 and out == want, os.path.basename(binary) + ": differs from the run on the plain file"
        assert len(lines) == 1 and lines[0][0] == "device" and lines[0][1] == "0" and int(lines[0][4]) >= 8, log[-2000:]
        assert len(re.findall(r"^\[T::bgzf\] reader=host reason=\d+ \(not a BGZF file\) member=0$", log, re.M)) == 1, log[-2000:]
        rc, out, log, lines = _cli(binary, [e2e["gz"]], False)
        assert rc == 0 and out == want and [x[0] for x in lines] == ["host"] and "reason=%d " % ma.GZIP_REASONS.index("FORCED") in log
    if R.have_ref():
        r = subprocess.run([R.REF_BIN, e2e["gz"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0 and r.stdout == want, "differs from the reference on the compressed file"


def test_cli_on_a_gzipped_paf_with_a_flipped_bit_takes_zlibs_road(e2e):
    rc_h, out_h, _, lines_h = _cli(ma.CLI_PATH, [e2e["flip"]], False)
    rc_d, out_d, log, lines = _cli(ma.CLI_PATH, [e2e["flip"]], True)
    assert (rc_d, out_d) == (rc_h, out_h)
    assert len(lines) == 1 and lines[0][0] == "host" and lines[0][1] not in ("0", str(ma.GZIP_REASONS.index("FORCED"))), log[-2000:]
