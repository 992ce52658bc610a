"""bgzip-compressed (BGZF) input inflated on the device (csrc/xfer.hip: k_bgzf_inflate / k_bgzf_crc, csrc/inflate_core.h; the member walk: host/ingest_gpu.c).

Stage: Ctx.bgzf_inflate against zlib on every path of the inflater -- stored, fixed and dynamic blocks, several blocks a member, every match geometry against
the 64 lanes, the 32 KiB history ring and the 8 KiB flush threshold -- with the block counts by type the kernel reports.  Refusal: every status of the
kernel and every refusal of the walk, by name and member; nothing stays loaded.  End to end: `miniasm x.paf.gz` and `miniasm -f x.fq.gz x.paf.gz` on bgzip'ed
files, byte for byte against the plain files, MA_BGZF_HOST=1 and the reference binary.

Sizes the design branches on: BGZF_WAVES = 4 members to a workgroup (3, 4, 5 members); the ring wraps at output position 32768; unflushed output is flushed as
soon as there are 8192 bytes of it, which behind a stored prefix (copied 256 bytes at a time) is at the multiples of 8192; the input window is fetched 512 bytes
at a time; the fast tables cover codes of up to 10 (literal/length) and 8 (distance) bits, longer ones take the canonical decoder.

Two cases of the issue cannot exist as it words them, because a BGZF member's total size is a 16-bit field (at most 65536 bytes with header and trailer):
`65536 incompressible bytes at level 0` do not fit one member -- here: 65280 incompressible bytes at level 0 (bgzip's own member size) and a hand-made member
of two stored blocks, 65000 + 490 bytes; and zlib never emits a distance above 32768 - 262, so `32768 random bytes twice at level 9` holds no distance of
32768 (and is incompressible, so it does not fit either) -- here the member is assembled by hand: the 32768 bytes stored, then matches of length 258 at
distance 32768, which the helper's parser confirms."""
import gzip
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import bgzfmodel as B
import miniasm_amd as ma
import refapi as R

pytestmark = pytest.mark.gpu

WAVES = 4  # csrc/xfer.hip: BGZF_WAVES


def _inflate(ctx, image, text, **counts):
    got, info = ctx.bgzf_inflate(image)
    assert info["reason"] == "OK" and info["reader"] == "device" and info["first_bad_member"] == -1, info
    assert info["text_bytes"] == len(text) and info["comp_bytes"] == len(image)
    assert got == text, "text differs from zlib's"
    assert gzip.decompress(image) == text, "the image itself is not what the test thinks"
    for k, v in counts.items():
        assert info[k] == v, (k, info)
    return info


def _blocks(image):
    """deflate blocks by type over the members of an image, from the helper's parser"""
    n = [0, 0, 0]
    for off, total in B.members_of(image):
        xlen = int.from_bytes(image[off + 10:off + 12], "little")
        for t in B.parse(image[off + 12 + xlen:off + total - 8])["blocks"]:
            n[t] += 1
    return dict(n_stored=n[0], n_fixed=n[1], n_dynamic=n[2])


def _rand(seed, n):
    return np.random.RandomState(seed).bytes(n)


def _texty(seed, n):
    rs = np.random.RandomState(seed)
    words = [b"read%d" % k for k in range(50)] + [b"\t", b"\n", b"+", b"-", b"12345", b"255"]
    out = b"".join(words[i] for i in rs.randint(0, len(words), n // 3))
    return (out * (n // len(out) + 1))[:n]


# ------------------------------------------------------------------------------------------------ stage: zlib's own streams
def test_marker_only_file_is_an_empty_text(gpu_ctx):
    _inflate(gpu_ctx, B.EOF_MARKER, b"", n_members=1, n_empty=1, n_fixed=1, n_stored=0, n_dynamic=0)


def test_one_member_of_one_byte(gpu_ctx):
    for eof in (True, False):
        _inflate(gpu_ctx, B.bgzf(b"x", eof=eof), b"x", n_members=1 + eof, n_empty=int(eof))


@pytest.mark.parametrize("isize", [65280, 65536])
def test_member_of_bgzips_size_and_of_the_largest_size(isize, gpu_ctx):
    data = _texty(isize, isize)
    img = B.bgzf(data, member_size=isize)
    _inflate(gpu_ctx, img, data, n_members=2, **_blocks(img))


@pytest.mark.parametrize("n", [WAVES - 1, WAVES, WAVES + 1, 4 * WAVES + 1])
@pytest.mark.parametrize("eof", [False, True])
def test_member_counts_at_the_workgroup_edges(n, eof, gpu_ctx):
    data = _texty(n, 3000 * n)
    img = B.bgzf(data, member_size=3000, eof=eof)
    _inflate(gpu_ctx, img, data, n_members=n + eof, n_empty=int(eof))


def test_empty_members_in_the_middle(gpu_ctx):
    data = _texty(5, 20000)
    img = B.bgzf(data, member_size=4000, empty_at=(0, 2, 3))
    _inflate(gpu_ctx, img, data, n_members=5 + 3 + 1, n_empty=4)


def test_incompressible_member_at_level_0(gpu_ctx):
    data = _rand(1, 65280)
    img = B.bgzf(data, level=0)
    n = _blocks(img)
    assert n["n_stored"] >= 1 and n["n_dynamic"] == 0
    _inflate(gpu_ctx, img, data, **n)


def test_two_stored_blocks_in_one_member(gpu_ctx):
    data = _rand(2, 65490)
    w = B.Bits()
    B.stored(w, 0, data[:65000])
    B.stored(w, 1, data[65000:])
    img = B.member(w.bytes(), data) + B.EOF_MARKER
    _inflate(gpu_ctx, img, data, n_stored=2, n_fixed=1, n_dynamic=0)


@pytest.mark.parametrize("mode", ["sync", "full"])
def test_stored_blocks_behind_unaligned_headers(mode, gpu_ctx):
    """a flush leaves an empty stored block whose header starts wherever the block before ended"""
    data = _texty(7, 30000)
    img = B.bgzf(data, flush_every=701, flush_mode=zlib.Z_SYNC_FLUSH if mode == "sync" else zlib.Z_FULL_FLUSH)
    n = _blocks(img)
    assert n["n_stored"] >= 42
    _inflate(gpu_ctx, img, data, **n)


def test_fixed_huffman_member(gpu_ctx):
    data = _texty(8, 40000)
    img = B.bgzf(data, strategy=zlib.Z_FIXED)
    n = _blocks(img)
    assert n["n_dynamic"] == 0 and n["n_fixed"] >= 2
    _inflate(gpu_ctx, img, data, **n)


def test_huffman_only_has_no_matches(gpu_ctx):
    data = _texty(9, 50000)
    img = B.bgzf(data, strategy=zlib.Z_HUFFMAN_ONLY)
    off, total = B.members_of(img)[0]
    assert B.parse(img[off + 18:off + total - 8])["matches"] == []
    _inflate(gpu_ctx, img, data, **_blocks(img))


@pytest.mark.parametrize("level,strategy,mem_level", [(1, zlib.Z_DEFAULT_STRATEGY, 8), (6, zlib.Z_DEFAULT_STRATEGY, 8), (9, zlib.Z_DEFAULT_STRATEGY, 9), (6, zlib.Z_RLE, 8),
                                                      (6, zlib.Z_DEFAULT_STRATEGY, 1), (9, zlib.Z_FILTERED, 1)])
def test_levels_strategies_and_many_blocks_a_member(level, strategy, mem_level, gpu_ctx):
    """memLevel 1: a new deflate block every 127 symbols or so, hundreds a member"""
    data = _texty(level * 16 + mem_level, 150000)
    img = B.bgzf(data, level=level, strategy=strategy, mem_level=mem_level)
    n = _blocks(img)
    if mem_level == 1:
        assert n["n_dynamic"] + n["n_fixed"] > 100
    _inflate(gpu_ctx, img, data, **n)


def test_run_of_one_byte(gpu_ctx):
    """distance 1, length 258 chains: every lane reads the same byte"""
    data = b"A" * 65536
    img = B.bgzf(data, member_size=65536)
    off, total = B.members_of(img)[0]
    m = B.parse(img[off + 18:off + total - 8])["matches"]
    assert any(ln == 258 and d == 1 for _, ln, d in m)
    _inflate(gpu_ctx, img, data)


@pytest.mark.parametrize("period", [2, 3, 63, 64, 65])
def test_overlapping_matches_against_the_lane_count(period, gpu_ctx):
    unit = _rand(period, period)
    data = (unit * (40000 // period + 1))[:40000]
    img = B.bgzf(data)
    off, total = B.members_of(img)[0]
    m = B.parse(img[off + 18:off + total - 8])["matches"]
    assert any(d == period and ln > d for _, ln, d in m), "an overlapping match at the period is what the case is for"
    _inflate(gpu_ctx, img, data)


# ------------------------------------------------------------------------------------------------ stage: members assembled by hand
def _fixed_block(w, final, tokens, text):
    """tokens: a literal byte, or (length, distance); appends what they produce to `text`"""
    w.put(final, 1).put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            w.code(*B.fixed_code(t))
            text.append(t)
        else:
            ln, dist = t
            ls = max(k for k in range(29) if B.LEN_BASE[k] <= ln and (k < 28 or ln == 258))
            if ln == 258:
                ls = 28
            w.code(*B.fixed_code(257 + ls)).put(ln - B.LEN_BASE[ls], B.LEN_EXTRA[ls])
            ds = max(k for k in range(30) if B.DIST_BASE[k] <= dist)
            w.code(ds, 5).put(dist - B.DIST_BASE[ds], B.DIST_EXTRA[ds])
            for _ in range(ln):
                text.append(text[-dist])
    w.code(*B.fixed_code(256))


def test_distance_32768(gpu_ctx):
    head = _rand(11, 32768)
    text, w = bytearray(head), B.Bits()
    B.stored(w, 0, head)
    _fixed_block(w, 1, [(258, 32768)] * 127, text)
    deflate = w.bytes()
    p = B.parse(deflate)
    assert p["text"] == bytes(text) and all(d == 32768 and ln == 258 for _, ln, d in p["matches"]) and len(p["matches"]) == 127
    _inflate(gpu_ctx, B.member(deflate, bytes(text)) + B.EOF_MARKER, bytes(text), n_stored=1, n_fixed=2)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7])
def test_matches_across_the_ring_wrap_and_the_flush_borders(k, gpu_ctx):
    """a stored prefix that ends 100 bytes in front of 8192 k (k = 4: the ring's wrap at 32768), then matches whose destination crosses the border -- a
    non-overlapping one, one at distance 1, one at a distance just short of the history (its source wraps when the destination does not) -- then one whose SOURCE
    straddles the border; the stored prefix leaves exactly 8192 (k - 1) bytes flushed, so the first match also takes the unflushed bytes over the threshold"""
    border = 8192 * k
    head = _rand(20 + k, border - 100)
    text, w = bytearray(head), B.Bits()
    B.stored(w, 0, head)
    far = min(len(head), 32768) - 3
    _fixed_block(w, 1, [(258, 300), 7, (258, 1), (200, far), (258, 697), (150, 64), (258, 65), 9, (97, 63)], text)
    deflate = w.bytes()
    p = B.parse(deflate)
    assert p["text"] == bytes(text)
    assert any(pos < border < pos + ln for pos, ln, _ in p["matches"]) and any(pos - d < border < pos - d + ln for pos, ln, d in p["matches"])
    _inflate(gpu_ctx, B.member(deflate, bytes(text)) + B.EOF_MARKER, bytes(text), n_stored=1, n_fixed=2)


CL_LENS = [4] * 13 + [5] * 6  # a complete code-length code: 13 / 16 + 6 / 32


def _rle(lens):
    """the HLIT + HDIST lengths as ONE run-length coded sequence: [(code-length symbol, extra value, first index, count)]"""
    out, i = [], 0
    while i < len(lens):
        v, r = lens[i], 1
        while i + r < len(lens) and lens[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            n = min(r, 138)
            out.append((18, n - 11, i, n) if n >= 11 else (17, n - 3, i, n))
            i += n
            continue
        out.append((v, 0, i, 1))
        i += 1
        r -= 1
        while r >= 3:
            n = min(r, 6)
            out.append((16, n - 3, i, n))
            i += n
            r -= n
    return out


def _dynamic_block(w, final, ll, dl, tokens, text):
    runs = _rle(ll + dl)
    B.dynamic_header(w, final, len(ll), len(dl), CL_LENS, [(s, x) for s, x, _, _ in runs])
    lc, dc = B.canonical(ll), (B.canonical(dl) if any(dl) else {})
    for t in tokens:
        if isinstance(t, int):
            w.code(*lc[t])
            text.append(t)
        else:
            ln, dist = t
            ls = max(k for k in range(29) if B.LEN_BASE[k] <= ln)
            w.code(*lc[257 + ls]).put(ln - B.LEN_BASE[ls], B.LEN_EXTRA[ls])
            ds = max(k for k in range(30) if B.DIST_BASE[k] <= dist)
            w.code(*dc[ds]).put(dist - B.DIST_BASE[ds], B.DIST_EXTRA[ds])
            for _ in range(ln):
                text.append(text[-dist])
    w.code(*lc[256])
    return runs


def _hand_dynamic(what):
    text, w = bytearray(), B.Bits()
    if what == "codes_of_15_bits":  # literals 65 .. 78 with codes of 1 .. 14 bits, literal 79 and the end of block with 15: complete; no distance code at all
        ll = [0] * 257
        for k in range(14):
            ll[65 + k] = k + 1
        ll[79] = ll[256] = 15
        runs = _dynamic_block(w, 1, ll, [0], [65, 79, 70, 78, 79, 66, 77, 79] * 40, text)
    elif what == "repeat_across_hlit_and_hdist":  # ... 3 at 256, then `repeat 6 times`: 257, 258, 259 and the distance lengths 0, 1, 2
        ll = [0] * 260
        ll[65] = 1
        ll[256] = ll[257] = ll[258] = ll[259] = 3
        runs = _dynamic_block(w, 1, ll, [3] * 8, [65, 65, 65, (5, 1), 65, (4, 3), (3, 13), 65, (5, 16)] * 30, text)
        assert any(s == 16 and i < 260 < i + n for s, _, i, n in runs), "the run was supposed to cross from the HLIT lengths into the HDIST lengths"
    elif what == "single_distance_code":  # one distance code of one bit: an incomplete code that is allowed
        ll = [0] * 258
        ll[65] = ll[66] = 2
        ll[256] = ll[257] = 2
        runs = _dynamic_block(w, 1, ll, [1], [65, 66, (3, 1), 65, (3, 1), (3, 1), 66] * 50, text)
    elif what == "no_distance_code_literals_only":
        ll = [0] * 257
        ll[10] = ll[65] = ll[67] = ll[256] = 2
        runs = _dynamic_block(w, 1, ll, [0], [65, 67, 67, 10] * 100, text)
    else:
        raise KeyError(what)
    return w.bytes(), bytes(text)


@pytest.mark.parametrize("what", ["codes_of_15_bits", "repeat_across_hlit_and_hdist", "single_distance_code", "no_distance_code_literals_only"])
def test_hand_assembled_dynamic_blocks(what, gpu_ctx):
    deflate, text = _hand_dynamic(what)
    assert zlib.decompress(deflate, -15) == text and len(text) > 100, "zlib must agree that the block is valid"
    if what == "codes_of_15_bits":
        assert B.parse(deflate)["max_code_len"] == 15
    _inflate(gpu_ctx, B.member(deflate, text) + B.EOF_MARKER, text, n_dynamic=1, n_fixed=1, n_stored=0)


def test_bc_behind_another_subfield(gpu_ctx):
    data = _texty(12, 9000)
    img = B.bgzf(data, member_size=3000, extra_before=B.subfield(b"XY", b"abcde") + B.subfield(b"BC", b"three"))  # (a `BC` of another length is not the one)
    _inflate(gpu_ctx, img, data, n_members=4)


@pytest.fixture(scope="module")
def paf(tmpdir_s):
    return R.pafgen(os.path.join(tmpdir_s, "bgzf.paf"), 3000, 38000, 31)


def test_paf_text_whose_lines_straddle_members(paf, gpu_ctx):
    data = open(paf, "rb").read()
    assert 1500000 < len(data) < 3000000
    img = B.bgzf(data)
    assert all(data[i - 1:i] != b"\n" for i in range(65280, len(data), 65280))
    _inflate(gpu_ctx, img, data, n_members=(len(data) + 65279) // 65280 + 1, n_empty=1, **_blocks(img))


def test_load_leaves_the_context_as_the_plain_loaders_do(paf, gpu_ctx):
    """target PAF: the parse of the inflated text counts what the parse of the plain text counts; target FASTX: the index of the inflated reads file"""
    data = open(paf, "rb").read()[:400000]
    data = data[:data.rfind(b"\n") + 1]
    L = ma.lib()
    infos = []
    for load in (lambda: ma._chk(L.mahip_paf_load_mem(gpu_ctx.h, data, len(data)), "paf_load_mem"), lambda: gpu_ctx.bgzf_load(B.bgzf(data), "paf")):
        r = load()
        assert r is None or (r["reason"] == "OK" and r["reader"] == "device")
        pi = ma.PafInfo()
        ma._chk(L.mahip_paf_parse_excl(gpu_ctx.h, 2000, 100, 1, 0, 0, 0.0, ma.C.byref(pi)), "paf_parse")
        infos.append((pi.n_lines, pi.n_records, pi.n_hits, pi.n_seq, pi.name_bytes))
        ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")
    assert infos[0] == infos[1] and infos[0][0] == data.count(b"\n")
    fq = b"".join(b"@r%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % k for k in range(3000))
    assert gpu_ctx.bgzf_load(B.bgzf(fq, member_size=5000), "fastx")["reason"] == "OK"
    fi = gpu_ctx.fastx_index()
    assert fi["regular"] and fi["n_records"] == 3000 and fi["format"] == "fastq"
    gpu_ctx.fastx_release()
    assert gpu_ctx.bgzf_last()["reader"] == "device"


# ------------------------------------------------------------------------------------------------ refusal
def _lits(n=200, seed=3):
    text, w = bytearray(), B.Bits()
    _fixed_block(w, 1, [int(x) for x in np.random.RandomState(seed).randint(32, 127, n)], text)
    return w.bytes(), bytes(text)


def _refusals():
    good = _texty(40, 5000)
    first = B.bgzf(good, eof=False)  # one good member in front: the bad one is member 1
    out = {}
    out["block_type_3"] = (first + B.member(B.Bits().put(1, 1).put(3, 2).bytes(), b"") + B.EOF_MARKER, "BAD_BTYPE", 1)
    w = B.Bits()
    B.stored(w, 1, b"stored bytes", nlen=0x1234)
    out["len_against_nlen"] = (first + B.member(w.bytes(), b"stored bytes") + B.EOF_MARKER, "STORED_LEN", 1)
    ll = [0] * 257
    ll[65] = ll[66] = ll[256] = 1  # three codes of one bit
    w = B.Bits()
    B.dynamic_header(w, 1, 257, 1, CL_LENS, [(s, x) for s, x, _, _ in _rle(ll + [0])])
    out["oversubscribed_lengths"] = (first + B.member(w.bytes() + b"\0\0\0\0", b"") + B.EOF_MARKER, "BAD_LENGTHS", 1)
    text, w = bytearray(b"a"), B.Bits()
    w.put(1, 1).put(1, 2).code(*B.fixed_code(97)).code(*B.fixed_code(257)).code(1, 5).code(*B.fixed_code(256))  # literal, then length 3 at distance 2
    out["distance_before_the_member"] = (first + B.member(w.bytes(), b"abab") + B.EOF_MARKER, "DIST_TOO_FAR", 1)
    d, t = _lits()
    out["one_symbol_too_many"] = (first + B.member(d, t, isize=len(t) - 1) + B.EOF_MARKER, "OUT_OVERFLOW", 1)
    out["deflate_bytes_cut_short"] = (first + B.member(d[:-3], t) + B.EOF_MARKER, "IN_EXHAUSTED", 1)
    out["isize_too_large_by_one"] = (first + B.member(d, t, isize=len(t) + 1) + B.EOF_MARKER, "OUT_SHORT", 1)
    w = B.Bits()
    B.stored(w, 1, t)
    m = B.member(w.bytes(), t)
    out["flipped_bit_under_a_stored_block"] = (first + B.flip_bit(m, 18 + 5 + 77, 3) + B.EOF_MARKER, "CRC", 1)
    out["first_bad_member_is_the_first_of_two"] = (B.member(d, t, isize=len(t) + 1) + first + B.flip_bit(m, 18 + 5 + 7, 1) + B.EOF_MARKER, "OUT_SHORT", 0)
    out["second_member_without_bc"] = (first + B.member(d, t, bc=False, extra_before=B.subfield(b"XY", b"12")) + B.EOF_MARKER, "NO_BC", 1)
    out["second_member_without_extra_field"] = (first + B.member(d, t, flg=0) + B.EOF_MARKER, "NO_BC", 1)
    out["bsize_past_the_end"] = (first + B.member(d, t, bsize=12 + 6 + len(d) + 8 + 40 - 1), "PAST_END", 1)
    out["bsize_smaller_than_the_header"] = (first + B.member(d, t, bsize=20), "PAST_END", 1)
    out["trailing_garbage"] = (first + B.EOF_MARKER + b"garbage behind the chain", "TRAILING", 2)
    out["trailing_short_garbage"] = (first + B.EOF_MARKER + b"\x1f\x8b\x08", "TRAILING", 2)
    out["fname_flag"] = (first + B.member(d, t, flg=4 | 8) + B.EOF_MARKER, "BAD_FLG", 1)
    out["isize_above_64k"] = (first + B.member(d, t, isize=65537) + B.EOF_MARKER, "ISIZE", 1)
    out["plain_gzip"] = (gzip.compress(good), "NOT_BGZF", 0)
    out["not_gzip_at_all"] = (b"\x1f\x8b but nothing like a member", "NOT_BGZF", 0)
    return out


REFUSALS = _refusals()


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusal_by_name_and_member(what, gpu_ctx):
    image, reason, member = REFUSALS[what]
    if ma.BGZF_REASONS.index("BAD_BTYPE") <= ma.BGZF_REASONS.index(reason) <= ma.BGZF_REASONS.index("CRC"):
        with pytest.raises(Exception):  # what the kernel refuses zlib refuses too
            gzip.decompress(image)
    text, info = gpu_ctx.bgzf_inflate(image)
    assert text is None and (info["reason"], info["first_bad_member"], info["reader"]) == (reason, member, "host"), info
    assert gpu_ctx.bgzf_last() == info
    for target in ("paf", "fastx"):  # nothing stays loaded
        assert gpu_ctx.bgzf_load(image, target)["reason"] == reason
    pi = ma.PafInfo()
    assert ma.lib().mahip_paf_parse_excl(gpu_ctx.h, 2000, 100, 1, 0, 0, 0.0, ma.C.byref(pi)) != 0 and b"no text loaded" in ma.lib().mahip_strerror()
    fi = ma.FastxInfo()
    assert ma.lib().mahip_fastx_index(gpu_ctx.h, ma.C.byref(fi)) != 0


def test_empty_reads_file_is_left_to_the_host(gpu_ctx):
    assert gpu_ctx.bgzf_load(B.EOF_MARKER, "fastx")["reason"] == "EMPTY"
    assert gpu_ctx.bgzf_load(B.EOF_MARKER, "paf")["reason"] == "OK"
    ma._chk(ma.lib().mahip_paf_release(gpu_ctx.h), "paf_release")


# ------------------------------------------------------------------------------------------------ end to end
needs_ref = pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def e2e(tmpdir_s):
    paf = R.pafgen(os.path.join(tmpdir_s, "bgzf_e2e.paf"), 400, 12000, 23, ["-L", "uniform"])
    exe = os.path.join(os.path.dirname(ma.PAFGEN_PATH), "readgen")
    fq = os.path.join(tmpdir_s, "bgzf_e2e.fq")
    subprocess.run([exe, "-q", "-s", "7", "-o", fq, paf], check=True, stderr=subprocess.DEVNULL)
    out = dict(paf=paf, fq=fq)
    for k in ("paf", "fq"):
        data = open(out[k], "rb").read()
        out[k + "_gz"] = out[k] + ".gz"
        with open(out[k + "_gz"], "wb") as f:
            f.write(B.bgzf(data, member_size=20011))  # lines and records straddle the members
    return out


def _cli(binary, args, bgzf_host=False):
    env = dict(os.environ, MA_PIPE_TIMING="1")
    env.pop("MA_BGZF_HOST", None)
    env.pop("MA_FASTX_HOST", None)
    if bgzf_host:
        env["MA_BGZF_HOST"] = "1"
    r = subprocess.run([binary] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    log = r.stderr.decode(errors="replace")
    assert r.returncode == 0, log[-2000:]
    readers = re.findall(r"^\[T::bgzf\] reader=(\w+)", log, re.M)
    useq = re.findall(r"^\[T::ug_seq\] reader=(\w+)", log, re.M)
    return r.stdout, readers, useq, log


@pytest.mark.parametrize("with_reads", [False, True], ids=["paf", "paf_and_reads"])
def test_cli_on_bgzipped_files(with_reads, e2e):
    """fails without the feature: no `[T::bgzf] reader=device` line, and the reads file is NOT_PLAIN"""
    plain = (["-f", e2e["fq"]] if with_reads else []) + [e2e["paf"]]
    comp = (["-f", e2e["fq_gz"]] if with_reads else []) + [e2e["paf_gz"]]
    want, readers, useq, _ = _cli(ma.CLI_PATH, plain)
    assert readers == [] and useq == (["device"] if with_reads else []) and b"\nS\t" in b"\n" + want
    binaries = [ma.CLI_PATH] + ([R.DROPIN_BIN] if os.path.exists(R.DROPIN_BIN) else [])
    for binary in binaries:
        out, readers, useq, log = _cli(binary, comp)
        assert out == want, os.path.basename(binary) + ": differs from the run on the plain files"
        assert readers == ["device"] * (2 if with_reads else 1), log[-2000:]
        assert useq == (["device"] if with_reads else [])
        out, readers, useq, log = _cli(binary, comp, bgzf_host=True)
        assert out == want and readers == [] and useq == (["host"] if with_reads else [])
        assert ("reason=%d " % ma.FASTX_REASONS.index("NOT_PLAIN") in log) == with_reads
    if R.have_ref():
        r = subprocess.run([R.REF_BIN] + comp, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0 and r.stdout == want, "differs from the reference on the compressed files"


def test_ingest_of_a_bgzipped_paf_reports_the_device_reader(e2e, gpu_ctx):
    a = ma.GpuIngest(gpu_ctx, e2e["paf"])
    hits, names = a.hits, a.names()
    a.close()
    b = ma.GpuIngest(gpu_ctx, e2e["paf_gz"])
    last = gpu_ctx.bgzf_last()
    assert last["reader"] == "device" and last["reason"] == "OK" and last["text_bytes"] == os.path.getsize(e2e["paf"]) and last["n_empty"] == 1
    assert b.names() == names and np.array_equal(b.hits, hits)
    b.close()


def test_corrupted_member_falls_back_to_zlib(e2e, tmpdir_s):
    """a member with a flaw zlib does not mind (a BSIZE that claims 40 bytes too many: the chain breaks for the walk, zlib never reads the field): the host road, the same output"""
    img = open(e2e["paf_gz"], "rb").read()
    mem = B.members_of(img)
    off, total = mem[3]
    bad = os.path.join(tmpdir_s, "bgzf_bad.paf.gz")
    with open(bad, "wb") as f:
        f.write(B.set_u16(img, off + 16, total - 1 + 40))
    want, _, _, _ = _cli(ma.CLI_PATH, [e2e["paf_gz"]], bgzf_host=True)
    out, readers, _, log = _cli(ma.CLI_PATH, [bad])
    assert out == want and readers == ["host"], log[-1500:]
    assert re.search(r"^\[T::bgzf\] reader=host reason=\d+ \(.*\) member=[34]$", log, re.M), log[-1500:]


def test_corrupted_payload_is_an_error_on_both_roads(e2e, tmpdir_s):
    """one flipped bit in a member's deflate bytes: the device refuses (status or CRC), zlib then reads what it reads -- the output is MA_BGZF_HOST=1's"""
    img = open(e2e["paf_gz"], "rb").read()
    off, total = B.members_of(img)[2]
    bad = os.path.join(tmpdir_s, "bgzf_flip.paf.gz")
    with open(bad, "wb") as f:
        f.write(B.flip_bit(img, off + total // 2, 2))

    def run(host):
        env = dict(os.environ, MA_PIPE_TIMING="1")
        env.pop("MA_BGZF_HOST", None)
        if host:
            env["MA_BGZF_HOST"] = "1"
        r = subprocess.run([ma.CLI_PATH, bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        return r.returncode, r.stdout, r.stderr.decode(errors="replace")
    rc_h, out_h, _ = run(True)
    rc_d, out_d, log = run(False)
    assert (rc_d, out_d) == (rc_h, out_h)
    assert re.search(r"^\[T::bgzf\] reader=host reason=\d+ .* member=2$", log, re.M), log[-1500:]


def test_plain_gzip_still_takes_the_host_road(e2e, tmpdir_s):
    gz = os.path.join(tmpdir_s, "bgzf_plain.paf.gz")
    with gzip.open(gz, "wb") as f:
        f.write(open(e2e["paf"], "rb").read())
    want, _, _, _ = _cli(ma.CLI_PATH, [e2e["paf"]])
    out, readers, _, log = _cli(ma.CLI_PATH, [gz])
    assert out == want and readers == ["host"] and "(not a BGZF file) member=0" in log
