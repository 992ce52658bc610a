"""Concatenated gzip members inflated on the device (csrc/xfer.hip: k_gz_member_scan / k_gz_heads, the chain over members, per-member history, windows and CRC;
headers and trailers: host/ingest_gpu.c), and the -f reads file on that road.

Stage: Ctx.gzip_inflate(..., members=True) against tests/gzipmembersmodel.py and zlib.  The rule everywhere: EITHER the reason is OK and the text equals
gzip.decompress of the image, OR the reason is not OK, there is no text and nothing stays loaded.  On OK every member row (comp_off, hdr_len, text_off, text_len,
crc, isize, n_items) and the candidate counts are EQUAL to the model's.  chunk = 1024 and 4096, texts of tens of KiB.

Chunks, bits and rows count from the first bit behind the FIRST member's header, so padding that header moves nothing against the chunk grid: the placement
cases pad the first member's deflate stream with a stored block instead.

Not covered at test size: texts above 4 GiB (64-bit offsets, the per-member ISIZE wrap) -- DESIGN 5."""
import gzip
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import bgzfmodel as B
import gzipmembersmodel as M
import gzipmodel as G
import miniasm_amd as ma
import refapi as R
from test_gpu_gzip import S, _in_use, _rand, _texty

pytestmark = pytest.mark.gpu

C = 1024


def _check(ctx, image, chunk=C, false_candidates=False):
    """accepted: the text is zlib's, the member rows and the candidate counts are the model's"""
    m = M.model(image, chunk)
    assert gzip.decompress(image) == m["text"], "the image is not what the test thinks"
    text, info = ctx.gzip_inflate(image, chunk, members=True)
    mi, rows = ctx.gzip_members_info(), ctx.gzip_members()
    assert info["reason"] == "OK" and info["reader"] == "device" and info["first_bad_item"] == -1 and mi["bad_member"] == -1, (info, mi)
    assert text == m["text"] and info["text_bytes"] == len(text)
    assert (mi["n_members"], mi["n_candidates"], mi["n_heads"]) == (len(m["rows"]), len(m["candidates"]), len(m["heads"])), (mi, m["candidates"], m["heads"])
    if not false_candidates:
        assert mi["n_candidates"] == mi["n_members"] - 1
    assert len(rows) == len(m["rows"])
    for k, (a, b) in enumerate(zip(rows, m["rows"])):
        assert a == b, (k, a, b)
    assert info["n_items"] == sum(r["n_items"] for r in rows)
    return info, mi, m


def _refused(ctx, image, reason, bad_member, chunk=C):
    before = _in_use(ctx)
    text, info = ctx.gzip_inflate(image, chunk, members=True)
    mi = ctx.gzip_members_info()
    assert text is None and (info["reason"], info["reader"]) == (reason, "host"), info
    assert mi["bad_member"] == bad_member, mi
    for target in ("paf", "fastx"):
        assert ctx.gzip_load(image, target, chunk, members=True)["reason"] == reason
    pi = ma.PafInfo()
    assert ma.lib().mahip_paf_parse_excl(ctx.h, 2000, 100, 1, 0, 0, 0.0, ma.C.byref(pi)) != 0 and b"no text loaded" in ma.lib().mahip_strerror()
    fi = ma.FastxInfo()
    assert ma.lib().mahip_fastx_index(ctx.h, ma.C.byref(fi)) != 0
    assert _in_use(ctx) == before, "device memory of the refused load is still held"
    return info, mi


EMPTY = G.gz(b"")  # what `gzip < /dev/null` writes: one final fixed block


# ------------------------------------------------------------------------------------------------ member counts
@pytest.mark.parametrize("n,chunk", [(2, 1024), (3, 1024), (3, 4096), (65, 1024)])
def test_member_counts(n, chunk, gpu_ctx):
    """65: more candidates than one wave of k_gz_heads' workgroups takes in a round (4 a workgroup), and more than 64"""
    image = M.cat(*[G.gz(_texty(100 + k, 30000 if n < 10 else 900 + 37 * k), 1 + k % 9, 1 + k % 8) for k in range(n)])
    info, mi, _ = _check(gpu_ctx, image, chunk)
    assert mi["n_members"] == n and mi["n_heads"] == n - 1


# ------------------------------------------------------------------------------------------------ a member's header against the chunk grid
@pytest.mark.parametrize("where,at", [("first_byte_of_a_chunk", 2 * C), ("last_byte_of_a_chunk", 2 * C - 1), ("straddles_a_border", 2 * C - 5), ("behind_a_trailer_that_straddles", 2 * C + 3)])
def test_member_header_against_the_chunk_border(where, at, gpu_ctx):
    s = S(40)
    s.dyn(s.lits(200) + [(100, 50)])
    s.pad_to_byte(at - 8 - 3)  # then a final fixed block of one 8-bit literal and the end-of-block: 3 + 8 + 7 = 18 bits from a whole byte, 3 bytes; and the trailer
    s.fix([65], final=1)
    first = s.image()
    assert len(first) - 10 == at, (len(first) - 10, at)  # the second member's header starts `at` bytes behind the first header
    second = G.gz(_texty(41, 20000), 1, 1, head=G.header(fname=b"second"))
    info, mi, m = _check(gpu_ctx, M.cat(first, second, G.gz(b"tail\n")))
    assert m["rows"][1]["comp_off"] - 10 == at and mi["n_members"] == 3


def test_several_whole_members_inside_one_chunk(gpu_ctx):
    """head items that start and end in the same chunk"""
    image = M.cat(*[G.gz(b"line %d\tof a tiny member\n" % k * 3, 6) for k in range(12)])
    assert len(image) < 4096
    info, mi, _ = _check(gpu_ctx, image, 4096)
    assert info["n_chunks"] == 1 and info["n_items"] == 12 and mi["n_members"] == 12


@pytest.mark.parametrize("where", ["first", "middle", "last", "twice_in_a_row", "only_empty_ones"])
def test_empty_member(where, gpu_ctx):
    a, b = G.gz(_texty(50, 20000), 1, 2), G.gz(_texty(51, 9000), 6, 8)
    image = dict(first=M.cat(EMPTY, a, b), middle=M.cat(a, EMPTY, b), last=M.cat(a, b, EMPTY), twice_in_a_row=M.cat(a, EMPTY, EMPTY, b), only_empty_ones=M.cat(EMPTY, EMPTY))[where]
    assert len(EMPTY) == 20
    info, mi, m = _check(gpu_ctx, image)
    assert [r["text_len"] for r in m["rows"]].count(0) == dict(twice_in_a_row=2, only_empty_ones=2).get(where, 1)


@pytest.mark.parametrize("kind", ["stored", "fixed", "dynamic"])
def test_first_block_of_a_later_member(kind, gpu_ctx):
    s = S(60)
    toks = s.lits(300) + [(200, 300), (258, 1)]
    if kind == "stored":
        s.sto(s.rs.bytes(5000))
    elif kind == "fixed":
        s.fix(toks)
    else:
        s.dyn(toks)
    s.dyn(s.lits(100) + [(100, 90)], final=1)
    first = G.gz(_texty(61, 25000), 1, 1)
    _check(gpu_ctx, M.cat(first, s.image(), G.gz(_rand(62, 7000), 0)))  # (the third: zlib's own level 0)


HEADS = dict(fname=G.header(fname=b"reads.paf"), extra=G.header(extra=B.subfield(b"XY", b"abcde") + B.subfield(b"BC", b"three")), comment=G.header(comment=b"a comment"),
             hcrc=G.header(hcrc=True), everything=G.header(fname=b"n", comment=b"c", extra=b"", hcrc=True, mtime=7, ftext=True))


@pytest.mark.parametrize("what", list(HEADS))
def test_header_fields_of_later_members_are_skipped(what, gpu_ctx):
    image = M.cat(G.gz(_texty(70, 15000), 1, 1), G.gz(_texty(71, 15000), 1, 1, head=HEADS[what]), G.gz(_texty(72, 3000), 6, 8, head=HEADS[what]))
    info, mi, m = _check(gpu_ctx, image)
    assert m["rows"][1]["hdr_len"] == len(HEADS[what])


# ------------------------------------------------------------------------------------------------ false candidates
def _with_stored(seed, inside):
    """a member whose middle block is stored and holds `inside`"""
    s = S(seed)
    s.dyn(s.lits(150) + [(60, 20)])
    s.sto(s.rs.bytes(700).replace(b"\x1f", b"\x20") + inside + s.rs.bytes(900).replace(b"\x1f", b"\x20"))
    s.dyn(s.lits(80), final=1)
    return s.image()


@pytest.mark.parametrize("where", ["first_member", "last_member", "with_a_header_that_parses"])
def test_false_candidate_inside_a_stored_block(where, gpu_ctx):
    magic = b"\x1f\x8b\x08\x00"
    inside = (magic + bytes(6) + b"xyz" + magic) if where != "with_a_header_that_parses" else 2 * G.gz(b"not a member: bytes of a stored block\n")
    fake, good = _with_stored(80, inside), G.gz(_texty(81, 12000), 1, 1)
    image = M.cat(good, good, fake) if where == "last_member" else M.cat(fake, good, good)
    info, mi, m = _check(gpu_ctx, image, false_candidates=True)
    assert mi["n_candidates"] > mi["n_members"] == 3 and mi["n_heads"] > 2  # (FLG 0 and 18 bytes behind it: the false ones parse as headers too, and get a head row)


def test_short_second_member_reaches_back_to_its_own_first_byte(gpu_ctx):
    first = G.gz(_texty(90, 50000), 1, 1)
    s = S(91)
    s.dyn(s.lits(500))
    n = 500
    toks = []
    while n < 20000:  # every match starts at the member's first byte
        ln = min(258, n)
        toks.append((ln, n))
        n += ln
    s.dyn(toks)
    s.pad_to_byte(((s.bit() >> 3) // C + 1) * C + 7)  # a further item: its window holds the member's first byte somewhere in the middle
    s.dyn([(258, len(s.text)), (100, len(s.text) + 258)] + s.lits(5), final=1)
    assert len(s.text) < 32768
    info, mi, m = _check(gpu_ctx, M.cat(first, s.image()))
    assert m["rows"][1]["n_items"] >= 2 and m["rows"][0]["text_len"] > 32768


# ------------------------------------------------------------------------------------------------ refusals
def _three():
    texts = [_texty(200 + k, 20000) for k in range(3)]
    return texts, [G.gz(t, 1, 1 + k) for k, t in enumerate(texts)]


def test_trailing_bytes_behind_the_last_member(gpu_ctx):
    _, mem = _three()
    _refused(gpu_ctx, M.cat(*mem) + b"trailing", "MULTI_MEMBER", 2)
    _refused(gpu_ctx, M.cat(*mem) + b"\x1f\x8b\x08\x00 short", "MULTI_MEMBER", 2)


def test_truncated_last_member(gpu_ctx):
    """the last 8 bytes that are left are read as the trailer; the stream in front of them ends early"""
    _, mem = _three()
    _refused(gpu_ctx, M.cat(mem[0], mem[1], G.gz(_texty(203, 400), 6, 8)[:-40]), "IN_EXHAUSTED", 2)


@pytest.mark.parametrize("what", ["crc", "isize"])
def test_wrong_trailer_in_member_2_of_3(what, gpu_ctx):
    texts, mem = _three()
    bad = B.set_u32(mem[1], len(mem[1]) - 8, zlib.crc32(texts[1]) ^ 0x10) if what == "crc" else B.set_u32(mem[1], len(mem[1]) - 4, len(texts[1]) + 1)
    info, mi = _refused(gpu_ctx, M.cat(mem[0], bad, mem[2]), what.upper(), 1)
    assert mi["n_members"] == (3 if what == "crc" else 2)  # (ISIZE is seen where the chain closes the member, the CRC when all the text is there)


def test_second_member_whose_first_token_is_a_match(gpu_ctx):
    """a distance may not reach in front of its own member, although the first member's text lies right in front of it: zlib fails on it too"""
    s = S(95)
    s.fix([(3, 1)], final=1)
    image = M.cat(G.gz(_texty(96, 9000), 1, 1), s.image())
    with pytest.raises(zlib.error):
        gzip.decompress(image)
    info, mi = _refused(gpu_ctx, image, "DIST_TOO_FAR", 1)
    assert info["first_bad_item"] == info["n_items"] - 1


def test_candidate_capacity_overflow(gpu_ctx, monkeypatch):
    image = M.cat(*[G.gz(_texty(97 + k, 3000), 1, 1) for k in range(5)])
    monkeypatch.setenv("MA_GZIP_CAND_CAP", "4")
    info, mi, _ = _check(gpu_ctx, image)
    assert mi["cand_cap"] == 4 == mi["n_candidates"]
    monkeypatch.setenv("MA_GZIP_CAND_CAP", "3")
    info, mi = _refused(gpu_ctx, image, "TOO_MANY_CANDIDATES", -1)
    assert mi["cand_cap"] == 3 and mi["n_candidates"] == 4 and info["n_items"] == 0


# ------------------------------------------------------------------------------------------------ further checks
def test_one_flipped_bit_is_never_a_wrong_text(gpu_ctx):
    texts, mem = _three()
    good, data = M.cat(*mem), b"".join(texts)
    rs = np.random.RandomState(98)
    seen = set()
    for _ in range(24):
        byte, bit = int(rs.randint(10, len(good))), int(rs.randint(0, 8))
        text, info = gpu_ctx.gzip_inflate(B.flip_bit(good, byte, bit), C, members=True)
        assert info["reason"] != "OK" or text == data, (byte, bit, info)
        assert (text is None) == (info["reason"] != "OK")
        seen.add(info["reason"])
    assert seen - {"OK"}, seen


def test_one_member_entry_points_still_refuse_a_second_member(gpu_ctx):
    good = G.gz(_texty(99, 20000), 1, 1)
    n = G.model(good, C)["n_items"]
    text, info = gpu_ctx.gzip_inflate(good + good, C)
    assert text is None and (info["reason"], info["first_bad_item"], info["reader"]) == ("MULTI_MEMBER", n - 1, "host"), info
    assert gpu_ctx.gzip_members_info()["n_members"] == 0 and gpu_ctx.gzip_members() == []
    for target in ("paf", "fastx"):
        assert gpu_ctx.gzip_load(good + good, target, C)["reason"] == "MULTI_MEMBER"
    text, info = gpu_ctx.gzip_inflate(good, C, members=True)  # one member through the members form: the same text, one member row
    assert text == gzip.decompress(good) and gpu_ctx.gzip_members_info()["n_members"] == 1 and info["n_items"] == n


# ------------------------------------------------------------------------------------------------ targets
def _cut(data, cuts, **kw):
    """the text as gzip members cut at the given bytes"""
    edges = [0] + list(cuts) + [len(data)]
    return M.cat(*[G.gz(data[a:b], 1, 8, **kw) for a, b in zip(edges, edges[1:])])


@pytest.fixture(scope="module")
def paf(tmpdir_s):
    return R.pafgen(os.path.join(tmpdir_s, "gzm.paf"), 400, 12000, 23, ["-L", "uniform"])


def test_load_for_the_paf_reader_gives_the_plain_files_parse(paf, gpu_ctx):
    data = open(paf, "rb").read()
    L = ma.lib()
    infos = []
    for load in (lambda: ma._chk(L.mahip_paf_load_mem(gpu_ctx.h, data, len(data)), "paf_load_mem"),
                 lambda: gpu_ctx.gzip_load(_cut(data, [len(data) // 3 + 5, 2 * len(data) // 3 + 11]), "paf", 4096, members=True)):
        r = load()
        assert r is None or (r["reason"] == "OK" and r["reader"] == "device" and r["text_bytes"] == len(data)), r
        pi = ma.PafInfo()
        ma._chk(L.mahip_paf_parse_excl(gpu_ctx.h, 2000, 100, 1, 0, 0, 0.0, ma.C.byref(pi)), "paf_parse")
        infos.append((pi.n_lines, pi.n_records, pi.n_hits, pi.n_seq, pi.name_bytes))
        ma._chk(L.mahip_paf_release(gpu_ctx.h), "paf_release")
    assert infos[0] == infos[1] and infos[0][0] == data.count(b"\n") and gpu_ctx.gzip_members_info()["n_members"] == 3


def test_load_for_the_reads_file_reader_gives_the_plain_loads_index(gpu_ctx):
    fq = b"".join(b"@r%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % k for k in range(3000))
    L = ma.lib()
    ma._chk(L.mahip_fastx_load_mem(gpu_ctx.h, fq, len(fq)), "fastx_load_mem")
    want = gpu_ctx.fastx_index()
    gpu_ctx.fastx_release()
    r = gpu_ctx.gzip_load(_cut(fq, [30007, 60011]), "fastx", C, members=True)
    assert r["reason"] == "OK" and gpu_ctx.gzip_members_info()["n_members"] == 3, r
    fi = gpu_ctx.fastx_index()
    gpu_ctx.fastx_release()
    assert fi == want and fi["n_records"] == 3000 and fi["format"] == "fastq"
    assert gpu_ctx.gzip_load(M.cat(EMPTY, EMPTY), "fastx", C, members=True)["reason"] == "EMPTY"


# ------------------------------------------------------------------------------------------------ end to end
def _cli(binary, args, device, chunk=4096):
    env = dict(os.environ, MA_PIPE_TIMING="1", MA_GZIP_DEVICE="1" if device else "0", MA_GZIP_CHUNK=str(chunk))
    for k in ("MA_BGZF_HOST", "MA_FASTX_HOST", "MA_FASTX_STREAM", "MA_GZIP_CAND_CAP"):
        env.pop(k, None)
    r = subprocess.run([binary] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    log = r.stderr.decode(errors="replace")
    assert r.returncode == 0, log[-2000:]
    return (r.stdout, log, re.findall(r"^\[T::gzip\] reader=(\w+) reason=(\d+) ", log, re.M), re.findall(r"^\[T::gzip_members\] members=(\d+) candidates=(\d+) ", log, re.M),
            re.findall(r"^\[T::ug_seq\] reader=(\w+)", log, re.M))


@pytest.fixture(scope="module")
def e2e(paf, tmpdir_s):
    exe = os.path.join(os.path.dirname(ma.PAFGEN_PATH), "readgen")
    fq = os.path.join(tmpdir_s, "gzm.fq")
    subprocess.run([exe, "-q", "-s", "7", "-o", fq, paf], check=True, stderr=subprocess.DEVNULL)
    out = dict(paf=paf, fq=fq)
    data = open(paf, "rb").read()
    out["paf_gz"] = paf + ".cat.gz"
    with open(out["paf_gz"], "wb") as f:
        f.write(_cut(data, [len(data) // 3 + 17, 2 * len(data) // 3 + 5], head=G.header(fname=b"part.paf", mtime=1700000000)))  # arbitrary bytes of the text: lines straddle the members
    reads = open(fq, "rb").read()
    starts = [m.start() + 1 for m in re.finditer(rb"\n@[^\n]*\n[ACGTN]+\n\+", reads)]  # where a record begins
    a, b = starts[len(starts) // 3], starts[2 * len(starts) // 3]
    for name, cuts in (("records", [a, b]), ("mid_sequence", [reads.index(b"\n", a) + 40, reads.index(b"\n", b) + 77])):
        out["fq_gz_" + name] = fq + "." + name + ".gz"
        with open(out["fq_gz_" + name], "wb") as f:
            f.write(_cut(reads, cuts))
    return out


def test_cli_on_a_paf_of_three_concatenated_gzip_pieces(e2e):
    """fails without the feature: the reader is `host` (MULTI_MEMBER) and there is no `[T::gzip_members]` line"""
    want, _, lines, mlines, _ = _cli(ma.CLI_PATH, [e2e["paf"]], True)
    assert lines == [] and mlines == [] and b"\nS\t" in b"\n" + want
    for binary in [ma.CLI_PATH] + ([R.DROPIN_BIN] if os.path.exists(R.DROPIN_BIN) else []):
        out, log, lines, mlines, _ = _cli(binary, [e2e["paf_gz"]], True)
        assert out == want, os.path.basename(binary) + ": differs from the run on the plain file"
        assert lines == [("device", "0")] and len(mlines) == 1 and mlines[0][0] == "3", log[-2000:]
        out, log, lines, mlines, _ = _cli(binary, [e2e["paf_gz"]], False)
        assert out == want and [x[0] for x in lines] == ["host"] and mlines == [] and "reason=%d " % ma.GZIP_REASONS.index("FORCED") in log
    if R.have_ref():
        r = subprocess.run([R.REF_BIN, e2e["paf_gz"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0 and r.stdout == want, "differs from the reference on the compressed file"


@pytest.mark.parametrize("cut", ["records", "mid_sequence"])
def test_cli_on_a_reads_file_of_three_concatenated_gzip_pieces(cut, e2e):
    """fails without the feature: the reads file is NOT_PLAIN and the host reader runs"""
    want, _, _, _, useq = _cli(ma.CLI_PATH, ["-f", e2e["fq"], e2e["paf"]], True)
    assert useq == ["device"] and b"\nS\t" in b"\n" + want and re.search(rb"^S\t\S+\t[ACGT]", want, re.M)
    args = ["-f", e2e["fq_gz_" + cut], e2e["paf"]]
    for binary in [ma.CLI_PATH] + ([R.DROPIN_BIN] if os.path.exists(R.DROPIN_BIN) else []):
        out, log, lines, mlines, useq = _cli(binary, args, True)
        assert out == want, os.path.basename(binary) + ": differs from the run on the plain file"
        assert useq == ["device"] and lines == [("device", "0")] and len(mlines) == 1 and mlines[0][0] == "3", log[-2000:]
        out, log, lines, mlines, useq = _cli(binary, args, False)
        assert out == want and useq == ["host"] and lines == [] and mlines == [], log[-2000:]
        assert "reason=%d " % ma.FASTX_REASONS.index("NOT_PLAIN") in log
    if R.have_ref():
        r = subprocess.run([R.REF_BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0 and r.stdout == want, "differs from the reference on the compressed reads file"
