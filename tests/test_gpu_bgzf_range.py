"""A rank's own range of a bgzip-compressed overlap file (include/mahip.h: mahip_bgzf_load_fd_range, mahip_bgzf_range_mem, mahip_text_first_nl; csrc/xfer.hip:
k_text_first_nl next to k_bgzf_inflate / k_bgzf_crc), in one process without a communicator: the range is a function of the file, the rank and the world.

Expected values come from tests/bgzfmodel.py (the images), the plain bytes and the restatement below of the range rule and of the member rule -- never from the
code under test.  Every case asserts from the model that it has the shape it was written for.  Everything is an integer or a byte string: equality throughout.

THE RANGE RULE.  T = the inflated size, nom(g) = T g // W, beg(g) = ls(nom(g)), end(g) = ls(nom(g + 1)) with end(W - 1) = T and end >= beg; ls(a) = 0 for
a <= 0, T for a >= T, else the byte behind the first newline at a position >= a - 1, T when there is none.
THE MEMBER RULE.  first_member = the first member whose text ends behind byte max(nom(g) - 1, 0) (empty members in front of it are skipped; the member count
when there is none).  Inflated at first: from there through the member that holds byte nom(g + 1) - 1, and MAHIP_BGZF_RANGE_AHEAD members more (nothing when
nom(g + 1) = 0).  While a border's newline does not lie in the inflated text and the chain has not ended, a round inflates the next batch: AHEAD members the first
round of a load, twice as many each further one.  The bound the issue sets on n_members_inflated counts "the members that intersect [max(nom - 1, 0), end)":
here that is every member with a byte in the interval, and every EMPTY member that stands strictly inside it (between two members that are inflated it is
uploaded and checked with them; one AT the interval's first byte stands in front of first_member and is not counted).

The issue words case 1 as "member_size = 256, fixed 64-byte lines, so a newline is the last byte of every fourth member"; with those two numbers a newline is
the last byte of EVERY member (and of every fourth line).  The numbers are kept: what the case needs is a newline that ends a member.

Left out on purpose: texts above 4 GiB (the 64-bit out_off rebasing of the table rows is read, not run), and the RCCL transport with more than one rank (nothing
here needs a communicator; tests/test_gpu_bgzf_sharded.py runs the ranks over the shared-memory double)."""
import os
import struct

import numpy as np
import pytest

import bgzfmodel as B
import miniasm_amd as ma
import refapi as R
import stages as ST

pytestmark = pytest.mark.gpu

AHEAD = ma.BGZF_RANGE_AHEAD  # include/mahip.h: MAHIP_BGZF_RANGE_AHEAD
WAVES = 4                    # csrc/xfer.hip: BGZF_WAVES


# ------------------------------------------------------------------------------------------------ the model
def ls(text, a):
    T = len(text)
    if a <= 0:
        return 0
    if a >= T:
        return T
    k = text.find(b"\n", a - 1)
    return T if k < 0 else k + 1


def table(image):
    """[(out_off, isize)] of the chain"""
    out, off = [], 0
    for p, total in B.members_of(image):
        isize = struct.unpack_from("<I", image, p + total - 4)[0]
        out.append((off, isize))
        off += isize
    return out


def model(text, image, g, W):
    T, mem = len(text), table(image)
    n = len(mem)
    assert sum(i for _, i in mem) == T
    nb, ne = T * g // W, (T if g == W - 1 else T * (g + 1) // W)
    beg = ls(text, nb)
    end = max(T if g == W - 1 else ls(text, ne), beg)

    def member_of(byte):
        return next((m for m in range(n) if mem[m][0] + mem[m][1] > byte), n)

    lo = max(nb - 1, 0)
    first, hi, rounds, ext = member_of(lo), None, 0, 0
    if ne > 0:
        hi, batch = min(member_of(ne - 1) + 1 + AHEAD, n), AHEAD
        for a, searched in ((nb, nb > 0), (ne, g < W - 1 and ne < T)):
            if not searched:
                continue
            q = text.find(b"\n", a - 1)
            while (q < 0 or q >= (mem[hi][0] if hi < n else T)) and hi < n:
                step = min(batch, n - hi)
                hi, ext, batch, rounds = hi + step, ext + step, batch * 2, rounds + 1
    inter = sum(1 for o, i in mem if (i and o < end and o + i > lo) or (not i and lo < o < end))
    return dict(T=T, nom=nb, nom_e=ne, beg=beg, end=end, first=first, hi=hi, rounds=rounds, bound=(inter + AHEAD + ext) if ne > 0 else 0, n=n)


def check_world(ctx, text, image, W):
    """every rank of one world against the model; -> [(model, range dict)]"""
    out, at = [], 0
    for g in range(W):
        m = model(text, image, g, W)
        got, rg, info = ctx.bgzf_range(image, g, W)
        assert info["reason"] == "OK" and info["reader"] == "device" and info["first_bad_member"] == -1, (g, W, info)
        assert (rg["text_bytes"], rg["beg"], rg["end"]) == (m["T"], m["beg"], m["end"]), (g, W, rg, m)
        assert got == text[m["beg"]:m["end"]], (g, W)
        assert rg["beg"] == at, "the ranges of a world tile the text"
        at = rg["end"]
        assert rg["first_member"] == m["first"], (g, W, rg, m)
        assert rg["n_rounds"] == m["rounds"], (g, W, rg, m)
        assert rg["n_members_inflated"] <= m["bound"], (g, W, rg, m)
        assert rg["n_members_inflated"] == (m["hi"] - m["first"] if m["hi"] is not None else 0), (g, W, rg, m)
        assert info["n_members"] == m["n"] and info["text_bytes"] == m["T"] and info["comp_bytes"] == len(image)
        out.append((m, rg))
    assert at == len(text)
    return out


def lines(n, width, seed=0):
    """n lines of `width` bytes, newline included, no two alike"""
    return b"".join((b"%06d:" % (k + seed)).ljust(width - 1, b"abcdefghijklmnopqrstuvwxyz"[k % 26:k % 26 + 1]) + b"\n" for k in range(n))


# ------------------------------------------------------------------------------------------------ 1. borders against members
@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("where", ["on_the_newline", "behind_it", "in_front_of_it"])
def test_borders_against_members(where, W, gpu_ctx):
    r = {"on_the_newline": 255, "behind_it": 0, "in_front_of_it": 254}[where]
    nom1 = 256 * 6 + r
    text = lines(nom1 * W // 64 + 2, 64)[:nom1 * W]  # T = W nom(1)
    assert len(text) == nom1 * W
    image = B.bgzf(text, member_size=256)
    mem = table(image)
    assert all(text[o + i - 1:o + i] == b"\n" for o, i in mem if i == 256), "a newline is the last byte of every full member"
    m = model(text, image, 1, W)
    assert m["nom"] == nom1
    if where == "on_the_newline":
        assert text[nom1:nom1 + 1] == b"\n" and (nom1 + 1) % 256 == 0 and m["beg"] == nom1 + 1 and m["first"] == nom1 // 256
    elif where == "behind_it":
        assert text[nom1 - 1:nom1] == b"\n" and nom1 % 256 == 0 and m["beg"] == nom1 and m["first"] == nom1 // 256 - 1, "the member BEFORE the nominal start holds byte nom - 1"
    else:
        assert text[nom1 + 1:nom1 + 2] == b"\n" and m["beg"] == nom1 + 2 and m["first"] == nom1 // 256
    check_world(gpu_ctx, text, image, W)


# ------------------------------------------------------------------------------------------------ 2. lines longer than the look-ahead
@pytest.mark.parametrize("tail", ["terminated", "open_to_the_end_of_the_chain"])
@pytest.mark.parametrize("eof", [True, False])
def test_lines_longer_than_the_look_ahead(tail, eof, gpu_ctx):
    width = 64 * (AHEAD + 3)
    text = lines(7, width)  # (7: no nominal border of a world of three falls on a line start)
    if tail == "open_to_the_end_of_the_chain":
        text += b"z" * (2 * width + 17)
    image = B.bgzf(text, member_size=64, eof=eof)
    res = check_world(gpu_ctx, text, image, 3)
    assert any(rg["n_rounds"] >= 1 for _, rg in res), "an end border needs an extension round"
    W = 16  # about 112 bytes a rank: most nominal ranges lie inside one line
    res = check_world(gpu_ctx, text, image, W)
    assert any(m["beg"] == m["end"] and m["nom"] < m["beg"] and m["nom_e"] <= m["beg"] for m, _ in res), "a rank whose whole nominal range lies inside one line"
    assert any(rg["n_rounds"] >= 2 for _, rg in res), "the batch doubles"
    if tail == "open_to_the_end_of_the_chain":
        last = [m for m, _ in res if m["nom"] > text.rfind(b"\n") + 1]
        assert last and all(m["beg"] == m["end"] == len(text) for m in last), "no newline to the end of the chain: the border is T"


# ------------------------------------------------------------------------------------------------ 3. empty members
def _empties_text():
    text = lines(48, 64)  # 12 members of 256 bytes; W = 2: nom(1) = 1536, the first byte of member 6
    assert len(text) // 2 == 1536
    return text


@pytest.mark.parametrize("eof", [True, False])
@pytest.mark.parametrize("what", ["holding_the_position_of_the_member_of_nom_minus_1", "in_front_of_and_behind_a_border", "several_in_a_row", "in_front_of_the_first_member"])
def test_empty_members(what, eof, gpu_ctx):
    text = _empties_text()
    if what == "holding_the_position_of_the_member_of_nom_minus_1":
        image = B.bgzf(text, member_size=256, eof=eof, empty_at=(5,))  # member 5 holds byte 1535 = nom(1) - 1; the empty one stands at its first byte
        mem = table(image)
        assert mem[5] == (1280, 0) and mem[6] == (1280, 256) and model(text, image, 1, 2)["first"] == 6
    elif what == "in_front_of_and_behind_a_border":
        image = B.bgzf(text, member_size=256, eof=eof, empty_at=(5, 6, 7))  # the border of the two ranks is byte 1536: an empty member at 1280, one AT 1536, one at 1792
        mem = table(image)
        assert (1536, 0) in mem and (1280, 0) in mem and (1792, 0) in mem and model(text, image, 1, 2)["beg"] == 1536
    elif what == "several_in_a_row":
        image = B.bgzf(text[:1536], member_size=256, eof=False) + B.EOF_MARKER * 3 + B.bgzf(text[1536:], member_size=256, eof=eof, empty_at=(0, 1))
        mem = table(image)
        assert mem[6:10] == [(1536, 0)] * 4 and mem[11] == (1792, 0)
        m = model(text, image, 0, 2)
        assert m["hi"] - m["first"] == 6 + AHEAD and m["hi"] <= 9, "the look-ahead of rank 0 is spent on empty members: the text ends at the border"
    else:
        image = B.bgzf(text, member_size=256, eof=eof, empty_at=(0,))
        assert table(image)[0] == (0, 0) and model(text, image, 0, 2)["first"] == 1
    assert (table(image)[-1][1] == 0) == eof
    for W in (2, 3, 5):
        check_world(gpu_ctx, text, image, W)
    got, info = gpu_ctx.bgzf_inflate(image)
    assert got == text


def test_only_empty_members(gpu_ctx):
    for image in (B.EOF_MARKER, B.EOF_MARKER * 3):
        for W in (1, 2):
            res = check_world(gpu_ctx, b"", image, W)
            assert all(rg["n_members_inflated"] == 0 and rg["first_member"] == m["n"] for m, rg in res)


# ------------------------------------------------------------------------------------------------ 4. degenerate worlds
def test_world_of_one_is_the_whole_text(gpu_ctx):
    text = lines(300, 100)
    image = B.bgzf(text, member_size=4000)
    (m, rg), = check_world(gpu_ctx, text, image, 1)
    assert (rg["beg"], rg["end"], rg["first_member"], rg["n_members_inflated"], rg["n_rounds"]) == (0, len(text), 0, m["n"], 0)
    whole, info = gpu_ctx.bgzf_inflate(image)
    assert whole == text and gpu_ctx.bgzf_range(image, 0, 1)[0] == whole


@pytest.mark.parametrize("what", ["more_ranks_than_lines", "more_ranks_than_members", "fewer_bytes_than_ranks", "no_newline_at_all", "unterminated_last_line"])
def test_degenerate_worlds(what, gpu_ctx):
    if what == "more_ranks_than_lines":
        text, ms, W = lines(3, 200), 64, 7
        assert text.count(b"\n") < W
    elif what == "more_ranks_than_members":
        text, ms, W = lines(40, 50), 1000, 5
        assert len(table(B.bgzf(text, member_size=ms))) < W
    elif what == "fewer_bytes_than_ranks":
        text, ms, W = b"a\nb", 2, 5
    elif what == "no_newline_at_all":
        text, ms, W = b"x" * 1000, 100, 4
    else:
        text, ms, W = lines(20, 64) + b"no newline behind this line", 256, 3
        assert not text.endswith(b"\n")
    image = B.bgzf(text, member_size=ms)
    res = check_world(gpu_ctx, text, image, W)
    if what == "no_newline_at_all":
        assert [(m["beg"], m["end"]) for m, _ in res] == [(0, 1000)] + [(1000, 1000)] * 3, "rank 0 owns all of it"
    if what == "fewer_bytes_than_ranks":
        assert any(m["nom_e"] == 0 for m, _ in res) and sorted(set((m["beg"], m["end"]) for m, _ in res)) == [(0, 0), (0, 2), (2, 2), (2, 3)]
    if what == "unterminated_last_line":
        assert res[-1][0]["end"] == len(text) and res[-1][1]["end"] == len(text)


# ------------------------------------------------------------------------------------------------ 5. member counts at the workgroup edge of the sub-range
@pytest.mark.parametrize("K", [1, WAVES, WAVES + 1, 2 * WAVES])
def test_member_counts_of_the_sub_range(K, gpu_ctx):
    """a sub-range of exactly K members, 4 = BGZF_WAVES to a workgroup: the whole chain of K members as a world of one (K = 1: without a marker, else the marker
    is the K-th); and, where the look-ahead leaves room, the middle rank of three on members of 4 lines each -- its first member is the one in front of its nominal
    start, whose newline ends it, its last the one that holds nom(2) - 1, then the look-ahead"""
    text = lines((K - 1) * 4 if K > 1 else 4, 64, seed=7 * K)
    image = B.bgzf(text, member_size=256, eof=K > 1)
    m = model(text, image, 0, 1)
    assert m["n"] == K and m["hi"] - m["first"] == K
    (m, rg), = check_world(gpu_ctx, text, image, 1)
    assert rg["n_members_inflated"] == K
    n = K - 1 - AHEAD
    if n >= 1:
        text = lines(3 * n * 4, 64, seed=K)
        image = B.bgzf(text, member_size=256, eof=False)
        m = model(text, image, 1, 3)
        assert m["nom"] == 256 * n and m["first"] == n - 1 and m["hi"] - m["first"] == K
        res = check_world(gpu_ctx, text, image, 3)
        assert res[1][1]["n_members_inflated"] == K


# ------------------------------------------------------------------------------------------------ 6. the search alone
@pytest.fixture(scope="module")
def xc():
    """a context of this module's own: its exchange buffer grows only when a case asks for more than any case before, so the case knows where it ends"""
    c = ma.Ctx(0)
    c._xcap = 0
    yield c
    c.close()


def _region(ctx, n):
    """device address of n bytes that END where exchange buffer 0 ends (mahip_xbuf reserves bytes + 256 rounded up to 256; the pool may hand out more): with
    the pool off and guard pages on, the byte behind the text faults"""
    need = n + 256
    if need + 256 > ctx._xcap:
        ctx._xcap = (need + 256 + 255) & ~255
    return ST.xbuf(ctx, 0, need) + ctx._xcap - n


def _search(ctx, d, text, lo, hi):
    want = text.find(b"\n", lo, hi) if hi > lo else -1
    got = ctx.text_first_nl(d, lo, hi)
    assert got == (None if want < 0 else want), (lo, hi, got, want)
    return got


def _upload(ctx, d, text):
    a = np.frombuffer(text, dtype=np.uint8).copy()
    assert ctx.memcpy_h2d(d, a.ctypes.data, len(a)) == 0, ma.lib().mahip_strerror()


def test_first_newline_at_every_alignment(xc):
    """a 4 KiB device text (the last 4 KiB of the exchange buffer: 16-byte aligned): `lo` and `hi` at every combination of 0, 1 and 15 mod 16, hi - lo of 0, 1, 15, 16 and 17, the
    newline at lo, at hi - 1, at hi and in front of lo (neither may be found) and absent"""
    n, gpu_ctx = 4096, xc
    d = _region(xc, n)
    assert d % 16 == 0
    spans = [(256 + fa, 1024 + ta) for fa in (0, 1, 15) for ta in (0, 1, 15)]
    spans += [(512 + fa, 512 + fa + ln) for fa in (0, 1, 15) for ln in (0, 1, 15, 16, 17)]
    spans += [(0, 0), (0, 1), (0, n), (1, n), (n - 17, n), (n - 1, n), (n, n)]
    n_found = 0
    for lo, hi in spans:
        for where in ("outside", "at_lo", "at_hi_minus_1", "absent", "both_ends"):
            t = bytearray(b"t" * n)
            if where == "outside":  # right in front of lo and at hi: not in [lo, hi)
                if lo > 0:
                    t[lo - 1] = 10
                if hi < n:
                    t[hi] = 10
            elif where == "at_lo" and lo < n:
                t[lo] = 10  # (an empty span must not find it)
            elif where == "at_hi_minus_1" and hi > 0:
                t[hi - 1] = 10  # (an empty span: this is in front of lo)
            elif where == "both_ends" and hi > lo:
                t[lo] = t[hi - 1] = 10
            _upload(gpu_ctx, d, bytes(t))
            n_found += _search(gpu_ctx, d, bytes(t), lo, hi) is not None
    assert n_found > 2 * len(spans)


def test_first_newline_behind_more_than_one_workgroups_bytes(xc):
    """a workgroup takes 4 x 1024 bytes a step, so the 4 KiB text of the case above is one workgroup's: here 3 workgroups' and a ragged rest, the only newline
    in the last 16 bytes; then the smallest of many, then of two in one 16-byte word"""
    n, gpu_ctx = 3 * 4096 + 1000, xc
    d = _region(xc, n)
    assert d % 16 == 8, "the text does not start at a 16-byte boundary"
    for lo in (0, 5):
        for back in (1, 7, 16):
            t = bytearray(b"u" * n)
            t[n - back] = 10
            _upload(gpu_ctx, d, bytes(t))
            assert _search(gpu_ctx, d, bytes(t), lo, n) == n - back
            assert _search(gpu_ctx, d, bytes(t), lo, n - back) is None
    t = bytearray(b"u" * n)
    for p in (4099, 4100, 4111, 4112, 8200, 12000, n - 1):
        t[p] = 10
    _upload(gpu_ctx, d, bytes(t))
    for lo in (0, 4099, 4100, 4101, 4112, 4113, 8201, 12001):
        _search(gpu_ctx, d, bytes(t), lo, n)
    _upload(gpu_ctx, d, b"\n" * n)
    for lo in (0, 3, 4097):
        assert _search(gpu_ctx, d, b"\n" * n, lo, n) == lo


# ------------------------------------------------------------------------------------------------ 7. the loaded context
@pytest.fixture(scope="module")
def paf_files(tmpdir_s):
    paf = R.pafgen(os.path.join(tmpdir_s, "bgzf_range.paf"), 300, 5000, 17, ["-L", "uniform"])
    text = open(paf, "rb").read()[:200000]
    text = text[:-1] if text.endswith(b"\n") else text  # an open last line
    assert len(text) > 150000 and not text.endswith(b"\n")
    plain, comp = os.path.join(tmpdir_s, "bgzf_range_cut.paf"), os.path.join(tmpdir_s, "bgzf_range_cut.paf.gz")
    image = B.bgzf(text, member_size=20011)
    with open(plain, "wb") as f:
        f.write(text)
    with open(comp, "wb") as f:
        f.write(image)
    return text, image, plain, comp


def _parse_cols(ctx):
    L = ma.lib()
    pi = ma.PafInfo()
    ma._chk(L.mahip_paf_parse_excl(ctx.h, 2000, 100, 1, 0, 0, 0.0, ma.C.byref(pi)), "paf_parse")
    flags, lstart = np.zeros(pi.n_lines + 1, dtype=np.uint8), np.zeros(pi.n_lines + 2, dtype=np.uint64)
    ma._chk(L.mahip_paf_cols_download(ctx.h, flags.ctypes.data, None, None, None, None, None, lstart.ctypes.data, None), "paf_cols_download")
    rep = ma.PafReport()
    ma._chk(L.mahip_paf_last(ctx.h, ma.C.byref(rep)), "paf_last")
    out = (pi.n_lines, pi.n_records, pi.n_hits, pi.n_seq, pi.name_bytes, rep.n_gran, rep.open_line, flags[:pi.n_lines].tobytes(), lstart[:pi.n_lines + 1].tobytes())
    ma._chk(L.mahip_paf_release(ctx.h), "paf_release")
    return out


@pytest.mark.parametrize("g,W", [(0, 3), (1, 3), (2, 3), (3, 7)])
def test_load_leaves_the_context_as_the_plain_range_loader_does(g, W, paf_files, gpu_ctx):
    text, image, plain, comp = paf_files
    m = model(text, image, g, W)
    assert 0 < m["end"] - m["beg"] < len(text) and (g == 0 or text[m["beg"] - 1:m["beg"]] == b"\n")
    L = ma.lib()
    L.mahip_paf_load_fd_range.argtypes = [ma.C.c_void_p, ma.C.c_int, ma.C.c_size_t, ma.C.c_size_t]
    fd = os.open(comp, os.O_RDONLY)
    try:
        rg, info = gpu_ctx.bgzf_load_range(fd, len(image), g, W)
    finally:
        os.close(fd)
    assert info["reason"] == "OK" and (rg["beg"], rg["end"], rg["text_bytes"], rg["first_member"]) == (m["beg"], m["end"], m["T"], m["first"])
    assert rg["n_members_inflated"] == m["hi"] - m["first"] <= m["bound"] and rg["n_rounds"] == 0
    mem = B.members_of(image)
    assert rg["comp_bytes_uploaded"] == mem[m["hi"] - 1][0] + mem[m["hi"] - 1][1] - 8 - (mem[m["first"]][0] + 18) < len(image)
    last = gpu_ctx.bgzf_last()
    assert last["reader"] == "device" and last == info
    a = _parse_cols(gpu_ctx)
    fd = os.open(plain, os.O_RDONLY)
    try:
        ma._chk(L.mahip_paf_load_fd_range(gpu_ctx.h, fd, m["beg"], m["end"] - m["beg"]), "paf_load_fd_range")
    finally:
        os.close(fd)
    b = _parse_cols(gpu_ctx)
    assert a == b and a[0] == text[m["beg"]:m["end"]].count(b"\n") + (not text[m["beg"]:m["end"]].endswith(b"\n"))


def test_cap_counts_the_ranks_own_bytes(paf_files, gpu_ctx):
    """MA_PAF_MAX_BYTES counts end - beg: a cap between a third and the whole of the text lets a rank of three load, and refuses the world of one as
    mahip_paf_load_fd refuses the plain file (an error, not a reason)"""
    text, image, plain, comp = paf_files
    os.environ["MA_PAF_MAX_BYTES"] = str(len(text) // 2)
    fd = os.open(comp, os.O_RDONLY)
    try:
        rg, info = gpu_ctx.bgzf_load_range(fd, len(image), 1, 3)
        assert info["reason"] == "OK" and rg["end"] - rg["beg"] < len(text) // 2
        ma._chk(ma.lib().mahip_paf_release(gpu_ctx.h), "paf_release")
        with pytest.raises(ma.GpuError, match="MA_PAF_MAX_BYTES"):
            gpu_ctx.bgzf_load_range(fd, len(image), 0, 1)
    finally:
        os.close(fd)
        del os.environ["MA_PAF_MAX_BYTES"]
    pi = ma.PafInfo()
    assert ma.lib().mahip_paf_parse_excl(gpu_ctx.h, 2000, 100, 1, 0, 0, 0.0, ma.C.byref(pi)) != 0 and b"no text loaded" in ma.lib().mahip_strerror()


# ------------------------------------------------------------------------------------------------ 8. a status in one range only
def test_status_in_one_range_only(tmpdir_s, gpu_ctx):
    text = lines(64, 64)
    good = B.bgzf(text, member_size=256, level=0)  # stored blocks: a flipped payload bit is a flipped text bit, and nothing else
    mem = B.members_of(good)
    bad_m, W = 9, 4
    off, total = mem[bad_m]
    at = off + 18 + 5 + 77
    assert good[at:at + 1] not in (b"\n", b"\x0b") and off + 18 + 5 + 256 + 8 == off + total
    image = B.flip_bit(good, at, 0)
    import gzip
    with pytest.raises(Exception):
        gzip.decompress(image)
    holders = []
    for g in range(W):
        m = model(text, good, g, W)
        assert m["rounds"] == 0
        got, rg, info = gpu_ctx.bgzf_range(image, g, W)
        if m["first"] <= bad_m < m["hi"]:
            holders.append(g)
            assert got is None and (info["reason"], info["first_bad_member"], info["reader"]) == ("CRC", bad_m, "host"), (g, info)
            assert (rg["beg"], rg["end"], rg["text_bytes"], rg["first_member"]) == (0, 0, len(text), m["first"])
        else:
            assert info["reason"] == "OK" and got == text[m["beg"]:m["end"]], (g, info)
    assert holders and len(holders) < W, holders
    path = os.path.join(tmpdir_s, "bgzf_range_crc.paf.gz")
    with open(path, "wb") as f:
        f.write(image)
    fd = os.open(path, os.O_RDONLY)
    try:
        rg, info = gpu_ctx.bgzf_load_range(fd, len(image), holders[0], W)
    finally:
        os.close(fd)
    assert (info["reason"], info["first_bad_member"]) == ("CRC", bad_m) and gpu_ctx.bgzf_last() == info
    pi = ma.PafInfo()
    assert ma.lib().mahip_paf_parse_excl(gpu_ctx.h, 2000, 100, 1, 0, 0, 0.0, ma.C.byref(pi)) != 0 and b"no text loaded" in ma.lib().mahip_strerror(), "nothing stays loaded"


def test_refusals_of_the_walk_and_of_the_arguments(gpu_ctx):
    import gzip
    got, rg, info = gpu_ctx.bgzf_range(gzip.compress(b"a\nb\n"), 0, 2)
    assert got is None and info["reason"] == "NOT_BGZF" and info["first_bad_member"] == 0
    image = B.bgzf(b"a\nb\n")
    for g, W in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ma.GpuError):
            gpu_ctx.bgzf_range(image, g, W)
    with pytest.raises(ma.GpuError, match="room for"):
        gpu_ctx.bgzf_range(image, 0, 1, out_cap=3)
