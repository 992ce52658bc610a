"""Plain gzip images for the tests of the chunked device inflater (tests/test_gpu_gzip.py), and a model of what it must report.

Built on bgzfmodel's bit writer and code tables.  gz() drives zlib's raw deflate with every knob (level, memLevel, strategy, flush points) under a hand-written
RFC 1952 header and trailer; fixed_block / dynamic_block / B.stored assemble streams block by block.  blocks() walks a VALID stream and returns every block
start (bit offset, type, BFINAL, bytes of output, end bit); model() turns that and a chunk size into the row every chunk must report -- sync_bit (the first
dynamic block start among the chunk's own bits; bit 0 for chunk 0), end_bit, out_len, status, on_chain -- and the reason of the whole load, by the rules of
include/mahip.h.  The model knows TRUE block starts only: a test whose image holds a false candidate states its rows by hand.  Pure Python; nothing here is
imported by the product."""
import struct
import zlib

import bgzfmodel as B

SPAN_MAX = 16  # csrc/gzip_core.h: GZ_SPAN_MAX
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


# ------------------------------------------------------------------------------------------------ header, trailer, zlib's streams
def header(fname=None, comment=None, extra=None, hcrc=False, mtime=0, reserved=0, ftext=False):
    flg = (1 if ftext else 0) | (2 if hcrc else 0) | (4 if extra is not None else 0) | (8 if fname is not None else 0) | (16 if comment is not None else 0) | reserved
    h = b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<I", mtime) + b"\x00\x03"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if fname is not None:
        h += fname + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    return h


def wrap(deflate, text, head=None, crc=None, isize=None):
    """a gzip member around raw deflate bytes; crc / isize default to those of `text`"""
    head = header() if head is None else head
    return head + deflate + struct.pack("<II", zlib.crc32(text) if crc is None else crc, (len(text) if isize is None else isize) & 0xffffffff)


def deflate(data, level=6, memlevel=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush_mode=zlib.Z_SYNC_FLUSH):
    """raw deflate of `data` with a flush (an empty stored block) after each position in flush_at"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, memlevel, strategy)
    out, last = b"", 0
    for p in sorted(flush_at):
        out += co.compress(data[last:p]) + co.flush(flush_mode)
        last = p
    return out + co.compress(data[last:]) + co.flush()


def gz(data, level=6, memlevel=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush_mode=zlib.Z_SYNC_FLUSH, head=None):
    return wrap(deflate(data, level, memlevel, strategy, flush_at, flush_mode), data, head)


# ------------------------------------------------------------------------------------------------ streams block by block
def _match(w, lcode, dcode, ln, dist):
    ls = 28 if ln == 258 else max(k for k in range(28) if B.LEN_BASE[k] <= ln)
    w.code(*lcode(257 + ls)).put(ln - B.LEN_BASE[ls], B.LEN_EXTRA[ls])
    ds = max(k for k in range(30) if B.DIST_BASE[k] <= dist)
    w.code(*dcode(ds)).put(dist - B.DIST_BASE[ds], B.DIST_EXTRA[ds])


def _tokens(w, lcode, dcode, tokens, text):
    """tokens: a literal byte, or (length, distance); appends what they produce to `text` (which must hold the history a distance reaches into)"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lcode(t))
            text.append(t)
        else:
            _match(w, lcode, dcode, *t)
            for _ in range(t[0]):
                text.append(text[-t[1]] if t[1] <= len(text) else 0)  # (in front of the stream: a stream made to be refused)
    w.code(*lcode(256))


def fixed_block(w, final, tokens, text):
    w.put(final, 1).put(1, 2)
    _tokens(w, B.fixed_code, lambda d: (d, 5), tokens, text)
    return w


CL_LENS = [4] * 13 + [5] * 6  # a complete code-length code


def dynamic_block(w, final, tokens, text, ll=None, dl=None):
    """a dynamic block; its codes unless ll / dl say otherwise: the fixed code's lengths made complete over 286 symbols (148 / 256 + 108 / 512 + 24 / 128 + 6 / 256
    = 1), and two distances of 4 bits, 28 of 5"""
    ll = [8] * 148 + [9] * 108 + [7] * 24 + [8] * 6 if ll is None else ll
    dl = [4, 4] + [5] * 28 if dl is None else dl
    assert sum(2.0 ** -x for x in ll if x) == 1.0 and sum(2.0 ** -x for x in dl if x) in (1.0, 0.5, 0)
    lens, syms, i = ll + dl, [], 0
    while i < len(lens):  # run-length code: 16 repeats the one before 3..6 times
        v, r = lens[i], 1
        while i + r < len(lens) and lens[i + r] == v:
            r += 1
        syms.append((v, 0))
        i += 1
        r -= 1
        while r >= 3:
            n = min(r, 6)
            syms.append((16, n - 3))
            i += n
            r -= n
    B.dynamic_header(w, final, len(ll), len(dl), CL_LENS, syms)
    lc, dc = B.canonical(ll), B.canonical(dl)
    _tokens(w, lambda s: lc[s], lambda d: dc[d], tokens, text)
    return w


def stored(w, final, data, text):
    B.stored(w, final, data)
    text += data
    return w


# ------------------------------------------------------------------------------------------------ what a stream holds
class _Bits:
    def __init__(self, d):
        self.d, self.pos = d, 0

    def get(self, n):
        p = self.pos
        if p + n > 8 * len(self.d):
            raise ValueError("the stream ends early")
        self.pos = p + n
        return (int.from_bytes(self.d[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << n) - 1)

    def sym(self, table, maxlen):
        p = self.pos
        w = int.from_bytes(self.d[p >> 3:(p >> 3) + 4], "little") >> (p & 7)
        c = 0
        for n in range(1, maxlen + 1):
            c = c << 1 | (w & 1)
            w >>= 1
            s = table.get((n, c))
            if s is not None:
                self.pos = p + n
                if self.pos > 8 * len(self.d):
                    raise ValueError("the stream ends early")
                return s
        raise ValueError("no code")


def _table(lens):
    return {(n, c): s for s, (c, n) in B.canonical(lens).items()} if any(lens) else {}


_FIXED = (_table(FIXED_LL), _table([5] * 30))


def blocks(stream, history=b""):
    """walks a VALID raw deflate stream -> ([dict(bit, type, final, out_len, end)], text, bit behind the final block)"""
    r, out, blk = _Bits(stream), bytearray(history), []
    h = len(history)
    while True:
        bit = r.pos
        final, typ = r.get(1), r.get(2)
        n0, too_far = len(out), False
        if typ == 0:
            r.pos = (r.pos + 7) & ~7
            n = r.get(16)
            if r.get(16) != (~n & 0xffff):
                raise ValueError("LEN / NLEN")
            if (r.pos >> 3) + n > len(stream):
                raise ValueError("the stream ends early")
            out += stream[r.pos >> 3:(r.pos >> 3) + n]
            r.pos += 8 * n
        elif typ == 3:
            raise ValueError("block type 3")
        else:
            if typ == 1:
                lt, dt, lm, dm = _FIXED[0], _FIXED[1], 9, 5
            else:
                hlit, hdist, hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
                cl = [0] * 19
                for s in B.CL_ORDER[:hclen]:
                    cl[s] = r.get(3)
                ct, lens = _table(cl), []
                while len(lens) < hlit + hdist:
                    s = r.sym(ct, 7)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + r.get(2))
                    else:
                        lens += [0] * ((3 + r.get(3)) if s == 17 else (11 + r.get(7)))
                if len(lens) != hlit + hdist:
                    raise ValueError("repeat overrun")
                lt, dt, lm, dm = _table(lens[:hlit]), _table(lens[hlit:]), max(lens[:hlit]), max(lens[hlit:])
            while True:
                s = r.sym(lt, lm)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    n = B.LEN_BASE[s - 257] + r.get(B.LEN_EXTRA[s - 257])
                    d = r.sym(dt, dm)
                    dist = B.DIST_BASE[d] + r.get(B.DIST_EXTRA[d])
                    if dist > len(out):  # in front of the stream: the block is marked, the missing bytes read as zeros
                        too_far = True
                        for _ in range(n):
                            out.append(out[-dist] if dist <= len(out) else 0)
                    elif dist >= n:
                        out += out[len(out) - dist:len(out) - dist + n]
                    else:
                        for _ in range(n):
                            out.append(out[-dist])
        blk.append(dict(bit=bit, type=typ, final=final, out_len=len(out) - n0, end=r.pos, too_far=too_far))
        if final:
            return blk, bytes(out[h:]), r.pos


def parse_header(image):
    """-> where the deflate stream starts, or None where the device reader says BAD_HEADER"""
    if len(image) < 18 or image[:3] != b"\x1f\x8b\x08" or image[3] & 0xe0:
        return None
    flg, p = image[3], 10
    if flg & 4:
        xlen = struct.unpack_from("<H", image, p)[0]
        x, xend = p + 2, p + 2 + xlen
        while xend - x >= 4:
            slen = struct.unpack_from("<H", image, x + 2)[0]
            if image[x:x + 2] == b"BC" and slen == 2:
                return None
            x += 4 + slen
        p = xend
    for bit in (8, 16):
        if flg & bit:
            p = image.index(b"\0", p) + 1
    if flg & 2:
        p += 2
    return p if p + 8 <= len(image) else None


def model(image, chunk):
    """dict(reason, first_bad_item, text (None unless OK), rows=[dict(sync_bit, end_bit, out_len, status, saw_final, on_chain)], n_items, n_synced, blocks, hdr)
    for an image whose first member's stream is VALID deflate (whatever stands behind it)"""
    hdr = parse_header(image)
    if hdr is None:
        return dict(reason="BAD_HEADER", first_bad_item=-1, text=None, rows=[], n_items=0, n_synced=0, blocks=[], hdr=None)
    payload = image[hdr:len(image) - 8]
    blk, text, _ = blocks(payload)
    CB = 8 * chunk
    n_chunks = max(1, -(-len(payload) // chunk))
    rows, fars = [], []
    for k in range(n_chunks):
        own_end = min((k + 1) * CB, 8 * len(payload))
        first = 0 if k == 0 else next((i for i, b in enumerate(blk) if b["type"] == 2 and k * CB <= b["bit"] < own_end), None)
        if first is None:
            rows.append(dict(sync_bit=None, end_bit=0, out_len=0, status="OK", saw_final=False, on_chain=False))
            fars.append(False)
            continue
        row = dict(sync_bit=blk[first]["bit"], out_len=0, status="OK", saw_final=False, on_chain=False)
        far = False
        i = first
        while True:
            if i > first:
                pos = blk[i - 1]["end"]
                row["end_bit"] = pos
                if blk[i - 1]["final"]:
                    row["saw_final"] = True
                    break
                if pos // CB - k > SPAN_MAX + 1:
                    row["status"] = "NO_SYNC"
                    break
                if blk[i]["type"] == 2 and pos >= (k + 1) * CB:
                    break
            row["out_len"] += blk[i]["out_len"]
            far = far or blk[i]["too_far"]
            i += 1
        rows.append(row)
        fars.append(far)
    # the chain
    reason, bad, cur, n_items, total, far_item = "OK", -1, 0, 0, 0, None
    while True:
        r = rows[cur]
        r["on_chain"] = True
        n_items += 1
        if fars[cur] and far_item is None:
            far_item = n_items - 1
        if r["status"] != "OK":
            reason, bad = r["status"], n_items - 1
            break
        total += r["out_len"]
        if r["saw_final"]:
            if hdr + (r["end_bit"] + 7) // 8 + 8 != len(image):
                reason, bad = "MULTI_MEMBER", n_items - 1
            break
        cur = r["end_bit"] // CB
        assert rows[cur]["sync_bit"] == r["end_bit"], "the model knows true block starts only: the chain cannot miss"
    crc, isize = struct.unpack("<II", image[-8:])
    if reason == "OK" and total & 0xffffffff != isize:
        reason = "ISIZE"
    if reason == "OK" and far_item is not None:  # (the decode pass: behind the chain and ISIZE)
        reason, bad = "DIST_TOO_FAR", far_item
    if reason == "OK" and zlib.crc32(text) != crc:
        reason = "CRC"
    return dict(reason=reason, first_bad_item=bad, text=text if reason == "OK" else None, rows=rows, n_items=n_items, n_synced=sum(r["sync_bit"] is not None for r in rows), blocks=blk, hdr=hdr)
