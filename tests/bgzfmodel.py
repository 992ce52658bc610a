"""BGZF images for the tests of the device inflater (tests/test_gpu_bgzf.py): a writer over zlib's raw deflate with every knob the kernel's paths hang on, a
bit-writer for the deflate blocks zlib does not emit on demand, a small parser of deflate streams (block types, lengths and distances: the tests assert from it
that an input holds what it was built for) and byte-level corrupters.  Pure Python; nothing here is imported by the product."""
import struct
import zlib

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ------------------------------------------------------------------------------------------------ members
def member(deflate, text=None, crc=None, isize=None, extra_before=b"", extra_after=b"", bc=True, flg=4, bsize=None):
    """one gzip member around raw deflate bytes; crc / isize default to those of `text`; extra_before / extra_after: other subfields around `BC`"""
    crc = zlib.crc32(text or b"") if crc is None else crc
    isize = len(text or b"") if isize is None else isize
    xlen = len(extra_before) + (6 if bc else 0) + len(extra_after)
    total = 12 + xlen + len(deflate) + 8
    assert total <= 65536 or bsize is not None, "a BGZF member holds at most 65536 bytes, header and trailer included"
    sub = extra_before + (b"BC" + struct.pack("<HH", 2, (total - 1 if bsize is None else bsize) & 0xffff) if bc else b"") + extra_after
    if not flg & 4:
        return b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff" + deflate + struct.pack("<II", crc, isize)
    return b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff" + struct.pack("<H", xlen) + sub + deflate + struct.pack("<II", crc, isize)


def subfield(si, data):
    return si + struct.pack("<H", len(data)) + data


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flush_every=0, flush_mode=zlib.Z_SYNC_FLUSH):
    """raw deflate of `data`; flush_every: a sync (or full) flush after every so many bytes -- an empty stored block each, and the blocks behind it start unaligned"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    out = b""
    if flush_every:
        for i in range(0, len(data), flush_every):
            out += co.compress(data[i:i + flush_every]) + co.flush(flush_mode)
    else:
        out = co.compress(data)
    return out + co.flush()


def bgzf(data, member_size=65280, eof=True, empty_at=(), extra_before=b"", **kw):
    """`data` as a BGZF image: members of member_size bytes of text (bgzip's own: 65280), an empty member in front of every member whose number is in empty_at,
    the end-of-file marker unless eof is false; the other arguments go to raw_deflate"""
    out, k = b"", 0
    for i in range(0, len(data), member_size):
        if k in empty_at:
            out += EOF_MARKER
        part = data[i:i + member_size]
        out += member(raw_deflate(part, **kw), part, extra_before=extra_before)
        k += 1
    return out + (EOF_MARKER if eof else b"")


def members_of(image):
    """[(offset, total size)] of a well-formed image (BC first or not)"""
    out, p = [], 0
    while p < len(image):
        xlen = struct.unpack_from("<H", image, p + 10)[0]
        x, total = p + 12, None
        while x < p + 12 + xlen:
            slen = struct.unpack_from("<H", image, x + 2)[0]
            if image[x:x + 2] == b"BC":
                total = struct.unpack_from("<H", image, x + 4)[0] + 1
            x += 4 + slen
        out.append((p, total))
        p += total
    return out


# ------------------------------------------------------------------------------------------------ a deflate bit-writer
class Bits:
    """deflate's bit order: fields least significant bit first, Huffman codes most significant bit first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, c, n):
        return self.put(int(format(c, "0%db" % n)[::-1], 2), n) if n else self

    def align(self):
        return self.put(0, (8 - self.n) % 8)

    def raw(self, b):
        assert self.n == 0
        self.out += b
        return self

    def bytes(self):
        return bytes(self.out + (bytes([self.acc]) if self.n else b""))


def canonical(lens):
    """code lengths -> {symbol: (code, length)}, RFC 1951 3.2.2"""
    out, code = {}, 0
    for n in range(1, max(lens) + 1):
        for s, ln in enumerate(lens):
            if ln == n:
                out[s] = (code, n)
                code += 1
        code <<= 1
    return out


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_header(w, final, hlit, hdist, cl_lens, cl_syms):
    """BFINAL, BTYPE 2, the counts, the 19 code-length code lengths (cl_lens by symbol) and the run-length coded lengths: cl_syms = [(symbol, extra bits value)]"""
    hclen = max(k for k, s in enumerate(CL_ORDER) if cl_lens[s]) + 1
    hclen = max(hclen, 4)
    w.put(final, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.put(cl_lens[s], 3)
    cc = canonical(cl_lens)
    for s, x in cl_syms:
        w.code(*cc[s])
        if s >= 16:
            w.put(x, {16: 2, 17: 3, 18: 7}[s])
    return w


def fixed_code(sym):
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xc0 + sym - 280, 8


def stored(w, final, data, nlen=None):
    w.put(final, 1).put(0, 2).align()
    w.put(len(data), 16).put((~len(data) if nlen is None else nlen) & 0xffff, 16)
    return w.raw(data)


# ------------------------------------------------------------------------------------------------ a deflate parser (what a stream holds)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def parse(deflate):
    """walks a VALID raw deflate stream: dict(blocks=[type], text, matches=[(position, length, distance)], max_code_len, n_dist_codes=[per dynamic block])"""
    pos = 0

    def bits(n):
        nonlocal pos
        v = 0
        for k in range(n):
            v |= (deflate[pos >> 3] >> (pos & 7) & 1) << k
            pos += 1
        return v

    def decoder(lens):
        table = {(c, n): s for s, (c, n) in canonical(lens).items()} if any(lens) else {}

        def dec():
            c = 0
            for n in range(1, 16):
                c = c << 1 | bits(1)
                if (c, n) in table:
                    return table[(c, n)]
            raise ValueError("no code")
        return dec

    out, blocks, matches, maxlen, ndist = bytearray(), [], [], 0, []
    while True:
        final, typ = bits(1), bits(2)
        blocks.append(typ)
        if typ == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            assert bits(16) == (~n & 0xffff)
            out += deflate[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
        else:
            if typ == 1:
                ll, dl = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for s in CL_ORDER[:hclen]:
                    cl[s] = bits(3)
                dec, lens = decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = dec()
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * ((3 + bits(3)) if s == 17 else (11 + bits(7)))
                assert len(lens) == hlit + hdist
                ll, dl = lens[:hlit], lens[hlit:]
                maxlen = max(maxlen, max(ll), max(dl))
                ndist.append(sum(1 for x in dl if x))
            ld, dd = decoder(ll), decoder(dl)
            while True:
                s = ld()
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    n = LEN_BASE[s - 257] + bits(LEN_EXTRA[s - 257])
                    d = dd()
                    dist = DIST_BASE[d] + bits(DIST_EXTRA[d])
                    matches.append((len(out), n, dist))
                    for _ in range(n):
                        out.append(out[-dist])
        if final:
            break
    return dict(blocks=blocks, text=bytes(out), matches=matches, max_code_len=maxlen, n_dist_codes=ndist)


# ------------------------------------------------------------------------------------------------ corrupters
def flip_bit(b, byte, bit=0):
    b = bytearray(b)
    b[byte] ^= 1 << bit
    return bytes(b)


def set_u32(b, off, v):
    return b[:off] + struct.pack("<I", v & 0xffffffff) + b[off + 4:]


def set_u16(b, off, v):
    return b[:off] + struct.pack("<H", v & 0xffff) + b[off + 2:]
