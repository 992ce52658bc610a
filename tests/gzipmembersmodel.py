"""Concatenated gzip members (`cat a.gz b.gz`) for the tests of the chunked device inflater's members form (tests/test_gpu_gzip_members.py), and a model of what
it must report.  Built on gzipmodel: cat() joins members; model() walks a VALID image member by member the way zlib's gzread does -- header, deflate stream,
trailer, next header -- and returns the text, one row per member (comp_off, hdr_len, text_off, text_len, crc, isize, n_items for a chunk size) and the positions
the member scan must list (every byte position behind the first header whose bytes read 1f 8b 08 and a FLG with bits 5..7 clear), with those whose header
parses.  As gzipmodel, it knows TRUE block starts only: n_items is right for images without a false block-start candidate.  Pure Python; nothing here is
imported by the product."""
import struct

import gzipmodel as G


def cat(*members):
    return b"".join(members)


def candidates(image, hdr0):
    """-> (every candidate position, those whose header parses)"""
    cand, heads, p = [], [], image.find(b"\x1f\x8b\x08", hdr0)
    while p >= 0 and p + 4 <= len(image):
        if not image[p + 3] & 0xe0:
            cand.append(p)
            try:
                if G.parse_header(image[p:]) is not None:
                    heads.append(p)
            except (ValueError, struct.error):  # a name without its zero, an extra field past the end
                pass
        p = image.find(b"\x1f\x8b\x08", p + 1)
    return cand, heads


def model(image, chunk):
    """dict(text, rows, candidates, heads) of a VALID image of one or more members"""
    CB = 8 * chunk
    hdr0 = G.parse_header(image)
    assert hdr0 is not None
    off, rows, text = 0, [], b""
    while True:
        hdr = G.parse_header(image[off:])
        assert hdr is not None, off
        blk, t, end = G.blocks(image[off + hdr:])
        assert not any(b["too_far"] for b in blk)
        tail = off + hdr + (end + 7) // 8
        crc, isize = struct.unpack_from("<II", image, tail)
        # the member's items: its head item from the first bit behind the header, then one from every dynamic block start that lies in a later chunk than the
        # item before it started in
        base = 8 * (off + hdr - hdr0)
        n_items, k = 1, base // CB
        for b in blk[1:]:
            if b["type"] == 2 and (base + b["bit"]) // CB > k:
                n_items, k = n_items + 1, (base + b["bit"]) // CB
        rows.append(dict(comp_off=off, hdr_len=hdr, text_off=len(text), text_len=len(t), crc=crc, isize=isize, n_items=n_items))
        text += t
        off = tail + 8
        if off == len(image):
            break
    cand, heads = candidates(image, hdr0)
    assert all(r["comp_off"] in heads for r in rows[1:])
    return dict(text=text, rows=rows, candidates=cand, heads=heads)
