"""The cut-and-carry reader of the streamed ingest (host/ingest_gpu.c: ma_cut_next) on its own, without a GPU and without Python in the process: the stand-alone
program tests/stream_cut_main.c, built as its header says with the address and undefined-behaviour sanitizers and run directly (nothing preloaded), reads a pipe in
reads of at most `chunk` bytes and cuts it into pieces of whole lines.  It checks itself that every piece but the last ends with a newline and that the pieces are
the input (byte count and hash); this module feeds it the inputs on which a cut can go wrong -- nothing, one byte, no newline at all, newlines only, a line of
exactly a piece, one byte less and one more, as first, middle and last line, and 300 KB of ordinary lines with and without the final newline -- and asserts the
piece count and the longest piece a 20-line model of the rule gives.  The library of the CPU build only supplies what the rest of ingest_gpu.c refers to."""
import os
import subprocess

import pytest

from test_emu_suite import EMU, ROOT, emu_built  # noqa: F401  (emu_built: the fixture that builds tests/emu)
from test_gpu_ingest_stream import gen

PIECES, CHUNKS = (256, 257, 1024), (1, 7, 4096)


def model(data, piece):
    """ma_cut_next's rule: the carry plus `piece` bytes are read; the input ending before that: what there is is the last piece.  Else the cut falls behind the
    last newline, the rest is the carry; without a newline another `piece` bytes are read.  -> (pieces, longest piece)"""
    at, carry, pieces, longest = 0, 0, 0, 0
    while True:
        target = carry + piece
        while True:
            buf = data[at:at + target]
            if len(buf) < target:  # a read came back empty
                return pieces + 1, max(longest, len(buf))
            nl = buf.rfind(b"\n")
            if nl >= 0:
                break
            target += piece
        pieces, longest = pieces + 1, max(longest, nl + 1)
        at, carry = at + nl + 1, target - (nl + 1)


def test_the_model_on_texts_cut_by_hand():
    assert model(b"", 256) == (1, 0) and model(b"x", 256) == (1, 1)
    assert model(b"a" * 255 + b"\n", 256) == (2, 256), "a text that ends with its first piece: the end shows only at the next read, as an empty last piece"
    assert model(b"a" * 254 + b"\n", 256) == (1, 255)
    assert model(b"a" * 256 + b"\n", 256) == (1, 257), "no newline in 256 bytes: read on; the input ends"
    assert model(b"ab\n" * 100, 256) == (2, 255)
    assert model(b"a" * 600 + b"\n" + b"b" * 10, 256) == (1, 611) and model(b"a" * 600 + b"\n" + b"b" * 200, 256) == (2, 601)


@pytest.fixture(scope="module")
def cutter(emu_built, tmp_path_factory):  # noqa: F811
    exe = str(tmp_path_factory.mktemp("cut") / "stream_cut")
    build = os.path.join(EMU, "_build")
    cmd = ["gcc", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "miniasm_amd", "host"), "-I" + os.path.join(ROOT, "miniasm_amd", "csrc"), os.path.join(ROOT, "tests", "stream_cut_main.c"),
           os.path.join(ROOT, "miniasm_amd", "host", "ingest_gpu.c"), "-L" + build, "-lminiasm_amd_emu", "-Wl,-rpath," + build, "-lz", "-lpthread", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and ("asan" in r.stdout or "ubsan" in r.stdout or "sanitize" in r.stdout):
        pytest.skip("the sanitizer runtime cannot be linked here: " + r.stdout[-300:])
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def run(exe, data, piece, chunk):
    r = subprocess.run([exe, str(piece), str(chunk)], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and not r.stderr, (piece, chunk, len(data), r.stderr.decode()[-2000:])
    word, pieces, nbytes, longest = r.stdout.split()
    assert word == b"OK" and int(nbytes) == len(data)
    return int(pieces), int(longest)


def line_of(n):
    """a line of exactly n bytes, newline included"""
    return b"L" * (n - 1) + b"\n"


def inputs(piece):
    out = {"empty": b"", "one_byte": b"x", "one_newline": b"\n", "no_newline": b"q" * 3000, "newlines_only": b"\n" * 3000}
    other = [b"short line %d\n" % i for i in range(60)]
    for d in (-1, 0, 1):
        exact = line_of(piece + d)
        out["first%+d" % d] = exact + b"".join(other)
        out["middle%+d" % d] = b"".join(other[:30]) + exact + b"".join(other[30:])
        out["last%+d" % d] = b"".join(other) + exact
        out["last_open%+d" % d] = b"".join(other) + exact[:-1]
    return out


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("piece", PIECES)
def test_cut_and_carry_on_small_inputs(piece, chunk, cutter):
    for name, data in inputs(piece).items():
        assert run(cutter, data, piece, chunk) == model(data, piece), (name, piece, chunk)


@pytest.fixture(scope="module")
def big():
    text = b"".join(gen(7000, 61))[:300000]
    text = text[:text.rfind(b"\n") + 1]
    assert len(text) > 299000 and text.endswith(b"\n")
    return text


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("piece", PIECES)
def test_cut_and_carry_on_ordinary_lines(piece, chunk, big, cutter):
    for data in (big, big[:-1]):
        got = run(cutter, data, piece, chunk)
        assert got == model(data, piece) and got[0] >= len(data) // piece
