#!/usr/bin/env python3
"""Wall time of `miniasm x.paf` on a bgzip-compressed (BGZF) overlap file inflated on the device, against the same command on the plain file, on a plain gzip
file and -- the yardstick -- on the BGZF file with MA_BGZF_HOST=1, which is the parent commit's road (zlib on one host thread; --parent path/to/its/miniasm
checks once that the two agree).  Input: pafgen text of --lines lines (10 M), written as plain gzip and as BGZF by Python's zlib (no bgzip needed).  Every
GPU step runs under its own `timeout -k 10`; the first one that fails ends the script.  Result: one JSON line with the walls of --reps runs each, the
[T::bgzf] laps and the kernel's GB/s of text; also written to --out.  The new road counts as faster only if the SLOWEST of its runs beats the FASTEST of the
yardstick's.

  python tools/bgzf_time.py --out profiles/bgzf_time.json

--range g/W times ONE rank's load in isolation instead (what one GPU can say about `MA_GPUS=W`): mahip_bgzf_load_fd_range for rank g of W on the BGZF file,
in this process through the ctypes harness, next to the whole-file mahip_bgzf_load_fd on the same file in the same run -- the yardstick: what every rank did
before the ranges.  One untimed load of each first (code objects, pinned slots, the pool's allocations), then --reps of each in turn; each load ends in a
stream wait, the wall is a host clock around it.  The walk lap is the whole chain's in both: it does not shrink with W.

  python tools/bgzf_time.py --range 4/8 --out profiles/bgzf_range_time.json"""
import argparse
import json
import os
import re
import struct
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "miniasm_amd", "bin")
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def write_compressed(src, gz, bgz, level):
    """one pass over the text: plain gzip (one stream) and BGZF (members of 65280 bytes of text, as bgzip makes them)"""
    co = zlib.compressobj(level, zlib.DEFLATED, 31)
    with open(src, "rb") as f, open(gz, "wb") as g, open(bgz, "wb") as b:
        while True:
            part = f.read(65280)
            if not part:
                break
            g.write(co.compress(part))
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            d = c.compress(part) + c.flush()
            b.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(part), len(part)))
        g.write(co.flush())
        b.write(EOF_MARKER)


def timed(cmd, env=None, limit=900):
    """one GPU step under its own time limit; anything but exit 0 ends the script (nothing more is started on the GPU)"""
    e = dict(os.environ, MA_PIPE_TIMING="1")
    e.pop("MA_BGZF_HOST", None)
    e.update(env or {})
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    dt = time.time() - t0
    log = r.stderr.decode(errors="replace")
    if r.returncode != 0:
        sys.exit("%s: exit %d after %.1f s\n%s" % (" ".join(cmd), r.returncode, dt, log[-3000:]))
    return dt, log, zlib.crc32(r.stdout)


def write_bgzf(src, bgz, level):
    with open(src, "rb") as f, open(bgz, "wb") as b:
        while True:
            part = f.read(65280)
            if not part:
                break
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            d = c.compress(part) + c.flush()
            b.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(part), len(part)))
        b.write(EOF_MARKER)


def range_mode(a):
    import ctypes as C
    sys.path.insert(0, ROOT)
    import miniasm_amd as ma
    g, W = (int(x) for x in a.range.split("/"))
    paf = os.path.join(a.tmp, "bgzf_time_%d.paf" % os.getpid())
    bgz = paf + ".gz"
    try:
        subprocess.run([os.path.join(BIN, "pafgen"), "-r", str(a.reads), "-n", str(a.lines), "-s", "4", "-o", paf], check=True, stderr=subprocess.DEVNULL)
        print("text: %d bytes" % os.path.getsize(paf), file=sys.stderr, flush=True)
        write_bgzf(paf, bgz, a.level)
        text_bytes = os.path.getsize(paf)
        os.remove(paf)
        n = os.path.getsize(bgz)
        print("BGZF: %d bytes" % n, file=sys.stderr, flush=True)
        L, ctx, fd = ma.lib(), ma.Ctx(0), os.open(bgz, os.O_RDONLY)

        def whole():
            bi = ma.BgzfInfo()
            t0 = time.time()
            ma._chk(L.mahip_bgzf_load_fd(ctx.h, fd, n, ma.BGZF_TARGETS["paf"], C.byref(bi)), "bgzf_load_fd")
            dt = time.time() - t0
            info = ma._bgzf_dict(bi)
            ma._chk(L.mahip_paf_release(ctx.h), "paf_release")
            return dt, info, None

        def part():
            t0 = time.time()
            rg, info = ctx.bgzf_load_range(fd, n, g, W)
            dt = time.time() - t0
            ma._chk(L.mahip_paf_release(ctx.h), "paf_release")
            return dt, info, rg

        res = {"lines": a.lines, "rank": g, "world": W, "bytes": {"bgzf": n, "text": text_bytes}, "whole": {"wall_ms": [], "laps_ms": []}, "range": {"wall_ms": [], "laps_ms": []}}
        for name, fn in (("whole", whole), ("range", part)):  # untimed
            dt, info, rg = fn()
            if info["reason"] != "OK" or info["text_bytes"] != text_bytes:
                sys.exit("%s: the file was not inflated on the device: %r" % (name, info))
            if rg:
                res["range"]["what"] = rg
        for _ in range(a.reps):
            for name, fn in (("whole", whole), ("range", part)):
                dt, info, rg = fn()
                res[name]["wall_ms"].append(round(dt * 1e3, 3))
                res[name]["laps_ms"].append({k: round(v, 3) for k, v in info["laps_ms"].items()})
        os.close(fd)
        ctx.close()
        res["ratio_slowest_range_over_fastest_whole"] = round(max(res["range"]["wall_ms"]) / min(res["whole"]["wall_ms"]), 4)
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        for v in (paf, bgz):
            if os.path.exists(v):
                os.remove(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10000000)
    ap.add_argument("--reads", type=int, default=300000)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--miniasm", default=os.path.join(BIN, "miniasm"), help="the binary under test (tests/emu/_build/miniasm tries the script without a GPU)")
    ap.add_argument("--parent", default=None, help="the parent commit's miniasm binary: one run on the BGZF file, to check that MA_BGZF_HOST=1 is its road")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--out", default=None)
    ap.add_argument("--range", default=None, metavar="g/W", help="time mahip_bgzf_load_fd_range for rank g of W alone, next to the whole-file load (see above)")
    a = ap.parse_args()
    if a.range:
        return range_mode(a)
    paf = os.path.join(a.tmp, "bgzf_time_%d.paf" % os.getpid())
    files = {"plain": paf, "gzip": paf + ".plain.gz", "bgzf": paf + ".gz"}
    try:
        subprocess.run([os.path.join(BIN, "pafgen"), "-r", str(a.reads), "-n", str(a.lines), "-s", "4", "-o", paf], check=True, stderr=subprocess.DEVNULL)
        write_compressed(paf, files["gzip"], files["bgzf"], a.level)
        res = {"lines": a.lines, "bytes": {k: os.path.getsize(v) for k, v in files.items()}, "wall_s": {}, "laps_ms": [], "inflate_gbps": []}
        out_crc = set()
        for name, fn, env in (("plain", files["plain"], None), ("gzip", files["gzip"], None), ("bgzf", files["bgzf"], None), ("bgzf_host", files["bgzf"], {"MA_BGZF_HOST": "1"})):
            walls = []
            for _ in range(a.reps):
                dt, log, crc = timed([a.miniasm, fn], env)
                walls.append(round(dt, 4))
                out_crc.add(crc)
                m = re.search(r"^\[T::bgzf\] reader=(\w+).*", log, re.M)
                if name == "bgzf":
                    if not m or m.group(1) != "device":
                        sys.exit("the BGZF file was not inflated on the device:\n" + log[-2000:])
                    lap = re.search(r"walk ([\d.]+) upload ([\d.]+) inflate ([\d.]+) crc ([\d.]+) ms \(inflate ([\d.]+) GB/s", m.group(0))
                    res["laps_ms"].append(dict(zip(("walk", "upload", "inflate", "crc"), map(float, lap.groups()[:4]))))
                    res["inflate_gbps"].append(float(lap.group(5)))
            res["wall_s"][name] = walls
        res["same_output"] = len(out_crc) == 1
        if a.parent:
            dt, _, crc = timed([a.parent, files["bgzf"]])
            res["wall_s"]["parent_bgzf"] = [round(dt, 4)]
            res["same_output"] = res["same_output"] and crc in out_crc
        res["ratio_slowest_new_over_fastest_yardstick"] = round(max(res["wall_s"]["bgzf"]) / min(res["wall_s"]["bgzf_host"]), 4)
        res["faster_beyond_spread"] = max(res["wall_s"]["bgzf"]) < min(res["wall_s"]["bgzf_host"])
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        for v in files.values():
            if os.path.exists(v):
                os.remove(v)


if __name__ == "__main__":
    main()
