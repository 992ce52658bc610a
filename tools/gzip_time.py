#!/usr/bin/env python3
"""Wall time of `miniasm x.paf.gz` on a PLAIN gzip overlap file (one deflate stream, zlib level 1: what `minimap2 ... | gzip -1` writes) with the chunked device
inflater (MA_GZIP_DEVICE=1) against the same command with MA_GZIP_DEVICE=0 -- the yardstick: zlib on one host thread, the parent commit's road.  Input: pafgen
text of --lines lines (10 M), compressed by Python's zlib.  The two settings alternate, --reps runs each.  Every GPU step runs under its own `timeout -k 10`;
the first one that fails ends the script.  Result: one JSON line with both sets of walls, the [T::gzip] laps of every device run and whether the outputs
agree; also written to --out.  The device road counts as faster only if the SLOWEST of its runs beats the FASTEST of the yardstick's: that decides the
default of MA_GZIP_DEVICE.

  python tools/gzip_time.py --out profiles/gzip_time.json"""
import argparse
import json
import os
import re
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "miniasm_amd", "bin")
LAPS = ("upload", "sync+count", "decode", "windows", "resolve", "crc")


def write_gzip(src, gz, level):
    co = zlib.compressobj(level, zlib.DEFLATED, 31)
    with open(src, "rb") as f, open(gz, "wb") as g:
        while True:
            part = f.read(1 << 22)
            if not part:
                break
            g.write(co.compress(part))
        g.write(co.flush())


def timed(cmd, env, limit=900):
    """one GPU step under its own time limit; anything but exit 0 ends the script (nothing more is started on the GPU)"""
    e = dict(os.environ, MA_PIPE_TIMING="1")
    e.pop("MA_BGZF_HOST", None)
    e.update(env)
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    dt = time.time() - t0
    log = r.stderr.decode(errors="replace")
    if r.returncode != 0:
        sys.exit("%s: exit %d after %.1f s\n%s" % (" ".join(cmd), r.returncode, dt, log[-3000:]))
    return dt, log, zlib.crc32(r.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10000000)
    ap.add_argument("--reads", type=int, default=300000)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=0, help="MA_GZIP_CHUNK (0: the default)")
    ap.add_argument("--miniasm", default=os.path.join(BIN, "miniasm"), help="the binary under test (tests/emu/_build/miniasm tries the script without a GPU)")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    paf = os.path.join(a.tmp, "gzip_time_%d.paf" % os.getpid())
    gz = paf + ".gz"
    try:
        subprocess.run([os.path.join(BIN, "pafgen"), "-r", str(a.reads), "-n", str(a.lines), "-s", "4", "-o", paf], check=True, stderr=subprocess.DEVNULL)
        write_gzip(paf, gz, a.level)
        res = {"lines": a.lines, "level": a.level, "bytes": {"plain": os.path.getsize(paf), "gzip": os.path.getsize(gz)}, "wall_s": {"device": [], "zlib": []}, "gzip_lines": [], "laps_ms": []}
        out_crc = set()
        for _ in range(a.reps):
            for name, dev in (("device", "1"), ("zlib", "0")):
                env = {"MA_GZIP_DEVICE": dev}
                if a.chunk:
                    env["MA_GZIP_CHUNK"] = str(a.chunk)
                dt, log, crc = timed([a.miniasm, gz], env)
                res["wall_s"][name].append(round(dt, 4))
                out_crc.add(crc)
                m = re.search(r"^\[T::gzip\] reader=(\w+).*", log, re.M)
                if name == "device":
                    if not m:
                        sys.exit("no [T::gzip] line:\n" + log[-2000:])
                    res["gzip_lines"].append(m.group(0))
                    lap = re.search(r"upload ([\d.]+) sync\+count ([\d.]+) decode ([\d.]+) windows ([\d.]+) resolve ([\d.]+) crc ([\d.]+) ms", m.group(0))
                    res["laps_ms"].append(dict(zip(LAPS, map(float, lap.groups()))) if lap else None)
        res["reader"] = sorted(set(re.search(r"reader=(\w+) reason=(\d+)", x).group(0) for x in res["gzip_lines"]))
        res["same_output"] = len(out_crc) == 1
        res["ratio_slowest_device_over_fastest_zlib"] = round(max(res["wall_s"]["device"]) / min(res["wall_s"]["zlib"]), 4)
        res["faster_beyond_spread"] = res["reader"] == ["reader=device reason=0"] and max(res["wall_s"]["device"]) < min(res["wall_s"]["zlib"])
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        for v in (paf, gz):
            if os.path.exists(v):
                os.remove(v)


if __name__ == "__main__":
    main()
