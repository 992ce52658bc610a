#!/usr/bin/env python3
"""Wall time of `miniasm x.paf.gz` on a PLAIN gzip overlap file (one deflate stream, zlib level 1: what `minimap2 ... | gzip -1` writes) with the chunked device
inflater (MA_GZIP_DEVICE=1) against the same command with MA_GZIP_DEVICE=0 -- the yardstick: zlib on one host thread, the parent commit's road.  Input: pafgen
text of --lines lines (10 M), compressed by Python's zlib.  The two settings alternate, --reps runs each.  Every GPU step runs under its own `timeout -k 10`;
the first one that fails ends the script.  Result: one JSON line with both sets of walls, the [T::gzip] laps of every device run and whether the outputs
agree; also written to --out.  The device road counts as faster only if the SLOWEST of its runs beats the FASTEST of the yardstick's: that decides the
default of MA_GZIP_DEVICE.

  python tools/gzip_time.py --out profiles/gzip_time.json

--members 1,8,64: the same text as that many CONCATENATED gzip members (`cat part*.paf.gz`: equal pieces cut at arbitrary bytes), one file per count.  The
yardstick is then --parent, the PARENT COMMIT's miniasm on the same files with the same MA_GZIP_DEVICE=1 (it inflates one member on the device and leaves
several to zlib); without --parent it is this binary with MA_GZIP_DEVICE=0.  Rounds alternate; the median of --reps is reported per count, with the [T::gzip]
laps, the [T::gzip_members] laps (scan, heads) and, for the `windows` lap, this binary against the parent where both took the device (one member) -- and the
windows lap per member count, which says whether one workgroup per member beats the serial chain.  --reads-file: the reads file of `-f` instead (readgen's
FASTQ for the same overlaps) as --members members; the overlap file stays plain.

  python tools/gzip_time.py --members 1,8,64 --parent ../parent/miniasm_amd/bin/miniasm --out profiles/gzip_members_time.json"""
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


def write_members(src, gz, level, n):
    """the file as n gzip members of equal size, cut at arbitrary bytes"""
    size = os.path.getsize(src)
    with open(src, "rb") as f, open(gz, "wb") as g:
        for k in range(n):
            left = size * (k + 1) // n - size * k // n
            co = zlib.compressobj(level, zlib.DEFLATED, 31)
            while left:
                part = f.read(min(left, 1 << 22))
                left -= len(part)
                g.write(co.compress(part))
            g.write(co.flush())


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else None


def members_main(a):
    counts = [int(x) for x in a.members.split(",")]
    base = os.path.join(a.tmp, "gzip_time_%d" % os.getpid())
    paf, fq = base + ".paf", base + ".fq"
    made = [paf]
    try:
        subprocess.run([os.path.join(BIN, "pafgen"), "-r", str(a.reads), "-n", str(a.lines), "-s", "4", "-o", paf], check=True, stderr=subprocess.DEVNULL)
        src = paf
        if a.reads_file:
            subprocess.run([os.path.join(BIN, "readgen"), "-q", "-s", "9", "-o", fq, paf], check=True, stderr=subprocess.DEVNULL)
            made.append(fq)
            src = fq
        sides = [("this", a.miniasm, "1"), ("parent", a.parent, "1")] if a.parent else [("this", a.miniasm, "1"), ("zlib", a.miniasm, "0")]
        res = {"what": "reads file (-f)" if a.reads_file else "overlap file", "pafgen": "-r %d -n %d -s 4" % (a.reads, a.lines), "level": a.level, "reps": a.reps, "yardstick": sides[1][0],
               "bytes": {"plain": os.path.getsize(src)}, "members": {}}
        for n in counts:
            gz = "%s.%d.gz" % (src, n)
            made.append(gz)
            write_members(src, gz, a.level, n)
            cmd = ["-f", gz, paf] if a.reads_file else [gz]
            r = {"bytes": os.path.getsize(gz), "wall_s": {k[0]: [] for k in sides}, "gzip_lines": {k[0]: [] for k in sides}, "laps_ms": {k[0]: [] for k in sides}, "member_laps_ms": [], "ug_seq": {k[0]: [] for k in sides}}
            out_crc = set()
            for _ in range(a.reps):
                for name, binary, dev in sides:
                    env = {"MA_GZIP_DEVICE": dev}
                    if a.chunk:
                        env["MA_GZIP_CHUNK"] = str(a.chunk)
                    dt, log, crc = timed([binary] + cmd, env)
                    out_crc.add(crc)
                    r["wall_s"][name].append(round(dt, 4))
                    print("%d members, %s: %.2f s" % (n, name, dt), file=sys.stderr, flush=True)
                    m = re.search(r"^\[T::gzip\] reader=(\w+).*", log, re.M)
                    r["gzip_lines"][name].append(m.group(0) if m else None)
                    lap = m and re.search(r"upload ([\d.]+) sync\+count ([\d.]+) decode ([\d.]+) windows ([\d.]+) resolve ([\d.]+) crc ([\d.]+) ms", m.group(0))
                    r["laps_ms"][name].append(dict(zip(LAPS, map(float, lap.groups()))) if lap else None)
                    u = re.search(r"^\[T::ug_seq\] reader=(\w+)", log, re.M)
                    r["ug_seq"][name].append(u.group(1) if u else None)
                    mm = re.search(r"^\[T::gzip_members\] members=(\d+) candidates=(\d+) heads=(\d+) .*scan ([\d.]+) heads ([\d.]+) ms", log, re.M)
                    if name == "this" and mm:
                        r["member_laps_ms"].append({"members": int(mm.group(1)), "candidates": int(mm.group(2)), "heads_parsed": int(mm.group(3)), "scan": float(mm.group(4)), "heads": float(mm.group(5))})
            r["same_output"] = len(out_crc) == 1
            r["median_wall_s"] = {k: median(v) for k, v in r["wall_s"].items()}
            r["median_windows_ms"] = {k: median([x["windows"] for x in v if x]) for k, v in r["laps_ms"].items()}
            r["ratio_this_over_yardstick"] = round(r["median_wall_s"]["this"] / r["median_wall_s"][sides[1][0]], 4)
            res["members"][str(n)] = r
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        for v in made:
            if os.path.exists(v):
                os.remove(v)


def timed(cmd, env, limit=900):
    """one GPU step under its own time limit; anything but exit 0 ends the script (nothing more is started on the GPU)"""
    e = dict(os.environ, MA_PIPE_TIMING="1")
    for k in ("MA_BGZF_HOST", "MA_FASTX_HOST", "MA_FASTX_STREAM", "MA_GZIP_CAND_CAP"):
        e.pop(k, None)
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
    ap.add_argument("--members", default=None, help="member counts, e.g. 1,8,64: the text as that many concatenated gzip members (see above)")
    ap.add_argument("--reads-file", action="store_true", help="with --members: compress the -f reads file, not the overlap file")
    ap.add_argument("--parent", default=None, help="with --members: the parent commit's miniasm, the yardstick")
    a = ap.parse_args()
    if a.members:
        return members_main(a)
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
