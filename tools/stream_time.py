#!/usr/bin/env python3
"""Wall time and peak host memory of `miniasm x.paf.gz` and of `... | miniasm -` with the streamed ingest (host/ingest_gpu.c: ma_hit_ingest_stream) against the
yardstick: the PARENT COMMIT's binary on the same file (--parent: its miniasm, built from a checkout of the parent), never this code.  Input: pafgen text of
--lines lines, compressed by `gzip -1` (what `minimap2 ... | gzip -1` writes).  Per input kind (the .gz file; the plain text on stdin) the settings alternate:
the parent's command line, then this build's for every MA_INGEST_PIECE of --pieces (MiB), --reps rounds; the median of each setting is reported, with the
[T::ingest_gpu] stream laps of every streamed run and the child's ru_maxrss.  Every GPU step runs under its own `timeout -k 10`; the first one that fails ends
the script.  Result: one JSON line, also written to --out.

The two yardsticks: wall at the chosen piece size <= 1.05 x the parent's (the +- 5 % box spread README.md states), and on the 100 M-line file max RSS
below the parent's by at least half of the file's text size.

--no-cont: the same for `miniasm -R x.paf.gz` (the .gz file only; -R on stdin is the host reader's).  The input gets a length spread (pafgen -d 0.1), and every
run must report `dropped N contained reads` with N > 0.  The parent's -R inflates the whole text first; this build runs under MA_STREAM_NOCONT=1.  From
[T::ingest_gpu] stream: -R ... the early and late drops and the records held at the peak against the records kept are recorded: what the single pass costs in HBM.

  python tools/stream_time.py --parent ../parent/miniasm_amd/bin/miniasm --lines 10000000 --out profiles/stream_time_10M.json"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "miniasm_amd", "bin")
LAPS = ("producer", "upload", "parse", "fold", "waited-for-input")


def timed(cmd, env, stdin_path, limit):
    """one GPU step under its own time limit, as a child of its own so that ru_maxrss is its alone; anything but exit 0 ends the script"""
    e = dict(os.environ, MA_PIPE_TIMING="1")
    e.update(env)
    t0 = time.time()
    # (RUSAGE_CHILDREN is a maximum over all children so far: a helper process per run makes it this run's)
    code = ("import resource, subprocess, sys\n"
            "r = subprocess.run(sys.argv[1:], stdin=open(%r, 'rb') if %r else subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE)\n"
            "import zlib\n"
            "sys.stdout.write('%%d %%d %%d\\n' %% (r.returncode, resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss, zlib.crc32(r.stdout)))\n"
            "sys.stderr.write(r.stderr.decode(errors='replace'))\n" % (stdin_path or "", bool(stdin_path)))
    r = subprocess.run([sys.executable, "-c", code, "timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    dt = time.time() - t0
    log = r.stderr.decode(errors="replace")
    rc, rss_kib, crc = (int(x) for x in r.stdout.split())
    if rc != 0:
        sys.exit("%s: exit %d after %.1f s\n%s" % (" ".join(cmd), rc, dt, log[-3000:]))
    return dt, log, crc, rss_kib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's miniasm: the yardstick")
    ap.add_argument("--lines", type=int, default=10000000)
    ap.add_argument("--reads", type=int, default=300000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pieces", default="16,64,256,1024", help="MA_INGEST_PIECE values, MiB")
    ap.add_argument("--kinds", default="gz,stdin", help="gz: the .gz file by name; stdin: the plain text on stdin")
    ap.add_argument("--no-cont", action="store_true", help="time `miniasm -R x.paf.gz` under MA_STREAM_NOCONT=1 against the parent's -R (kind gz only)")
    ap.add_argument("--miniasm", default=os.path.join(BIN, "miniasm"), help="the binary under test")
    ap.add_argument("--limit", type=int, default=600, help="seconds per run")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    paf = os.path.join(a.tmp, "stream_time_%d.paf" % os.getpid())
    gz = paf + ".gz"
    pieces = [int(x) for x in a.pieces.split(",") if x]
    opts = ["-R"] if a.no_cont else []
    own = {"MA_STREAM_NOCONT": "1"} if a.no_cont else {}
    kinds = ["gz"] if a.no_cont else a.kinds.split(",")
    try:
        subprocess.run([os.path.join(BIN, "pafgen"), "-r", str(a.reads), "-n", str(a.lines), "-s", "4", "-o", paf] + (["-d", "0.1"] if a.no_cont else []), check=True, stderr=subprocess.DEVNULL)
        with open(gz, "wb") as g:
            subprocess.run(["gzip", "-1", "-c", paf], check=True, stdout=g)
        res = {"no_cont": bool(a.no_cont), "lines": a.lines, "reps": a.reps, "bytes": {"plain": os.path.getsize(paf), "gzip": os.path.getsize(gz)}, "kinds": {}}
        print("input ready: %d bytes of text, %d compressed" % (res["bytes"]["plain"], res["bytes"]["gzip"]), flush=True)
        for kind in kinds:
            settings = [("parent", a.parent, {})] + [("piece_%dMiB" % p, a.miniasm, dict(own, MA_INGEST_PIECE=str(p << 20))) for p in pieces]
            runs = {name: {"wall_s": [], "maxrss_kib": [], "laps_s": [], "pieces": [], "excl": []} for name, _, _ in settings}
            crcs = set()
            for rep in range(a.reps):
                for name, binary, env in settings:
                    cmd, stdin_path = ([binary] + opts + [gz], None) if kind == "gz" else ([binary] + opts + ["-"], paf)
                    dt, log, crc, rss = timed(cmd, env, stdin_path, a.limit)
                    crcs.add(crc)
                    runs[name]["wall_s"].append(round(dt, 4))
                    runs[name]["maxrss_kib"].append(rss)
                    m = re.search(r"\[T::ingest_gpu\] stream: pieces=(\d+) piece=\d+ B producer ([\d.]+) upload ([\d.]+) parse ([\d.]+) fold ([\d.]+) waited-for-input ([\d.]+) s", log)
                    if name != "parent":
                        if not m:
                            sys.exit("no [T::ingest_gpu] stream line:\n" + log[-2000:])
                        runs[name]["pieces"].append(int(m.group(1)))
                        runs[name]["laps_s"].append(dict(zip(LAPS, (float(x) for x in m.groups()[1:]))))
                    if a.no_cont:
                        d = re.search(r"dropped (\d+) contained reads", log)
                        if not d or int(d.group(1)) == 0:
                            sys.exit("the input does not trigger the -R pre-filter:\n" + log[-2000:])
                        x = re.search(r"\[T::ingest_gpu\] stream: -R dropped early (\d+) lines, late (\d+) lines \((\d+) records\); held (\d+) records at the peak, kept (\d+)", log)
                        if name != "parent":
                            if not x:
                                sys.exit("no [T::ingest_gpu] stream: -R line:\n" + log[-2000:])
                            runs[name]["excl"].append(dict(zip(("dropped_reads", "early_lines", "late_lines", "late_records", "peak_records", "kept_records"), [int(d.group(1))] + [int(v) for v in x.groups()])))
                    print("%s rep %d %s: %.2f s, max RSS %.0f MiB" % (kind, rep, name, dt, rss / 1024.0), flush=True)
            for name in runs:
                runs[name]["wall_median_s"] = round(statistics.median(runs[name]["wall_s"]), 4)
                runs[name]["maxrss_median_kib"] = int(statistics.median(runs[name]["maxrss_kib"]))
            base = runs["parent"]
            for name in runs:
                if name != "parent":
                    runs[name]["wall_vs_parent"] = round(runs[name]["wall_median_s"] / base["wall_median_s"], 4)
                    runs[name]["rss_saved_vs_text"] = round((base["maxrss_median_kib"] - runs[name]["maxrss_median_kib"]) * 1024.0 / res["bytes"]["plain"], 4)
            res["kinds"][kind] = {"runs": runs, "outputs_agree": len(crcs) == 1}
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        for p in (paf, gz):
            if os.path.exists(p):
                os.remove(p)


if __name__ == "__main__":
    main()
