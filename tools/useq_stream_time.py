#!/usr/bin/env python3
"""Wall time, [T::ug_seq] laps and peak host memory of `miniasm -f reads.fq.gz x.paf` and of `... -f - x.paf` with the streamed device reader of the reads file
(csrc/useq.hip: mahip_useq_stream_*, host/unitig_gfa.c: ug_seq_stream) against the yardstick: the PARENT COMMIT's binary on the same files
(--parent: its miniasm, built from a checkout of the parent), never this build's own host road.  Input: the BASELINE configs[2] stand-in (pafgen -r 1200000
-n 40000000 -s 4, divided by --div); reads from readgen as FASTQ and as FASTA wrapped at 60, each compressed by `gzip -1`.  Per input (the two .gz files by name;
the plain FASTQ on `-f -`) the settings alternate: the parent's command line; this build with MA_FASTX_STREAM unset (nothing changed: within the box's +- 5 % of
the parent); this build with MA_FASTX_STREAM=1 for every MA_FASTX_PIECE of --pieces (MiB); --reps rounds, the median of each setting is reported, with the
[T::ug_seq] line's laps and the child's ru_maxrss.  Every GPU step runs under its own `timeout -k 10`; the first one that fails ends the script.  Result: one
JSON line, also written to --out.

  python tools/useq_stream_time.py --parent ../parent/miniasm_amd/bin/miniasm --div 4 --out profiles/useq_stream_time.json"""
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


def timed(cmd, env, stdin_path, limit):
    """one GPU step under its own time limit, as a child of its own so that ru_maxrss is its alone; anything but exit 0 ends the script"""
    e = dict(os.environ, MA_PIPE_TIMING="1")
    for k in ("MA_FASTX_STREAM", "MA_FASTX_PIECE", "MA_FASTX_HOST"):
        e.pop(k, None)
    e.update(env)
    t0 = time.time()
    # (RUSAGE_CHILDREN is a maximum over all children so far: a helper process per run makes it this run's)
    code = ("import resource, subprocess, sys, zlib\n"
            "r = subprocess.run(sys.argv[1:], stdin=open(%r, 'rb') if %r else subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE)\n"
            "sys.stdout.write('%%d %%d %%d\\n' %% (r.returncode, resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss, zlib.crc32(r.stdout)))\n"
            "sys.stderr.write(r.stderr.decode(errors='replace'))\n" % (stdin_path or "", bool(stdin_path)))
    r = subprocess.run([sys.executable, "-c", code, "timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    dt = time.time() - t0
    log = r.stderr.decode(errors="replace")
    rc, rss_kib, crc = (int(x) for x in r.stdout.split())
    if rc != 0:
        sys.exit("%s: exit %d after %.1f s\n%s" % (" ".join(cmd), rc, dt, log[-3000:]))
    return dt, log, crc, rss_kib


def ug_seq_line(log):
    """the [T::ug_seq] line -> dict(reader, handover, laps in ms by name, ug_seq_ms = their sum)"""
    t = [ln for ln in log.splitlines() if ln.startswith("[T::ug_seq]")]
    if len(t) != 1:
        return None
    head, _, tail = t[0].partition(" : ")
    out = {"reader": re.search(r"reader=(\w+)", head).group(1)}
    m = re.search(r"handover=(\w+)", head)
    if m:
        out["handover"] = m.group(1)
    m = re.search(r"pieces=(\d+)", head)
    if m:
        out["pieces"] = int(m.group(1))
    laps = {k: float(v) for k, v in re.findall(r"([a-z][a-z-]*) ([\d.]+)", tail)}
    out["laps_ms"] = laps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's miniasm: the yardstick")
    ap.add_argument("--div", type=int, default=1, help="divide the stand-in's 1.2 M reads / 40 M lines by this")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pieces", default="16,64,256", help="MA_FASTX_PIECE values, MiB")
    ap.add_argument("--inputs", default="fastq_gz,fasta60_gz,fastq_stdin")
    ap.add_argument("--miniasm", default=os.path.join(BIN, "miniasm"), help="the binary under test (tests/emu/_build/miniasm tries the script without a GPU)")
    ap.add_argument("--limit", type=int, default=600, help="seconds per run")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    base = os.path.join(a.tmp, "useq_stream_time_%d" % os.getpid())
    paf, fq, fa = base + ".paf", base + ".fq", base + ".fa"
    made = [paf, fq, fa, fq + ".gz", fa + ".gz"]
    pieces = [int(x) for x in a.pieces.split(",") if x]
    try:
        subprocess.run([os.path.join(BIN, "pafgen"), "-r", str(1200000 // a.div), "-n", str(40000000 // a.div), "-s", "4", "-o", paf], check=True, stderr=subprocess.DEVNULL)
        subprocess.run([os.path.join(BIN, "readgen"), "-q", "-s", "9", "-o", fq, paf], check=True, stderr=subprocess.DEVNULL)
        subprocess.run([os.path.join(BIN, "readgen"), "-w", "60", "-s", "9", "-o", fa, paf], check=True, stderr=subprocess.DEVNULL)
        for fn in (fq, fa):
            with open(fn + ".gz", "wb") as g:
                subprocess.run(["gzip", "-1", "-c", fn], check=True, stdout=g)
        res = {"pafgen": "-r %d -n %d -s 4" % (1200000 // a.div, 40000000 // a.div), "reps": a.reps, "bytes": {os.path.basename(p)[len(os.path.basename(base)):]: os.path.getsize(p) for p in made},
               "inputs": {}}
        print("inputs ready: %s" % res["bytes"], flush=True)
        for inp in a.inputs.split(","):
            reads, stdin_path = {"fastq_gz": (fq + ".gz", None), "fasta60_gz": (fa + ".gz", None), "fastq_stdin": ("-", fq)}[inp]
            settings = [("parent", a.parent, {}), ("stream_unset", a.miniasm, {})]
            settings += [("stream_%dMiB" % p, a.miniasm, {"MA_FASTX_STREAM": "1", "MA_FASTX_PIECE": str(p << 20)}) for p in pieces]
            runs = {name: {"wall_s": [], "maxrss_kib": [], "ug_seq": []} for name, _, _ in settings}
            crcs = set()
            for rep in range(a.reps):
                for name, binary, env in settings:
                    dt, log, crc, rss = timed([binary, "-f", reads, paf], env, stdin_path, a.limit)
                    crcs.add(crc)
                    u = ug_seq_line(log)
                    if name.startswith("stream_") and name != "stream_unset" and (u is None or u["reader"] != "stream"):
                        sys.exit("%s %s: the streamed reader did not run:\n%s" % (inp, name, log[-2000:]))
                    runs[name]["wall_s"].append(round(dt, 4))
                    runs[name]["maxrss_kib"].append(rss)
                    runs[name]["ug_seq"].append(u)
                    print("%s rep %d %s: %.2f s, max RSS %.0f MiB, %s" % (inp, rep, name, dt, rss / 1024.0, u), flush=True)
            for name in runs:
                runs[name]["wall_median_s"] = round(statistics.median(runs[name]["wall_s"]), 4)
                runs[name]["maxrss_median_kib"] = int(statistics.median(runs[name]["maxrss_kib"]))
                # wall of ma_ug_seq's reading: the calling thread's laps (the producer's run beside them); the host reader's line carries none, so only streamed runs have it
                sums = [sum(v for k, v in u["laps_ms"].items() if k != "producer") for u in runs[name]["ug_seq"] if u and u["reader"] == "stream"]
                runs[name]["ug_seq_median_ms"] = round(statistics.median(sums), 3) if sums else None
            for name in runs:
                if name != "parent":
                    runs[name]["wall_vs_parent"] = round(runs[name]["wall_median_s"] / runs["parent"]["wall_median_s"], 4)
            res["inputs"][inp] = {"runs": runs, "outputs_agree": len(crcs) == 1}
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        for p in made:
            if os.path.exists(p):
                os.remove(p)


if __name__ == "__main__":
    main()
