#!/usr/bin/env python3
"""Wall time, [T::text] laps and peak host memory of the record dumps (`miniasm -p paf -S2`, `-p paf`, `-p sg -S5`, `-p sg`, `-p bed`) with the device text writer
(csrc/text_dev.hpp) against the yardstick: the PARENT COMMIT's binary on the same file (--parent: its miniasm, built from a checkout of the parent),
never this build's own host road.  Input: the BASELINE configs[2] stand-in (pafgen -r 1200000 -n 40000000 -s 4, divided by --div), or with --small the 80 000-line
input of the tests (pafgen -r 3000 -n 80000 -s 41).  Per dump the settings alternate: the parent's command line; this build with MA_TEXT_DEVICE=0 (nothing changed:
within the parent's own spread); this build with MA_TEXT_DEVICE=1 for every MA_TEXT_SLAB of --slabs (Mi records).  --reps rounds (at least 5 for a result that
decides anything).  The unitig GFA (--dumps ug,ug_S6,ug_f; DESIGN 3.20, the ug kind) has inputs of its own: `ug` runs on the graph-heavy input (pafgen -L fixed,
50 lines per read: -r 2000000 -n 100000000 -s 4, divided by --div), `ug_S6` and `ug_f` (-p ug -f <a FASTQ readgen makes for that PAF>) on the noisy input
(-r 1000000 -n 50000000 -s 3 -L uniform -d 0.35 -x 0.03, divided by --div); `ug_f` also runs MA_TEXT_DEVICE=1 with MA_USEQ_PLAN_HOST=1 (the placement plan on the host, as
before it was made on the device) and records the [T::ug_plan] line and the `unitigs/graph to host` lap of [T::tail] of every run; median and min-max of each setting are reported, with the [T::text] line, the child's ru_maxrss and the CRC-32 of the output, which must be the
same in every setting.  Stdout of every run goes to one file in the work directory.  Every GPU step runs under its own `timeout -k 10`; the first one that fails
ends the script.  Result: one JSON line, also written to --out (merged into what --out already holds for other --div / dumps).

  python tools/text_time.py --parent ../parent/miniasm_amd/bin/miniasm --div 1 --out profiles/text_time.json"""
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
DUMPS = {"paf_S2": ["-p", "paf", "-S2"], "paf": ["-p", "paf"], "sg_S5": ["-p", "sg", "-S5"], "sg": ["-p", "sg"], "bed": ["-p", "bed"],
         "ug": ["-p", "ug"], "ug_S6": ["-p", "ug", "-S6"], "ug_f": ["-p", "ug"]}
UG_INPUT = {"ug": "graph", "ug_S6": "noisy", "ug_f": "noisy"}  # the unitig GFA's own inputs; ug_f adds -f <reads>


def timed(cmd, env, out_path, limit):
    """one GPU step under its own time limit, as a child of its own so that ru_maxrss is its alone; anything but exit 0 ends the script"""
    e = dict(os.environ, MA_PIPE_TIMING="1")
    for k in ("MA_TEXT_DEVICE", "MA_TEXT_SLAB", "MA_USEQ_PLAN_HOST"):
        e.pop(k, None)
    e.update(env)
    # (RUSAGE_CHILDREN is a maximum over all children so far: a helper process per run makes it this run's; the clock runs around the command alone)
    code = ("import resource, subprocess, sys, time\n"
            "t0 = time.time()\n"
            "r = subprocess.run(sys.argv[2:], stdin=subprocess.DEVNULL, stdout=open(sys.argv[1], 'wb'), stderr=subprocess.PIPE)\n"
            "sys.stdout.write('%d %d %.6f\\n' % (r.returncode, resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss, time.time() - t0))\n"
            "sys.stderr.write(r.stderr.decode(errors='replace'))\n")
    r = subprocess.run([sys.executable, "-c", code, out_path, "timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    log = r.stderr.decode(errors="replace")
    rc, rss_kib, dt = r.stdout.split()
    if int(rc) != 0:
        sys.exit("%s: exit %s after %s s\n%s" % (" ".join(cmd), rc.decode(), dt.decode(), log[-3000:]))
    import zlib
    crc, n = 0, 0
    with open(out_path, "rb") as f:
        for blk in iter(lambda: f.read(64 << 20), b""):
            crc, n = zlib.crc32(blk, crc), n + len(blk)
    return float(dt), log, crc, n, int(rss_kib)


def text_line(log):
    """the [T::text] line -> dict(road, slabs, slab_records, lines, bytes, slow_lines, laps_ms by name), None when the binary prints none (the parent)"""
    t = [ln for ln in log.splitlines() if ln.startswith("[T::text]")]
    if len(t) != 1:
        return None
    m = re.match(r"\[T::text\] (\S+) (device|host)", t[0])
    out = {"road": m.group(2)}
    m = re.search(r"(\d+) slabs of (\d+) records, (\d+) lines, (\d+) bytes, (?:(\d+) sequence bytes, )?(\d+) slow lines; names ([\d.]+)  export ([\d.]+)  format ([\d.]+)  copy\+write ([\d.]+) ms", t[0])
    if m:
        g = m.groups()
        out.update(slabs=int(g[0]), slab_records=int(g[1]), lines=int(g[2]), bytes=int(g[3]), slow_lines=int(g[5]),
                   laps_ms={"names": float(g[6]), "export": float(g[7]), "format": float(g[8]), "copy_write": float(g[9])})
        if g[4] is not None:
            out["seq_bytes"] = int(g[4])
    return out


def plan_laps(log):
    """-p ug -f: the [T::ug_plan] line (road; the plan's own ms on the device road, the reason otherwise; None: the binary prints none) and the `unitigs/graph to host`
    lap of [T::tail], ms -- the fetch that brings the members down and unpacks ma_ug_t when the plan is the host's (the host walk itself has no lap of its own)"""
    out = {"plan": None, "ug_to_host_ms": None}
    m = re.search(r"^\[T::ug_plan\] (device|host)(?:: .*; ([\d.]+) ms| \((.*)\))$", log, flags=re.M)
    if m:
        out["plan"] = {"road": m.group(1), "ms": float(m.group(2))} if m.group(1) == "device" else {"road": "host", "reason": m.group(3)}
    m = re.search(r"^\[T::tail\] names\+sub [\d.]+  device cleaners [\d.]+  unitigs/graph to host ([\d.]+) ms$", log, flags=re.M)
    if m:
        out["ug_to_host_ms"] = float(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's miniasm: the yardstick")
    ap.add_argument("--div", type=int, default=1, help="divide the stand-in's 1.2 M reads / 40 M lines by this")
    ap.add_argument("--small", action="store_true", help="the tests' 80 000-line input instead (the small end)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slabs", default="1,4,16", help="MA_TEXT_SLAB values, Mi records")
    ap.add_argument("--dumps", default=",".join(DUMPS))
    ap.add_argument("--miniasm", default=os.path.join(BIN, "miniasm"), help="the binary under test (tests/emu/_build/miniasm tries the script without a GPU)")
    ap.add_argument("--limit", type=int, default=300, help="seconds per run")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    base = os.path.join(a.tmp, "text_time_%d" % os.getpid())
    paf, out_path = base + ".paf", base + ".out"
    extra = {"graph": base + ".graph.paf", "noisy": base + ".noisy.paf", "reads": base + ".noisy.fq"}
    extra_gen = {"graph": ["-r", str(2000000 // a.div), "-n", str(100000000 // a.div), "-s", "4", "-L", "fixed"],
                 "noisy": ["-r", str(1000000 // a.div), "-n", str(50000000 // a.div), "-s", "3", "-L", "uniform", "-d", "0.35", "-x", "0.03"]}
    gen = ["-r", "3000", "-n", "80000", "-s", "41"] if a.small else ["-r", str(1200000 // a.div), "-n", str(40000000 // a.div), "-s", "4"]
    key = "small" if a.small else "div%d" % a.div
    slabs = [int(x) for x in a.slabs.split(",") if x]
    try:
        if any(d not in UG_INPUT for d in a.dumps.split(",")):
            subprocess.run([os.path.join(BIN, "pafgen")] + gen + ["-o", paf], check=True, stderr=subprocess.DEVNULL)
        res = {"pafgen": " ".join(gen), "reps": a.reps, "paf_bytes": os.path.getsize(paf) if os.path.exists(paf) else 0, "dumps": {}}
        print("input ready: %d bytes" % res["paf_bytes"], flush=True)
        for dump in a.dumps.split(","):
            paf_d, tail = paf, []
            if dump in UG_INPUT:  # made when the first dump asks for it
                paf_d = extra[UG_INPUT[dump]]
                if not os.path.exists(paf_d):
                    subprocess.run([os.path.join(BIN, "pafgen")] + extra_gen[UG_INPUT[dump]] + ["-o", paf_d], check=True, stderr=subprocess.DEVNULL)
                    res.setdefault("pafgen_" + UG_INPUT[dump], " ".join(extra_gen[UG_INPUT[dump]]))
                if dump == "ug_f":
                    if not os.path.exists(extra["reads"]):
                        subprocess.run([os.path.join(BIN, "readgen"), "-q", "-s", "7", "-o", extra["reads"], paf_d], check=True, stderr=subprocess.DEVNULL)
                    tail = ["-f", extra["reads"]]
            settings = [("parent", a.parent, {}), ("device_off", a.miniasm, {"MA_TEXT_DEVICE": "0"})]
            settings += [("device_%dMi" % s, a.miniasm, {"MA_TEXT_DEVICE": "1", "MA_TEXT_SLAB": str(s << 20)}) for s in slabs]
            if dump == "ug_f":  # the device text road with the plan forced to the host: what MA_TEXT_DEVICE=1 did before the plan was made on the device
                settings += [("device_%dMi_host_plan" % slabs[-1], a.miniasm, {"MA_TEXT_DEVICE": "1", "MA_TEXT_SLAB": str(slabs[-1] << 20), "MA_USEQ_PLAN_HOST": "1"})]
            runs = {name: {"wall_s": [], "maxrss_kib": [], "text": None} for name, _, _ in settings}
            crcs, sizes = set(), set()
            for rep in range(a.reps):
                for name, binary, env in settings:
                    dt, log, crc, n, rss = timed([binary] + DUMPS[dump] + tail + [paf_d], env, out_path, a.limit)
                    crcs.add(crc), sizes.add(n)
                    t = text_line(log)
                    if name == "device_off" and dump in UG_INPUT:  # (with the switch off a -p ug run prints what the parent prints: no [T::text] line)
                        if t is not None:
                            sys.exit("%s %s: a [T::text] line with the switch off:\n%s" % (dump, name, log[-2000:]))
                    elif name.startswith("device_") and (t is None or t["road"] != ("host" if name == "device_off" else "device")):
                        sys.exit("%s %s: the wrong formatter ran:\n%s" % (dump, name, log[-2000:]))
                    runs[name]["wall_s"].append(round(dt, 4))
                    runs[name]["maxrss_kib"].append(rss)
                    runs[name]["text"] = t
                    if dump == "ug_f":
                        pl = plan_laps(log)
                        runs[name].setdefault("ug_to_host_ms", []).append(pl["ug_to_host_ms"])
                        runs[name].setdefault("plan_ms", []).append(pl["plan"]["ms"] if pl["plan"] and pl["plan"]["road"] == "device" else None)
                        runs[name]["plan"] = pl["plan"]
                        want_road = None if name in ("parent", "device_off") else "host" if name.endswith("_host_plan") else "device"
                        if (pl["plan"] or {}).get("road") != want_road:
                            sys.exit("%s %s: the wrong placement plan ran:\n%s" % (dump, name, log[-2000:]))
                    print("%s %s rep %d %s: %.3f s, max RSS %.0f MiB, %d bytes, %s" % (key, dump, rep, name, dt, rss / 1024.0, n, t), flush=True)
            for name in runs:
                w = runs[name]["wall_s"]
                runs[name].update(wall_median_s=round(statistics.median(w), 4), wall_min_s=min(w), wall_max_s=max(w), maxrss_median_kib=int(statistics.median(runs[name]["maxrss_kib"])))
            spread = runs["parent"]["wall_max_s"] - runs["parent"]["wall_min_s"]
            for name in runs:
                if name != "parent":
                    runs[name]["wall_vs_parent"] = round(runs[name]["wall_median_s"] / runs["parent"]["wall_median_s"], 4)
                    runs[name]["below_parent_by_more_than_its_spread"] = runs[name]["wall_median_s"] < runs["parent"]["wall_median_s"] - spread
            res["dumps"][dump] = {"runs": runs, "parent_spread_s": round(spread, 4), "output_bytes": sorted(sizes), "crc32": sorted("%08x" % c for c in crcs), "outputs_agree": len(crcs) == 1}
            if len(crcs) != 1:
                sys.exit("%s %s: the settings' outputs differ: %s" % (key, dump, res["dumps"][dump]["crc32"]))
        print(json.dumps({key: res}))
        if a.out:
            whole = {}
            if os.path.exists(a.out):
                with open(a.out) as f:
                    whole = json.load(f)
            whole.setdefault(key, {"pafgen": res["pafgen"], "reps": a.reps, "paf_bytes": res["paf_bytes"], "dumps": {}})
            whole[key]["dumps"].update(res["dumps"])
            with open(a.out, "w") as f:
                json.dump(whole, f, indent=1, sort_keys=True)
                f.write("\n")
    finally:
        for p in (paf, out_path) + tuple(extra.values()):
            if os.path.exists(p):
                os.remove(p)


if __name__ == "__main__":
    main()
