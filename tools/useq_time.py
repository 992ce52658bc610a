#!/usr/bin/env python3
"""Wall time of `miniasm -f reads paf` with the reads file read on the device, against the same command with MA_FASTX_HOST=1 and -- the yardstick -- against
the PARENT commit's binary on the same files (--parent path/to/its/miniasm; built elsewhere).  Input: the BASELINE configs[2] stand-in (pafgen -r 1200000
-n 40000000 -s 4, divided by --div) and three reads files made from it by readgen: FASTQ, FASTA on one line, FASTA wrapped at 60.  Every GPU step runs under its own
`timeout -k 10`; the first one that fails ends the script.  The reference (CPU only) runs once per file format AFTER the timed runs, so that it takes no page
cache or memory bandwidth from them: the three in the background side by side, each on a core of its own, each with its own wall time.  Result:
medians of --reps runs, the [T::ug_seq] laps, [T::ingest_gpu] load of the PAF for comparison, file sizes -> --out (JSON).

  python tools/useq_time.py --div 1 --parent /somewhere/parent/bin/miniasm --out profiles/useq_fastx.json"""
import argparse
import atexit
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "miniasm_amd", "bin")
REF = os.path.join(ROOT, "oracle", "_ref", "miniasm_ref")


def timed(cmd, out, env=None, limit=900):
    """one GPU step under its own time limit; anything but exit 0 ends the script (nothing more is started on the GPU)"""
    e = dict(os.environ, MA_PIPE_TIMING="1")
    e.update(env or {})
    t0 = time.time()
    with open(out, "wb") as f:
        r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=f, stderr=subprocess.PIPE, env=e)
    dt = time.time() - t0
    log = r.stderr.decode(errors="replace")
    if r.returncode != 0:
        sys.exit("%s: exit %d after %.1f s\n%s" % (" ".join(cmd), r.returncode, dt, log[-3000:]))
    return dt, log


def save(path, res):
    """after every step: a run that is cut short leaves what it had measured"""
    with open(path + ".tmp", "w") as f:
        json.dump(res, f, indent=1)
    os.replace(path + ".tmp", path)


def md5(path):
    return subprocess.run(["md5sum", path], stdout=subprocess.PIPE, check=True).stdout.split()[0].decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--div", type=int, default=1, help="divide the stand-in's 1.2 M reads / 40 M lines by this")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--miniasm", default=os.path.join(BIN, "miniasm"), help="the binary under test (tests/emu/_build/miniasm tries the script without a GPU)")
    ap.add_argument("--parent", default=None, help="the parent commit's miniasm binary")
    ap.add_argument("--tmp", default="/tmp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "useq_fastx.json"))
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--ref-limit", type=float, default=600, help="seconds after which a reference run still going is ended and recorded as such")
    ap.add_argument("--keep", action="store_true", help="leave the generated files in --tmp")
    a = ap.parse_args()
    if not a.keep:  # tens of GB: gone however the script ends
        atexit.register(lambda: [os.remove(os.path.join(a.tmp, fn)) for fn in os.listdir(a.tmp) if fn.startswith("useq_time")])
    paf = os.path.join(a.tmp, "useq_time.paf")
    subprocess.run([os.path.join(BIN, "pafgen"), "-r", str(1200000 // a.div), "-n", str(40000000 // a.div), "-s", "4", "-o", paf], check=True, stderr=subprocess.DEVNULL)
    res = {"pafgen": "-r %d -n %d -s 4" % (1200000 // a.div, 40000000 // a.div), "paf_bytes": os.path.getsize(paf), "reps": a.reps, "files": {}}
    forms = {"fastq": ["-q"], "fasta": [], "fasta_wrap60": ["-w", "60"]}
    for name, opts in forms.items():
        fn = os.path.join(a.tmp, "useq_time_%s" % name)
        subprocess.run([os.path.join(BIN, "readgen")] + opts + ["-s", "9", "-o", fn, paf], check=True, stderr=subprocess.DEVNULL)
        res["files"][name] = {"reads_bytes": os.path.getsize(fn)}
    for name in forms:
        fn, row = os.path.join(a.tmp, "useq_time_%s" % name), res["files"][name]
        runs = [("device", a.miniasm, {}), ("host", a.miniasm, {"MA_FASTX_HOST": "1"})]
        if a.parent:
            runs.append(("parent", a.parent, {}))
        for tag, binary, env in runs:
            walls, laps, loads = [], [], []
            for _ in range(a.reps):
                dt, log = timed([binary, "-f", fn, paf], fn + "." + tag + ".gfa", env)
                walls.append(dt)
                m = re.search(r"\[T::ug_seq\] (.*)", log)
                if m and "reader=device" in m.group(1):
                    laps.append({k: float(v) for k, v in re.findall(r"(load|index|lookup|place|download) ([0-9.]+)", m.group(1))})
                row.setdefault(tag, {})["ug_seq"] = m.group(1) if m else None
                m = re.search(r"\[T::ingest_gpu\] load ([0-9.]+) s", log)
                if m:
                    loads.append(float(m.group(1)))
            row[tag].update({"wall_s": walls, "median_s": statistics.median(walls), "md5": md5(fn + "." + tag + ".gfa")})
            if loads:  # the PAF's own file -> HBM lap, for comparison with the reads file's
                row[tag]["paf_load_s"] = statistics.median(loads)
                row[tag]["paf_load_GBps"] = res["paf_bytes"] / statistics.median(loads) / 1e9
            if laps:
                row[tag]["laps_ms"] = {k: statistics.median(x[k] for x in laps) for k in laps[0]}
                row[tag]["load_GBps"] = row["reads_bytes"] / row[tag]["laps_ms"]["load"] / 1e6
            if tag == "device" and len(laps) != a.reps:
                sys.exit("%s: the device reader did not run: %s" % (name, row[tag]["ug_seq"]))
            print(name, tag, "median %.3f s" % row[tag]["median_s"], row[tag]["ug_seq"] or "", flush=True)
            save(a.out, res)
        assert row["device"]["md5"] == row["host"]["md5"] and (not a.parent or row["parent"]["md5"] == row["device"]["md5"]), "outputs differ: %s" % name
        if a.parent:
            row["parent_over_device"] = row["parent"]["median_s"] / row["device"]["median_s"]
    w, u = res["files"]["fasta_wrap60"]["device"], res["files"]["fasta"]["device"]
    res["wrapped_over_unwrapped"] = {k: (w["median_s"] / u["median_s"] if k == "wall" else w["laps_ms"][k] / max(u["laps_ms"][k], 1e-6)) for k in ("wall", "index", "lookup", "place")}
    save(a.out, res)
    refs = {}
    try:
        if not a.no_ref and os.path.exists(REF):
            for k, name in enumerate(forms):
                fn = os.path.join(a.tmp, "useq_time_%s" % name)
                refs[name] = (subprocess.Popen(["taskset", "-c", str(2 + k), REF, "-f", fn, paf], stdout=open(fn + ".ref.gfa", "wb"), stderr=subprocess.DEVNULL), time.time())
        left = dict(refs)
        while left:
            for name, (p, t0) in list(left.items()):
                if p.poll() is not None:
                    fn = os.path.join(a.tmp, "useq_time_%s" % name)
                    res["files"][name]["reference"] = {"wall_s": time.time() - t0, "rc": p.returncode, "md5": md5(fn + ".ref.gfa")}
                    del left[name]
                elif time.time() - t0 > a.ref_limit:
                    p.kill()
                    p.wait()
                    res["files"][name]["reference"] = {"wall_s": None, "rc": "ended after %g s" % a.ref_limit}
                    del left[name]
            time.sleep(0.05)
    finally:
        for p, _ in refs.values():
            if p.poll() is None:
                p.kill()
                p.wait()
    for name in refs:
        r = res["files"][name]["reference"]
        assert r["rc"] != 0 or r["md5"] == res["files"][name]["device"]["md5"], "differs from the reference: %s" % name
        if r["rc"] == 0:
            res["files"][name]["reference_over_device"] = r["wall_s"] / res["files"][name]["device"]["median_s"]
    save(a.out, res)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
