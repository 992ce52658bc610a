"""bench.py helpers that can be checked without a GPU: the mapping from the timed scopes of the bench line to the kernels of
the committed rocprofv3 PMC runs (profiles/rNN_pmc_traffic_<workload>.json)."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(m)
    finally:
        sys.argv = argv
    return m


def test_pmc_traffic_scopes_sum_their_kernels():
    b = _bench()
    d = {k.replace("void ", ""): v for k, v in json.load(open(os.path.join(ROOT, "profiles", "r01_pmc_traffic_cfg2.json"))).items()}
    per = lambda v: v["fetch_bytes_x2"] + v["write_bytes"]
    fused = sum(per(v) for k, v in d.items() if k.startswith("k_hit_sub<true,"))
    plain = sum(per(v) for k, v in d.items() if k.startswith("k_hit_sub<false,"))
    assert fused > 0 and plain > 0
    if any(os.path.exists(os.path.join(ROOT, "profiles", "%s_pmc_traffic_cfg2.json" % r)) for r in ("r02", "r03a", "r03")):
        return  # a newer profile of this workload takes precedence: the arithmetic below is about the r01 file
    names, src = b.pmc_profile("cfg2")
    assert src.startswith("profiles/r01_pmc_traffic_cfg2.json")
    assert b.pmc_traffic(names, "k_hit_sub<cut+flt>") == round(fused)   # one launch of each size-class kernel per timed scope
    assert b.pmc_traffic(names, "k_hit_sub") == round(plain)
    assert abs(b.pmc_traffic(names, "k_hit_keys") - 800e6) < 5e6         # 640 MB of strided record reads + 160 MB of keys
    assert b.pmc_traffic(names, "no_such_kernel") is None
    assert b.pmc_profile("no_such_workload") == (None, None)             # counters belong to the profiled workload only
    names4, src4 = b.pmc_profile("cfg4")
    assert "commit" in src4 and b.pmc_traffic(names4, "k_hit_sub<gather>") > 1e10


def test_result_line_stays_short():
    """the round-6 record (22 KB on one line) was not read back where round 5's 15 KB line was: the result line keeps the figures and
    drops the prose and the legs' tables, which stay in the full record"""
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_cfg4.json")))
    line = b.compact_line(full)
    assert len(json.dumps(line)) < 12000
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "gfa_identical", "parity", "summary", "config"):
        assert line[k] == full[k], k
    assert line["roofline"]["sort_group"] == full["roofline"]["sort_group"]
    assert line["kernels"] == [{k: v for k, v in row.items() if k not in b.PROSE_KEYS} for row in full["kernels"]]
    assert all(leg["ms_per_step"] == full["legs"][n]["ms_per_step"] for n, leg in line["legs"].items() if "ms_per_step" in leg)
    assert "note" in full["roofline"] and "note" not in line["roofline"] and "kernels" not in line["legs"]["graph_heavy"]


def test_dump_outputs(tmp_path):
    """--dump-outputs: the GFA text whole when it fits the budget, else a seeded sample of whole lines; the same text gives the same files"""
    import numpy as np
    b = _bench()
    gfa = b"".join(b"S\tutg%06dl\t*\tLN:i:%d\n" % (i, 1000 + 37 * i) for i in range(2000))
    assert b.dump_outputs(str(tmp_path / "all"), gfa) == (2000, 2000)
    text = np.load(tmp_path / "all" / "gfa_text.npy")
    assert text.dtype == np.float32 and bytes(text.astype(np.uint8)) == gfa
    assert np.array_equal(np.load(tmp_path / "all" / "gfa_lines.npy"), np.arange(2000, dtype=np.float64))
    budget = 40000
    for d in ("s1", "s2"):
        kept, total = b.dump_outputs(str(tmp_path / d), gfa, budget=budget)
        assert 0 < kept < total == 2000
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= budget
    for f in ("gfa_text.npy", "gfa_lines.npy"):
        assert np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f))
    idx = np.load(tmp_path / "s1" / "gfa_lines.npy").astype(np.int64)
    lines = gfa.split(b"\n")
    assert np.all(np.diff(idx) > 0) and bytes(np.load(tmp_path / "s1" / "gfa_text.npy").astype(np.uint8)) == b"".join(lines[i] + b"\n" for i in idx)


def test_count_lines(tmp_path):
    """count_lines counts byte ranges in parallel: every newline once, whatever the size against the number of ranges"""
    import random
    b = _bench()
    rng = random.Random(3)
    for size in (0, 1, 5, 7, 8, 9, 4096, 100003):
        data = bytes(rng.choice(b"ab\n") for _ in range(size))
        p = tmp_path / ("t%d" % size)
        p.write_bytes(data)
        for workers in (1, 3, 8):
            assert b.count_lines(str(p), workers) == data.count(b"\n"), (size, workers)
