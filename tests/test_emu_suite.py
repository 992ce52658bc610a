"""The `-m gpu` parity tests, run WITHOUT a GPU: the product's kernel sources (miniasm_amd/csrc/*.hip, unmodified) are
compiled a second time for the CPU against tests/emu -- a fiber-based stand-in for the HIP runtime that models wave64
shuffles, ballots, DPP controls, barriers and atomics -- and the GPU test modules are run against that build in a
subprocess (`-p emu_plugin` swaps the library path of the ctypes harness).  This is test infrastructure: it proves the
kernels' logic (every stage bit-exact against the oracle and the reference library) on the box that has no GPU; it says
nothing about speed, stream ordering or memory-model behaviour, which only the `-m gpu` run on an MI355X covers.

By default a subset runs; MA_EMU_FULL=1 runs every GPU test module except the BASELINE-scale inputs and the RCCL tests (about 25 minutes
on 8 cores).  The default `-m "not gpu"` selection of this file took 12 min 46 s of wall time on 8 cores before tests/test_gpu_graph_edges.py was
added; that module adds about half a minute (15 s in normal order, 16 s reversed with guard pages), so none of its cases is held back for MA_EMU_FULL.
tests/test_gpu_clean_edges.py adds about a minute: 30 s in normal order (its three child processes and the 8 193-bubble input, 2 s, included) and 30 s
reversed with guard pages.  Its 196 608 / 196 609-entry probes take 63 s alone and are held back for MA_EMU_FULL=1, so by default the CPU build does not reach
bubble tiers 3 and 4; they run by default under `-m gpu`.
tests/test_gpu_sort_edges.py adds about three minutes: 62 to 69 s in normal order for its 217 cases (the 526 337-id case takes under a second, so it is not held
back) and 131 s reversed with guard pages, the latter measured while other builds were using the box.  Its production-form case (67 M records) skips itself on
the CPU build.
tests/test_gpu_ingest_edges.py adds about two minutes: 45 s in normal order for its 68 tests (about 700 texts; the group-fallback texts of 4 to 8.5 MiB take
4 s together, so none is held back for MA_EMU_FULL) and 58 s reversed with guard pages, both measured while other builds were using the box.
tests/test_gpu_shard_edges.py adds about three minutes: 71 s in normal order for its 60 tests (about 90 walks of the sharded head on up to eight contexts; the slowest
test, four walks over the 56 000-record input, takes 7 s, so none is held back for MA_EMU_FULL) and 100 s reversed with guard pages, the latter measured while other
builds were using the box.
tests/test_gpu_xfer_edges.py and tests/test_gpu_scan_edges.py (run by tests/test_xfer_scan_emu.py) add about two minutes: 23 s + 26 s in normal order (70 + 25
tests; the 132 MiB round trips take about a second each, the three 2048 x 2048-element scan cases 5 to 6 s each, so nothing is held back for MA_EMU_FULL), 43 s
together reversed with guard pages, and 10 s of build + 13 s of run for the copy workers under the thread sanitizer.
tests/test_gpu_ingest_shard_edges.py adds about three quarters of a minute: 16 s in normal order for its 141 tests (five runs of 2, 3, 5, 8 and 3 child processes, 139
cases in all: 2.3 s, 2.2 s, 3.0 s, 5.8 s and 0.3 s of wall time, most of it process start-up, so nothing is held back for MA_EMU_FULL) and 26 s reversed with guard
pages (2.8 s, 2.9 s, 4.9 s, 13.0 s and 0.4 s), both on 16 cores.
tests/test_gpu_ingest_stream_edges.py (run by tests/test_ingest_stream_emu.py) adds about a minute and three quarters: 50 s in normal order for its 69 tests and 50 s reversed
with guard pages and the pool off, both on 8 cores.  Its slowest case, the refusal in the middle of a stream (five runs of the command line, the module's shared
input included), takes 14 s, the two truncated gzip streams 4 s each, the two crowded probe chains 2 to 4 s each and the child process with the pool off 5 s, so nothing
is held back for MA_EMU_FULL.  tests/test_stream_cut_cpu.py (the cut-and-carry reader as a stand-alone program under the address and undefined-behaviour
sanitizers) takes 5 s, its build included."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
FULL = os.environ.get("MA_EMU_FULL", "0") == "1"


@pytest.fixture(scope="module")
def emu_built(built):
    r = subprocess.run(["make", "-C", EMU, "-j8", "all", "_build/emu_selftest"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return True


def run_gpu_tests(args, timeout, extra_env=None):
    env = dict(os.environ)
    env.update(extra_env or {})
    env["PYTHONPATH"] = EMU + os.pathsep + env.get("PYTHONPATH", "")
    env.pop("MINIASM_AMD_LIB", None)
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-p", "emu_plugin", "-x", "-q", "-p", "no:cacheprovider"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    tail = r.stdout[-6000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and " failed" not in tail, tail
    return tail


def test_emulator_selftest(emu_built):
    """the stand-in itself: shuffles, ballot, every DPP control the kernels use, barriers with early exits, divergent loops"""
    r = subprocess.run([os.path.join(EMU, "_build", "emu_selftest")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout


def test_kernels_stage_parity_on_cpu(emu_built):
    """tests/test_gpu_parity.py: every HIP pass against the oracle and the reference library (incl. the second tiers)"""
    sel = [] if FULL else ["-k", "lognormal or noisy or lowid or deep_groups or sort_random or sub_ or random_hit"]
    run_gpu_tests(["tests/test_gpu_parity.py"] + sel, 3000)


def test_fused_hit_passes_on_cpu(emu_built):
    """tests/test_gpu_fused_hits.py: the fused hit passes of the resident pipeline stage by stage against the oracle and the reference library,
    the reads on every size edge of the coverage kernel under run stride 0 / 1 / 2 (the deep_vertices input only with MA_EMU_FULL=1: a minute alone)"""
    run_gpu_tests(["tests/test_gpu_fused_hits.py"] + ([] if FULL else ["-k", "not deep_vertices"]), 3000)


@pytest.mark.parametrize("stride", ["1", "0"])
def test_sort_does_not_depend_on_the_run_stride_hint(stride, emu_built):
    """the hit sort takes RUNS of records when told how a query's own records stand in the array (mahip_set_run_stride; the stage tests default to 2 = ma_hit_read's
    layout).  A hint that does not fit the data -- stride 1 on mirrored records: too few runs; random hit arrays under any stride -- must cost time, never correctness:
    the same stage tests with the other hints (0 = no hint: one key per record)"""
    run_gpu_tests(["tests/test_gpu_parity.py", "-k", "lognormal or noisy or sort_random or random_hit or deep_groups"], 3000, {"MA_TEST_RUN_STRIDE": stride})


def test_kernels_with_reversed_schedule_and_guard_pages(emu_built):
    """the same kernels with lanes, waves and blocks executed in DESCENDING order (code that leans on lock-step execution or on launch order
    without a barrier breaks) and every device allocation ending at a faulting page (an out-of-bounds access crashes)"""
    env = {"EMU_ORDER": "reverse", "EMU_GUARD": "1", "MA_DEV_POOL": "0"}  # (the pool hands out pieces of bigger allocations: no guard page behind them)
    run_gpu_tests(["tests/test_gpu_parity.py", "-k", "noisy or deep_groups or sort_random", "tests/test_gpu_ingest.py"], 3000, env)
    run_gpu_tests(["tests/test_gpu_fused_hits.py", "-k", "group_size_edges"], 3000, env)  # tier B's global scratch (4097 and 9001 hits) ends at a guard page too
    run_gpu_tests(["tests/test_gpu_graph_edges.py"], 3000, env)  # the arc sort's rows, the reduction's neighbour lists and the cleanup's tails at their size edges
    run_gpu_tests(["tests/test_gpu_clean_edges.py"] + CLEAN_EDGES_SEL, 3000, env)  # the bubble tables, stacks and stamp arrays at their borders; the wave form without lock-step
    run_gpu_tests(["tests/test_gpu_ingest_edges.py"], 3000, env)  # the staged over-read in front of a tile, the n + 64 padding of the text, s_lend[256], lstart[L], cnt[n_gran]
    run_gpu_tests(["tests/test_gpu_sort_edges.py"], 3000, env)  # rkey[r00 - 1], the n + 128 padding of sidx, the rows / chunk sums / totals of the radix histograms and the tile minima of the group starts
    run_gpu_tests(["tests/test_gpu_shard_edges.py"], 3000, env)  # the Rr-sized grids of the coverage sweeps and of the arc sort on a read range, goff[q_hi], the stride-padded row blocks of the imports
    run_gpu_tests(["tests/test_gpu_ingest_shard_edges.py"], 3000, env)  # the stride-padded row and name blocks of the merged dictionary, keep[] / pos[] of the route's extraction, the send and receive buffers of the exchange


def test_kernels_graph_api_on_cpu(emu_built):
    """tests/test_gpu_graph_api.py, test_gpu_graph_fuzz.py: device cleaners and unitigs after every call, through the per-symbol ABI (pipeline graphs,
    hand-made rings and hubs, random graphs with random scripts)"""
    run_gpu_tests(["tests/test_gpu_graph_api.py", "tests/test_gpu_graph_fuzz.py"] + ([] if FULL else ["-k", "not noisy_big"]), 1800)


def test_graph_size_edges_on_cpu(emu_built):
    """tests/test_gpu_graph_edges.py: the graph kernels at every size edge they branch on (arcs per read, arcs per vertex and per expanded neighbour, arc counts
    of the cleanup), every one against the oracle and the reference library; a quarter of a minute"""
    run_gpu_tests(["tests/test_gpu_graph_edges.py"], 1800)


def test_sort_size_edges_on_cpu(emu_built):
    """tests/test_gpu_sort_edges.py: the hit sort's own result (sidx, goff) and its report at every size the sort branches on, runs path, record paths, shard
    form and order sort; only the production-form case (67 M records) needs a real device and skips itself here"""
    run_gpu_tests(["tests/test_gpu_sort_edges.py"], 1800)


def test_shard_edges_on_cpu(emu_built):
    """tests/test_gpu_shard_edges.py: the sharded head phase by phase in one process (one context per rank, the exchanges done by the test through the ABI) on
    read-range tables with borders at the deep and the many-arc reads, empty ranges, one rank owning every read, a world larger than the dictionary; against
    the oracle, the one-context chain and the reference library"""
    run_gpu_tests(["tests/test_gpu_shard_edges.py"], 1800)


def test_ingest_shard_edges_on_cpu(emu_built):
    """tests/test_gpu_ingest_shard_edges.py: the sharded PAF ingest and the record routing rank by rank -- 2, 3, 5 and 8 child processes over the shared-memory
    double, each with a context of the CPU build -- against tests/pafmodel.py on the whole text and the stated balance rule; a quarter of a minute"""
    run_gpu_tests(["tests/test_gpu_ingest_shard_edges.py"], 1800)


CLEAN_EDGES_SEL = [] if FULL else ["-k", "not border[3]"]  # the 196 608 / 196 609-entry probes (tiers 3 and 4): MA_EMU_FULL=1


def test_cleaner_and_unitig_size_edges_on_cpu(emu_built):
    """tests/test_gpu_clean_edges.py: cleaners, unitigs and the scan at every size they branch on, the child-process cases included, every one against the
    reference library"""
    run_gpu_tests(["tests/test_gpu_clean_edges.py"] + CLEAN_EDGES_SEL, 3000)


def test_tie_filter_on_cpu(emu_built):
    """tests/test_gpu_cli.py: push conflicts the reference's arc sort cannot see -- the hit walk is skipped, every dump equals the reference's byte for byte; and the
    realistic inputs (jittered coordinates, lines grouped by target) through both walks"""
    run_gpu_tests(["tests/test_gpu_cli.py", "-k", "out_of_sight or in_sight_only or (tie_rich and jitter and default)"], 3000)


def test_ingest_size_edges_on_cpu(emu_built):
    """tests/test_gpu_ingest_edges.py: the device PAF reader stage by stage (tile parser against byte-wise kernel, tile geometry, group fallback, stale bl, both
    dictionary forms and the table growth, query runs, records, -R) against a model, the host reader and the reference library; three quarters of a minute"""
    run_gpu_tests(["tests/test_gpu_ingest_edges.py"], 1800)


def test_kernels_ingest_on_cpu(emu_built):
    """tests/test_gpu_ingest.py: device PAF parser + dictionary against the host reader and the reference"""
    run_gpu_tests(["tests/test_gpu_ingest.py"], 1800)


@pytest.mark.skipif(not FULL, reason="MA_EMU_FULL=1 runs the CLI and sharded suites on the emulator (about 20 minutes)")
def test_cli_suite_on_cpu(emu_built):
    run_gpu_tests(["tests/test_gpu_cli.py", "-k", "not baseline_scale"], 5000)


def test_sharded_suite_on_cpu(emu_built):
    """tests/test_gpu_sharded.py: `MA_GPUS=N miniasm` -- host/sharded.c, N forked ranks over the shared-memory double of the collectives --
    against the single-rank run and the reference binary (tie-rich input included).  The torch-driven virtual-rank test needs a real device."""
    sel = "not rccl and not virtual_ranks" + ("" if FULL else " and (2-lognormal or 3-noisy or tie_order or hold_only or their_own_records or never_leaves or byte_range_ingest_at_its_edges)")
    run_gpu_tests(["tests/test_gpu_sharded.py", "-k", sel], 5000)


@pytest.mark.parametrize("mode", ["options", "text", "ranks"])
def test_randomised_reference_vs_kernels_on_cpu(mode, emu_built):
    """tools/fuzz_emu.py, a fixed slice of it: random generator parameters x random options x every dump format ("options"), damaged PAF text
    ("text"), and the same through `MA_GPUS=2` ("ranks"): the reference binary's bytes against the CPU build of the kernels"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "miniasm_ref")):
        pytest.skip("oracle/_ref not built")
    n = 150 if FULL else 30
    args = {"options": ["--seed", "101"], "text": ["--seed", "102", "--text"], "ranks": ["--seed", "103", "--ranks", "2"]}[mode]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_emu.py"), "--cases", str(n)] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=3000)
    assert r.returncode == 0 and "0 mismatches" in r.stdout.splitlines()[-1], r.stdout[-3000:]


@pytest.mark.parametrize("mode", ["default", "no_tail_ctx"])
def test_bench_py_runs_on_the_cpu_build(mode, emu_built, tmp_path):
    """bench.py itself -- Workload (file -> device parse -> records by read range), Runner with its worker thread, the profiled steps, the
    text-resident leg, the reference run and the GFA comparison, the JSON line -- executed against the CPU build of the kernels with a numpy-backed
    stand-in for the few torch calls it makes (tests/emu/fake_torch).  Default: the second context + hand-over thread; `no_tail_ctx`: one context.
    Numbers mean nothing here; the control flow, the parity check and the shape of the line do."""
    import json
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "miniasm_ref")):
        pytest.skip("oracle/_ref not built")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.path.join(EMU, "fake_torch") + os.pathsep + env.get("PYTHONPATH", "")
    env["MINIASM_AMD_LIB"] = os.path.join(EMU, "_build", "libminiasm_amd_emu.so")
    env["MA_BENCH_DIR"] = str(tmp_path)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--reads", "2500", "--lines", "70000", "--seed", "5", "--steps", "3", "--warmup", "1", "--full", "--no-legs",
           "--dump-outputs", str(tmp_path / "dump")]
    if mode == "no_tail_ctx":
        cmd.append("--no-tail-ctx")
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "bench.py prints ONE JSON line"
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["vs_baseline"] is None
    assert d["gfa_identical"] is True and d["parity"]["gfa_md5"] == d["parity"]["ref_md5"]
    assert d["roofline"]["bound"] == "hbm" and d["cpu_baseline"]["kind"] == "reference" and d["cpu_baseline"]["cores"] == 1
    assert d["from_text"] and d["from_text"]["value"] > 0
    assert ("second context" in d["config"]["pipelining"]) == (mode == "default")
    assert d["roofline"]["sort_group"]["alg_bytes_per_step"] == 112.0 * d["config"]["per_gpu_hits"] and "k_hit_sub<gather>" in d["roofline"]["sort_group"]["kernels"]
    assert all(k["alg_GBs"] is None for k in d["kernels"] if k["name"] in ("k_hit_keys", "k_radix_scatter", "k_radix_hist", "k_hit_goff"))
    import hashlib
    import numpy as np
    dumped = bytes(np.load(tmp_path / "dump" / "gfa_text.npy").astype(np.uint8))  # --dump-outputs: the GFA of the last timed step, whole at this size
    assert hashlib.md5(dumped).hexdigest() == d["parity"]["gfa_md5"]
    assert json.load(open(d["full_record"]))["value"] == d["value"]


@pytest.mark.parametrize("ranks", [1, 2])
def test_plain_bench_py_run_on_the_cpu_build(ranks, emu_built, tmp_path):
    """bench.py without --full, on the CPU build: the headline only (no reference run, no instrumented steps, no legs), on a text the run
    writes afresh and removes once it is in HBM; the GFA of its last timed step (--dump-outputs) is the reference's on the same seeded text.
    Two ranks: launched as the driver launches them (see test_bench_py_on_two_ranks_on_the_cpu_build), rank 0 writes the text for both."""
    import json
    import numpy as np
    ref_bin = os.path.join(ROOT, "oracle", "_ref", "miniasm_ref")
    if not os.path.exists(ref_bin):
        pytest.skip("oracle/_ref not built")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.path.join(EMU, "fake_torch") + os.pathsep + env.get("PYTHONPATH", "")
    env["MINIASM_AMD_LIB"] = os.path.join(EMU, "_build", "libminiasm_amd_emu.so")
    work = tmp_path / "work"
    env["MA_BENCH_DIR"] = str(work)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--reads", "2500", "--lines", "70000", "--seed", "5", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "dump")]
    procs = []
    for rank in range(ranks):
        e = env if ranks == 1 else dict(env, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(ranks), MASTER_ADDR="127.0.0.1",
                                        MASTER_PORT=str(20000 + os.getpid() % 20000), MA_FAKE_DIST_DIR=str(tmp_path), MA_BENCH_ONE_GPU_DEBUG="1")
        procs.append(subprocess.Popen(cmd + ([] if ranks == 1 else ["--gpus", str(ranks)]), cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        try:
            o, err = p.communicate(timeout=1800)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, err[-3000:]
        outs.append(o)
    lines = [l for l in outs[0].splitlines() if l.strip()]
    assert len(lines) == 1 and all(o.strip() == "" for o in outs[1:]), "rank 0 prints ONE JSON line"
    d = json.loads(lines[0])
    assert d["n_gpus"] == ranks and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["vs_baseline"] is None
    assert (d["metric"], d["unit"], d["higher_is_better"], d["dtype"]) == ("PAF overlaps processed/sec (hit-filter->trans-reduce->GFA)", "overlaps/s", True, "u32")
    assert d["cpu_baseline"] is None and d["gfa_identical"] is None and d["roofline"] is None and d["kernels"] == []
    assert d["legs"] == {} and d["latency"] is None and d["e2e"] is None and d["from_text"] is None
    assert not [f for _, _, fs in os.walk(tmp_path) for f in fs if ".paf" in f], "the run's text is gone, and no other text was written"
    paf = str(tmp_path / "same.paf")
    subprocess.run([os.path.join(ROOT, "miniasm_amd", "bin", "pafgen"), "-r", "2500", "-n", "70000", "-s", "5", "-o", paf], check=True, stderr=subprocess.DEVNULL)
    ref = subprocess.run([ref_bin, paf], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    with open(paf, "rb") as f:
        assert d["config"]["global_overlaps"] == f.read().count(b"\n")
    assert bytes(np.load(tmp_path / "dump" / "gfa_text.npy").astype(np.uint8)) == ref


@pytest.mark.parametrize("grid", [0, 16])
def test_bench_py_on_two_ranks_on_the_cpu_build(grid, emu_built, tmp_path):
    """`bench.py --gpus 2` as the driver launches it (one process per rank, RANK / WORLD_SIZE / MASTER_* in the environment), on the CPU build:
    the control plane is a file-based stand-in for torch.distributed, the collectives go through the shared-memory double
    (MA_BENCH_ONE_GPU_DEBUG, the hook bench.py has for one-GPU boxes), rank 0 runs its tail on a second context.  A one-rank run first leaves
    the reference's GFA in the work directory; the two-rank line must say `gfa_identical: true` against it and report whole-job throughput."""
    import json
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "miniasm_ref")):
        pytest.skip("oracle/_ref not built")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.path.join(EMU, "fake_torch") + os.pathsep + env.get("PYTHONPATH", "")
    env["MINIASM_AMD_LIB"] = os.path.join(EMU, "_build", "libminiasm_amd_emu.so")
    env["MA_BENCH_DIR"] = str(tmp_path)
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--reads", "2500", "--lines", "70000", "--seed", "5", "--steps", "2", "--warmup", "1", "--full"]
    if grid:  # a tie-rich input: the ranks (which hold only their own records, and say where they stood in the input) have to restore the reference's order of tied hits
        base += ["--grid", str(grid), "--model", "uniform", "--reads", "3000", "--lines", "80000"]
    r = subprocess.run(base + ["--no-legs", "--no-text"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-3000:]
    one = json.loads(r.stdout.strip().splitlines()[-1])
    assert one["gfa_identical"] is True
    assert (one["tie_groups"] > 0) == bool(grid)
    procs = []
    for rank in range(2):
        e = dict(env, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(20000 + os.getpid() % 20000),
                 MA_FAKE_DIST_DIR=str(tmp_path), MA_BENCH_ONE_GPU_DEBUG="1")
        procs.append(subprocess.Popen(base + ["--gpus", "2"], cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        try:
            o, err = p.communicate(timeout=1800)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, err[-3000:]
        outs.append(o)
    assert outs[1].strip() == "", "only rank 0 prints"
    d = json.loads(outs[0].strip().splitlines()[-1])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert d["gfa_identical"] is True and d["parity"]["gfa_md5"] == one["parity"]["ref_md5"]
    assert d["tie_groups"] == one["tie_groups"] and (not grid or "hit walk" in d["tie_path"])  # tie-rich: both walks ran on the shards too
    assert d["config"]["global_overlaps"] == one["config"]["global_overlaps"] and d["config"]["per_gpu_hits"] < one["config"]["per_gpu_hits"]
    ph = d["phases"]  # where a sharded step spends its time: one entry per phase of host/sharded.c, [max, min] over the ranks
    assert set(ph["phase_ms"]) >= {"sort", "sub#1", "x:sub0", "x:arc blocks", "rank 0: cleanup+symm"} and all(len(v) == 2 and v[0] >= v[1] >= 0 for v in ph["phase_ms"].values())
    assert ph["exchange_bytes_per_rank"]["x:sub0"] > 0 and ph["head_wall_ms_max"] >= ph["head_wall_ms_min"] > 0 and ph["rank0_tail_wall_ms"] > 0
