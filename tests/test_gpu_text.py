"""The device text writer of the record dumps (csrc/text_dev.hpp over csrc/text_core.h): -p paf, -p sg and -p bed formatted on the GPU.
Stage cases through Ctx.text_format (hand-made records, names and kept intervals; the yardstick is the Python model of tests/textmodel.py, byte for byte, and
the report: lines, bytes, slabs, lines that took the slow path) at every record count, slab size, name length and tile alignment the kernels branch on;
then the command line with MA_TEXT_DEVICE=1 against the reference binary (against MA_TEXT_DEVICE=0 where oracle/_ref is not built), and the memory sink."""
import os
import re

import numpy as np
import pytest

import miniasm_amd as ma
import refapi as R
import textmodel as TM

pytestmark = pytest.mark.gpu

KINDS = ("paf", "sg", "bed")


def make_case(kind, n, names, seed=1):
    """n records (bed: one per read) with moderate random values over the given names"""
    rnd = np.random.RandomState(seed * 1000 + n)
    R_ = len(names)
    sub = np.zeros(R_, dtype=ma.SUB_DT)
    sub["sdel"] = rnd.randint(0, 3000, R_)
    sub["e"] = sub["sdel"] + rnd.randint(0, 40000, R_)
    if kind == "bed":
        dele = (rnd.randint(0, 5, R_) == 0).astype(np.uint8)
        sub["e"][rnd.randint(0, 7, R_) == 0] = 0
        sub["sdel"][sub["e"] == 0] = 0
        return None, sub, dele
    if kind == "paf":
        rec = np.zeros(n, dtype=ma.HIT_DT)
        rec["qns"] = rnd.randint(0, R_, n).astype(np.uint64) << np.uint64(32) | rnd.randint(0, 10 ** rnd.randint(1, 6), n).astype(np.uint64)
        for f in ("qe", "ts", "te", "bldel"):
            rec[f] = rnd.randint(0, 10 ** rnd.randint(1, 7), n)
        rec["tn"] = rnd.randint(0, R_, n)
        rec["mlrev"] = rnd.randint(0, 100000, n).astype(np.uint32) | (rnd.randint(0, 2, n).astype(np.uint32) << np.uint32(31))
        return rec, sub, None
    rec = np.zeros(n, dtype=ma.ARC_DT)
    rec["ul"] = rnd.randint(0, 2 * R_, n).astype(np.uint64) << np.uint64(32) | rnd.randint(0, 10 ** rnd.randint(1, 6), n).astype(np.uint64)
    rec["v"] = rnd.randint(0, 2 * R_, n)
    rec["oldel"] = rnd.randint(0, 30000, n)
    return rec, sub, None


def check(ctx, kind, rec, names, sub, dele, slab, want_slow=None):
    want = TM.lines(kind, rec, names, sub, dele)
    text, info = ctx.text_format(kind, rec, names, sub=sub, dele=dele, slab=slab)
    assert text == b"".join(want), "%s, %d records, slab %r: the text differs from the model" % (kind, len(want), slab)
    n = len(want)
    assert info["road"] == "device" and info["reason"] == "OK" and info["kind"] == kind
    assert info["n_records"] == n and info["n_lines"] == sum(1 for x in want if x) and info["text_bytes"] == len(text)
    eff = info["slab_records"]
    assert eff == TM.slab_records(kind, slab, max([len(x) for x in names] + [0]))
    assert info["n_slabs"] == (n + eff - 1) // eff
    assert info["max_name"] == max([len(x) for x in names] + [0])
    if want_slow is None:  # what the model says about the waves that outgrow the tile (None: one is too close to call)
        want_slow = TM.slow_lines([len(x) for x in want], eff)
    if want_slow is not None:
        assert info["n_slow_lines"] == want_slow
    return text, info


def short_names(n, seed=3):
    rnd = np.random.RandomState(seed)
    return [b"n%d_" % i + b"x" * rnd.randint(0, 12) for i in range(n)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_record_counts_and_slab_sizes(gpu_ctx, n):
    """every record count around the wave (64) and the length kernel's block (256), under slabs of 1, 64, n - 1, n and n + 1 records"""
    for kind in KINDS:
        names = short_names(n if kind == "bed" else 37)
        rec, sub, dele = make_case(kind, n, names)
        for slab in sorted({s for s in (1, 64, n - 1, n, n + 1) if s > 0}) + [None]:
            if slab == 1 and n == 1000 and kind != "paf":
                continue  # (a thousand one-record slabs once are enough)
            check(gpu_ctx, kind, rec, names, sub, dele, slab)


def test_name_lengths(gpu_ctx):
    """names of 1, 7, 8, 9, 15, 16, 17, 255 and 256 bytes in every position of a line"""
    names = [bytes([97 + k % 26]) * ln for k, ln in enumerate((1, 7, 8, 9, 15, 16, 17, 255, 256))]
    for kind in KINDS:
        rec, sub, dele = make_case(kind, 400, names, seed=2)
        if kind == "bed":
            dele[:] = 0
        check(gpu_ctx, kind, rec, names, sub, dele, None)
        check(gpu_ctx, kind, rec, names, sub, dele, 100)


def test_a_name_longer_than_the_tile_takes_the_slow_path(gpu_ctx):
    """one name of 70 000 bytes among short ones: the waves that hold one of its lines do not fit the LDS tile and write straight to device memory; the report says so"""
    names = short_names(50)
    names[17] = b"L" * 70000
    for kind in KINDS:
        n = 50 if kind == "bed" else 300
        rec, sub, dele = make_case(kind, n, names, seed=4)
        if kind == "bed":
            dele[:] = 0
            sub["sdel"][17], sub["e"][17] = 1, 9
        elif kind == "paf":
            rec["tn"][5], rec["qns"][200] = 17, (17 << 32) | 12
        else:
            rec["v"][5], rec["ul"][200] = 17 << 1, (17 << 1 | 1) << 32 | 77
        for slab in (None, 64, 100):
            lens = [len(x) for x in TM.lines(kind, rec, names, sub, dele)]
            slow = TM.slow_lines(lens, TM.slab_records(kind, slab, 70000))
            assert slow is not None and slow >= 1
            check(gpu_ctx, kind, rec, names, sub, dele, slab, want_slow=slow)


def test_tile_starts_on_every_residue_mod_16(gpu_ctx):
    """bed lines sized so that the text of every wave is 385 bytes: the waves' stretches start at 0, 1, 2, ... mod 16, each with its own head, body of 16-byte
    stores and tail; and waves of 1 to 40 bytes, shorter than one aligned store"""
    names = ([b"a"] * 63 + [b"bb"]) * 17
    sub = np.zeros(len(names), dtype=ma.SUB_DT)
    sub["sdel"], sub["e"] = 1, 2
    lens = [len(x) for x in TM.lines("bed", None, names, sub, None)]
    assert {sum(lens[:w * 64]) % 16 for w in range(17)} == set(range(16))
    check(gpu_ctx, "bed", None, names, sub, None, None)
    for keep in range(1, 8):  # a wave with `keep` lines of 6 bytes, then 64 - keep skipped reads
        dele = np.ones(len(names), dtype=np.uint8)
        for w in range(17):
            dele[w * 64:w * 64 + keep] = 0
        check(gpu_ctx, "bed", None, names, sub, dele, None)
    # paf and sg: the same idea with random line lengths; the model says which residues the wave starts reach
    for kind in ("paf", "sg"):
        nm = short_names(37)
        rec, sub2, _ = make_case(kind, 64 * 60, nm, seed=6)
        lens = np.cumsum([0] + [len(x) for x in TM.lines(kind, rec, nm, sub2, None)])
        assert {int(lens[w * 64]) % 16 for w in range(60)} == set(range(16))
        check(gpu_ctx, kind, rec, nm, sub2, None, None)


@pytest.mark.parametrize("kind,with_sub", [("paf", True), ("sg", True), ("sg", False), ("bed", True)])
def test_value_edges_in_every_field(gpu_ctx, kind, with_sub):
    """0, 9, 10, ..., 10^9, 2^31 - 1 in every integer field, 2^31 and 2^32 - 1 (negative text) in those printed from a uint32_t, both strands"""
    rec, names, sub, dele = TM.edge_case(kind, with_sub)
    text, _ = check(gpu_ctx, kind, rec, names, sub, dele, None)
    check(gpu_ctx, kind, rec, names, sub, dele, 7)
    if kind != "bed":
        assert b"-2147483648" in text and b"2147483647" in text


def test_bed_rows_skipped(gpu_ctx):
    """all rows skipped, none, every other one, only the last one kept; skipped by del and by s == e"""
    n = 300
    names = short_names(n)
    sub = np.zeros(n, dtype=ma.SUB_DT)
    sub["sdel"], sub["e"] = np.arange(n), np.arange(n) + 500
    pats = {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "alternating": (np.arange(n) & 1).astype(np.uint8), "last_kept": (np.arange(n) != n - 1).astype(np.uint8)}
    for name, dele in pats.items():
        for slab in (None, 64, 7):
            text, info = check(gpu_ctx, "bed", None, names, sub, dele, slab)
            assert info["n_lines"] == int((dele == 0).sum()), name
        sub2 = sub.copy()
        sub2["e"][dele != 0] = sub2["sdel"][dele != 0]  # the same rows, skipped because their interval is empty
        check(gpu_ctx, "bed", None, names, sub2, None, None)
    assert check(gpu_ctx, "bed", None, names, sub, pats["all"], None)[0] == b""


# ---- end to end: the command line (FILE sink) and ma_pipeline_device_mem (memory sink)

INPUTS = {  # tests/test_gpu_cli.py: INPUTS (the generation arguments are copied)
    "noisy": dict(reads=4000, lines=90000, seed=63, extra=["-L", "uniform", "-d", "0.35", "-x", "0.03"]),
    "longnames": dict(reads=3000, lines=80000, seed=41, extra=["-N", "m64011_190830_220126/"]),
}
DUMPS = [["-p", "bed"], ["-p", "paf", "-S2"], ["-p", "paf", "-S3"], ["-p", "paf", "-S4"], ["-p", "paf"],
         ["-p", "sg", "-S5"], ["-p", "sg", "-S6"], ["-p", "sg", "-S7"], ["-p", "sg", "-S9"], ["-p", "sg", "-S10"], ["-p", "sg"],
         ["-R", "-p", "paf"], ["-1", "-2", "-p", "sg"], ["-b", "-p", "sg", "-S5"]]
_paf = {}


def _input(tmpdir_s, name):
    if name not in _paf:
        cfg = INPUTS[name]
        _paf[name] = R.pafgen(os.path.join(tmpdir_s, "text_%s.paf" % name), cfg["reads"], cfg["lines"], cfg["seed"], cfg["extra"])
    return _paf[name]


def _text_line(log):
    m = re.search(r"^\[T::text\] (\S+) (device|host)\b(.*)$", log, flags=re.M)
    assert m, "no [T::text] line:\n" + log[-800:]
    return m


@pytest.mark.parametrize("args", DUMPS, ids=lambda a: " ".join(a))
@pytest.mark.parametrize("name", list(INPUTS))
def test_cli_dumps_written_on_the_device(name, args, tmpdir_s, monkeypatch):
    """MA_TEXT_DEVICE=1, default slab and slabs of 1000 records: the reference binary's bytes (without oracle/_ref: the host formatter's), and the log says `device`"""
    paf = _input(tmpdir_s, name)
    monkeypatch.setenv("MA_PIPE_TIMING", "1")
    monkeypatch.setenv("MA_TEXT_DEVICE", "0")
    monkeypatch.delenv("MA_TEXT_SLAB", raising=False)
    host_out, host_log = R.run_cli(ma.CLI_PATH, args, paf)
    assert _text_line(host_log).group(2) == "host"
    if R.have_ref():
        want, _ = R.run_cli(R.REF_BIN, args, paf)
        assert host_out == want
    else:
        want = host_out
    assert len(want) > 1000
    monkeypatch.setenv("MA_TEXT_DEVICE", "1")
    for slab in (None, "1000"):
        if slab:
            monkeypatch.setenv("MA_TEXT_SLAB", slab)
        out, log = R.run_cli(ma.CLI_PATH, args, paf)
        assert out == want, "%s %s, MA_TEXT_SLAB=%s: bytes differ" % (name, " ".join(args), slab)
        m = _text_line(log)
        assert m.group(1) == args[args.index("-p") + 1] and m.group(2) == "device", m.group(0)
        lines, nbytes = (int(x) for x in re.search(r"(\d+) lines, (\d+) bytes", m.group(3)).groups())
        assert lines == out.count(b"\n") and nbytes == len(out)
        if slab:
            assert int(re.search(r"(\d+) slabs of 1000 records", m.group(3)).group(1)) >= lines // 1000


@pytest.mark.parametrize("fmt,stage", [("paf", 2), ("paf", 100), ("sg", 5), ("sg", 100), ("bed", 100)])
def test_memory_sink_gives_the_file_sinks_bytes(fmt, stage, tmpdir_s, monkeypatch):
    """ma_pipeline_device_mem with the device road: the block it returns holds what the command line writes to its stream; the context reports the road it took"""
    paf = _input(tmpdir_s, "noisy")
    opt = ma.default_opt()
    outs = {}
    for dev in ("0", "1"):
        monkeypatch.setenv("MA_TEXT_DEVICE", dev)
        monkeypatch.setenv("MA_TEXT_SLAB", "500")
        ing = ma.Ingest(paf, opt)
        ctx = ma.Ctx(0)
        ctx.hits_upload(ing.hits, ing.n_seq)
        outs[dev] = ma.run_resident(ctx, opt, ing, fmt, stage)
        last = ctx.text_last()
        if dev == "1":
            assert last["road"] == "device" and last["kind"] == fmt and last["text_bytes"] == len(outs[dev]) and last["n_slabs"] >= 2 and last["n_slow_lines"] == 0
        else:
            assert last["road"] in (None, "host")
        ing.close()
        ctx.close()
    assert len(outs["1"]) > 1000 and outs["1"] == outs["0"]
    cli, _ = R.run_cli(ma.CLI_PATH, ["-p", fmt, "-S%d" % stage], paf)
    assert cli == outs["1"]
