"""tests/test_gpu_ingest_stream_excl.py runs WITHOUT a GPU, on the CPU build of the kernel sources (tests/emu, see tests/test_emu_suite.py): -R in the streamed PAF
ingest -- the verdicts against provisional ids, the early drop, the flags and the lengths column across every growth, the retirement and renumbering at the end
of the stream, and the host layer under MA_STREAM_NOCONT=1 -- against the whole parse, the model, the host reader and the reference, once in normal order and
once with lanes, waves and blocks in DESCENDING order and every device allocation ending at a faulting page (the pool off: it would hide the page), so that a
flag, a length or a record written one element outside its buffer faults here and not on a GPU."""
import pytest

from test_emu_suite import emu_built, run_gpu_tests  # noqa: F401  (emu_built: the fixture that builds tests/emu)


def test_streamed_exclusion_on_cpu(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_ingest_stream_excl.py"], 1800)


def test_streamed_exclusion_with_reversed_schedule_and_guard_pages(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_ingest_stream_excl.py"], 1800, {"EMU_ORDER": "reverse", "EMU_GUARD": "1", "MA_DEV_POOL": "0"})  # (without the pool its growth counts are asserted)
