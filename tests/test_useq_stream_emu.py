"""tests/test_gpu_useq_stream.py run WITHOUT a GPU, on the CPU build of the kernel sources (tests/emu, see tests/test_emu_suite.py): the streamed device reader of
the reads file -- window, consumed prefix, verdict, probe with its match list, placement by match, handover -- against the whole-file reader, the Python model and
the reference binary, once in normal order and once with lanes, waves and blocks in DESCENDING order and every device allocation ending at a faulting page (the
pool off: it would hide the page)."""
import pytest

from test_emu_suite import emu_built, run_gpu_tests  # noqa: F401  (emu_built: the fixture that builds tests/emu)


def test_useq_stream_on_cpu(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_useq_stream.py"], 1800)


def test_useq_stream_with_reversed_schedule_and_guard_pages(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_useq_stream.py"], 1800, {"EMU_ORDER": "reverse", "EMU_GUARD": "1", "MA_DEV_POOL": "0"})
