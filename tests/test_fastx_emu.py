"""tests/test_gpu_fastx.py run WITHOUT a GPU, on the CPU build of the kernel sources (tests/emu, see tests/test_emu_suite.py): the device reader of the
reads file -- line index, form check, name lookup, placement -- against the reference binary and the Python model, once in normal order and once with
lanes, waves and blocks in DESCENDING order and every device allocation ending at a faulting page (the pool off: it would hide the page).

Measured: 3 min 10 s to 4 min 40 s of wall time for both runs together, by the load of the box (half of it each).  The end-to-end matrix is what costs: about 45 inputs, each run five times (reference, CLI
and drop-in, with and without MA_FASTX_HOST=1) at about 0.6 s a process; the stage tests, the 524 400-line scan case among them, take 20 s.  A smaller PAF does not
help: the inputs tried at half the size leave one unitig, or none that the reference answers under -b."""
import pytest

from test_emu_suite import emu_built, run_gpu_tests  # noqa: F401  (emu_built: the fixture that builds tests/emu)


def test_fastx_reader_on_cpu(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_fastx.py"], 1800)


def test_fastx_reader_with_reversed_schedule_and_guard_pages(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_fastx.py"], 1800, {"EMU_ORDER": "reverse", "EMU_GUARD": "1", "MA_DEV_POOL": "0"})
