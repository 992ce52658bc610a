"""tests/test_gpu_text_ug.py run WITHOUT a GPU, on the CPU build of the kernel sources (tests/emu, see tests/test_emu_suite.py): the device writer of the unitig GFA
-- stage cases against the Python model, the command line against the reference binary with and without a reads file, the memory sink -- once in normal order and
once with lanes, waves and blocks in DESCENDING order and every device allocation ending at a faulting page (the pool off: it would hide the page; an arena or a
text buffer that ends at a page is also one that does not start at a multiple of 16: the chunk copies' source and the tile's head and tail bytes move).
About two minutes each on 16 cores, most of it the runs of the command line."""
import pytest

from test_emu_suite import emu_built, run_gpu_tests  # noqa: F401  (emu_built: the fixture that builds tests/emu)


def test_ug_text_writer_on_cpu(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_text_ug.py"], 3000)


def test_ug_text_writer_with_reversed_schedule_and_guard_pages(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_text_ug.py"], 3000, {"EMU_ORDER": "reverse", "EMU_GUARD": "1", "MA_DEV_POOL": "0"})
