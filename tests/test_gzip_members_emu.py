"""tests/test_gpu_gzip_members.py run WITHOUT a GPU, on the CPU build of the kernel sources (tests/emu, see tests/test_emu_suite.py): the member scan, the head
items, the chain over concatenated members, per-member history, windows and CRC pieces, the wiring into the PAF reader and the -f reads file -- against
tests/gzipmembersmodel.py, zlib, the plain files and the reference binary, once in normal order and once with lanes, waves and blocks in DESCENDING order and
every device allocation ending at a faulting page (the pool off: it would hide the page), so that a read or a write one byte outside the compressed bytes, the
candidate list, the head rows, the windows, the piece table or the text faults here and not on a GPU."""
import pytest

from test_emu_suite import emu_built, run_gpu_tests  # noqa: F401  (emu_built: the fixture that builds tests/emu)


def test_gzip_members_on_cpu(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_gzip_members.py"], 1800)


def test_gzip_members_with_reversed_schedule_and_guard_pages(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_gzip_members.py"], 1800, {"EMU_ORDER": "reverse", "EMU_GUARD": "1", "MA_DEV_POOL": "0"})
