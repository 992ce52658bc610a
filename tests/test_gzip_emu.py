"""tests/test_gpu_gzip.py run WITHOUT a GPU, on the CPU build of the kernel sources (tests/emu, see tests/test_emu_suite.py): the chunked device inflater of
plain gzip input -- header and trailer, the per-chunk search and count, the chain, the symbol decode, the window chain, resolve and CRC, the wiring into the PAF
reader -- against tests/gzipmodel.py, zlib, the plain files and the reference binary, once in normal order and once with lanes, waves and blocks in DESCENDING
order and every device allocation ending at a faulting page (the pool off: it would hide the page), so that a read or a write one byte outside the compressed
bytes, the symbol scratch, the windows or the text faults here and not on a GPU.  The kernels' lanes share LDS between barriers only; the reversed order runs
lane 63 first and breaks code that leans on lock step."""
import pytest

from test_emu_suite import emu_built, run_gpu_tests  # noqa: F401  (emu_built: the fixture that builds tests/emu)


def test_gzip_inflater_on_cpu(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_gzip.py"], 1800)


def test_gzip_inflater_with_reversed_schedule_and_guard_pages(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_gzip.py"], 1800, {"EMU_ORDER": "reverse", "EMU_GUARD": "1", "MA_DEV_POOL": "0"})
