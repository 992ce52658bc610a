"""tests/test_gpu_bgzf_range.py run WITHOUT a GPU, on the CPU build of the kernel sources (tests/emu, see tests/test_emu_suite.py): a rank's own range of a
bgzip-compressed overlap file -- the member sub-range, the rebased table, the batches of the extension rounds, k_text_first_nl and the placement of the text --
against tests/bgzfmodel.py, the plain bytes and the stated range rule, once in normal order and once with lanes, waves and blocks in DESCENDING order and every
device allocation ending at a faulting page (the pool off: it would hide the page), so that a read or a write one byte outside a sub-range's compressed bytes,
its table, a batch's text or the rank's text faults here and not on a GPU.  The unaligned head and tail of k_text_first_nl are the likely place: the stage
cases search texts that end at the last byte of their allocation.

Measured: 3 s in normal order and 4 s reversed with guard pages (38 tests each)."""
from test_emu_suite import emu_built, run_gpu_tests  # noqa: F401  (emu_built: the fixture that builds tests/emu)


def test_bgzf_ranges_on_cpu(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_bgzf_range.py"], 1800)


def test_bgzf_ranges_with_reversed_schedule_and_guard_pages(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_bgzf_range.py"], 1800, {"EMU_ORDER": "reverse", "EMU_GUARD": "1", "MA_DEV_POOL": "0"})
