"""tests/test_gpu_ingest_stream.py and tests/test_gpu_ingest_stream_edges.py run WITHOUT a GPU, on the CPU build of the kernel sources (tests/emu, see tests/test_emu_suite.py): the streamed PAF ingest --
the fold of a piece's names into the persistent table, its rebuild, the appended arena, the grown record buffer, the stale bl across pieces, and the host layer's
producer thread with its cut and carry -- against the whole parse, the host reader and the reference, once in normal order and once with lanes, waves and blocks
in DESCENDING order and every device allocation ending at a faulting page (the pool off: it would hide the page), so that a probe, an arena write or a record
one element outside its buffer faults here and not on a GPU."""
import pytest

from test_emu_suite import emu_built, run_gpu_tests  # noqa: F401  (emu_built: the fixture that builds tests/emu)


def test_streamed_ingest_on_cpu(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_ingest_stream.py"], 1800)
    run_gpu_tests(["tests/test_gpu_ingest_stream_edges.py"], 1800)  # the overflow road of the fold, equal tags, the wrap, every growth at its edge, the bl walk, the host layer's ends


def test_streamed_ingest_with_reversed_schedule_and_guard_pages(emu_built):  # noqa: F811
    env = {"EMU_ORDER": "reverse", "EMU_GUARD": "1", "MA_DEV_POOL": "0"}
    run_gpu_tests(["tests/test_gpu_ingest_stream.py"], 1800, env)
    run_gpu_tests(["tests/test_gpu_ingest_stream_edges.py"], 1800, env)  # (without the pool its growth counts of the arena and the per-id arrays are equalities)
