"""tests/test_gpu_xfer_edges.py and tests/test_gpu_scan_edges.py run WITHOUT a GPU, on the CPU build of the kernel sources (tests/emu, see
tests/test_emu_suite.py): the staged copy at every worker / slice / slot edge and the device-wide scan at every size edge of its three forms, once in normal
order and once with lanes, waves and blocks in DESCENDING order and every device allocation -- the copy workers' pinned slots included -- ending at a faulting
page (the pool off: it would hide the page), so that a slice one byte too long, a read behind the scan's input or a published word behind the chain's state
array faults here and not on a GPU.  Nothing is held back for MA_EMU_FULL: the 2048 x 2048-element scans take 5 to 6 s each here and the 132 MiB copies about
a second.

The copy workers are also run under the thread sanitizer, by a stand-alone program (tests/emu/xfer_drive.cpp, `make -C tests/emu tsan`): the stand-in
runtime's copies are memmoves on the calling thread, so two workers whose slices overlap by a byte are a reported race even where the bytes agree.  The
program is a child process; nothing is preloaded anywhere.  A second stand-alone program (tests/emu/lookback_selftest.cpp) walks sc_look_back over published
words written by hand."""
import os
import subprocess

import pytest

from test_emu_suite import EMU, emu_built, run_gpu_tests  # noqa: F401  (emu_built: the fixture that builds tests/emu)

MODULES = ["tests/test_gpu_xfer_edges.py", "tests/test_gpu_scan_edges.py"]


def test_staged_copy_and_scan_on_cpu(emu_built):  # noqa: F811
    run_gpu_tests(MODULES, 1800)


def test_staged_copy_and_scan_with_reversed_schedule_and_guard_pages(emu_built):  # noqa: F811
    run_gpu_tests(MODULES, 1800, {"EMU_ORDER": "reverse", "EMU_GUARD": "1", "MA_DEV_POOL": "0"})


def test_look_back_over_hand_made_words(built):
    """tests/emu/lookback_selftest.cpp: sc_look_back over 1, 2, 3 and 64 steps of 64 predecessors.  A launch of the CPU build has at most 8 blocks in flight, so
    the scan cases above never take a second step; on the device they do when the timing has it so"""
    r = subprocess.run(["make", "-C", EMU, "_build/lookback_selftest"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    for order in ("", "reverse"):
        r = subprocess.run([os.path.join(EMU, "_build", "lookback_selftest")], env=dict(os.environ, EMU_ORDER=order, EMU_GUARD="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:]


def test_copy_workers_under_the_thread_sanitizer(built):
    r = subprocess.run(["make", "-C", EMU, "-j8", "tsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    env.pop("MA_XFER_THREADS", None)
    r = subprocess.run([os.path.join(EMU, "_build_tsan", "xfer_drive")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "ThreadSanitizer" not in r.stdout, r.stdout[-4000:]
