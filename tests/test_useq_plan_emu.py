"""tests/test_gpu_useq_plan.py run WITHOUT a GPU, on the CPU build of the kernel sources (tests/emu, see tests/test_emu_suite.py): the placement plan made on the
device -- stage cases against the Python model, the placement through the plan whole and streamed, the refusals -- once in normal order and once with lanes, waves
and blocks in DESCENDING order and every device allocation ending at a faulting page (the pool off: it would hide the page); then the command line on every road,
which also takes the host code of the planned placement and of the late ma_ug_t fetch through the CPU build."""
import pytest

from test_emu_suite import emu_built, run_gpu_tests  # noqa: F401  (emu_built: the fixture that builds tests/emu)


def test_placement_plan_on_cpu(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_useq_plan.py", "-k", "not cli"], 1500)


def test_placement_plan_with_reversed_schedule_and_guard_pages(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_useq_plan.py", "-k", "not cli"], 1500, {"EMU_ORDER": "reverse", "EMU_GUARD": "1", "MA_DEV_POOL": "0"})


def test_placement_plan_command_line_on_cpu(emu_built):  # noqa: F811
    run_gpu_tests(["tests/test_gpu_useq_plan.py", "-k", "cli"], 3000)
