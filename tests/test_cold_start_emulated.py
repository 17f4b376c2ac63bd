"""pomgpu_cold_start -- initialize.f:24-36 after read_input, from the reference's grid, init and clim files without PnetCDF -- through the
host builds of the unmodified sources (tests/emu): the header checks, the refusals, the window of a tile, the life cycle and every
kernel's index arithmetic, bit for bit against tests/cold_start_expect.py.  The device runs the same checks (test_gpu_cold_start.py)."""
import os
import subprocess

import pytest

import cold_start_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("size,nml", [((8, 8, 6), {}), ((20, 17, 6), {}), ((65, 49, 21), {}), ((66, 50, 21), {}), ((65, 49, 21), dict(npg=2)), ((64, 48, 50), {}), ((65, 49, 21), dict(ramp=0.0))],
                         ids=str)
def test_state_after_cold_start_equals_the_expectation(tmp_path, size, nml):
    C.state_equals_the_expectation(EMU, tmp_path, size, nml)


@pytest.mark.parametrize("case", ["archipelago", "seamount"])
def test_four_steps_after_it_equal_the_oracle_and_an_uploaded_state(tmp_path, case):
    C.steps_after_it(EMU, tmp_path, case)


def test_tiles_read_their_window_and_step_like_the_single_tile(tmp_path):
    C.tiles(EMU, tmp_path)


def test_many_runs_per_variable(tmp_path):
    C.many_runs_per_variable(EMU, tmp_path)


def test_float_files_and_files_of_another_writer(tmp_path):
    C.other_writers_files(EMU, tmp_path)


def test_every_refusal_leaves_the_state_as_it_was(tmp_path):
    C.refusals(EMU, tmp_path)


def test_cold_start_forcing_files_run_restart_and_on(tmp_path):
    C.cold_start_to_restart_and_on(EMU, tmp_path)


def test_cold_start_on_a_context_that_has_stepped(tmp_path):
    C.on_a_context_that_has_stepped(EMU, tmp_path)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_equal_gpu_finish_initial_on_the_same_library(tmp_path, variant):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    C.f32_equals_gpu_finish_initial(VARIANTS[variant], tmp_path)
