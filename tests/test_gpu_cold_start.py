"""pomgpu_cold_start on an MI355X: the checks of tests/cold_start_checks.py with the product library against tests/cold_start_expect.py's
restatement and the CPU oracle, bit for bit; the fp32 study builds against model.gpu_finish_initial on the same library."""
import pytest

import cold_start_checks as C
from extpom_amd import lib

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("size,nml", [((8, 8, 6), {}), ((20, 17, 6), {}), ((65, 49, 21), {}), ((66, 50, 21), {}), ((65, 49, 21), dict(npg=2)), ((64, 48, 50), {}), ((65, 49, 21), dict(ramp=0.0))],
                         ids=str)
def test_state_after_cold_start_equals_the_expectation(tmp_path, size, nml):
    C.state_equals_the_expectation(LIB, tmp_path, size, nml)


@pytest.mark.parametrize("case", ["archipelago", "seamount"])
def test_four_steps_after_it_equal_the_oracle_and_an_uploaded_state(tmp_path, case):
    C.steps_after_it(LIB, tmp_path, case)


def test_many_runs_per_variable(tmp_path):
    C.many_runs_per_variable(LIB, tmp_path)


def test_float_files_and_files_of_another_writer(tmp_path):
    C.other_writers_files(LIB, tmp_path)


def test_every_refusal_leaves_the_state_as_it_was(tmp_path):
    C.refusals(LIB, tmp_path)


def test_cold_start_forcing_files_run_restart_and_on(tmp_path):
    C.cold_start_to_restart_and_on(LIB, tmp_path)


def test_cold_start_on_a_context_that_has_stepped(tmp_path):
    C.on_a_context_that_has_stepped(LIB, tmp_path)


@pytest.mark.parametrize("path", [lib.LIBPATH_F32, lib.LIBPATH_F32A], ids=["f32", "f32a"])
def test_fp32_builds_equal_gpu_finish_initial_on_the_same_library(tmp_path, path):
    C.f32_equals_gpu_finish_initial(path, tmp_path)


def test_tiles_read_their_window_and_step_like_the_single_tile():
    """four contexts on GPU 0 with the event-ordered mover of tests/forcing_files_checks.py: a process of its own, as that harness is (torch
    and the library must share one HIP runtime, so torch is imported first there)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_cold_start_tiles.py")], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "COLD-START-TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
