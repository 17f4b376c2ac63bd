"""pomgpu_ztosig on an MI355X: the checks of tests/ztosig_checks.py with the product library against tests/ztosig_expect.py's restatement
and the reference's recorded digests (tests/golden/ztosig.json), bit for bit; the fp32 study builds against the fp64 result rounded
once."""
import pytest

import ztosig_checks as C
from extpom_amd import lib
from ztosig_expect import SHAPES

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("salt", [False, True], ids=["T", "S"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_ztosig_equals_the_expectation_and_the_references_digest(shape, salt):
    C.standalone_equals_the_expectation(LIB, shape, salt)


def test_trimmed_tile_keeps_its_padding():
    C.trimmed_tile_keeps_its_padding(LIB)


def test_refusals_and_a_context_that_has_stepped():
    C.refusals_and_a_stepped_context(LIB)


@pytest.mark.parametrize("path", [lib.LIBPATH_F32, lib.LIBPATH_F32A], ids=["f32", "f32a"])
def test_fp32_builds_round_once_at_the_store(path):
    C.standalone_equals_the_expectation(path, (20, 17, 5, 6), f32=True)
    C.standalone_equals_the_expectation(path, (65, 49, 33, 21), salt=True, f32=True)


def test_tiles_equal_the_single_tile_on_their_window():
    """four contexts on GPU 0 with the event-ordered mover of tests/forcing_files_checks.py: a process of its own, as that harness is (torch
    and the library must share one HIP runtime, so torch is imported first there)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_ztosig_tiles.py")], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "ZTOSIG-TILES-OK" in r.stdout and "ZTOSIG-FILE-TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- the cold start from z-level files (pomgpu_set_z_inputs) -------------------------------------------------------------------------------
import ztosig_files_checks as F                                # noqa: E402


@pytest.mark.parametrize("init_z,clim_z", [(True, False), (False, True), (True, True), (False, False)])
def test_state_after_a_z_level_cold_start_equals_the_expectation(tmp_path, init_z, clim_z):
    F.state_equals_the_expectation(LIB, tmp_path, (20, 17, 6), init_z, clim_z)


@pytest.mark.parametrize("size,kind,chunk_kb,nml", [((65, 49, 21), "f", None, {}), ((66, 50, 21), "d", 1, {}), ((8, 8, 6), "d", None, {}), ((64, 48, 50), "f", 1, dict(npg=2))], ids=str)
def test_z_level_cold_start_float_files_and_small_runs(tmp_path, size, kind, chunk_kb, nml):
    F.state_equals_the_expectation(LIB, tmp_path, size, True, True, kind=kind, chunk_kb=chunk_kb, nml=nml)


@pytest.mark.parametrize("case", ["archipelago", "seamount"])
def test_four_steps_after_a_z_level_cold_start_equal_the_oracle(tmp_path, case):
    F.steps_after_it(LIB, tmp_path, case)


def test_every_new_refusal_leaves_the_state_as_it_was(tmp_path):
    F.refusals(LIB, tmp_path)
    F.tile_window_must_fit(LIB, tmp_path)


def test_restore_interior_from_a_z_level_clim_file_across_the_month_wrap(tmp_path):
    F.restore_across_the_month_wrap(LIB, tmp_path)


def test_restore_interior_from_a_z_level_clim_file_on_tiles_with_neighbours(tmp_path):
    F.restore_on_tiles(LIB, tmp_path)


@pytest.mark.parametrize("path", [lib.LIBPATH_F32, lib.LIBPATH_F32A], ids=["f32", "f32a"])
def test_fp32_builds_of_the_z_level_cold_start_round_once(tmp_path, path):
    F.f32_rounds_once(path, tmp_path)
