"""pomgpu_ztosig -- initialize.f:547-667, z-level T and S onto the sigma levels -- through the host builds of the unmodified sources
(tests/emu): every index and every operation of the kernels, the refusals and the exchange on tiles, bit for bit against
tests/ztosig_expect.py and the reference's recorded output.  The device runs the same checks (test_gpu_ztosig.py)."""
import os
import subprocess

import pytest

import ztosig_checks as C
from ztosig_expect import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("salt", [False, True], ids=["T", "S"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_ztosig_equals_the_expectation_and_the_references_digest(shape, salt):
    C.standalone_equals_the_expectation(EMU, shape, salt)


def test_trimmed_tile_keeps_its_padding():
    C.trimmed_tile_keeps_its_padding(EMU)


def test_tiles_equal_the_single_tile_on_their_window():
    C.tiles(EMU)


def test_refusals_and_a_context_that_has_stepped():
    C.refusals_and_a_stepped_context(EMU)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_round_once_at_the_store(variant):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    C.standalone_equals_the_expectation(VARIANTS[variant], (20, 17, 5, 6), f32=True)
    C.standalone_equals_the_expectation(VARIANTS[variant], (65, 49, 33, 21), salt=True, f32=True)


# ---- the cold start from z-level files (pomgpu_set_z_inputs) -------------------------------------------------------------------------------
import ztosig_files_checks as F                                # noqa: E402


@pytest.mark.parametrize("init_z,clim_z", [(True, False), (False, True), (True, True), (False, False)])
def test_state_after_a_z_level_cold_start_equals_the_expectation(tmp_path, init_z, clim_z):
    F.state_equals_the_expectation(EMU, tmp_path, (20, 17, 6), init_z, clim_z)


@pytest.mark.parametrize("size,kind,chunk_kb,nml", [((65, 49, 21), "f", None, {}), ((66, 50, 21), "d", 1, {}), ((8, 8, 6), "d", None, {}), ((64, 48, 50), "f", 1, dict(npg=2))], ids=str)
def test_z_level_cold_start_float_files_and_small_runs(tmp_path, size, kind, chunk_kb, nml):
    F.state_equals_the_expectation(EMU, tmp_path, size, True, True, kind=kind, chunk_kb=chunk_kb, nml=nml)


@pytest.mark.parametrize("case", ["archipelago", "seamount"])
def test_four_steps_after_a_z_level_cold_start_equal_the_oracle(tmp_path, case):
    F.steps_after_it(EMU, tmp_path, case)


def test_tiles_read_their_window_on_every_side_and_step_like_the_single_tile(tmp_path):
    F.tiles(EMU, tmp_path)


def test_every_new_refusal_leaves_the_state_as_it_was(tmp_path):
    F.refusals(EMU, tmp_path)
    F.tile_window_must_fit(EMU, tmp_path)


def test_restore_interior_from_a_z_level_clim_file_across_the_month_wrap(tmp_path):
    F.restore_across_the_month_wrap(EMU, tmp_path)


def test_restore_interior_from_a_z_level_clim_file_on_tiles_with_neighbours(tmp_path):
    F.restore_on_tiles(EMU, tmp_path)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_of_the_z_level_cold_start_round_once(tmp_path, variant):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    F.f32_rounds_once(VARIANTS[variant], tmp_path)
