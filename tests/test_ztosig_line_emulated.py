"""pomgpu_ztosig_line and pomgpu_set_z_lateral -- the line form of ztosig for z-level lateral files, bounds_forcing.f:636-716 -- through the
host builds of the unmodified sources (tests/emu): every index and every operation of the kernel, the fetch, the registration and its
refusals, bit for bit against tests/ztosig_line_expect.py and the reference's recorded output.  The device runs the same checks
(test_gpu_ztosig_line.py)."""
import os
import subprocess

import pytest

import ztosig_line_checks as C
import ztosig_line_files_checks as F
from ztosig_line_expect import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def variants():
    for v in VARIANTS:
        subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), v], stdout=subprocess.DEVNULL)
    return VARIANTS


@pytest.mark.parametrize("salt", [False, True], ids=["T", "S"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_edge_equals_the_expectation_and_the_references_digest(shape, salt):
    C.standalone_equals_the_expectation(EMU, shape, salt)


def test_trimmed_tile_keeps_its_padding():
    C.trimmed_tile_keeps_its_padding(EMU)


def test_tiles_equal_the_single_tile_on_their_piece_without_a_message_round():
    C.tiles(EMU)


def test_refusals_and_a_context_that_has_stepped():
    C.refusals_and_a_stepped_context(EMU)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_give_the_fp64_line(variants, variant):
    C.standalone_equals_the_expectation(variants[variant], (20, 17, 5, 6))
    C.standalone_equals_the_expectation(variants[variant], (65, 49, 33, 21), salt=True)


# ---- z-level lbry files (pomgpu_set_z_lateral) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,kind,chunk_kb", [("archipelago", "d", None), ("seamount", "f", 1)], ids=str)
def test_one_run_across_lateral_records_equals_the_oracle_and_the_setters(tmp_path, case, kind, chunk_kb):
    F.file_setters_oracle(EMU, tmp_path, case, kind=kind, chunk_kb=chunk_kb)


def test_the_smallest_grid(tmp_path):
    F.file_setters_oracle(EMU, tmp_path, "seamount", size=(8, 8, 6), setters=False)


def test_init_clim_and_lbry_all_on_z_after_a_cold_start(tmp_path):
    F.all_on_z_after_a_cold_start(EMU, tmp_path)


def test_tiles_map_their_lines_from_the_file_and_step_like_the_single_tile(tmp_path):
    F.tiles(EMU, tmp_path)


def test_setting_off_is_todays_behaviour(tmp_path):
    F.setting_off(EMU, tmp_path)


def test_every_new_refusal_leaves_the_state_as_it_was(tmp_path):
    F.refusals(EMU, tmp_path)
    F.tile_window_must_fit(EMU, tmp_path)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_fetch_the_fp64_record(tmp_path, variants, variant):
    F.f32_record_equals_fp64(EMU, variants[variant], tmp_path)
