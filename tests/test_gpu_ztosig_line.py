"""pomgpu_ztosig_line and pomgpu_set_z_lateral on an MI355X: the checks of tests/ztosig_line_checks.py and tests/ztosig_line_files_checks.py
with the product library against tests/ztosig_line_expect.py's restatement and the reference's recorded digests
(tests/golden/ztosig_line.json), bit for bit; the fp32 study builds against the same fp64 lines."""
import pytest

import ztosig_line_checks as C
import ztosig_line_files_checks as F
from extpom_amd import lib
from ztosig_line_expect import SHAPES

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("salt", [False, True], ids=["T", "S"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_edge_equals_the_expectation_and_the_references_digest(shape, salt):
    C.standalone_equals_the_expectation(LIB, shape, salt)


def test_trimmed_tile_keeps_its_padding():
    C.trimmed_tile_keeps_its_padding(LIB)


def test_tiles_equal_the_single_tile_on_their_piece_without_a_message_round():
    C.tiles(LIB)


def test_refusals_and_a_context_that_has_stepped():
    C.refusals_and_a_stepped_context(LIB)


@pytest.mark.parametrize("path", [lib.LIBPATH_F32, lib.LIBPATH_F32A], ids=["f32", "f32a"])
def test_fp32_builds_give_the_fp64_line(path):
    C.standalone_equals_the_expectation(path, (20, 17, 5, 6))
    C.standalone_equals_the_expectation(path, (65, 49, 33, 21), salt=True)


# ---- z-level lbry files (pomgpu_set_z_lateral) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,chunk_kb", [("d", None), ("f", 1)], ids=str)
@pytest.mark.parametrize("case", ["archipelago", "seamount"])
def test_one_run_across_lateral_records_equals_the_oracle_and_the_setters(tmp_path, case, kind, chunk_kb):
    F.file_setters_oracle(LIB, tmp_path, case, kind=kind, chunk_kb=chunk_kb)


def test_the_smallest_grid(tmp_path):
    F.file_setters_oracle(LIB, tmp_path, "seamount", size=(8, 8, 6), setters=False)


@pytest.mark.parametrize("case", ["archipelago", "seamount"])
def test_init_clim_and_lbry_all_on_z_after_a_cold_start(tmp_path, case):
    F.all_on_z_after_a_cold_start(LIB, tmp_path, case=case)


def test_tiles_map_their_lines_from_the_file_and_step_like_the_single_tile():
    """four contexts on GPU 0 with the event-ordered mover of tests/forcing_files_checks.py: a process of its own, as that harness is (torch
    and the library must share one HIP runtime, so torch is imported first there)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_ztosig_line_tiles.py")], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "ZTOSIG-LINE-FILE-TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_setting_off_is_todays_behaviour(tmp_path):
    F.setting_off(LIB, tmp_path)


def test_every_new_refusal_leaves_the_state_as_it_was(tmp_path):
    F.refusals(LIB, tmp_path)
    F.tile_window_must_fit(LIB, tmp_path)


@pytest.mark.parametrize("path", [lib.LIBPATH_F32, lib.LIBPATH_F32A], ids=["f32", "f32a"])
def test_fp32_builds_fetch_the_fp64_record(tmp_path, path):
    F.f32_record_equals_fp64(LIB, path, tmp_path)
