"""pomgpu_set_lateral_sides on an MI355X: the checks of tests/lateral_sides_checks.py with the product library against
tests/lateral_sides_expect.py's restatement, the CPU oracle fed its records and the setter path, bit for bit; the fp32 study builds
against the same fp64 records."""
import pytest

import lateral_sides_checks as C
import lateral_sides_expect as LS
from extpom_amd import lib
from forcing_files_checks import BASE

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("dtype,chunk_kb", [("d", None), ("f", 1)], ids=["double", "float_1KiB_chunks"])
def test_four_sided_file_equals_the_oracle_and_the_setters_across_record_changes(tmp_path, dtype, chunk_kb):
    C.file_setters_oracle(LIB, tmp_path, "archipelago", dtype=dtype, chunk_kb=chunk_kb)


@pytest.mark.parametrize("nml", [dict(BASE), dict(BASE, cont_bry=7)], ids=["base", "cont_bry"])
def test_seamount_east_and_west_equals_the_oracle_and_the_setters(tmp_path, nml):
    C.file_setters_oracle(LIB, tmp_path, "seamount", mask=LS.EAST | LS.WEST, nml=nml)


@pytest.mark.parametrize("size,case", [((8, 8, 6), "seamount"), ((20, 17, 6), "archipelago")], ids=str)
def test_every_mask_with_a_file_of_the_on_sides_only(tmp_path, size, case):
    C.every_mask(LIB, tmp_path, size, case=case)


def test_the_default_mask_is_todays_reader(tmp_path):
    C.default_is_todays(LIB, tmp_path)


@pytest.mark.parametrize("case,size", [("archipelago", (65, 49, 21)), ("seamount", (8, 8, 6))], ids=str)
def test_z_levels_on_four_sides_equal_the_oracle_and_the_setters(tmp_path, case, size):
    C.z_file_setters_oracle(LIB, tmp_path, case, size=size)


def test_init_clim_and_a_four_sided_lbry_all_on_z_after_a_cold_start(tmp_path):
    C.all_on_z_after_a_cold_start(LIB, tmp_path)


def test_tiles_read_their_pieces_of_four_sides_and_step_like_the_single_tile():
    """four contexts on GPU 0 with the event-ordered mover of tests/forcing_files_checks.py: a process of its own, as that harness is (torch
    and the library must share one HIP runtime, so torch is imported first there)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_lateral_sides_tiles.py")], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "LATERAL-SIDES-TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_every_refusal_leaves_the_state_and_the_registration_as_they_were(tmp_path):
    C.refusals(LIB, tmp_path)


@pytest.mark.parametrize("path", [lib.LIBPATH_F32, lib.LIBPATH_F32A], ids=["f32", "f32a"])
def test_fp32_builds_fetch_the_fp64_record(tmp_path, path):
    C.f32_record_equals_fp64(LIB, path, tmp_path)
