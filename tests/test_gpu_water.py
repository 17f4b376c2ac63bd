"""pomgpu_water, pomgpu_set_water_files / _record and pomgpu_set_surface_sss on an MI355X: the checks of tests/water_checks.py with the
product library against the CPU oracle, bit for bit at 65x49x21 (the file forms at 8x8x6, the refusals at 9x8x6); the fp32-storage build
file path against setter path."""
import pytest

import water_checks as chk
from extpom_amd import lib

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)
CASES = ["archipelago", "seamount"]


@pytest.mark.parametrize("case", CASES)
def test_start_reads_records_zero_and_one(tmp_path, case):
    chk.start_from_record_zero(LIB, tmp_path, case)


@pytest.mark.parametrize("cont_bry", [0, 7])
@pytest.mark.parametrize("case", CASES)
def test_record_change_at_iwater(tmp_path, case, cont_bry):
    chk.across_a_record_change(LIB, tmp_path, case, cont_bry)


@pytest.mark.parametrize("case", CASES)
def test_last_step_reads_one_more_record(tmp_path, case):
    chk.last_step_reads_one_more(LIB, tmp_path, case)


@pytest.mark.parametrize("case", CASES)
def test_sss_into_ssurf(tmp_path, case):
    chk.sss_into_ssurf(LIB, tmp_path, case)


def test_file_forms(tmp_path):
    chk.file_forms(LIB, tmp_path)


def test_refusals(tmp_path):
    chk.refusals(LIB, tmp_path)


def test_fp32_storage_build_file_path_equals_setter_path(tmp_path):
    chk.file_equals_setters_f32(lib.LIBPATH_F32, tmp_path)


def test_tiles_equal_the_single_tile_and_add_no_round():
    """four contexts on GPU 0 with the event-ordered mover of tests/gpu_tiles_threads.py: a process of its own, as that harness is (torch
    and the library must share one HIP runtime, so torch is imported first there)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_water_tiles.py")], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "WATER-TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
