"""pomgpu_set_forcing_files on an MI355X: the checks of tests/forcing_files_checks.py with the product library against the CPU oracle,
bit for bit at 65x49x21 (the taper also at 8x8x6 and 66x50x21); the fp32 study builds file path against setter path."""
import pytest

import forcing_files_checks as chk
from extpom_amd import lib

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("variant", list(chk.VARIANTS))
@pytest.mark.parametrize("case", ["archipelago", "seamount"])
def test_file_path_equals_setter_path_equals_oracle(tmp_path, case, variant):
    chk.file_setters_oracle(LIB, tmp_path, case, variant)


@pytest.mark.parametrize("size", [(8, 8, 6), (65, 49, 21), (66, 50, 21)], ids=str)
def test_wind_taper(tmp_path, size):
    chk.taper_alone(LIB, tmp_path, size)


def test_file_layouts(tmp_path):
    chk.layouts(LIB, tmp_path)


def test_restore_interior_across_a_record_change(tmp_path):
    chk.restore_across_a_record_change(LIB, tmp_path)


def test_exact_records_to_iend_and_one_fewer(tmp_path):
    chk.exact_records_to_iend(LIB, tmp_path)


def test_refusals_at_registration(tmp_path):
    chk.refusals(LIB, tmp_path)


@pytest.mark.parametrize("path", [lib.LIBPATH_F32, lib.LIBPATH_F32A], ids=["f32", "f32a"])
def test_fp32_builds_file_path_equals_setter_path(tmp_path, path):
    chk.file_equals_setters_f32(path, tmp_path)


def test_tiles_file_path_equals_setter_path():
    """four contexts on GPU 0 with the event-ordered mover of tests/gpu_tiles_threads.py: a process of its own, as that harness is (torch
    and the library must share one HIP runtime, so torch is imported first there)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_forcing_tiles.py")], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "FORCING-TILES-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
