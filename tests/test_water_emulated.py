"""pomgpu_water, pomgpu_set_water_files / _record and pomgpu_set_surface_sss -- `water` (bounds_forcing.f:986-1020), read_water_pnetcdf
(io_pnetcdf.F:3227-3272) and bounds_forcing.f:979 uncommented -- through the host build of the unmodified sources (tests/emu): the schedule
(no cont_bry, records from 0, no iend guard), the header checks, the fetch and the index arithmetic of the kernels, bit for bit against
the CPU oracle with the restatement of tests/water_expect.py written into its state.  The checks are tests/water_checks.py;
tests/test_gpu_water.py runs the same ones on the device."""
import os
import subprocess

import pytest

import water_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
EMU_F32 = os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so")
CASES = ["archipelago", "seamount"]


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("case", CASES)
def test_start_reads_records_zero_and_one(tmp_path, case):
    chk.start_from_record_zero(EMU, tmp_path, case)


@pytest.mark.parametrize("cont_bry", [0, 7])
@pytest.mark.parametrize("case", CASES)
def test_record_change_at_iwater(tmp_path, case, cont_bry):
    chk.across_a_record_change(EMU, tmp_path, case, cont_bry)


@pytest.mark.parametrize("case", CASES)
def test_last_step_reads_one_more_record(tmp_path, case):
    chk.last_step_reads_one_more(EMU, tmp_path, case)


@pytest.mark.parametrize("case", CASES)
def test_sss_into_ssurf(tmp_path, case):
    chk.sss_into_ssurf(EMU, tmp_path, case)


def test_file_forms(tmp_path):
    chk.file_forms(EMU, tmp_path)


def test_refusals(tmp_path):
    chk.refusals(EMU, tmp_path)


def test_fp32_storage_build_file_path_equals_setter_path(tmp_path):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), "f32"], stdout=subprocess.DEVNULL)
    chk.file_equals_setters_f32(EMU_F32, tmp_path)


def test_tiles_equal_the_single_tile_and_add_no_round(tmp_path):
    chk.tiles_equal_single_tile(EMU, tmp_path)
