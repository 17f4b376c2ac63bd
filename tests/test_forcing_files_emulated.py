"""pomgpu_set_forcing_files -- the reference's forcing readers (io_pnetcdf.F:2912-3621) without PnetCDF -- through the host build of the
unmodified sources (tests/emu): the header parser, the refusals, the fetch schedule and the index arithmetic of the unpack kernels, bit
for bit against the CPU oracle fed the records tests/forcing_expect.py restates.  The checks are tests/forcing_files_checks.py;
tests/test_gpu_forcing_files.py runs the same ones on the device."""
import os
import subprocess

import pytest

import forcing_files_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
EMU_VARIANT = {v: os.path.join(ROOT, "tests", "_emu_" + v, "libpomgpu_emu_" + v + ".so") for v in ("f32", "f32a")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("variant", list(chk.VARIANTS))
@pytest.mark.parametrize("case", ["archipelago", "seamount"])
def test_file_path_equals_setter_path_equals_oracle(tmp_path, case, variant):
    chk.file_setters_oracle(EMU, tmp_path, case, variant)


@pytest.mark.parametrize("size", [(8, 8, 6), (65, 49, 21), (66, 50, 21)], ids=str)
def test_wind_taper(tmp_path, size):
    chk.taper_alone(EMU, tmp_path, size)


def test_file_layouts(tmp_path):
    chk.layouts(EMU, tmp_path)


def test_restore_interior_across_a_record_change(tmp_path):
    chk.restore_across_a_record_change(EMU, tmp_path)


def test_exact_records_to_iend_and_one_fewer(tmp_path):
    chk.exact_records_to_iend(EMU, tmp_path)


def test_refusals_at_registration(tmp_path):
    chk.refusals(EMU, tmp_path)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_file_path_equals_setter_path(tmp_path, variant):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.file_equals_setters_f32(EMU_VARIANT[variant], tmp_path)


@pytest.mark.parametrize("timing", ["side stream at once", "side stream as late as possible"])
def test_tiles_file_path_equals_setter_path(tmp_path, monkeypatch, timing):
    """both side-stream timings of the host build (tests/emu/hip/hip_runtime.h: POMGPU_EMU_DEFER_SIDE runs the second stream's work at the
    latest moment the device could)"""
    if timing.endswith("possible"):
        monkeypatch.setenv("POMGPU_EMU_DEFER_SIDE", "1")
    else:
        monkeypatch.delenv("POMGPU_EMU_DEFER_SIDE", raising=False)
    chk.tiles_file_equals_setters(EMU, tmp_path)
