"""pomgpu_set_lateral_sides -- the lbry file feeding any of the four open boundaries -- through the host builds of the unmodified sources
(tests/emu): the setting, the registration and its refusals, k_lat_unpack under every mask and the eight-line k_ztosig_line launch, bit for
bit against tests/lateral_sides_expect.py and the CPU oracle.  The device runs the same checks (test_gpu_lateral_sides.py).
THE HOST BUILD IS SLOW, so of check 1 the second context fed by the setters runs on the NC_DOUBLE archipelago variant alone (the oracle,
the stricter bar, on all), and the cold start on z levels runs on archipelago only."""
import os
import subprocess

import pytest

import lateral_sides_checks as C
import lateral_sides_expect as LS
from forcing_files_checks import BASE

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


@pytest.mark.parametrize("dtype,chunk_kb,setters", [("d", None, True), ("f", 1, False)], ids=["double", "float_1KiB_chunks"])
def test_four_sided_file_equals_the_oracle_and_the_setters_across_record_changes(tmp_path, dtype, chunk_kb, setters):
    C.file_setters_oracle(EMU, tmp_path, "archipelago", dtype=dtype, chunk_kb=chunk_kb, setters=setters)


@pytest.mark.parametrize("nml", [dict(BASE), dict(BASE, cont_bry=7)], ids=["base", "cont_bry"])
def test_seamount_east_and_west_equals_the_oracle(tmp_path, nml):
    C.file_setters_oracle(EMU, tmp_path, "seamount", mask=LS.EAST | LS.WEST, nml=nml, setters=False)


@pytest.mark.parametrize("size,case", [((8, 8, 6), "seamount"), ((20, 17, 6), "archipelago")], ids=str)
def test_every_mask_with_a_file_of_the_on_sides_only(tmp_path, size, case):
    C.every_mask(EMU, tmp_path, size, case=case)


def test_the_default_mask_is_todays_reader(tmp_path):
    C.default_is_todays(EMU, tmp_path)


@pytest.mark.parametrize("case,size", [("archipelago", (65, 49, 21)), ("seamount", (8, 8, 6))], ids=str)
def test_z_levels_on_four_sides_equal_the_oracle(tmp_path, case, size):
    C.z_file_setters_oracle(EMU, tmp_path, case, size=size, setters=False)


def test_init_clim_and_a_four_sided_lbry_all_on_z_after_a_cold_start(tmp_path):
    C.all_on_z_after_a_cold_start(EMU, tmp_path)


def test_tiles_read_their_pieces_of_four_sides_and_step_like_the_single_tile(tmp_path):
    C.tiles(EMU, tmp_path)


def test_every_refusal_leaves_the_state_and_the_registration_as_they_were(tmp_path):
    C.refusals(EMU, tmp_path)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_fetch_the_fp64_record(tmp_path, variants, variant):
    C.f32_record_equals_fp64(EMU, variants[variant], tmp_path)
