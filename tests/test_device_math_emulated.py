"""divi, gpow15 and proft_rad_q through pomgpu_math_probe on the host build of the unmodified kernel sources (tests/emu): the checks
of tests/device_math_checks.py.  gpow15 and proft_rad_q run here as written (with the host's libm under proft_rad_q); divi is the plain
quotient in this build, so its checks cover the path to the entry only -- the algorithm runs in tests/test_gpu_device_math.py."""
import os
import subprocess

import pytest

import device_math_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
POW_SETS = ["tables", "binades", "physical", "special"]


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


def test_probe_refuses_bad_arguments_and_runs_every_block():
    chk.probe_refusals(EMU)


def test_pow_inputs_reach_every_row_of_both_tables():
    chk.pow_inputs_reach_every_table_row()


@pytest.mark.parametrize("name", POW_SETS)
def test_libm_pow_is_within_one_ulp_of_the_exact_power(name):
    chk.pow_libm_is_within_one_ulp_of_exact(name)


@pytest.mark.parametrize("name", POW_SETS)
def test_gpow15_is_libm_pow_bit_for_bit(name):
    chk.pow_bits(EMU, name)


def test_dens_on_extreme_salinity_is_the_oracles():
    chk.dens_on_extreme_salinity(EMU)


def test_rad_q_fixture_holds_every_family():
    chk.rad_fixture_holds_what_it_should()


def test_rad_q_fixture_is_what_the_generator_makes():
    """where g++ and libquadmath exist: the stored inputs and REAL(16) values are regenerated and must be the stored ones"""
    if not chk.golden_maker().have_compiler():
        pytest.skip("no g++ here: the stored fixture is used as it is")
    chk.rad_fixture_is_current()


def test_proft_rad_q_is_the_quad_expression_rounded_once():
    chk.rad_q_bits(EMU)


@pytest.mark.parametrize("op", ["DIVI", "DIVI_F32"])
def test_divi_is_the_ieee_quotient(op):
    chk.divi_bits(EMU, op)


def test_divi_at_the_documented_floor():
    chk.divi_floor_bits(EMU)
