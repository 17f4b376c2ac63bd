"""divi, gpow15 and proft_rad_q on an MI355X, through pomgpu_math_probe of the product library: the checks of
tests/device_math_checks.py.  Here divi is the reciprocal-and-two-corrections algorithm, nearbyint / ldexp / ilogb / fmod / exp under
proft_rad_q are the device library's, and the tables of gpow15 are the ones in device memory."""
import pytest

import device_math_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)
POW_SETS = ["tables", "binades", "physical", "special"]


def test_probe_refuses_bad_arguments_and_runs_every_block():
    chk.probe_refusals(LIB)


@pytest.mark.parametrize("name", POW_SETS)
def test_gpow15_is_libm_pow_bit_for_bit(name):
    chk.pow_bits(LIB, name)


def test_dens_on_extreme_salinity_is_the_oracles():
    chk.dens_on_extreme_salinity(LIB)


def test_proft_rad_q_is_the_quad_expression_rounded_once():
    chk.rad_q_bits(LIB)


@pytest.mark.parametrize("op", ["DIVI", "DIVI_F32"])
def test_divi_is_the_ieee_quotient(op):
    chk.divi_bits(LIB, op)


def test_divi_at_the_documented_floor():
    chk.divi_floor_bits(LIB)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_run_the_same_functions(variant):
    """the entry exists in all three builds; dens and the column solves stay fp64 in the study variants"""
    from extpom_amd import lib as L
    path = {"f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant]
    chk.pow_bits(path, "special")
    chk.divi_floor_bits(path)
