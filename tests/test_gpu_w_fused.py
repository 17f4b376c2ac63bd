"""w formed inside the q2 / q2l advection march, on an MI355X: the checks of tests/w_fused_checks.py with the product library
against the CPU oracle, bit for bit; the three builds against POMGPU_W_NOFUSE (the fp32-arithmetic variant has no fused kernel)."""
import pytest

import w_fused_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("nml", list(chk.NAMELISTS))
@pytest.mark.parametrize("case", chk.CASES)
def test_unobserved_steps_every_case_and_namelist(case, nml):
    chk.unobserved_steps(LIB, case, chk.NAMELISTS[nml], (65, 49, 21))


def test_inputs_exercise_the_fused_march():
    chk.unobserved_steps(LIB, "archipelago", None, (65, 49, 21), need=("w", "w_surface", "w_bottom", "vfluxf", "land_inside", "q2"))


@pytest.mark.parametrize("size", chk.SIZES[1:], ids=str)
def test_unobserved_steps_every_shape(size):
    chk.unobserved_steps(LIB, "archipelago", None, size)


def test_unobserved_steps_256x192x50():
    chk.unobserved_steps(LIB, "archipelago", None, (256, 192, 50), calls=(2, 1))


@pytest.mark.parametrize("switch", list(chk.KEEP))
def test_paths_that_keep_the_pair(switch):
    chk.unobserved_steps(LIB, "archipelago", None, (65, 49, 21), switch=switch)


def test_unmasked_surface_flux_on_land():
    chk.land_forced(LIB)


def test_switch_flipped_on_a_live_context():
    chk.switch_flipped_live(LIB)


def test_routine_by_routine_host_is_fused():
    chk.routine_by_routine(LIB)


def test_stand_alone_vertvl_keeps_its_kernel():
    chk.stand_alone_entry_points(LIB)


@pytest.mark.parametrize("variant", ["f64", "f32", "f32a"])
def test_fused_equals_pair(variant):
    from extpom_amd import lib as L
    chk.fused_equals_pair({"f64": None, "f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant], fuses=variant != "f32a")
