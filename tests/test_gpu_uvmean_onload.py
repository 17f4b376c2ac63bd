"""The depth-mean correction of u, v applied on load, on an MI355X: the checks of tests/uvmean_onload_checks.py with the product
library against the CPU oracle, bit for bit; the three builds against POMGPU_UVMEAN_PASS (the fp32-arithmetic variant keeps the pass)."""
import pytest

import uvmean_onload_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("nml", list(chk.NAMELISTS))
@pytest.mark.parametrize("case", chk.CASES)
def test_unobserved_steps_every_case_and_namelist(case, nml):
    chk.unobserved_steps(LIB, case, chk.NAMELISTS[nml], (65, 49, 21), onload=nml not in chk.FALLBACK_NML)


def test_inputs_exercise_the_correction():
    chk.unobserved_steps(LIB, "archipelago", None, (65, 49, 21), need=chk.ALL_NEEDS)


@pytest.mark.parametrize("size", chk.SIZES[1:], ids=str)
def test_unobserved_steps_every_shape(size):
    chk.unobserved_steps(LIB, "archipelago", None, size)


def test_kb_beyond_the_register_kernels_keeps_the_pass():
    chk.unobserved_steps(LIB, "archipelago", None, chk.SIZE_FALLBACK, onload=False)


def test_unobserved_steps_256x192x50():
    chk.unobserved_steps(LIB, "archipelago", None, (256, 192, 50), calls=(2, 1))


@pytest.mark.parametrize("switch", chk.KEEP)
def test_paths_that_keep_the_pass(switch):
    chk.unobserved_steps(LIB, "archipelago", None, (65, 49, 21), switch=switch)


def test_switch_flipped_on_a_live_context():
    chk.switch_flipped_live(LIB)


def test_routine_by_routine_host_corrects_on_load():
    chk.routine_by_routine(LIB)


def test_upload_of_u_before_mode_internal_falls_back():
    chk.routine_by_routine(LIB, upload_u=True)


def test_upload_of_another_u_before_mode_internal():
    chk.upload_changes_u(LIB)


def test_stand_alone_entry_points_keep_their_kernels():
    chk.stand_alone_entry_points(LIB)


@pytest.mark.parametrize("variant", ["f64", "f32", "f32a"])
def test_onload_equals_pass(variant):
    from extpom_amd import lib as L
    chk.onload_equals_pass({"f64": None, "f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant], onload=variant != "f32a")
