"""aam and aam2d formed inside advct's march, on an MI355X: the checks of tests/aam_fused_checks.py with the product library against
the CPU oracle, bit for bit; the three builds against POMGPU_AAM_NOFUSE (the fp32-arithmetic variant has no fused kernel)."""
import pytest

import aam_fused_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("nml", list(chk.NAMELISTS))
@pytest.mark.parametrize("case", chk.CASES)
def test_unobserved_steps_every_case_and_namelist(case, nml):
    chk.unobserved_steps(LIB, case, chk.NAMELISTS[nml], (65, 49, 21), copies=0 if nml in ("default", "mode4", "npg2") else None)


def test_inputs_exercise_the_fused_march():
    chk.unobserved_steps(LIB, "archipelago", None, (65, 49, 21), need=("aam_new", "rim_keeps_init", "aam2d_varies", "land_inside"))


@pytest.mark.parametrize("size", chk.SIZES[1:], ids=str)
def test_unobserved_steps_every_shape(size):
    chk.unobserved_steps(LIB, "archipelago", None, size, copies=0)


def test_unobserved_steps_256x192x50():
    chk.unobserved_steps(LIB, "archipelago", None, (256, 192, 50), calls=(2, 1), copies=0)


def test_aam_nofuse_keeps_the_pair():
    chk.unobserved_steps(LIB, "archipelago", None, (65, 49, 21), switch="AAM_NOFUSE")


@pytest.mark.parametrize("switch", chk.STILL_FUSED)
def test_single_field_marches_read_the_current_buffer(switch):
    chk.unobserved_steps(LIB, "archipelago", None, (65, 49, 21), switch=switch, copies=0)


def test_nadv1_copies_in_front_of_advt1():
    chk.unobserved_steps(LIB, "seamount", dict(nadv=1), (20, 17, 6), calls=(3,), copies=1)


def test_both_parities_observed_and_an_upload_at_the_odd_one():
    chk.both_parities(LIB)


def test_both_parities_with_the_time_mean_on():
    chk.both_parities(LIB, mean=True)


def test_restart_written_and_read_at_the_odd_parity(tmp_path):
    chk.restart_at_the_odd_parity(LIB, tmp_path)


def test_address_handed_out_ends_the_fusion():
    chk.address_handed_out(LIB)


def test_switch_flipped_on_a_live_context():
    chk.switch_flipped_live(LIB)


def test_stand_alone_entry_points_after_fused_steps():
    chk.stand_alone_entry_points(LIB)


def test_routine_by_routine_host_keeps_the_pair_without_a_copy_per_step():
    chk.routine_by_routine(LIB)


@pytest.mark.parametrize("variant", ["f64", "f32", "f32a"])
def test_fused_equals_pair(variant):
    from extpom_amd import lib as L
    chk.fused_equals_pair({"f64": None, "f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant], fuses=variant != "f32a")
