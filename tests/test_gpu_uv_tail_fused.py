"""profu / profv fused with the velocity filter, uf and vf on demand, on an MI355X: the checks of tests/uv_tail_fused_checks.py with
the product library against the CPU oracle, bit for bit; the fp32 study builds lazy against eager; the same steps twice."""
import pytest

import uv_tail_fused_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("nml", list(chk.NAMELISTS))
@pytest.mark.parametrize("case", chk.CASES)
def test_unobserved_steps_every_case_and_namelist(case, nml):
    chk.unobserved_steps(LIB, case, chk.NAMELISTS[nml], (65, 49, 21))


@pytest.mark.parametrize("size", chk.SIZES_FUSED[1:], ids=str)
def test_unobserved_steps_every_shape(size):
    chk.unobserved_steps(LIB, "archipelago", None, size)


@pytest.mark.parametrize("case", ["seamount", "island"])
def test_unobserved_steps_one_interior_column(case):
    chk.unobserved_steps(LIB, case, None, (8, 8, 6))


@pytest.mark.parametrize("size", chk.SIZES_FALLBACK, ids=str)
def test_unobserved_steps_fallback_shapes(size):
    chk.unobserved_steps(LIB, "archipelago", None, size, fused=False)


def test_unobserved_steps_256x192x50():
    chk.unobserved_steps(LIB, "archipelago", None, (256, 192, 50), calls=(2, 1))


@pytest.mark.parametrize("name", ["uf", "vf"])
@pytest.mark.parametrize("point", chk.POINTS)
def test_routine_by_routine_uf_vf_read_at_any_point(point, name):
    chk.routine_by_routine(LIB, "archipelago", point, name)


@pytest.mark.parametrize("what", ["u", "uf", "state", "restart", "tune"])
def test_writer_after_unobserved_steps(what, tmp_path):
    chk.writer_after_steps(LIB, what, tmp_path)


def test_address_handed_out_ends_the_fusion():
    chk.address_handed_out(LIB)


def test_switch_flipped_on_a_live_context():
    chk.switch_flipped_live(LIB)


def test_launch_counts():
    chk.launch_counts(LIB)


@pytest.mark.parametrize("variant", ["f64", "f32", "f32a"])
def test_lazy_equals_eager(variant):
    from extpom_amd import lib as L
    chk.lazy_equals_eager({"f64": None, "f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant])


def test_same_steps_twice_identical_bits():
    """20 steps twice in one context and once in a second: a bottom friction racing with the neighbours' filter shows here"""
    chk.deterministic(LIB)
