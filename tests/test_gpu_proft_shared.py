"""proft of T and S in one lane, on an MI355X: the checks of tests/proft_shared_checks.py with the product library against the CPU
oracle, bit for bit; the three builds against POMGPU_PROFT_TWIN."""
import pytest

import proft_shared_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("nbct,nbcs", chk.PAIRS)
@pytest.mark.parametrize("case", chk.CASES)
def test_every_pair_of_surface_conditions(case, nbct, nbcs):
    chk.whole_steps(LIB, case, (65, 49, 21), nbct, nbcs)


@pytest.mark.parametrize("nbc", [1, 3])
@pytest.mark.parametrize("size", chk.SHAPES, ids=str)
def test_every_shape(size, nbc):
    chk.whole_steps(LIB, "archipelago", size, nbc, nbc)


def test_whole_steps_256x192x50():
    """the headline's instantiation (KBT = 50) on more than one workgroup row and column"""
    chk.whole_steps(LIB, "archipelago", (256, 192, 50))


@pytest.mark.parametrize("nbc", [1, 3])
def test_switch_keeps_the_twin(nbc):
    chk.whole_steps(LIB, "archipelago", (65, 49, 21), nbc, nbc, switch=True)


@pytest.mark.parametrize("nbc", [1, 3])
def test_switch_flipped_on_a_live_context(nbc):
    chk.switch_flipped_live(LIB, nbc)


@pytest.mark.parametrize("variant", ["f64", "f32", "f32a"])
def test_lane_equals_twin(variant):
    from extpom_amd import lib as L
    chk.lane_equals_twin({"f64": None, "f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant])
