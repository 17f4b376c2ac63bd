"""Round trips through tclim, sclim, rmean read only where bits change, on an MI355X: the checks of tests/rt_flags_checks.py with the
product library against the CPU oracle, bit for bit -- one, two and three column blocks, a last workgroup of one row, land inside, and
the climatology as the case makes it, far from the field everywhere, and far from it in a seeded 30 % of the cells; the two fp32
builds flags against POMGPU_RT_LOAD against 4 x run(1)."""
import pytest

import rt_flags_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("clim", chk.CLIMS)
@pytest.mark.parametrize("case,size", chk.SHAPES, ids=chk.SHAPE_IDS)
def test_same_bits_every_way(case, size, clim):
    chk.same_bits_every_way(LIB, case, size, clim)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_same_bits_every_way(variant):
    from extpom_amd import lib as L
    chk.same_bits_every_way({"f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant], "archipelago", (65, 49, 21), "part", oracle=False)


def test_switch_on_a_live_context():
    chk.switch_on_a_live_context(LIB)


def test_decision_address_handed_out():
    chk.decision_address_handed_out(LIB)


def test_decision_advt2_single():
    chk.decision_advt2_single(LIB)


def test_decision_stand_alone_pair():
    chk.decision_stand_alone_pair(LIB)


@pytest.mark.parametrize("how", ["download", "upload"])
def test_observer_between_routines(how):
    chk.observer_between_routines(LIB, how)


def test_upload_changes_rho():
    chk.upload_changes_rho(LIB)
