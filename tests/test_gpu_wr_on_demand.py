"""wr only when something reads it, on an MI355X: the checks of tests/wr_on_demand_checks.py with the product library against the CPU
oracle, bit for bit, at 65x49x21 and once at 256x192x50; the fp32 study builds lazy against eager."""
import pytest

import wr_on_demand_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("warm", [False, True], ids=["iint1", "warm"])
@pytest.mark.parametrize("case,nml", [("seamount", dict()), ("basin", dict(nadv=1)), ("archipelago", dict(mode=2)), ("seamount", dict(mode=4)),
                                      ("archipelago", dict(npg=2)), ("basin", dict()), ("archipelago", dict())], ids=str)
def test_several_steps_without_observation(case, nml, warm):
    chk.unobserved_steps(LIB, case, nml, warm)


def test_several_steps_without_observation_256x192x50():
    chk.unobserved_steps(LIB, "seamount", None, False, size=(256, 192, 50), calls=(2, 1))


@pytest.mark.parametrize("point", chk.POINTS)
def test_routine_by_routine_wr_read_at_any_point(point):
    chk.routine_by_routine(LIB, "archipelago", True, point)


def test_launch_counts():
    chk.launch_counts(LIB)


def test_launch_counts_routine_by_routine():
    chk.launch_counts_by_routine(LIB)


def test_standalone_realvertvl_reads_etf():
    chk.standalone_reads_etf(LIB)


@pytest.mark.parametrize("what", ["et", "w", "state"])
def test_writer_between_step_and_read(what):
    chk.writer_between_step_and_read(LIB, what)


def test_output_file_brings_wr_up_to_date(tmp_path):
    chk.output_file(LIB, tmp_path)


@pytest.mark.parametrize("name", ["wr", "et"])
def test_address_handed_out_ends_the_deferral(name):
    chk.address_handed_out(LIB, name)


def test_switch_flipped_on_a_live_context():
    chk.switch_flipped_live(LIB)


def test_dti2_changed_while_wr_is_pending():
    chk.dti2_changed_while_pending(LIB)


@pytest.mark.parametrize("variant", ["f64", "f32", "f32a"])
def test_lazy_equals_eager(variant):
    from extpom_amd import lib as L
    chk.lazy_equals_eager({"f64": None, "f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant])
