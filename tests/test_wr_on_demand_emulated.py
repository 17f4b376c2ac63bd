"""wr only when something reads it, on the host build of the unmodified kernel sources (tests/emu): the checks of
tests/wr_on_demand_checks.py against the CPU oracle, bit for bit, and the launch counts from the library's own event profile."""
import os
import subprocess

import pytest

import wr_on_demand_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("warm", [False, True], ids=["iint1", "warm"])
@pytest.mark.parametrize("nml", chk.NAMELISTS, ids=str)
@pytest.mark.parametrize("case", chk.CASES)
def test_several_steps_without_observation(case, nml, warm):
    """run(2), run(1), run(2) with nothing read in between, then one download: every array that is not scratch, wr included"""
    chk.unobserved_steps(EMU, case, nml, warm)


def test_one_long_run_without_observation():
    chk.unobserved_steps(EMU, "archipelago", None, False, calls=(7,))


@pytest.mark.parametrize("point", chk.POINTS)
@pytest.mark.parametrize("case,warm", [("seamount", False), ("archipelago", True)], ids=["seamount-iint1", "archipelago-warm"])
def test_routine_by_routine_wr_read_at_any_point(case, warm, point):
    """the Fortran host's sequence for three steps; wr alone is read after one kind of call in every step and is the oracle's wr of
    the last completed step -- also after the last external substep, which has rewritten etf"""
    chk.routine_by_routine(EMU, case, warm, point)


def test_launch_counts():
    """run(5): no realvertvl; the download after it: one; with POMGPU_WR_NODEFER: five"""
    chk.launch_counts(EMU)


def test_launch_counts_routine_by_routine():
    """check_velocity after every step: no realvertvl, no k_restore_fields, no k_roundtrip in three steps"""
    chk.launch_counts_by_routine(EMU)


def test_standalone_realvertvl_reads_etf():
    chk.standalone_reads_etf(EMU)


@pytest.mark.parametrize("what", ["et", "w", "state"])
def test_writer_between_step_and_read(what):
    """an upload after unobserved steps finds wr formed from the state before it"""
    chk.writer_between_step_and_read(EMU, what)


def test_output_file_brings_wr_up_to_date(tmp_path):
    chk.output_file(EMU, tmp_path)


@pytest.mark.parametrize("name", ["wr", "et"])
def test_address_handed_out_ends_the_deferral(name):
    """after pomgpu_device_3d / pomgpu_device_2d the library cannot see reads or writes: realvertvl at the end of every step"""
    chk.address_handed_out(EMU, name)


def test_switch_flipped_on_a_live_context():
    chk.switch_flipped_live(EMU)


def test_dti2_changed_while_wr_is_pending():
    chk.dti2_changed_while_pending(EMU)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_lazy_equals_eager(variant):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.lazy_equals_eager(VARIANTS[variant])


def test_fp64_lazy_equals_eager():
    chk.lazy_equals_eager(EMU)
