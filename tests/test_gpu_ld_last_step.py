"""l and dtef stored only in the last step of a pomgpu_run call, on an MI355X: the checks of tests/ld_last_step_checks.py with the
product library against the CPU oracle, bit for bit, at the shapes where every phase of k_profq's walk down and both workgroup shapes
exist; the two fp32 builds run(4) against 4 x run(1)."""
import pytest

import ld_last_step_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("eager", [False, True], ids=["default", "LD_EAGER"])
@pytest.mark.parametrize("case,size,switch", chk.SHAPES, ids=chk.SHAPE_IDS)
def test_same_bits_either_way(case, size, switch, eager):
    chk.same_bits_either_way(LIB, case, size, switch, eager)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_same_bits_either_way(variant):
    from extpom_amd import lib as L
    chk.same_bits_either_way({"f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant], "archipelago", (65, 49, 21), oracle=False)


@pytest.mark.parametrize("case,size,switch", chk.SHAPES, ids=chk.SHAPE_IDS)
def test_last_step_stores_every_cell(case, size, switch):
    chk.last_step_stores_every_cell(LIB, case, size, switch)


@pytest.mark.parametrize("eager", [False, True], ids=["default", "LD_EAGER"])
def test_decision_run(eager):
    chk.decision_run(LIB, eager)


def test_decision_advance():
    chk.decision_advance(LIB)


def test_decision_address_handed_out():
    chk.decision_address_handed_out(LIB)


def test_decision_direct_calls():
    chk.decision_direct_calls(LIB)


def test_decision_tune_placement():
    """on the device alone: the host build's pomgpu_tune_placement tries nothing (there is no placement to measure)"""
    chk.decision_tune_placement(LIB)


def test_observers_between_calls(tmp_path):
    chk.observers_between_calls(LIB, tmp_path)
