"""l and dtef stored only in the last step of a pomgpu_run call, on the host builds of the unmodified kernel sources (tests/emu): the
checks of tests/ld_last_step_checks.py -- run(4) against 4 x run(1) and the CPU oracle, bit for bit, and the host's decision from the
event profile's count profq_ld_store.  (The host build keeps every elimination vector in memory: the shapes choose the phases of the
walk on the device, tests/test_gpu_ld_last_step.py; here they run the same host logic and the same kernel body.)"""
import os
import subprocess

import pytest

import ld_last_step_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("eager", [False, True], ids=["default", "LD_EAGER"])
@pytest.mark.parametrize("case,size,switch", chk.SHAPES, ids=chk.SHAPE_IDS)
def test_same_bits_either_way(case, size, switch, eager):
    chk.same_bits_either_way(EMU, case, size, switch, eager)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_same_bits_either_way(variant):
    """no oracle for the fp32 study builds: run(4) against 4 x run(1)"""
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.same_bits_either_way(VARIANTS[variant], "archipelago", (65, 49, 21), oracle=False)


@pytest.mark.parametrize("case,size,switch", chk.SHAPES, ids=chk.SHAPE_IDS)
def test_last_step_stores_every_cell(case, size, switch):
    chk.last_step_stores_every_cell(EMU, case, size, switch)


@pytest.mark.parametrize("eager", [False, True], ids=["default", "LD_EAGER"])
def test_decision_run(eager):
    chk.decision_run(EMU, eager)


def test_decision_advance():
    chk.decision_advance(EMU)


def test_decision_address_handed_out():
    chk.decision_address_handed_out(EMU)


def test_decision_direct_calls():
    chk.decision_direct_calls(EMU)


def test_decision_step_in_front_of_a_record_step_stores():
    chk.decision_record_step(EMU)


def test_decision_two_tiles_with_exchange_hook():
    import test_kernels_emulated_tiles as T
    chk.decision_two_tiles(EMU, T)


def test_observers_between_calls(tmp_path):
    chk.observers_between_calls(EMU, tmp_path)
