"""The tracers' files, means and inventory on the host build of the unmodified kernel sources (tests/emu): the checks of
tests/tracer_files_checks.py.  The emulation runs one lane at a time and has no lanes to shuffle between: the reduction tree of the
inventory is covered by tests/test_gpu_tracer_files.py, here the entry point's own scan stands in for it."""
import os
import subprocess

import pytest

import mean_output_checks as moc
import tracer_files_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("size,ntr", [((9, 8, 5), 1), ((11, 7, 5), 3), ((20, 17, 6), 8), ((65, 49, 21), 3)], ids=ids)
def test_round_trip_of_every_element(tmp_path, size, ntr):
    chk.round_trip(EMU, tmp_path, size, ntr)


def test_a_file_with_tr_alone_is_an_initial_file(tmp_path):
    chk.initial_file(EMU, tmp_path)


@pytest.mark.parametrize("size,adv", [((20, 17, 6), (2, 1)), ((20, 17, 6), (2, 2)), ((20, 17, 6), (1, 1)), ((65, 49, 21), (2, 1))], ids=ids)
def test_the_file_is_the_state(tmp_path, size, adv):
    """(2, 2) is the case that needs trfNN"""
    chk.file_is_the_state(EMU, tmp_path, "archipelago", size, adv)


def test_output_kind(tmp_path):
    chk.output_kind(EMU, tmp_path)


@pytest.mark.parametrize("chained", [False, True], ids=["io_wait", "run_right_after_the_write"])
def test_mean_file_and_means_equal_the_restatement(tmp_path, chained):
    chk.mean_file(EMU, tmp_path, chained)


def test_the_nine_fields_are_as_without_tracers(tmp_path):
    chk.nine_fields_unchanged(EMU, tmp_path)


def test_allocation_rules_of_the_tracer_accumulators():
    chk.allocation_rules(EMU)


@pytest.mark.parametrize("size", [(11, 7, 5), (9, 8, 5)], ids=ids)
def test_every_element_of_every_tracer_accumulator(size):
    chk.every_element(EMU, size)


@pytest.mark.parametrize("size,ntr", [((9, 8, 5), 1), ((11, 7, 5), 3), ((20, 17, 6), 8), ((65, 49, 21), 2)], ids=ids)
def test_inventory_equals_the_restatement(size, ntr):
    chk.inventory(EMU, size, ntr)


def test_inventory_masks_the_land():
    chk.inventory(EMU, (20, 17, 6), 2, land_huge=True)


def test_a_decaying_tracer_does_not_gain_inventory():
    chk.decay_does_not_grow(EMU)


def test_refusals_leave_everything_as_it_was(tmp_path):
    chk.refusals(EMU, tmp_path)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_refuse(tmp_path, variant):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.fp32_builds_refuse(VARIANTS[variant], tmp_path)


@pytest.mark.parametrize("split", [(1, 2), (2, 2)], ids=str)
def test_tiles_write_one_file_and_read_their_patches(tmp_path, split):
    chk.tiles(EMU, split[0], split[1], tmp_path)


def test_launch_counts_with_tracers():
    chk.launch_counts(EMU)


def test_launch_counts_without_tracers_are_the_parents():
    moc.launch_counts(EMU)
