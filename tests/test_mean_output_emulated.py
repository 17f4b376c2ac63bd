"""The time-mean output on the host build of the unmodified kernel sources (tests/emu): the checks of tests/mean_output_checks.py -- the
accumulators against a numpy restatement fed by a twin context, bit for bit; the mean file against the snapshot file; launch counts
from the library's own event profile; the 2x2 wide-halo tiles under both timings of the side stream."""
import os
import subprocess

import pytest

import mean_output_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
EMU_F32 = os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so")


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("case,size,how", chk.MATRIX, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_every_field_equals_the_restatement(case, size, how):
    """all nine fields on every cell of (im, jm) after 7 steps and, through the switch, after 3 more; the state is the mean-off run's"""
    chk.every_field(EMU, case, size, how)


def test_every_field_with_file_forcing(tmp_path):
    """steps that fetch forcing records lie inside both intervals"""
    chk.every_field(EMU, "archipelago", (20, 17, 6), "run", tmp=tmp_path, forcing=True)


@pytest.mark.parametrize("chained", [False, True], ids=["io_wait", "run_right_after_the_write"])
def test_mean_file_matches_snapshot_file_and_restatement(tmp_path, chained):
    chk.mean_file(EMU, tmp_path, chained)


def test_laziness_is_kept():
    """run(5) with the mean on launches what run(5) launches with it off, and k_mean_accum five times"""
    chk.launch_counts(EMU)


def test_switching_on_a_live_context():
    chk.switching(EMU)


def test_refusals_leave_state_and_count(tmp_path):
    chk.refusals(EMU, tmp_path)


def test_refused_in_the_fp32_storage_build():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), "f32"], stdout=subprocess.DEVNULL)
    chk.refused_in_fp32_storage(EMU_F32)


@pytest.mark.parametrize("size", chk.SIZES + [(11, 7, 5)], ids=lambda s: "x".join(map(str, s)))
def test_every_element_of_every_accumulator(size):
    """uploaded random fields accumulated through the entry point: the head element of an 8-byte-aligned array and the tail element of
    an odd-length one, which a model state keeps at zero (11x7x5: n2 and n3 odd, 9x8x5 both even)"""
    chk.every_element(EMU, size)


def test_entry_point_in_the_host_sequence():
    chk.entry_point(EMU)


@pytest.mark.parametrize("timing", ["side stream at once", "side stream as late as possible"])
def test_tiles_mean_equals_the_single_tile(timing, monkeypatch):
    """2x2 tiles of 67x59x11, wide-halo external mode: owned cells, message rounds and state, under both timings of the side stream
    (tests/emu/hip/hip_runtime.h)"""
    if timing.endswith("possible"):
        monkeypatch.setenv("POMGPU_EMU_DEFER_SIDE", "1")
    else:
        monkeypatch.delenv("POMGPU_EMU_DEFER_SIDE", raising=False)
    chk.tiles(EMU)
