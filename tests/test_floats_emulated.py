"""Lagrangian floats on the host build of the unmodified kernel sources (tests/emu): the checks of tests/float_checks.py against
tests/float_expect.py, bit for bit.  The emulation runs one lane at a time; the float kernels have no lane that talks to another, so what
the device adds is its own arithmetic, covered by tests/test_gpu_floats.py.  The not-finite cases run here alone: their result is defined,
the source is the same, and a device run would add nothing.  The tests named pin_* hold the expectation itself and pass without the feature,
by design."""
import os
import subprocess

import numpy as np
import pytest

import float_checks as chk
import float_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


# ---- pins of the expectation ----------------------------------------------------------------------------------------------------------------
def test_pin_L_is_exact_for_equal_ends():
    p = np.array([1.0 / 3.0, -0.0, 1.0e300, 5.0e-324])
    assert np.array_equal(X.L(p, p, np.array([0.3, 0.9, 0.5, 0.7])).view(np.uint64), (p + 0.0).view(np.uint64))


def test_pin_levels_bracket_sigma():
    a, _ = chk.start("seamount", None, (8, 8, 6))
    zz, z = np.asarray(a.zz).ravel(), np.asarray(a.z).ravel()
    sig = np.array([0.0, -0.01, float(zz[0]), -0.3, float(zz[2]), -0.9, float(zz[4]), -0.99, -1.0])
    k, k2, fz, alone = X.levels_zz(a, sig)
    assert alone.tolist() == [True, True, True, False, False, False, True, True, True]
    assert (k[alone] == k2[alone]).all() and set(k[alone].tolist()) == {1, 5}
    for q in np.flatnonzero(~alone):
        assert zz[k[q] - 1] >= sig[q] > zz[k[q]] and k2[q] == k[q] + 1 and 0.0 <= fz[q] < 1.0
    kw, kw2, fw = X.levels_z(a, sig)
    assert kw[0] == 1 and fw[0] == 0.0 and kw[-1] == 5 and fw[-1] == 1.0
    for q in range(sig.size - 1):
        assert z[kw[q] - 1] >= sig[q] > z[kw[q]] and kw2[q] == kw[q] + 1


def test_pin_float_free_run_is_the_oracles():
    """the flow the in-step checks lean on: run(1) four times equals the oracle's four steps"""
    from oracle.pyoracle import OracleTile
    from extpom_amd.model import PomGpu
    a, b = chk.start("archipelago", None, (20, 17, 6))
    OracleTile(a).run(4)
    g = PomGpu(b, libpath=EMU)
    for _ in range(4):
        g.run(1)
    g.download()
    assert not chk.diff(a, b)
    g.close()


# ---- 1: float_step alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speed", list(chk.SPEEDS))
@pytest.mark.parametrize("size", chk.SIZES, ids=str)
@pytest.mark.parametrize("case", chk.CASES)
def test_float_step_against_the_expectation(case, size, speed):
    chk.step_alone(EMU, case, size, speed, need_branches=size == chk.SIZES[0])


@pytest.mark.parametrize("n", chk.COUNTS)
def test_float_counts_at_the_wave_block_and_grid_edges(n):
    chk.counts(EMU, n)


def test_not_finite_fields_and_positions():
    chk.not_finite(EMU)


# ---- 2: without the expectation ---------------------------------------------------------------------------------------------------------------
def test_zero_flow_moves_nobody():
    chk.zero_flow(EMU)


def test_uniform_flow_is_exact():
    chk.uniform_flow(EMU)


def test_solid_body_rotation_in_closed_form():
    chk.solid_body(EMU)


def test_permuting_the_floats_permutes_the_result():
    chk.permutation(EMU)


def test_one_float_alone_equals_itself_among_70001():
    chk.one_among_many(EMU)


def test_two_contexts_give_the_same_bits():
    chk.two_contexts(EMU)


# ---- 3: in the step -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("case", chk.CASES)
def test_run_equals_step_download_expectation(case, mode):
    chk.in_step(EMU, case, mode)


def test_floats_do_not_touch_the_flow():
    chk.no_interference(EMU, size=(20, 17, 6))


def test_launch_counts():
    chk.launch_counts(EMU, size=(20, 17, 6))


def test_mode_2_floats_rest():
    chk.mode_2_rests(EMU)


def test_no_active_float_on_land_after_20_steps():
    chk.never_on_land(EMU, size=(20, 17, 6))


# ---- 4: files ----------------------------------------------------------------------------------------------------------------------------------
def test_file_shows_the_floats_and_matches_the_schema(tmp_path):
    chk.file_shows_the_floats(EMU, tmp_path)


def test_checkpoint_continues_the_run(tmp_path):
    chk.checkpoint(EMU, tmp_path)


def test_initial_file_with_positions_alone(tmp_path):
    chk.initial_file(EMU, tmp_path)


def test_file_refusals_change_nothing(tmp_path):
    chk.file_refusals(EMU, tmp_path)


# ---- 5: hosts ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    chk.refusals(EMU)


def test_a_tile_refuses_floats():
    chk.tile_refuses(EMU)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_refuse(variant):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.fp32_builds_refuse(VARIANTS[variant])
