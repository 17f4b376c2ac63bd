"""The restore rate as a field -- pomgpu_set_restore_rate_file / _record, restore_interior's load, k_ts_update<2> and what the library knows
about taurstrb, taurstrf -- through the host builds of the unmodified sources (tests/emu): every index and every operation of the kernels,
bit for bit against tests/restore_rate_expect.py and the reference's recorded ztosig_ output.  The device runs the same checks
(test_gpu_restore_rate.py).  Here too: the restatement against the reference's compiled ztosig_ where it is built, and against the
oracle's restore_interior at a uniform rate."""
import os
import subprocess

import pytest

import restore_rate_checks as C
import restore_rate_expect as R
from oracle.refharness import have_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


# ---- the expectation itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not have_ref(65, 49, 21), reason="reference build not present")
@pytest.mark.parametrize("shape,steep", [(s, False) for s in R.SHAPES] + [(R.SHAPES[-1], True)], ids=str)
def test_restatement_equals_the_references_ztosig_on_the_rate_inputs(shape, steep):
    from test_ztosig_vs_reference import reference_ztosig
    im, jm, ks, kb = shape
    zs, rate, zz, h = R.make_rate(im, jm, ks, kb, steep=steep)
    R.assert_rates_are_demanding(zs, rate, h, natural=im >= 20)
    want, got = reference_ztosig(zs, rate, zz, h), R.mapped(zs, rate, zz, h)
    assert R.same_bits(want, got)
    gold = C.golden(C.golden_key(shape, steep))
    assert R.digest(want) == gold["reference"] and R.digest(rate) == gold["inputs"]["rate"]


def test_restatement_of_restore_interior_equals_the_oracle_at_a_uniform_rate():
    C.restatement_equals_the_oracle_at_a_uniform_rate()


# ---- the library --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind,chunk_kb,layout,nrec", [
    ((8, 8, 2, 6), "d", None, "unlimited", 4), ((8, 8, 5, 6), "f", None, "fixed", 4), ((20, 17, 5, 6), "d", 1, "unlimited", 4),
    ((20, 17, 5, 6), "f", 1, "unlimited", 1), ((20, 17, 5, 6), "d", None, "none", 1), ((20, 17, 5, 6), "f", None, "fixed", 1),
    ((65, 49, 33, 21), "d", 1, "unlimited", 4)], ids=str)
def test_rate_file_equals_the_setter_fed_the_mapped_records(tmp_path, shape, kind, chunk_kb, layout, nrec):
    C.file_equals_setter(EMU, tmp_path, shape, kind=kind, chunk_kb=chunk_kb, layout=layout, nrec=nrec, version=1 if layout == "fixed" else 2)


def test_a_map_that_goes_below_zero_is_the_references(tmp_path):
    C.file_equals_setter(EMU, tmp_path, (65, 49, 33, 21), layout="none", nrec=1, steep=True)


def test_rate_file_beside_t_and_s_from_the_clim_file(tmp_path):
    C.ts_from_the_clim_file(EMU, tmp_path)


def test_tiles_equal_the_global_map_cut_to_their_window(tmp_path):
    C.tiles(EMU, tmp_path)


@pytest.mark.parametrize("case", ["archipelago", "seamount"])
def test_four_steps_after_a_load_equal_the_oracle_in_all_three_forms(tmp_path, case):
    C.steps_after_a_load(EMU, tmp_path, case)


def test_a_rate_mirror_written_from_outside_the_step_is_used():
    C.a_written_mirror_is_used(EMU)


def test_every_new_refusal_leaves_the_state_as_it_was(tmp_path):
    C.refusals(EMU, tmp_path)


def test_without_a_rate_source_restore_interior_is_the_references():
    C.no_rate_source_is_the_reference(EMU)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_round_the_rate_once(tmp_path, variant):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    C.f32_rounds_once(VARIANTS[variant], tmp_path)
