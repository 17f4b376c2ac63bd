"""profu / profv fused with the velocity filter, uf and vf on demand, on the host build of the unmodified kernel sources (tests/emu):
the checks of tests/uv_tail_fused_checks.py against the CPU oracle, bit for bit, and the launch counts from the library's own event
profile.  The emulated grid is serial: a bottom friction that read the live ub, vb instead of the snapshot would see every column
already filtered that runs before it, every time."""
import os
import subprocess

import pytest

import uv_tail_fused_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("nml", list(chk.NAMELISTS))
@pytest.mark.parametrize("case", chk.CASES)
def test_unobserved_steps_every_case_and_namelist(case, nml):
    """run(2), run(1), run(3), one download: every array that is not scratch, uf and vf included"""
    chk.unobserved_steps(EMU, case, chk.NAMELISTS[nml], (65, 49, 21))


@pytest.mark.parametrize("size", chk.SIZES_FUSED[1:], ids=str)
def test_unobserved_steps_every_shape(size):
    chk.unobserved_steps(EMU, "archipelago", None, size)


@pytest.mark.parametrize("case", ["seamount", "island"])
def test_unobserved_steps_one_interior_column(case):
    chk.unobserved_steps(EMU, case, None, (8, 8, 6))


@pytest.mark.parametrize("size", chk.SIZES_FALLBACK, ids=str)
def test_unobserved_steps_fallback_shapes(size):
    """no interior (7x9x6), kb above and below the register kernels' range (65, 5: k_advu_profu / k_advv_profv run, and only there): the
    fused kernel does not run, the state is the oracle's"""
    chk.unobserved_steps(EMU, "archipelago", None, size, fused=False)


@pytest.mark.parametrize("name", ["uf", "vf"])
@pytest.mark.parametrize("point", chk.POINTS)
def test_routine_by_routine_uf_vf_read_at_any_point(point, name):
    chk.routine_by_routine(EMU, "archipelago", point, name)


@pytest.mark.parametrize("what", ["u", "uf", "state", "restart", "tune"])
def test_writer_after_unobserved_steps(what, tmp_path):
    chk.writer_after_steps(EMU, what, tmp_path)


def test_address_handed_out_ends_the_fusion():
    chk.address_handed_out(EMU)


def test_switch_flipped_on_a_live_context():
    chk.switch_flipped_live(EMU)


def test_launch_counts():
    """run(5): five fused kernels, five rim filters, no unfused filter, no copy; the download after it: one copy per component"""
    chk.launch_counts(EMU)


def test_fp64_lazy_equals_eager():
    chk.lazy_equals_eager(EMU)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_lazy_equals_eager(variant):
    """the unfused filter reads uf back rounded to the storage type: the fused kernel must round what it keeps in registers"""
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.lazy_equals_eager(VARIANTS[variant])
