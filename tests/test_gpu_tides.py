"""Tides on an MI355X: the checks of tests/tide_checks.py with the product library against tests/tide_expect.py -- the device's own
arithmetic in bcond(2), every external path (the two-substep pass and the one-launch loop included), the phasor table as kernel arguments,
256 lanes a block in the analysis."""
import os
import subprocess
import sys

import pytest

import tide_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tide_phasors_equal_the_c_librarys():
    chk.phasors(LIB)


@pytest.mark.parametrize("with_un", [True, False], ids=["un", "el_only"])
@pytest.mark.parametrize("nc", chk.NCS)
@pytest.mark.parametrize("case,size", chk.CASES, ids=[c for c, _ in chk.CASES])
def test_run_with_a_tide_equals_the_oracle(case, size, nc, with_un):
    chk.forcing(LIB, case, size, nc, with_un)


@pytest.mark.parametrize("kw", [dict(lramp=True), dict(time0=0.75), dict(nml=dict(mode=2), path="mode2"), dict(nml=dict(mode=4)), dict(sides=("west", "north")),
                                dict(lramp=True, time0=0.75, nml=dict(mode=4), sides=("east",))],
                         ids=["lramp", "time0", "mode2", "mode4", "two_sides", "all_at_once"])
def test_run_with_a_tide_ramp_time0_modes(kw):
    chk.forcing(LIB, "island", (20, 17, 6), 2, True, **kw)


@pytest.mark.parametrize("case,size", [chk.CASES[0], chk.CASES[2]], ids=["island", "seamount"])
@pytest.mark.parametrize("path", list(chk.PATHS))
def test_every_external_path_carries_the_tide(path, case, size):
    if path == "mode2":
        chk.forcing(LIB, case, size, 2, True, nml=dict(mode=2), path=path)
    else:
        chk.forcing(LIB, case, size, 2, True, path=path)


def test_the_pair_path_is_left_out_below_sixteen_cells():
    """archipelago 8 x 8: the two-substep pass does not take tiles under 16 cells a side; the one-substep kernel carries the tide there"""
    chk.forcing(LIB, "archipelago", (8, 8, 6), 2, True, path="pair", excluded=True)


def test_the_tide_changes_the_flow():
    chk.tide_matters(LIB)


def test_routine_by_routine_host_gets_the_tide():
    chk.stand_alone(LIB)


def test_four_tiles_equal_one_with_the_tide():
    """in a process of its own: four contexts on one GPU, one host thread and one stream each, the event-ordered mover (torch first)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tide_tiles.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TIDE TILES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_no_table_is_a_context_that_never_heard_of_tides():
    chk.off_means_off(LIB)


def test_zero_coefficients_are_no_tide_and_one_launch_a_step():
    chk.zero_tide_is_no_tide(LIB)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("steps", [1, 2, 7])
def test_harmonic_sums_and_matrix_bit_for_bit(steps, every):
    chk.harmonic_sums(LIB, steps, every)


def test_harmonic_sums_eight_constituents_more_than_one_block():
    chk.harmonic_sums(LIB, 3, 1, nc=8, case="seamount", size=(65, 49, 21))


def test_harmonic_solve_against_numpy():
    chk.harmonic_solve(LIB)


def test_closed_form_signal_comes_back_with_its_phase():
    chk.closed_form(LIB)


def test_harmonic_launch_counts():
    chk.harmonic_launches(LIB)


def test_refusals_change_nothing():
    chk.refusals(LIB)


# ---- 6: files ------------------------------------------------------------------------------------------------------------------------------------
def test_harmonics_file_matches_its_schema_and_the_solve(tmp_path):
    chk.harmonics_file(LIB, tmp_path)


def test_tide_file_equals_set_tides(tmp_path):
    chk.tide_file(LIB, tmp_path)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_refuse(variant):
    from extpom_amd import lib as L
    chk.fp32_builds_refuse({"f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant])


FDIR = os.path.join(ROOT, "extpom_amd", "fortran")
FLANG = "/opt/rocm/lib/llvm/bin/flang"


@pytest.mark.skipif(not os.path.exists(FLANG), reason="AMD flang not installed")
def test_fortran_driver_runs_tides_and_harmonics(tmp_path):
    """pom_gpu_main --cold ... --tides --harmonics 2 over eight steps (four samples for the three unknowns of one constituent) with in/arch.tide.nc: its harmonics file holds, variable by variable and bit
    for bit, the Python host's of the same run (set_tide_file, set_harmonic_analysis(every=2)); its state differs from the run without --tides"""
    import numpy as np
    import cold_start_checks as C
    import cold_start_expect as E
    import tide_expect as X
    import __graft_entry__ as ge
    from scipy.io import netcdf_file
    ge.build_hip()
    subprocess.check_call(["make", "-C", FDIR, "IM=65", "JM=49", "KB=21"], stdout=subprocess.DEVNULL)
    size = (65, 49, 21)
    nml = dict(dte=6.0, isplit=60, days=1.0, ramp=0.0)
    os.mkdir(tmp_path / "in")
    os.mkdir(tmp_path / "out")
    paths = E.write_files(tmp_path / "in", E.case_fields(C.CASE, *size, **nml), stem="arch")
    (tmp_path / "pom.nml").write_text(f"&pom_nml\n title = 'tides'\n netcdf_file = 'arch'\n wrk_pth = '{tmp_path}/'\n mode = 3\n nadv = 2\n nitera = 1\n sw = 0.5\n"
                                      " npg = 1\n dte = 6.\n isplit = 60\n days = 1\n nread_rst = 0\n prtd1 = 1\n prtd2 = 1\n/\n")
    nc = 1
    chk.write_tide_file(tmp_path / "in" / "arch.tide.nc", X.OMEGA[:nc], X.make_lines(nc, size[0], size[1]))
    exe = os.path.join(FDIR, "pom_gpu_main")
    r = subprocess.run([exe, "--cold", "state.out", "8", "--tides", "--harmonics", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout and "arch.tide.nc" in r.stdout and "arch.harmonics.nc" in r.stdout, r.stdout + r.stderr
    g, b, _ = C.cold(None, paths, C.one_tile(size[0], size[1]), size[2], nml)
    g.set_forcing_files(clim=paths[2])                        # as the driver does with the clim file it finds
    g.set_tide_file(tmp_path / "in" / "arch.tide.nc")
    g.set_harmonic_analysis(True, every=2)
    g.run(8)
    assert g.harmonic_count() == 4
    mine = str(tmp_path / "mine.harmonics.nc")
    g.write_file("harmonics", mine, title="tides")
    g.io_wait()
    g.close()
    chk.KW = dict(chk.KW, title="tides")
    chk.check_harmonics_header(tmp_path / "out" / "arch.harmonics.nc", nc, size[0], size[1])
    with netcdf_file(mine, "r", mmap=False) as fa, netcdf_file(str(tmp_path / "out" / "arch.harmonics.nc"), "r", mmap=False) as fb:
        for k in fa.variables:
            x, y = np.array(fa.variables[k].data, dtype=np.float64), np.array(fb.variables[k].data, dtype=np.float64)
            assert chk.same_bits(np.atleast_1d(x), np.atleast_1d(y)), k
        assert float(fb.variables["count"].data) == 4.0 and np.any(np.array(fb.variables["elb_amp"].data) > 0.0)
    with_tide = open(tmp_path / "state.out", "rb").read()
    r = subprocess.run([exe, "--cold", "state.out", "8"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout, r.stdout + r.stderr
    assert open(tmp_path / "state.out", "rb").read() != with_tide
