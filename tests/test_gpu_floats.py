"""Lagrangian floats on an MI355X: the checks of tests/float_checks.py with the product library against tests/float_expect.py, bit for
bit -- the device's own fp64 division, floor and fmin / fmax, 256 lanes a block and the gathers.  The not-finite cases are checked on the
host build alone (tests/test_floats_emulated.py): their result is defined and the source is the same."""
import os
import subprocess

import pytest

import float_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)


@pytest.mark.parametrize("speed", list(chk.SPEEDS))
@pytest.mark.parametrize("size", chk.SIZES, ids=str)
@pytest.mark.parametrize("case", chk.CASES)
def test_float_step_against_the_expectation(case, size, speed):
    chk.step_alone(LIB, case, size, speed, need_branches=size == chk.SIZES[0])


@pytest.mark.parametrize("n", chk.COUNTS)
def test_float_counts_at_the_wave_block_and_grid_edges(n):
    chk.counts(LIB, n)


def test_zero_flow_moves_nobody():
    chk.zero_flow(LIB)


def test_uniform_flow_is_exact():
    chk.uniform_flow(LIB)


def test_solid_body_rotation_in_closed_form():
    chk.solid_body(LIB)


def test_permuting_the_floats_permutes_the_result():
    chk.permutation(LIB)


def test_one_float_alone_equals_itself_among_70001():
    chk.one_among_many(LIB)


def test_two_contexts_give_the_same_bits():
    chk.two_contexts(LIB)


@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("case", chk.CASES)
def test_run_equals_step_download_expectation(case, mode):
    chk.in_step(LIB, case, mode)


def test_floats_do_not_touch_the_flow():
    chk.no_interference(LIB)


def test_launch_counts():
    chk.launch_counts(LIB)


def test_mode_2_floats_rest():
    chk.mode_2_rests(LIB)


def test_no_active_float_on_land_after_20_steps():
    chk.never_on_land(LIB)


def test_file_shows_the_floats_and_matches_the_schema(tmp_path):
    chk.file_shows_the_floats(LIB, tmp_path)


def test_checkpoint_continues_the_run(tmp_path):
    chk.checkpoint(LIB, tmp_path)


def test_initial_file_with_positions_alone(tmp_path):
    chk.initial_file(LIB, tmp_path)


def test_file_refusals_change_nothing(tmp_path):
    chk.file_refusals(LIB, tmp_path)


def test_refusals():
    chk.refusals(LIB)


def test_a_tile_refuses_floats():
    chk.tile_refuses(LIB)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_refuse(variant):
    from extpom_amd import lib as L
    chk.fp32_builds_refuse({"f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant])


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "extpom_amd", "fortran")
FLANG = "/opt/rocm/lib/llvm/bin/flang"


@pytest.mark.skipif(not os.path.exists(FLANG), reason="AMD flang not installed")
def test_fortran_driver_moves_and_writes_the_floats(tmp_path):
    """pom_gpu_main --cold ... --floats --mean over two output intervals of three steps, in/arch.floats.nc an initial file any tool can
    write: its two float files and arch.floats.rst.nc hold the Python host's floats and samples of the same run; without --floats the
    driver's files are the same bytes and no float file appears"""
    import numpy as np
    import cold_start_checks as C
    import cold_start_expect as E
    import float_expect as X
    import __graft_entry__ as ge
    from scipy.io import netcdf_file
    ge.build_hip()
    subprocess.check_call(["make", "-C", FDIR, "IM=65", "JM=49", "KB=21"], stdout=subprocess.DEVNULL)
    size = (65, 49, 21)
    nml = dict(dte=6.0, isplit=60, days=1.0, ramp=0.0)
    os.mkdir(tmp_path / "in")
    os.mkdir(tmp_path / "out")
    paths = E.write_files(tmp_path / "in", E.case_fields(C.CASE, *size, **nml), stem="arch")
    (tmp_path / "pom.nml").write_text(f"&pom_nml\n title = 'floats'\n netcdf_file = 'arch'\n wrk_pth = '{tmp_path}/'\n mode = 3\n nadv = 2\n nitera = 1\n sw = 0.5\n"
                                      " npg = 1\n dte = 6.\n isplit = 60\n days = 1\n nread_rst = 0\n prtd1 = 0.0125\n prtd2 = 0.0125\n/\n")   # iprint = 3
    g, b, _ = C.cold(None, paths, C.one_tile(size[0], size[1]), size[2], nml)
    g.set_forcing_files(clim=paths[2])                        # as the driver does with the clim file it finds
    x, y, s, kind, ids = chk.seeds(b)
    chk.hand_file(tmp_path / "in" / "arch.floats.nc", dict(x=x, y=y, sig=s, kind=kind, id=ids))
    exe = os.path.join(FDIR, "pom_gpu_main")
    r = subprocess.run([exe, "--cold", "state.out", "6", "--floats", "--mean"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout and r.stdout.count("writing file") == 5 and "arch.floats.nc" in r.stdout, r.stdout + r.stderr
    g.read_floats(tmp_path / "in" / "arch.floats.nc")

    def same(name):
        chk.check_header(tmp_path / "out" / name, x.size, title="floats", time_start="")
        F, S = g.floats(), g.float_sample()
        with netcdf_file(str(tmp_path / "out" / name), "r", mmap=False) as f:
            for k in chk.KEYS:
                assert np.array_equal(chk.bits(np.array(f.variables[k].data, dtype=F[k].dtype)), chk.bits(F[k])), (name, k)
            for k in X.SAMPLES:
                assert np.array_equal(chk.bits(np.array(f.variables[k].data, dtype=np.float64)), chk.bits(S[k])), (name, k)
        return F

    g.run(3)
    F1 = same("arch.floats.0001.nc")
    g.run(3)
    F2 = same("arch.floats.0002.nc")
    same("arch.floats.rst.nc")
    assert not np.array_equal(F1["x"], F2["x"]) and (F2["status"] == X.ACTIVE).any()
    g.close()
    keep = {n: open(tmp_path / n, "rb").read() for n in ("state.out", "out/arch.0001.nc", "out/arch.0002.nc")}
    for n in os.listdir(tmp_path / "out"):
        os.remove(tmp_path / "out" / n)
    r = subprocess.run([exe, "--cold", "state.out", "6", "--mean"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout and r.stdout.count("writing file") == 2, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "out")) == ["arch.0001.nc", "arch.0002.nc"]
    assert all(open(tmp_path / n, "rb").read() == v for n, v in keep.items())
