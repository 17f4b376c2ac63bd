"""The tracers' files, means and inventory on an MI355X: the checks of tests/tracer_files_checks.py with the product library -- the
asynchronous writer, the pinned band reader and its kernel, k_mean_accum's 16-byte form on the tracers' table and the reduction tree of
the inventory, none of which the host emulation has."""
import os
import subprocess
import sys

import pytest

import mean_output_checks as moc
import tracer_files_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "extpom_amd", "fortran")
FLANG = "/opt/rocm/lib/llvm/bin/flang"
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("size,ntr", [((9, 8, 5), 1), ((11, 7, 5), 3), ((20, 17, 6), 8), ((65, 49, 21), 3)], ids=ids)
def test_round_trip_of_every_element(tmp_path, size, ntr):
    chk.round_trip(LIB, tmp_path, size, ntr)


def test_a_file_with_tr_alone_is_an_initial_file(tmp_path):
    chk.initial_file(LIB, tmp_path)


@pytest.mark.parametrize("size,adv", [((20, 17, 6), (2, 1)), ((20, 17, 6), (2, 2)), ((20, 17, 6), (1, 1)), ((65, 49, 21), (2, 1))], ids=ids)
def test_the_file_is_the_state(tmp_path, size, adv):
    """(2, 2) is the case that needs trfNN"""
    chk.file_is_the_state(LIB, tmp_path, "archipelago", size, adv)


def test_output_kind(tmp_path):
    chk.output_kind(LIB, tmp_path)


@pytest.mark.parametrize("chained", [False, True], ids=["io_wait", "run_right_after_the_write"])
def test_mean_file_and_means_equal_the_restatement(tmp_path, chained):
    chk.mean_file(LIB, tmp_path, chained)


def test_the_nine_fields_are_as_without_tracers(tmp_path):
    chk.nine_fields_unchanged(LIB, tmp_path)


def test_allocation_rules_of_the_tracer_accumulators():
    chk.allocation_rules(LIB)


@pytest.mark.parametrize("size", [(11, 7, 5), (9, 8, 5), (65, 49, 21)], ids=ids)
def test_every_element_of_every_tracer_accumulator(size):
    """65x49x21: more than one workgroup per tracer and an odd n3"""
    chk.every_element(LIB, size)


@pytest.mark.parametrize("size,ntr", [((9, 8, 5), 1), ((11, 7, 5), 3), ((20, 17, 6), 8), ((65, 49, 21), 2)], ids=ids)
def test_inventory_equals_the_restatement(size, ntr):
    """65x49x21: thirteen workgroups, so the finishing workgroup adds partials; the others: one workgroup with idle lanes"""
    chk.inventory(LIB, size, ntr)


def test_inventory_masks_the_land():
    chk.inventory(LIB, (20, 17, 6), 2, land_huge=True)


def test_a_decaying_tracer_does_not_gain_inventory():
    chk.decay_does_not_grow(LIB)


def test_refusals_leave_everything_as_it_was(tmp_path):
    chk.refusals(LIB, tmp_path)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_refuse(tmp_path, variant):
    from extpom_amd import lib as L
    chk.fp32_builds_refuse({"f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant], tmp_path)


def test_launch_counts_with_tracers():
    chk.launch_counts(LIB)


def test_launch_counts_without_tracers_are_the_parents():
    moc.launch_counts(LIB)


@pytest.mark.skipif(not os.path.exists(FLANG), reason="AMD flang not installed")
def test_fortran_driver_reads_and_writes_the_tracer_files(tmp_path):
    """pom_gpu_main --cold ... --tracers 2 --mean over two output intervals of three steps, in/arch.tracer.nc written by the Python host:
    its two tracer mean files and arch.tracer.rst.nc hold the Python host's tracer_mean, tr, trb of the same run; without --tracers the
    driver's files are the same bytes and no tracer file appears"""
    import numpy as np
    import cold_start_checks as C
    import cold_start_expect as E
    import __graft_entry__ as ge
    from tracer_checks import independent
    ge.build_hip()
    subprocess.check_call(["make", "-C", FDIR, "IM=65", "JM=49", "KB=21"], stdout=subprocess.DEVNULL)
    size = (65, 49, 21)
    kbm1 = size[2] - 1
    nml = dict(dte=6.0, isplit=60, days=1.0, ramp=0.0)
    os.mkdir(tmp_path / "in")
    os.mkdir(tmp_path / "out")
    paths = E.write_files(tmp_path / "in", E.case_fields(C.CASE, *size, **nml), stem="arch")
    (tmp_path / "pom.nml").write_text(f"&pom_nml\n title = 'tracers'\n netcdf_file = 'arch'\n wrk_pth = '{tmp_path}/'\n mode = 3\n nadv = 2\n nitera = 1\n sw = 0.5\n"
                                      " npg = 1\n dte = 6.\n isplit = 60\n days = 1\n nread_rst = 0\n prtd1 = 0.0125\n prtd2 = 0.0125\n/\n")   # iprint = 3

    def host():
        g, b, _ = C.cold(None, paths, C.one_tile(size[0], size[1]), size[2], nml)
        g.set_forcing_files(clim=paths[2])                    # as the driver does with the clim file it finds
        g.set_tracers(2)
        return g, b

    g, b = host()                                             # the tracers' initial file: trb, tr, nbc and lam of two tracers
    for n in (1, 2):
        t = independent(b, seed=70 + n)
        g.tracer_upload(n, "trb", t["trb"])
        g.tracer_upload(n, "tr", t["tr"])
        g.set_tracer(n, nbc=1 if n == 1 else 3, decay=1.0e-5 * n)
    g.write_file("tracer_restart", tmp_path / "in" / "arch.tracer.nc")
    g.io_wait()
    g.close()
    exe = os.path.join(FDIR, "pom_gpu_main")
    r = subprocess.run([exe, "--cold", "state.out", "6", "--tracers", "2", "--mean"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout and r.stdout.count("writing file") == 5 and "arch.tracer.nc" in r.stdout, r.stdout + r.stderr
    g, b = host()
    g.read_tracers(tmp_path / "in" / "arch.tracer.nc")
    assert g.tracer_get(2) == (3, 2.0e-5)
    for n in (1, 2):
        g.set_mean_output(True)
        g.run(3)
        v = chk.read_file(tmp_path / "out" / f"arch.tracer.{n:04d}.nc")
        chk.check_header(tmp_path / "out" / f"arch.tracer.{n:04d}.nc", "output", 2, b, title="tracers", time_start="")
        for k in (1, 2):
            assert chk.same_bits(v[chk.nn("tr", k)][0], g.tracer_mean(k)[:kbm1]), (n, k)
            assert np.any(v[chk.nn("tr", k)] != 0.)
    v = chk.read_file(tmp_path / "out" / "arch.tracer.rst.nc")
    for k in (1, 2):
        for arr in ("tr", "trb"):
            assert chk.same_bits(v[chk.nn(arr, k)], g.tracer_download(k, arr)), (k, arr)
        assert (v[chk.nn("nbc", k)], v[chk.nn("lam", k)]) == g.tracer_get(k)
    g.close()
    keep = {n: open(tmp_path / n, "rb").read() for n in ("state.out", "out/arch.0001.nc", "out/arch.0002.nc")}
    for n in os.listdir(tmp_path / "out"):
        os.remove(tmp_path / "out" / n)
    r = subprocess.run([exe, "--cold", "state.out", "6", "--mean"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout and r.stdout.count("writing file") == 2, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "out")) == ["arch.0001.nc", "arch.0002.nc"]
    assert all(open(tmp_path / n, "rb").read() == x for n, x in keep.items())


@pytest.mark.parametrize("split", [(1, 2), (2, 2)], ids=str)
def test_tiles_write_one_file_and_read_their_patches(split):
    """thread tiles in a child process (tests/gpu_tracer_files_tiles.py)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tracer_files_tiles.py"), str(split[0]), str(split[1])],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "TRACER FILES TILES OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
