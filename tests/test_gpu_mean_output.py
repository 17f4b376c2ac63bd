"""The time-mean output on an MI355X: the checks of tests/mean_output_checks.py with the product library -- the accumulators against the
numpy restatement fed by a twin context, bit for bit; the mean file through the asynchronous writer, also with steps enqueued right
behind the call; launch counts; 2x2 wide-halo tiles as four contexts on one GPU; the Fortran driver with --mean."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mean_output_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "extpom_amd", "fortran")
FLANG = "/opt/rocm/lib/llvm/bin/flang"


@pytest.mark.parametrize("case,size,how", chk.MATRIX, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_every_field_equals_the_restatement(case, size, how):
    chk.every_field(LIB, case, size, how)


def test_every_field_with_file_forcing(tmp_path):
    chk.every_field(LIB, "archipelago", (20, 17, 6), "run", tmp=tmp_path, forcing=True)


@pytest.mark.parametrize("size", [(20, 17, 6), (65, 49, 21)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("chained", [False, True], ids=["io_wait", "run_right_after_the_write"])
def test_mean_file_matches_snapshot_file_and_restatement(tmp_path, chained, size):
    chk.mean_file(LIB, tmp_path, chained, size=size)


def test_laziness_is_kept():
    chk.launch_counts(LIB)


def test_switching_on_a_live_context():
    chk.switching(LIB)


def test_refusals_leave_state_and_count(tmp_path):
    chk.refusals(LIB, tmp_path)


def test_refused_in_the_fp32_storage_build():
    from extpom_amd import lib as L
    chk.refused_in_fp32_storage(L.LIBPATH_F32)


@pytest.mark.parametrize("size", chk.SIZES + [(11, 7, 5)], ids=lambda s: "x".join(map(str, s)))
def test_every_element_of_every_accumulator(size):
    """uploaded random fields accumulated through the entry point: the head element of an 8-byte-aligned array and the tail element of
    an odd-length one, which a model state keeps at zero (11x7x5: n2 and n3 odd, 9x8x5 both even)"""
    chk.every_element(LIB, size)


def test_entry_point_in_the_host_sequence():
    chk.entry_point(LIB)


def test_tiles_mean_equals_the_single_tile():
    """in a process of its own: the mover between the four contexts needs torch, imported before the library"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_mean_output_tiles.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "MEAN-OUTPUT-TILES-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.skipif(not os.path.exists(FLANG), reason="AMD flang not installed")
def test_fortran_driver_writes_the_mean_files(tmp_path):
    """pom_gpu_main --cold ... --mean over two output intervals of three steps: the nine variables of its two files are the Python
    host's means of the same run"""
    import cold_start_checks as C
    import cold_start_expect as E
    import __graft_entry__ as ge
    from scipy.io import netcdf_file
    ge.build_hip()
    subprocess.check_call(["make", "-C", FDIR, "IM=65", "JM=49", "KB=21"], stdout=subprocess.DEVNULL)
    size = (65, 49, 21)
    nml = dict(dte=6.0, isplit=60, days=1.0, ramp=0.0)
    os.mkdir(tmp_path / "in")
    os.mkdir(tmp_path / "out")
    paths = E.write_files(tmp_path / "in", E.case_fields(C.CASE, *size, **nml), stem="arch")
    (tmp_path / "pom.nml").write_text(f"&pom_nml\n title = 'mean'\n netcdf_file = 'arch'\n wrk_pth = '{tmp_path}/'\n mode = 3\n nadv = 2\n nitera = 1\n sw = 0.5\n"
                                      " npg = 1\n dte = 6.\n isplit = 60\n days = 1\n nread_rst = 0\n prtd1 = 0.0125\n prtd2 = 0.0125\n/\n")   # iprint = 3
    r = subprocess.run([os.path.join(FDIR, "pom_gpu_main"), "--cold", "state.out", "6", "--mean"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout and r.stdout.count("writing file") == 2, r.stdout + r.stderr
    g, b, _ = C.cold(None, paths, C.one_tile(size[0], size[1]), size[2], nml)
    g.set_forcing_files(clim=paths[2])                        # as the driver does with the clim file it finds
    for n in (1, 2):
        g.set_mean_output(True)
        g.run(3)
        with netcdf_file(str(tmp_path / "out" / f"arch.{n:04d}.nc"), "r", mmap=False) as f:
            for k in chk.FIELDS:
                v = np.array(f.variables[k].data, dtype=np.float64)[0]
                m = g.mean(k)
                assert chk.same_bits(v, m if v.ndim == 2 else m[:v.shape[0]]), (n, k)
            assert np.any(f.variables["u"].data != 0.)
    g.close()
