"""The stand-alone Fortran driver with a z-level lateral file: `pom_gpu_main --cold-z <state.out> <nsteps> --lbry-z` sets pom_lbry_on_z,
which pomgpu_open_forcing_files passes on (pomgpu_set_z_lateral) before it names <wrk_pth>in/<netcdf_file>.lbry.nc.  After four steps it
leaves the bits PomGpu.set_z_inputs(init, clim, lbry) + cold_start + set_forcing_files and the same steps leave; without the option the
library refuses the file for its level count and the driver reports it."""
import os
import subprocess

import numpy as np
import pytest

import cold_start_expect as E
import ztosig_files_checks as F
import ztosig_line_files_checks as L
from extpom_amd.layout import BLK2D, BLK3D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "extpom_amd", "fortran")
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SIZE = (65, 49, 21)
NML = dict(dte=6.0, isplit=60, days=1.0, ramp=0.0)      # ramp: the driver leaves it as the reference's COMMON holds it at initialize, zero

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(FLANG), reason="AMD flang not installed")]


def _drive(tmp, nsteps, *more):
    (tmp / "pom.nml").write_text(f"&pom_nml\n title = 'cold'\n netcdf_file = 'case'\n wrk_pth = '{tmp}/'\n mode = 3\n nadv = 2\n nitera = 1\n sw = 0.5\n"
                                 " npg = 1\n dte = 6.\n isplit = 60\n days = 1\n nread_rst = 0\n/\n")
    return subprocess.run([os.path.join(FDIR, "pom_gpu_main"), "--cold-z", "state.out", str(nsteps), *more], cwd=tmp, capture_output=True, text=True, timeout=300)


def _bad(st, b2, b3):
    return ([n for i, n in enumerate(BLK2D) if not E.same_bits(st.blk2d[i], b2[i])] + [n for i, n in enumerate(BLK3D) if not E.same_bits(st.blk3d[i], b3[i])])


def test_driver_with_a_z_level_lateral_file_equals_the_python_path(tmp_path):
    import __graft_entry__ as ge
    ge.build_hip()
    subprocess.check_call(["make", "-C", FDIR, "IM=65", "JM=49", "KB=21"], stdout=subprocess.DEVNULL)
    im, jm, kb = SIZE
    os.mkdir(tmp_path / "in")
    f, paths = F.z_inputs(tmp_path / "in", SIZE, nml=NML)
    tile = F.one_tile(im, jm)
    a, _ = F.expected_state_z(paths, tile, kb, True, True, **NML)
    raw_l = L.raw_lbry_z(a, 2)
    lbry = L.write_lbry_z(tmp_path / "in" / "case.lbry.nc", raw_l)
    r = _drive(tmp_path, 4, "--lbry-z")
    assert r.returncode == 0 and "error_status   0" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(tmp_path / "state.out", dtype="<f8")
    n2, n3 = a.blk2d.size, a.blk3d.size
    b2, b3 = raw[:n2].reshape(a.blk2d.shape), raw[n2:n2 + n3].reshape(a.blk3d.shape)
    g, b, _ = F.cold(None, paths, tile, kb, True, True, NML)
    g.set_z_inputs(init=True, clim=True, lbry=True)
    g.set_forcing_files(lbry=lbry, clim=paths[2])             # the driver hands the library the files it finds
    g.run(4)
    g.download()
    g.close()
    assert b.u.any() and int(b.error_status) == 0 and not _bad(b, b2, b3), _bad(b, b2, b3)
    # the mapped lines have reached the state: the same steps without the lateral file leave other bits
    g, c, _ = F.cold(None, paths, tile, kb, True, True, NML)
    g.set_forcing_files(clim=paths[2])
    g.run(4)
    g.download()
    g.close()
    assert _bad(c, b2, b3)
    r = _drive(tmp_path, 1)                                   # without the option: a sigma-level file is expected
    assert "variable temp.east has the dimension lengths (unlimited, 7, 49), wanted (records, 21, 49)" in r.stdout + r.stderr, r.stdout + r.stderr
