"""The stand-alone Fortran driver (extpom_amd/fortran/pom_gpu_main) started cold with water files present:
<wrk_pth>in/<netcdf_file>.water.0000.nc makes pomgpu_open_forcing_files register them (no flag), and `water` runs in the reference's
position; `--sss` makes `surface` set ssurf from the sfrc file's SSS.  After three steps the driver leaves the bits PomGpu.cold_start, the
same registrations and the same steps leave (compared as tests/test_gpu_fortran_forcing_files.py compares)."""
import os
import subprocess

import numpy as np
import pytest

import cold_start_checks as C
import cold_start_expect as E
import forcing_expect as fx
import water_expect as wx
from extpom_amd.layout import BLK2D, BLK3D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "extpom_amd", "fortran")
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SIZE = (65, 49, 21)
STEPS = 3

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(FLANG), reason="AMD flang not installed")]


def _drive(tmp, nsteps, shape2, shape3, nbcs, *flags):
    (tmp / "pom.nml").write_text(f"&pom_nml\n title = 'cold'\n netcdf_file = 'arch'\n wrk_pth = '{tmp}/'\n mode = 3\n nadv = 2\n nitera = 1\n sw = 0.5\n"
                                 f" npg = 1\n dte = 6.\n isplit = 60\n days = 1\n nread_rst = 0\n nbcs = {nbcs}\n/\n")
    r = subprocess.run([os.path.join(FDIR, "pom_gpu_main"), "--cold", "state.out", str(nsteps)] + list(flags), cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(tmp / "state.out", dtype="<f8")
    n2, n3 = int(np.prod(shape2)), int(np.prod(shape3))
    return raw[:n2].reshape(shape2), raw[n2:n2 + n3].reshape(shape3)


def _bad(st, b2, b3):
    return ([n for i, n in enumerate(BLK2D) if not E.same_bits(st.blk2d[i], b2[i])]
            + [n for i, n in enumerate(BLK3D) if not E.same_bits(st.blk3d[i], b3[i])])


@pytest.mark.parametrize("sss", [False, True], ids=["water", "water-sfrc-sss"])
def test_cold_driver_with_water_files_equals_the_python_path(tmp_path, sss):
    import __graft_entry__ as ge
    ge.build_hip()
    subprocess.check_call(["make", "-C", FDIR, "IM=65", "JM=49", "KB=21"], stdout=subprocess.DEVNULL)
    im, jm, kb = SIZE
    nml = dict(dte=6.0, isplit=60, days=1.0, ramp=0.0, nbcs=3 if sss else 1)
    os.mkdir(tmp_path / "in")
    paths = E.write_files(tmp_path / "in", E.case_fields(C.CASE, *SIZE, **nml), stem="arch")
    tile = C.one_tile(im, jm)
    g, b, _ = C.cold(None, paths, tile, kb, nml)              # the Python path: the same cold start ...
    g.download()
    prefix = str(tmp_path / "in" / "arch")
    raw = wx.raw_water(b, (0, 1))
    wx.write_all(prefix, raw, dtype="f")
    sfrc = fx.write_sfrc(prefix + ".sfrc.nc", fx.raw_sfrc(b, 2)) if sss else None
    b2, b3 = _drive(tmp_path, STEPS, b.blk2d.shape, b.blk3d.shape, nml["nbcs"], *(["--sss"] if sss else []))
    g.set_forcing_files(sfrc=sfrc, clim=paths[2])             # ... the registrations pomgpu_open_forcing_files makes ...
    g.set_water_files(prefix)
    if sss:
        g.set_surface_sss(True)
    before = b.copy()
    g.run(STEPS)                                              # ... and the same steps
    g.download()
    g.close()
    assert not _bad(b, b2, b3), _bad(b, b2, b3)
    assert E.same_bits(b.wssurfb[:jm, :im], raw[0]) and E.same_bits(b.wssurff[:jm, :im], raw[1]) and b.wssurf.any()
    if sss:
        assert not E.same_bits(b.ssurf, before.ssurf) and b.wusurf.any()
