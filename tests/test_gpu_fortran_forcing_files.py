"""The stand-alone Fortran driver (extpom_amd/fortran/pom_gpu_main) with file forcing and no PnetCDF: given
<wrk_pth>in/<netcdf_file>.sfrc.nc and .lbry.nc it leaves the bits the Python file path leaves after the same steps (and the oracle fed
the records tests/forcing_expect.py restates); without the files it prints and computes what it did before."""
import os
import subprocess

import numpy as np
import pytest

import forcing_expect as fx
import forcing_files_checks as chk
from extpom_amd.layout import BLK2D, BLK3D
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "extpom_amd", "fortran")
FLANG = "/opt/rocm/lib/llvm/bin/flang"
STEPS = 32                                                    # dti = 360 s: lateral_bc changes record at 10, 20, 30, the surface fields at 30

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(FLANG), reason="AMD flang not installed")]


def _build():
    import __graft_entry__ as ge
    ge.build_hip()
    subprocess.check_call(["make", "-C", FDIR, "IM=65", "JM=49", "KB=21"], stdout=subprocess.DEVNULL)


def _drive(tmp, a, nsteps, nml_extra=""):
    with open(tmp / "state.in", "wb") as f:
        np.array([a.im, a.jm, -1, -1, -1, -1, nsteps, len(a.restore_records), a.bdry.size], dtype="<i4").tofile(f)
        for blk in (a.blk1d, a.blk2d, a.blk3d, a.bdry):
            blk.tofile(f)
        f.write(a.con.tobytes())
        for tr, sr in a.restore_records:
            np.ascontiguousarray(tr).tofile(f)
            np.ascontiguousarray(sr).tofile(f)
    (tmp / "pom.nml").write_text("&pom_nml\n title = 'forced'\n netcdf_file = 'arch'\n" + nml_extra + " mode = 3\n nadv = 2\n"
                                 " nitera = 1\n sw = 0.5\n npg = 1\n dte = 6.\n isplit = 60\n days = 1\n/\n")
    r = subprocess.run([os.path.join(FDIR, "pom_gpu_main"), "state.in", "state.out"], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(tmp / "state.out", dtype="<f8")
    n2, n3 = a.blk2d.size, a.blk3d.size
    return r.stdout, raw[:n2].reshape(a.blk2d.shape), raw[n2:n2 + n3].reshape(a.blk3d.shape)


def _bad(st, b2, b3, skip=chk.SCRATCH):
    return ([n for i, n in enumerate(BLK2D) if n not in skip and not chk.same_bits(st.blk2d[i], b2[i])]
            + [n for i, n in enumerate(BLK3D) if n not in skip and not chk.same_bits(st.blk3d[i], b3[i])])


def test_driver_with_forcing_files_equals_the_python_file_path(tmp_path):
    _build()
    a, raw_s, raw_l = chk.start("archipelago", chk.BASE, STEPS)
    b = a.copy()
    os.mkdir(tmp_path / "in")
    sfrc = fx.write_sfrc(tmp_path / "in" / "arch.sfrc.nc", raw_s, dtype="f")
    lbry = fx.write_lbry(tmp_path / "in" / "arch.lbry.nc", raw_l, version=1)
    out, b2, b3 = _drive(tmp_path, a, STEPS, nml_extra=f" wrk_pth = '{tmp_path}/'\n")
    assert "error_status   0" in out, out
    g = PomGpu(b)
    g.set_forcing_files(sfrc=sfrc, lbry=lbry)
    g.run(STEPS)
    g.download()
    g.close()
    assert not _bad(b, b2, b3, skip=()), _bad(b, b2, b3, skip=())
    OracleTile(a).run(STEPS)
    assert not _bad(a, b2, b3), _bad(a, b2, b3)
    assert not chk.same_bits(a.wusurff, a.wusurfb)            # the forcing did run


def test_driver_without_the_files_prints_and_computes_what_it_did(tmp_path):
    _build()
    a, _, _ = chk.start("archipelago", chk.BASE, 1)
    del a.forcing_records, a.lateral_records                  # constant forcing
    out, b2, b3 = _drive(tmp_path, a, 5)
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 2 and lines[0].startswith("domain_stats:") and lines[1].split() == ["pom_gpu_main:", "steps", "5", "error_status", "0"], out
    OracleTile(a).run(5)
    assert not _bad(a, b2, b3), _bad(a, b2, b3)
