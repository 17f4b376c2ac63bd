"""The Fortran driver (extpom_amd/fortran/pom_gpu_main) with and without <wrk_pth>in/<netcdf_file>.restore_tau_interior.nc: with the file
it registers it beside the forcing files and ends where PomGpu.set_restore_rate_file ends (tests/test_gpu_restore_rate.py holds that path to
the oracle); without it, where the oracle ends, as ever."""
import os
import subprocess

import numpy as np
import pytest

import restore_rate_checks as C
import restore_rate_expect as R
from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial
from test_fortran_host import FDIR, SCRATCH, _build, needs_flang

pytestmark = pytest.mark.gpu
NSTEPS = 5


def _drive(tmp, a):
    with open(tmp / "state.in", "wb") as f:
        np.array([a.im, a.jm, -1, -1, -1, -1, NSTEPS, len(a.restore_records), a.bdry.size], dtype="<i4").tofile(f)
        for blk in (a.blk1d, a.blk2d, a.blk3d, a.bdry):
            blk.tofile(f)
        f.write(a.con.tobytes())
        for tr, sr in a.restore_records:
            np.ascontiguousarray(tr).tofile(f)
            np.ascontiguousarray(sr).tofile(f)
    (tmp / "pom.nml").write_text(f"&pom_nml\n title = 'island'\n netcdf_file = 'case'\n wrk_pth = '{tmp}/'\n mode = 3\n nadv = 2\n"
                                 " nitera = 1\n sw = 0.5\n npg = 1\n dte = 6.\n isplit = 30\n days = 1\n/\n")
    r = subprocess.run([os.path.join(FDIR, "pom_gpu_main"), "state.in", "state.out"], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(tmp / "state.out", dtype="<f8")
    n2, n3 = a.blk2d.size, a.blk3d.size
    return raw[:n2].reshape(a.blk2d.shape), raw[n2:n2 + n3].reshape(a.blk3d.shape)


def _differ(st, b2, b3):
    bad = [n for i, n in enumerate(BLK2D) if n not in SCRATCH and not np.array_equal(st.blk2d[i], b2[i])]
    return bad + [n for i, n in enumerate(BLK3D) if n not in SCRATCH and not np.array_equal(st.blk3d[i], b3[i])]


@needs_flang
def test_fortran_driver_with_and_without_the_rate_file(tmp_path):
    _build()
    a = make_case("island", 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    zs, rate, zz, h = R.make_rate(65, 49, 9, 21, grid=(a.zz, a.h))
    mp = R.mapped(zs, rate, zz, h)
    assert (mp >= 0.0).all() and (mp <= 2.0).all()
    # without the file: the oracle
    (tmp_path / "without").mkdir()
    b2, b3 = _drive(tmp_path / "without", a)
    o = a.copy()
    OracleTile(o).run(NSTEPS)
    assert not _differ(o, b2, b3), _differ(o, b2, b3)
    # with it: the library's own Python path, and not the oracle's uniform rate
    w = tmp_path / "with"
    (w / "in").mkdir(parents=True)
    path = C.write_rate(w / "in" / "case.restore_tau_interior.nc", zs, [rate])
    c2, c3 = _drive(w, a)
    g = PomGpu(a.copy())
    g.set_restore_rate_file(path)
    g.run(NSTEPS)
    g.download()
    g.close()
    assert not _differ(g.st, c2, c3), _differ(g.st, c2, c3)
    assert R.same_bits(g.st.taurstrf[:, :a.jm, :a.im], mp) and "t" in _differ(o, c2, c3)
