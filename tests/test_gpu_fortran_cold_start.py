"""The stand-alone Fortran driver (extpom_amd/fortran/pom_gpu_main) started cold: `pom_gpu_main --cold <state.out> <nsteps>` takes no
state dump -- read_input's constants, pom.nml, then cold_start_files on <wrk_pth>in/<netcdf_file>.grid.nc, .init.nc, .clim.nc.  With no
step it leaves the expectation of tests/cold_start_expect.py; after four steps the bits PomGpu.cold_start and the same steps leave."""
import os
import subprocess

import numpy as np
import pytest

import cold_start_checks as C
import cold_start_expect as E
from extpom_amd.layout import BLK2D, BLK3D
from extpom_amd.model import PomGpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "extpom_amd", "fortran")
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SIZE = (65, 49, 21)
NML = dict(dte=6.0, isplit=60, days=1.0, ramp=0.0)      # ramp: the driver leaves it as the reference's COMMON holds it at initialize, zero

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(FLANG), reason="AMD flang not installed")]


def _drive(tmp, nsteps, shape2, shape3):
    (tmp / "pom.nml").write_text(f"&pom_nml\n title = 'cold'\n netcdf_file = 'arch'\n wrk_pth = '{tmp}/'\n mode = 3\n nadv = 2\n nitera = 1\n sw = 0.5\n"
                                 " npg = 1\n dte = 6.\n isplit = 60\n days = 1\n nread_rst = 0\n/\n")
    r = subprocess.run([os.path.join(FDIR, "pom_gpu_main"), "--cold", "state.out", str(nsteps)], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(tmp / "state.out", dtype="<f8")
    n2, n3 = int(np.prod(shape2)), int(np.prod(shape3))
    return r.stdout, raw[:n2].reshape(shape2), raw[n2:n2 + n3].reshape(shape3)


def _bad(st, b2, b3, skip=E.SCRATCH):
    return ([n for i, n in enumerate(BLK2D) if n not in skip and not E.same_bits(st.blk2d[i], b2[i])]
            + [n for i, n in enumerate(BLK3D) if n not in skip and not E.same_bits(st.blk3d[i], b3[i])])


def test_driver_started_cold_equals_the_expectation_and_the_python_path(tmp_path):
    import __graft_entry__ as ge
    ge.build_hip()
    subprocess.check_call(["make", "-C", FDIR, "IM=65", "JM=49", "KB=21"], stdout=subprocess.DEVNULL)
    im, jm, kb = SIZE
    os.mkdir(tmp_path / "in")
    f = E.case_fields(C.CASE, *SIZE, **NML)
    E.assert_case_is_demanding(f, kb, [C.one_tile(im, jm)])
    paths = E.write_files(tmp_path / "in", f, stem="arch")
    tile = C.one_tile(im, jm)
    a, _ = E.expected_state(paths, tile, kb, **NML)
    out, b2, b3 = _drive(tmp_path, 0, a.blk2d.shape, a.blk3d.shape)
    assert out.count("reading file") == 3, out
    assert not _bad(a, b2, b3), _bad(a, b2, b3)               # no step: the state initialize leaves
    out, b2, b3 = _drive(tmp_path, 4, a.blk2d.shape, a.blk3d.shape)
    g, b, _ = C.cold(None, paths, tile, kb, NML)
    g.set_forcing_files(clim=paths[2])                        # the driver hands the library the clim file it finds (restore_interior)
    g.run(4)
    g.download()
    g.close()
    assert b.u.any() and b.drhox.any() and not a.drhox.any() and not _bad(b, b2, b3, skip=()), _bad(b, b2, b3, skip=())
