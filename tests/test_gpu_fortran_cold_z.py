"""The stand-alone Fortran driver started cold from z-level files: `pom_gpu_main --cold-z <state.out> <nsteps>` sets pom_init_on_z and
pom_clim_on_z, which cold_start_files and pomgpu_open_forcing_files pass on (pomgpu_set_z_inputs).  With no step it leaves the
expectation of tests/ztosig_files_checks.py; after four steps the bits PomGpu.set_z_inputs + cold_start and the same steps leave, the
months of restore_interior mapped from the z-level clim file on either path."""
import os
import subprocess

import numpy as np
import pytest

import cold_start_expect as E
import ztosig_files_checks as F
from extpom_amd.layout import BLK2D, BLK3D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "extpom_amd", "fortran")
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SIZE = (65, 49, 21)
NML = dict(dte=6.0, isplit=60, days=1.0, ramp=0.0)      # ramp: the driver leaves it as the reference's COMMON holds it at initialize, zero

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(FLANG), reason="AMD flang not installed")]


def _drive(tmp, nsteps, shape2, shape3):
    (tmp / "pom.nml").write_text(f"&pom_nml\n title = 'cold'\n netcdf_file = 'case'\n wrk_pth = '{tmp}/'\n mode = 3\n nadv = 2\n nitera = 1\n sw = 0.5\n"
                                 " npg = 1\n dte = 6.\n isplit = 60\n days = 1\n nread_rst = 0\n/\n")
    r = subprocess.run([os.path.join(FDIR, "pom_gpu_main"), "--cold-z", "state.out", str(nsteps)], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout, r.stdout + r.stderr
    raw = np.fromfile(tmp / "state.out", dtype="<f8")
    n2, n3 = int(np.prod(shape2)), int(np.prod(shape3))
    return raw[:n2].reshape(shape2), raw[n2:n2 + n3].reshape(shape3)


def _bad(st, b2, b3, skip=E.SCRATCH):
    return ([n for i, n in enumerate(BLK2D) if n not in skip and not E.same_bits(st.blk2d[i], b2[i])]
            + [n for i, n in enumerate(BLK3D) if n not in skip and not E.same_bits(st.blk3d[i], b3[i])])


def test_driver_started_cold_from_z_level_files_equals_the_python_path(tmp_path):
    import __graft_entry__ as ge
    ge.build_hip()
    subprocess.check_call(["make", "-C", FDIR, "IM=65", "JM=49", "KB=21"], stdout=subprocess.DEVNULL)
    im, jm, kb = SIZE
    os.mkdir(tmp_path / "in")
    f, paths = F.z_inputs(tmp_path / "in", SIZE, nml=NML)
    tile = F.one_tile(im, jm)
    a, _ = F.expected_state_z(paths, tile, kb, True, True, **NML)
    b2, b3 = _drive(tmp_path, 0, a.blk2d.shape, a.blk3d.shape)
    assert not _bad(a, b2, b3), _bad(a, b2, b3)               # no step: the state initialize leaves
    b2, b3 = _drive(tmp_path, 4, a.blk2d.shape, a.blk3d.shape)
    g, b, _ = F.cold(None, paths, tile, kb, True, True, NML)
    g.set_forcing_files(clim=paths[2])                        # the driver hands the library the clim file it finds (restore_interior)
    g.run(4)
    g.download()
    g.close()
    assert b.u.any() and b.tb[kb - 1].any() and not _bad(b, b2, b3, skip=()), _bad(b, b2, b3, skip=())
