"""The stand-alone Fortran driver with a four-sided lateral file: `pom_gpu_main --cold-z <state.out> <nsteps> --lbry-sides 15` sets
pom_lbry_sides, which pomgpu_open_forcing_files passes on (pomgpu_set_lateral_sides) before it names <wrk_pth>in/<netcdf_file>.lbry.nc.
After four steps it leaves the bits the CPU oracle leaves when fed tests/lateral_sides_expect.py's records; once more with --lbry-z (the
option may stand before or after --lbry-sides) and temp / salt of all four sides on z levels.  Without the option the same file feeds east
and south alone, which leaves other bits."""
import os
import subprocess

import numpy as np
import pytest

import cold_start_expect as E
import forcing_files_checks as ffc
import lateral_sides_expect as LS
import ztosig_files_checks as F
from extpom_amd.layout import BLK2D, BLK3D
from oracle.pyoracle import OracleTile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "extpom_amd", "fortran")
FLANG = "/opt/rocm/lib/llvm/bin/flang"
SIZE = (65, 49, 21)
# ramp: the driver leaves it as the reference's COMMON holds it at initialize, zero.  isplit = 30 (dti = 180 s), as in the cold-start check of
# tests/ztosig_line_files_checks.py: at 360 s the state these z-level fields start is not stable and the oracle and the library part ways
NML = dict(dte=6.0, isplit=30, days=1.0, ramp=0.0)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(FLANG), reason="AMD flang not installed")]


def _drive(tmp, nsteps, *more):
    (tmp / "pom.nml").write_text(f"&pom_nml\n title = 'cold'\n netcdf_file = 'case'\n wrk_pth = '{tmp}/'\n mode = 3\n nadv = 2\n nitera = 1\n sw = 0.5\n"
                                 " npg = 1\n dte = 6.\n isplit = 30\n days = 1\n nread_rst = 0\n/\n")
    r = subprocess.run([os.path.join(FDIR, "pom_gpu_main"), "--cold-z", "state.out", str(nsteps), *more], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout, r.stdout + r.stderr
    return np.fromfile(tmp / "state.out", dtype="<f8")


def _bad(st, raw):
    n2, n3 = st.blk2d.size, st.blk3d.size
    b2, b3 = raw[:n2].reshape(st.blk2d.shape), raw[n2:n2 + n3].reshape(st.blk3d.shape)
    return ([n for i, n in enumerate(BLK2D) if n not in E.SCRATCH and not E.same_bits(st.blk2d[i], b2[i])]
            + [n for i, n in enumerate(BLK3D) if n not in E.SCRATCH and not E.same_bits(st.blk3d[i], b3[i])])


def test_driver_with_a_four_sided_lateral_file_equals_the_oracle(tmp_path):
    import __graft_entry__ as ge
    ge.build_hip()
    subprocess.check_call(["make", "-C", FDIR, "IM=65", "JM=49", "KB=21"], stdout=subprocess.DEVNULL)
    im, jm, kb = SIZE
    os.mkdir(tmp_path / "in")
    f, paths = F.z_inputs(tmp_path / "in", SIZE, nml=NML)
    tile = F.one_tile(im, jm)
    init, _ = F.expected_state_z(paths, tile, kb, True, True, **NML)
    # the driver hands the library the clim file it finds: restore_interior's records 1, 2 are months 11, 12 of it (io_pnetcdf.F:3316), mapped
    mp = F.mapped(F.read_files(paths), kb, False, True, months=(10, 11))
    init.restore_records = [(np.ascontiguousarray(mp["Tclim"][m]), np.ascontiguousarray(mp["Sclim"][m])) for m in (10, 11)]
    _, nl, _, _ = ffc.schedule(init, 4)
    lbry = tmp_path / "in" / "case.lbry.nc"
    for onz, options in ((False, ("--lbry-sides", "15")), (True, ("--lbry-sides", "15", "--lbry-z")), (True, ("--lbry-z", "--lbry-sides", "15"))):
        raw_l = LS.raw_lbry_z(init, nl) if onz else LS.raw_lbry(init, nl)
        (LS.write_lbry_z if onz else LS.write_lbry)(lbry, raw_l, 15)
        a = init.copy()
        a.lateral_records = (LS.lateral_records_z if onz else LS.lateral_records)(a, raw_l, 15)
        OracleTile(a).run(4)
        assert int(a.error_status) == 0 and a.u.any()
        raw = _drive(tmp_path, 4, *options)
        assert not _bad(a, raw), (options, _bad(a, raw))
        if not onz:                                           # the same file under the default mask: west and north fall back to tclim, sclim and zero
            two = init.copy()
            two.lateral_records = LS.lateral_records(two, raw_l, LS.EAST | LS.SOUTH)
            OracleTile(two).run(4)
            raw2 = _drive(tmp_path, 4)
            assert not _bad(two, raw2), _bad(two, raw2)
            assert _bad(a, raw2), "the west and north lines have reached the state"
