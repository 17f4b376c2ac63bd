"""TEST HELPER shared by tests/test_restart_read_emulated.py and tests/test_gpu_restart_read.py: the state the reference's
read_restart_pnetcdf (io_pnetcdf.F:2420-2768) would leave, built on the CPU WITHOUT the code under test -- a fresh initial state,
the 37 restart fields assigned from the file as scipy.io.netcdf_file reads it, d = h + el, dt = h + et, time0 = time = the file's
time, iint = 0 -- and the writers of odd restart files (other variable order, extra variables, broken ones) for the reader's
by-name lookup and its refusals.  The scenarios that the host build and the device run alike (a file written by the library,
the state after a read, reading into a live context, the refusals) live here too, with the library's path as a parameter
(None: the product library on device 0), so that the two test files cannot drift apart."""
import os

import numpy as np
import pytest
from scipy.io import netcdf_file

from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D, RESTART_2D, RESTART_3D

SCRATCH = {"tps", "fluxua", "fluxva", "zflux"}
RESTART = RESTART_2D + RESTART_3D
UNTOUCHED = [n for n in BLK2D + BLK3D if n not in RESTART and n not in ("d", "dt")]


def same_bits(x, y):
    """bit for bit (uint64 view): sees the sign of a zero, takes equal NaN patterns for equal"""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def diff(a, b, names=None):
    return [n for n in (names or BLK2D + BLK3D) if n not in SCRATCH and not same_bits(a.field(n), b.field(n))]


def file_values(path):
    """({name: float64 array}, time, iint) of a restart file, read by scipy"""
    with netcdf_file(str(path), "r", mmap=False) as f:
        vals = {n: np.array(f.variables[n][:], dtype=np.float64) for n in RESTART}
        return vals, float(np.asarray(f.variables["time"][:]).ravel()[0]), float(np.asarray(f.variables["iint"][...]).ravel()[0])


def assign_from_file(st, path):
    """what the reference's reader does to a state: X(1:im,1:jm[,1:kb]) of the 37 fields from the tile's window of the file, d, dt, time0, time"""
    vals, time, iint = file_values(path)
    im, jm, io, jo = st.im, st.jm, st.i_off, st.j_off
    for n, v in vals.items():
        st.field(n)[..., :jm, :im] = v[..., jo:jo + jm, io:io + im]
    st.d[:jm, :im] = st.h[:jm, :im] + st.el[:jm, :im]
    st.dt[:jm, :im] = st.h[:jm, :im] + st.et[:jm, :im]
    st.time0 = time
    st.time = time
    return st, time, iint


def expected_state(case, im, jm, kb, nml, path):
    """fresh make_case + oracle_finish_initial, then the file: the start of the oracle's continuation"""
    from oracle.pyoracle import oracle_finish_initial
    a = make_case(case, im, jm, kb, **nml)
    oracle_finish_initial(a)
    assign_from_file(a, path)
    assert a.iint == 0
    return a


def write_foreign_restart(path, vals, time, iint, kb, jm, im, version=2, drop=(), as_float=(), z_len=None):
    """a restart file as ANOTHER writer might lay it out (scipy): the 39 variables in reversed order, two extra variables, extra
    attributes, other dimension names.  drop / as_float / z_len break it on purpose."""
    with netcdf_file(str(path), "w", version=version) as f:
        f.history = "written by a test"
        f.createDimension("one", 1)
        f.createDimension("levels", z_len or kb)
        f.createDimension("rows", jm)
        f.createDimension("cols", im)
        f.createDimension("spare", 3)
        x = f.createVariable("extra_first", "d", ("spare",))
        x[:] = [1.0, 2.0, 3.0]
        x.note = "not a restart field"
        for n in reversed(RESTART):
            if n in drop:
                continue
            dims = ("levels", "rows", "cols") if n in RESTART_3D else ("rows", "cols")
            v = f.createVariable(n, "f" if n in as_float else "d", dims)
            a = vals[n]
            if n in RESTART_3D and z_len and z_len != kb:
                a = np.concatenate([a] + [a[-1:]] * (z_len - kb))
            v[:] = a
            v.units = "whatever"
        e = f.createVariable("extra_mid", "i", ("spare",))
        e[:] = [7, 8, 9]
        t = f.createVariable("time", "d", ("one",))
        t[:] = [time]
        t.units = "days since then"
        s = f.createVariable("iint", "d", ())
        s[...] = iint


# ---- scenarios shared by the emulated and the device tests (libpath: the host build, a study variant, or None = libpomgpu.so) -------
M = 6                                                           # steps of every continuation
START = "2000-01-01 00:00:00 +00:00"


def make_gpu(st, libpath=None):
    from extpom_amd.model import PomGpu
    return PomGpu(st, device=0, libpath=libpath)


def fresh(case, nml, grid=(65, 49, 21)):
    from oracle.pyoracle import oracle_finish_initial
    a = make_case(case, *grid, **nml)
    oracle_finish_initial(a)
    return a


def written(tmp_path, case, nml, steps, grid=(65, 49, 21), name="restart.nc", libpath=None):
    """`steps` steps of the library from the initial state, then its own restart file; returns (path, the state written)"""
    a = fresh(case, nml, grid)
    g = make_gpu(a, libpath)
    g.run(steps)
    g.write_file("restart", tmp_path / name, title=case, time_start=START)
    g.io_wait()
    g.download()
    g.close()
    return tmp_path / name, a


def check_read_state(b, init, path):
    """b: downloaded after read_restart into a context created on `init`"""
    vals, time, iint = file_values(path)
    for n in RESTART:
        assert same_bits(b.field(n), vals[n]), n
    assert same_bits(b.d, init.h + vals["el"]) and same_bits(b.dt, init.h + vals["et"])
    assert b.time0 == time and b.time == time, (b.time0, b.time, time)
    bad = diff(b, init, UNTOUCHED)
    assert not bad and same_bits(b.bdry, init.bdry) and same_bits(b.blk1d, init.blk1d), bad


def reading_into_a_live_context(tmp_path, writing, libpath=None):
    """run(2) plus ONE mode_external call with isplit = 7 leaves an odd substep held back for its partner; read_restart completes
    what is pending, then overwrites: exactly the state of the round trip, and run(M) continues like the oracle.  writing: a
    restart file of that context is still in flight when the reader is called."""
    from oracle.pyoracle import OracleTile
    nml = dict(isplit=7)
    path, a = written(tmp_path, "seamount", nml, 3, libpath=libpath)
    b = fresh("seamount", nml)
    g = make_gpu(b, libpath)
    g.run(2)
    g.set_con(iint=3)
    g.call("get_time")
    g.get_con()
    g.call("lateral_viscosity")
    g.call("mode_interaction")
    g.set_con(iext=1)
    g.call("mode_external")
    if writing:
        g.write_file("restart", tmp_path / "other.nc", title="seamount", time_start=START)
    g.read_restart(path)
    g.download()
    live = b.copy()                                             # everything the reader does not touch is the live run's
    for n in RESTART:
        assert same_bits(b.field(n), a.field(n)), n
    assert same_bits(b.d, b.h + a.el) and same_bits(b.dt, b.h + a.et) and b.time0 == a.time and b.time == a.time
    # the continuation: the oracle from the same arrays with iint = 0 (pom.f restarts its step counter)
    g.set_con(iint=0, iext=0)
    live.iint = 0
    live.iext = 0
    ot = OracleTile(live)
    for n in range(1, M + 1):
        ot.run(1)
        g.run(1)
        g.download()
        assert not diff(live, b), f"step {n}: {diff(live, b)}"
    g.close()
    if writing:
        assert os.path.getsize(tmp_path / "other.nc") == os.path.getsize(path)   # same header, same length: the writer was joined, not cut off


def refusals_leave_the_state_untouched(tmp_path, libpath=None):
    """each refusal through PomGpuError with error_status == 1 and the named cause in pomgpu_last_error; a download shows the
    state unchanged, and a good read succeeds once error_status is cleared"""
    from extpom_amd.lib import PomGpuError
    path, a = written(tmp_path, "island", {}, 2, libpath=libpath)
    vals, time, iint = file_values(path)
    raw = open(path, "rb").read()
    bad = {}
    write_foreign_restart(tmp_path / "no_q2lb.nc", vals, time, iint, 21, 49, 65, drop=("q2lb",))
    bad["no_q2lb.nc"] = ("q2lb", "absent")
    write_foreign_restart(tmp_path / "t_float.nc", vals, time, iint, 21, 49, 65, as_float=("t",))
    bad["t_float.nc"] = ("variable t ", "NC_DOUBLE")
    write_foreign_restart(tmp_path / "z22.nc", vals, time, iint, 21, 49, 65, z_len=22)
    bad["z22.nc"] = ("(22, 49, 65)", "(21, 49, 65)")
    open(tmp_path / "short.nc", "wb").write(raw[:-1000])
    bad["short.nc"] = ("q2lb", "beyond the file")
    open(tmp_path / "cdf5.nc", "wb").write(b"CDF\x05" + raw[4:])
    bad["cdf5.nc"] = ("CDF version 5",)
    open(tmp_path / "empty.nc", "wb").close()
    bad["empty.nc"] = ("empty",)
    bad["missing.nc"] = ("cannot open",)
    b = fresh("island", {})
    g = make_gpu(b, libpath)
    g.run(1)
    g.download()
    before = b.copy()

    def refused(name, words, **kw):
        with pytest.raises(PomGpuError) as e:
            g.read_restart(tmp_path / name, **kw)
        msg = g.L.pomgpu_last_error(g.h).decode()
        assert str(tmp_path / name) in msg and all(w in msg for w in words) and "status -1" in str(e.value), (name, msg)
        g.get_con()
        assert b.error_status == 1
        g.download()
        assert not diff(b, before, BLK2D + BLK3D) and same_bits(b.bdry, before.bdry), name
        assert b.time0 == before.time0 and b.time == before.time and b.iint == 1
        g.set_con(error_status=0)
    for name, words in bad.items():
        refused(name, words)
    b.i_off = 3                                                 # a tile offset beyond the grid
    refused("restart.nc", ("does not fit the global grid",))
    b.i_off = 0
    refused("restart.nc", ("does not fit the global grid",), im_global=64)
    g.read_restart(path)                                        # and a good one succeeds afterwards
    g.download()
    for n in RESTART:
        assert same_bits(b.field(n), a.field(n)), n
    assert b.error_status == 0
    g.close()
