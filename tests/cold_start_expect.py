"""TEST HELPER shared by the cold-start tests: writers of the reference's three input files (<...>.grid.nc, .init.nc, .clim.nc) with
scipy.io.netcdf_file, and the state the reference's initialize (initialize.f:24-36) would leave from them, restated in numpy WITHOUT
the code under test: read_grid_pnetcdf (io_pnetcdf.F:2085-2263), read_initial_ts_pnetcdf (:2771-2842), read_clim_ts_pnetcdf
(:2845-2909), read_grid (initialize.f:317-389) and initial_conditions (:392-463); the tail (the two dens calls, update_initial, baropg)
is cases.finish_initial with the oracle's dens / baropg.  sin and log are math.sin / math.log per element: numpy's vector paths need
not equal libm, which is what the reference and the library call.

On a tile the restatement replaces the reference's exchange2d_mpi of dum, dvm, aru, arv by what the exchange delivers: the owner's
value, i.e. the same formula on the cells of the global arrays."""
import math

import numpy as np
from scipy.io import netcdf_file

from extpom_amd.cases import finish_initial, make_case
from extpom_amd.layout import BLK2D, BLK3D, PomState
from extpom_amd.namelist import apply_constants, run_constants

SCRATCH = {"tps", "fluxua", "fluxva", "zflux"}
GRID_PLANES = {"dx": "dx", "dy": "dy", "lon_rho": "east_e", "lat_rho": "north_e", "lon_u": "east_u", "lat_u": "north_u", "lon_v": "east_v",
               "lat_v": "north_v", "lon_psi": "east_c", "lat_psi": "north_c", "angle": "rot", "h": "h", "fsm": "fsm"}
NREC_CLIM = 12
EXTRA_LEVELS = 3            # Level is longer than kb-1: the file's levels kb .. kb+1 must not arrive


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def diff(a, b):
    """every array of blk2d and blk3d but the four scratch arrays, bdry, blk1d and blkcon: the names that differ"""
    out = [n for n in BLK2D + BLK3D if n not in SCRATCH and not same_bits(a.field(n), b.field(n))]
    out += [n for n, x, y in (("bdry", a.bdry, b.bdry), ("blk1d", a.blk1d, b.blk1d)) if not same_bits(x, y)]
    if a.con.tobytes() != b.con.tobytes():
        out += ["con." + n for n in a.con.dtype.names if a.con[n].tobytes() != b.con[n].tobytes()]
    return out


def case_fields(case, im, jm, kb, as_float=False, **nml):
    """the GLOBAL fields of the three files, from make_case's single-tile state: the grid as it stands there but lat_rho, which is in
    degrees (the model's north_e is in metres; read_grid takes the sine of it); T, S = tb, sb on kb-1+EXTRA_LEVELS levels; Tclim, Sclim
    as NREC_CLIM records that all differ.  as_float: every value is representable in fp32 (an NC_FLOAT file set holds the same numbers)."""
    g = make_case(case, im, jm, kb, **nml)
    f = {n: g.field(m).copy() for n, m in GRID_PLANES.items()}
    f["lat_rho"] = 30.0 + 15.0 * g.north_e / float(g.north_e.max())
    f["z"], f["zz"] = g.z.copy(), g.zz.copy()
    nlev = kb - 1 + EXTRA_LEVELS
    k = np.arange(nlev)[:, None, None]
    src = np.minimum(k, kb - 2)
    f["T"] = np.take_along_axis(g.tb, np.broadcast_to(src, (nlev, jm, im)), 0) + 0.25 * (k >= kb - 1)
    f["S"] = np.take_along_axis(g.sb, np.broadcast_to(src, (nlev, jm, im)), 0) + 0.125 * (k >= kb - 1)
    r = np.arange(1, NREC_CLIM + 1, dtype=np.float64)[:, None, None, None]
    f["Tclim"] = (g.tclim[None] + 0.01 * r) * g.fsm[None, None]
    f["Sclim"] = (g.sclim[None] + 0.002 * r) * g.fsm[None, None]
    f["Level"] = np.arange(1.0, nlev + 1.0)
    if as_float:
        f = {n: v.astype(np.float32).astype(np.float64) for n, v in f.items()}
    return f


def assert_case_is_demanding(f, kb, tiles=()):
    """what the issue wants the generated input to hold, asserted on the fields themselves"""
    dx, dy, fsm = f["dx"], f["dy"], f["fsm"]
    for a in (dx, dy):                               # each varies along i AND along j
        assert (np.ptp(a, axis=0) > 0).any() and (np.ptp(a, axis=1) > 0).any(), "dx, dy depend on one index only"
    assert (fsm[2:-2, 2:-2] == 0).any() and set(np.unique(fsm)) == {0.0, 1.0}, "no interior land"
    assert np.abs(f["lat_rho"]).max() <= 90.0
    assert not np.array_equal(f["T"], f["S"])
    t10 = f["Tclim"][9]
    assert not np.array_equal(t10, f["Tclim"][8]) and not np.array_equal(t10, f["Tclim"][10]) and not np.array_equal(t10[:kb - 1], f["T"][:kb - 1])
    assert f["T"].shape[0] > kb - 1 and (f["T"][kb - 1] != 0).any() and (f["S"][kb - 1] != 0).any(), "the file's level kb is zero"
    for t in tiles:
        io, jo = t.i_off, t.j_off
        assert 2.0 * 7.29e-5 * math.sin(f["lat_rho"][jo + t.jm // 2 - 1, io + t.im // 2 - 1] * (math.pi / 180.0)) != 0.0
        if io > 0:                                   # land in the window line (global column i_off) and on the ghost line (i_off + 1)
            assert (fsm[jo:jo + t.jm, io - 1] == 0).any() and (fsm[jo:jo + t.jm, io] == 0).any(), (io, jo)
        if jo > 0:
            assert (fsm[jo - 1, io:io + t.im] == 0).any() and (fsm[jo, io:io + t.im] == 0).any(), (io, jo)


def write_files(d, f, kind="d", fsm_kind="b", version=2, shuffle=False, drop=(), retype=None, reshape=None, clim_records=NREC_CLIM,
                fixed_clim=False, tag="", stem="case"):
    """the three files; kind: "d" NC_DOUBLE, "f" NC_FLOAT; fsm_kind also "b" NC_BYTE, "h" NC_SHORT, "i" NC_INT.  shuffle: the variables in
    reversed order with extra variables and attributes and other dimension names.  drop / retype {name: kind} / reshape {name: dims}
    break a file on purpose.  Returns (grid, init, clim) paths."""
    retype, reshape = retype or {}, reshape or {}
    jm, im = f["dx"].shape
    X, Y = ("cols", "rows") if shuffle else ("x", "y")
    paths = [str(d / f"{stem}{tag}.{s}.nc") for s in ("grid", "init", "clim")]

    def put(nc, name, dims, a, k):
        if name in drop:
            return
        v = nc.createVariable(name, retype.get(name, k), reshape.get(name, dims))
        if name in reshape:                          # a deliberately misshapen variable: any values
            a = np.resize(a, tuple(s or 1 for s in v.shape))
        v[:] = a
        if shuffle:
            v.note = "an attribute the reader skips"

    with netcdf_file(paths[0], "w", version=version) as nc:
        nc.createDimension("z", len(f["z"]))
        nc.createDimension(Y, jm)
        nc.createDimension(X, im)
        nc.createDimension("short", im - 1)
        names = ["z", "zz"] + list(GRID_PLANES)
        if shuffle:
            nc.history = "written by a test"
            put(nc, "extra", (Y, X), f["h"] * 2.0, "d")
            names = names[::-1]
        for n in names:
            put(nc, n, ("z",) if n in ("z", "zz") else (Y, X), f[n], kind if n != "fsm" else fsm_kind)
    with netcdf_file(paths[1], "w", version=version) as nc:
        nc.createDimension("Time", None)
        nc.createDimension("Level", len(f["Level"]))
        nc.createDimension(Y, jm)
        nc.createDimension(X, im)
        nc.createDimension("short", im - 1)
        order = ["S", "Level", "T"] if shuffle else ["Level", "T", "S"]
        if shuffle:
            put(nc, "Time", ("Time",), np.array([0.5]), "d")
        for n in order:
            put(nc, n, ("Level",) if n == "Level" else ("Time", "Level", Y, X), f[n] if n == "Level" else f[n][None], kind)
    with netcdf_file(paths[2], "w", version=version) as nc:
        nc.createDimension("month", clim_records if fixed_clim else None)
        nc.createDimension("zlev", f["Tclim"].shape[1])
        nc.createDimension(Y, jm)
        nc.createDimension(X, im)
        nc.createDimension("short", im - 1)
        for n in (["Sclim", "Tclim"] if shuffle else ["Tclim", "Sclim"]):
            put(nc, n, ("month", "zlev", Y, X), f[n][:clim_records], kind)
    return paths


def assert_file_types(paths, kind, fsm_kind, version=2):
    """the generated files hold what was asked for: the format version, NC_DOUBLE or NC_FLOAT throughout, fsm in its own type"""
    want = {n: (fsm_kind if n == "fsm" else kind) for n in ["z", "zz", "Level", "T", "S", "Tclim", "Sclim"] + list(GRID_PLANES)}
    seen = {}
    for p in paths:
        with open(p, "rb") as fh:
            assert fh.read(4) == b"CDF" + bytes([version]), p
        with netcdf_file(p, "r", mmap=False) as nc:
            seen.update({n: v.typecode() for n, v in nc.variables.items() if n in want})
    assert seen == want, {n: (seen.get(n), want[n]) for n in want if seen.get(n) != want[n]}


def blank_state(tile, kb, **nml):
    """what a host has before initialize_arrays: the COMMON blocks zero, read_input's constants in blkcon"""
    st = PomState(tile.im_local, tile.jm_local, kb, tile.im, tile.jm)
    st.n_west, st.n_east, st.n_south, st.n_north = tile.n_west, tile.n_east, tile.n_south, tile.n_north
    st.i_off, st.j_off = tile.i_off, tile.j_off
    apply_constants(st, run_constants(None, **nml))
    return st


def read_files(paths):
    """{name: float64 array} of every variable the readers ask for, as scipy delivers them"""
    out = {}
    for p in paths:
        with netcdf_file(p, "r", mmap=False) as nc:
            for n, v in nc.variables.items():
                out[n] = np.array(v[:], dtype=np.float64)
    return out


def expected_readers(paths, tile, kb, **nml):
    """read_grid + initial_conditions up to the first dens call, restated on one tile; returns (state, cflmin)"""
    v = read_files(paths)
    st = blank_state(tile, kb, **nml)
    im, jm, io, jo = tile.im, tile.jm, tile.i_off, tile.j_off
    A = (slice(0, jm), slice(0, im))
    G = (slice(jo, jo + jm), slice(io, io + im))
    st.dx, st.dy, st.h = 1.0, 1.0, 1.0                       # io_pnetcdf.F:2159-2171, the whole padded arrays
    st.z, st.zz = v["z"][:kb], v["zz"][:kb]
    for n, m in GRID_PLANES.items():
        st.field(m)[A] = v[n][G]
    st.dz[:kb - 1] = st.z[:kb - 1] - st.z[1:]
    st.dzz[:kb - 1] = st.zz[:kb - 1] - st.zz[1:]
    # masks (:2243-2256): a cell whose western / southern neighbour is land; the neighbour of column 1 of a tile with a west neighbour is
    # the owner's cell, global column i_off -- what exchange2d_mpi delivers is the owner's result of the same statement
    fs = v["fsm"]
    dum, dvm = fs.copy(), fs.copy()
    dum[:, 1:][(fs[:, :-1] == 0) & (fs[:, 1:] != 0)] = 0.0
    dvm[1:, :][(fs[:-1, :] == 0) & (fs[1:, :] != 0)] = 0.0
    st.dum[A], st.dvm[A] = dum[G], dvm[G]
    if io == 0 and tile.n_west != -1 or jo == 0 and tile.n_south != -1:
        raise ValueError("a tile at the global edge has no neighbour there")
    deg2rad = st.pi / 180.0
    for j in range(jm):
        for i in range(im):
            st.cor[j, i] = 2.0 * 7.29e-5 * math.sin(st.north_e[j, i] * deg2rad)
    st.period = (2.0 * st.pi) / abs(st.cor[jm // 2 - 1, im // 2 - 1]) / 86400.0
    st.art = st.dx * st.dy                                   # whole-array statement: 1 in the padding
    dx, dy = v["dx"], v["dy"]
    aru, arv = np.zeros_like(dx), np.zeros_like(dx)
    aru[1:, 1:] = 0.25 * (dx[1:, 1:] + dx[1:, :-1]) * (dy[1:, 1:] + dy[1:, :-1])
    arv[1:, 1:] = 0.25 * (dx[1:, 1:] + dx[:-1, 1:]) * (dy[1:, 1:] + dy[:-1, 1:])
    aru[:, 0], arv[:, 0] = aru[:, 1], arv[:, 1]              # initialize.f:373-376, then :378-381
    aru[0, :], arv[0, :] = aru[1, :], arv[1, :]
    st.aru[A], st.arv[A] = aru[G], arv[G]
    st.d = st.h + st.el
    st.dt = st.h + st.et
    cfl = 0.5 / np.sqrt(1.0 / st.dx ** 2 + 1.0 / st.dy ** 2) / np.sqrt(st.grav * (st.h + st.small)) * st.fsm
    cflmin = float(cfl[cfl > 0].min()) if (cfl > 0).any() else float(np.finfo(np.float64).max)
    A3 = (slice(0, kb - 1),) + A
    st.tb[A3] = v["T"][0][(slice(0, kb - 1),) + G]           # record 1, levels 1..kb-1; level kb stays +0.0
    st.sb[A3] = v["S"][0][(slice(0, kb - 1),) + G]
    st.tclim[(slice(None),) + A] = v["Tclim"][9][(slice(None),) + G]
    st.sclim[(slice(None),) + A] = v["Sclim"][9][(slice(None),) + G]
    return st, cflmin


def bottom_friction(st):
    """initialize.f:524-544 on (1:im, 1:jm), math.log per element"""
    st.cbc = 0.0
    zk = 1.0 + st.zz[st.kb - 2]
    for j in range(st.jm):
        for i in range(st.im):
            t = st.kappa / math.log(zk * st.h[j, i] / st.z0b)
            st.cbc[j, i] = min(st.cbcmax, max(st.cbcmin, t * t))      # "**2" is a product in Fortran; Python's float ** 2 is pow()
    return st


def expected_state(paths, tile, kb, dens=None, baropg=None, **nml):
    """the whole of initialize.f:24-36 on one tile; dens / baropg default to the oracle's; returns (state, cflmin)"""
    st, cflmin = expected_readers(paths, tile, kb, **nml)
    if dens is None:
        from oracle.pyoracle import OracleTile
        ot = OracleTile(st)
        dens = lambda s, si, ti, rho: ot.call("dens", ot.a3(si), ot.a3(ti), ot.a3(rho))
        baropg = lambda s: ot.call("baropg_mcc" if int(s.npg) == 2 else "baropg")
    finish_initial(st, dens, baropg)
    # update_initial's loop runs over (1:im, 1:jm) (initialize.f:481-493); finish_initial assigns whole arrays, which is the same thing on
    # make_case's states (h = 0 in the padding of a trimmed tile) but not behind the readers' default h = 1
    for n in ("l", "q2b", "q2lb", "kh", "km", "kq", "aam", "q2", "q2l"):
        st.field(n)[:, tile.jm:, :] = 0.0
        st.field(n)[:, :, tile.im:] = 0.0
    bottom_friction(st)
    return st, cflmin
