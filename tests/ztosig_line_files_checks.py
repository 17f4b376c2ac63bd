"""The checks of z-level lateral files (pomgpu_set_z_lateral + pomgpu_set_forcing_files), each taking the library to load (None: the product
library on device 0), shared by tests/test_ztosig_line_emulated.py and tests/test_gpu_ztosig_line.py.  The lbry file is
tests/forcing_expect.py's with temp / salt .east / .south on the levels of a variable `z` it gains here; the expected records are that
helper's restatement of the reader with tests/ztosig_line_expect.py's mapped lines where the reader's sigma-level arrays would be -- each
tile with ITS depth line and its piece of the line -- and the bar is the CPU oracle fed those records and a second context fed them through
set_lateral_records: 64-bit patterns, every array, bdry and blkcon."""
import os
import threading

import numpy as np
import pytest
from scipy.io import netcdf_file

import forcing_expect as fx
import forcing_files_checks as ffc
import ztosig_line_expect as ZL
from extpom_amd import decomp
from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D
from extpom_amd.lib import PomGpuError
from extpom_amd.model import PomGpu
from forcing_files_checks import diff, same_bits, status
from oracle.pyoracle import OracleTile, oracle_finish_initial

KS_LBRY = 7
SIZE = (65, 49, 21)
STEPS = 21                                                    # ibc = 10 at dti = 360 s: lateral_bc reads records 1, 2 at step 1, 3 at step 10, 4 at step 20
ZVARS = (("temp.east", 0, False, 4), ("salt.east", 0, True, 5), ("temp.south", 1, False, 12), ("salt.south", 1, True, 13))   # name, edge, S-like, place in LATERAL_ORDER


def levels(ks, hmax):
    return 5.0 + np.round((0.8 * hmax - 5.0) * (np.arange(ks) / (ks - 1.0)) ** 1.5 * 8.0) / 8.0


def raw_lbry_z(g, nrec, ks=KS_LBRY, kind="d", seed=14):
    """forcing_expect.raw_lbry of the single-tile state g with the four T, S lines on ks z levels: (nrec, ks, jm | im), another line every
    record, missing values at the points 2 and n-1 so that the copied ends show; kind "f": every number a float32, as the file holds it"""
    raw = fx.raw_lbry(g, nrec)
    rng = np.random.default_rng(seed)
    zs = levels(ks, float(g.h.max()))
    hh = g.h[:g.jm, :g.im]
    for name, edge, salt, _ in ZVARS:
        hl = ZL.depth_line(hh, edge)
        lines = []
        for r in range(nrec):
            _, ln = ZL.random_line(zs, hl, rng, salt)
            ln[0, 1], ln[0, -2] = 0.0, 0.005
            lines.append(ln)
        a = np.stack(lines)
        raw[name] = fx.f32(a) if kind == "f" else a
    raw["z"] = fx.f32(zs) if kind == "f" else zs
    return raw


def write_lbry_z(path, raw, kind="d", version=2, drop=(), zdims=None, ztype=None, zvalues=None, levels_of=None):
    """the lbry file with its level variable `z`: temp, salt as (time, z, y | x), zeta, u, v as ever.  drop / zdims / ztype / zvalues /
    levels_of ({name: level count}) break the file on purpose"""
    path = str(path)
    jm, im = raw["zeta.east"].shape[1], raw["zeta.south"].shape[1]
    z = raw["z"] if zvalues is None else np.asarray(zvalues, dtype=np.float64)
    with netcdf_file(path, "w", version=version) as nc:
        nc.createDimension("time", None)
        nc.createDimension("z", len(z))
        nc.createDimension("y", jm)
        nc.createDimension("x", im)
        made = {}

        def lev(n):
            if n == len(z):
                return "z"
            if n not in made:
                made[n] = f"lev{n}"
                nc.createDimension(made[n], n)
            return made[n]

        if "z" not in drop:
            v = nc.createVariable("z", ztype or kind, zdims or ("z",))
            v[:] = z if zdims is None else np.resize(z, v.shape)
        for n in fx.LBRY:
            if n in drop:
                continue
            a = raw[n]
            if levels_of and n in levels_of:
                a = np.resize(a, (a.shape[0], levels_of[n], a.shape[2]))
            along = "y" if n.endswith(".east") else "x"
            dims = ("time", along) if a.ndim == 2 else ("time", lev(a.shape[1]), along)
            nc.createVariable(n, kind, dims)[:] = a
    return path


def lateral_records_z(st, raw, nrec=None):
    """forcing_expect.lateral_records with tbe sbe tbs sbs mapped from the z-level lines: the tile's piece of each line with one window point
    towards every neighbour, the tile's own depth line, a copied end only where the tile has no neighbour; zero beyond jm / im"""
    nrec = raw["zeta.east"].shape[0] if nrec is None else nrec
    sig = dict(raw)
    for name, _, _, _ in ZVARS:
        sig[name] = np.zeros((raw[name].shape[0], st.kb, raw[name].shape[2]))
    recs = fx.lateral_records(st, sig, nrec)
    hh = st.h[:st.jm, :st.im]
    for r, rec in enumerate(recs):
        for name, edge, _, at in ZVARS:
            aj = ZL.along_j(edge)
            off, n = (st.j_off, st.jm) if aj else (st.i_off, st.im)
            lo, hi = (st.n_south, st.n_north) if aj else (st.n_west, st.n_east)
            t = ZL.ztosig_line(raw["z"], ZL.window_of(raw[name][r], off, n), st.zz[:st.kb], ZL.depth_line(hh, edge), edge, lo == -1, hi == -1)
            out = np.zeros_like(rec[at])
            out[:, :n] = t
            rec[at] = out
    return recs


def assert_records_are_demanding(st, recs, land=False):
    kb, jm, im = st.kb, st.jm, st.im
    assert len(recs) >= 3
    for at, n in ((4, jm), (5, jm), (12, im), (13, im)):
        a = [r[at] for r in recs]
        assert all(x[kb - 1].any() and np.isfinite(x).all() for x in a) and not same_bits(a[0], a[1]) and not same_bits(a[1], a[2])
        assert same_bits(a[0][:, 0], a[0][:, 1]) and same_bits(a[0][:, n - 1], a[0][:, n - 2]) and a[0][:, 0].any() and a[0][:, n - 1].any()
    assert not same_bits(recs[0][4], recs[0][5]), "T is not S"
    if land:
        assert (recs[0][4][:, 1:jm - 1] == 0).all(axis=0).any() or (recs[0][12][:, 1:im - 1] == 0).all(axis=0).any(), "a point with hl <= 1"


# ---- 1: file path = setter path = oracle ------------------------------------------------------------------------------------------------
def file_setters_oracle(lib, tmp, case, size=SIZE, kind="d", chunk_kb=None, setters=True, steps=STEPS):
    a, raw_s, _ = ffc.start(case, ffc.BASE, steps, size=size)
    _, nl, _, ibc = ffc.schedule(a, steps)
    assert ibc == 10 and nl >= 4
    raw_l = raw_lbry_z(a, nl, kind=kind)
    a.lateral_records = lateral_records_z(a, raw_l)
    assert_records_are_demanding(a, a.lateral_records, land=case == "archipelago" and size == SIZE)
    b, s = a.copy(), a.copy()
    sfrc = fx.write_sfrc(tmp / "case.sfrc.nc", raw_s)
    lbry = write_lbry_z(tmp / "case.lbry.nc", raw_l, kind=kind)
    with netcdf_file(lbry, "r", mmap=False) as nc:
        assert nc.variables["temp.east"].typecode() == kind and nc.variables["temp.east"].shape[1:] == (KS_LBRY, size[1])
        assert same_bits(nc.variables["salt.south"][:], raw_l["salt.south"]), "the file holds the numbers the expectation was made of"
    g = PomGpu(b, libpath=lib)
    if chunk_kb:
        g.switch("IO_CHUNK_KB", chunk_kb)
    g.set_z_inputs(lbry=True)
    g.set_forcing_files(sfrc=sfrc, lbry=lbry)
    g.run(steps)                                              # ONE call across every record change
    OracleTile(a).run(steps)
    g.download()
    assert int(a.error_status) == 0 and not diff(a, b), diff(a, b)
    g.close()
    if setters:
        h = PomGpu(s, libpath=lib)
        ffc.step_with_setters(h, steps)
        h.download()
        assert not diff(b, s, skip=()), diff(b, s, skip=())   # two contexts of one library: the scratch arrays too
        h.close()


# ---- 2: init, clim and lbry all on z, after a cold start ----------------------------------------------------------------------------------
def all_on_z_after_a_cold_start(lib, tmp, case="archipelago", size=SIZE, steps=STEPS):
    """levels 9 (init), 6 (clim) and 7 (lbry), all different: the cold start of tests/ztosig_files_checks.py, then one run across three
    lateral records.  dti = 180 s here (ibc = 20: records 1, 2 at step 1, 3 at step 20): the rough state a start from these z-level fields
    leaves is not stable at the forcing check's dti = 360 s -- velocities of 1000 m/s after five steps, with or without a lateral file"""
    import ztosig_files_checks as zfc
    assert len({zfc.KS_INIT, zfc.KS_CLIM, KS_LBRY}) == 3
    im, jm, kb = size
    nml = dict(dte=6.0, isplit=30)
    f, paths = zfc.z_inputs(tmp, size, case=case, nml=nml)
    tile = zfc.one_tile(im, jm)
    a, _ = zfc.expected_state_z(paths, tile, kb, True, True, **nml)
    recs = zfc.records(paths, tile, kb, True)
    a.restore_records = recs
    _, nl, _, ibc = ffc.schedule(a, steps)
    assert ibc == 20 and nl == 3
    raw_l = raw_lbry_z(a, nl)
    a.lateral_records = lateral_records_z(a, raw_l)
    assert_records_are_demanding(a, a.lateral_records)
    lbry = write_lbry_z(tmp / "case.lbry.nc", raw_l)
    g, b, _ = zfc.cold(lib, paths, tile, kb, True, True, nml, recs=recs)
    g.set_z_inputs(init=True, clim=True, lbry=True)
    g.set_forcing_files(lbry=lbry)
    OracleTile(a).run(steps)
    g.run(steps)
    g.download()
    g.close()
    assert int(a.error_status) == 0 and a.u.any() and a.el.any() and float(np.abs(a.u).max()) < 20.0
    assert not diff(a, b), diff(a, b)


# ---- 3: tiles -----------------------------------------------------------------------------------------------------------------------------
TILE_GRID, TILE_KB, TILE_STEPS = (37, 29), 6, 4


def tiles(lib, tmp):
    """2x2 tiles of 37x29x6, the east and north ones trimmed, under the wide halo and the library's exchange: every rank names the same
    z-level lbry file with its own i0, j0 and maps all four lines with ITS h.  After lateral_bc's first call each tile's bdry holds the
    restatement's lines of its window (records 1 and 2), ghost ends included, with no message round spent on them; after four steps the
    cells a tile owns equal the single tile's.  NC_FLOAT and POMGPU_IO_CHUNK_KB at its minimum on two of the ranks' reads"""
    from forcing_files_checks import Board, device_mover, host_mover
    mover = host_mover if lib is not None else device_mover
    IMg, JMg = TILE_GRID
    nml = dict(dte=6.0, isplit=8)                            # the wide halo wants tiles of isplit + 7 cells
    one = make_case("archipelago", IMg, JMg, TILE_KB, **nml)
    oracle_finish_initial(one)
    iml, jml = decomp.local_size(IMg, JMg, 2, 2)
    tl = [decomp.make_tile(r, IMg, JMg, iml, jml, n_proc=4) for r in range(4)]
    assert len({(t.im, t.jm) for t in tl}) == 4 and any(t.im < t.im_local for t in tl) and any(t.jm < t.jm_local for t in tl)
    _, nl, _, _ = ffc.schedule(one, TILE_STEPS)
    raw_l = raw_lbry_z(one, nl, kind="f")
    sj, si = tl[2].j_off, tl[1].i_off                         # the seams: a missing value at either ghost end whose fill needs the window point
    for name, edge, _, _ in ZVARS:
        c = sj if edge == 0 else si
        raw_l[name][:, 0, c - 1:c + 3] = (21.0, 0.0, 0.0, 22.0)
    lbry = write_lbry_z(tmp / "tiles.lbry.nc", raw_l, kind="f")
    board, out, errs = Board(4), {}, []

    def rank(r):
        try:
            tile = tl[r]
            st = make_case("archipelago", IMg, JMg, TILE_KB, tile=tile, **nml)
            for n in BLK2D + BLK3D:                           # the finished initial state, cut to the tile
                st.field(n)[..., :tile.jm, :tile.im] = one.field(n)[..., tile.j_off:tile.j_off + tile.jm, tile.i_off:tile.i_off + tile.im]
            for n in ("tbe", "sbe", "tbw", "sbw"):
                st.field(n)[:, :tile.jm] = one.field(n)[:, tile.j_off:tile.j_off + tile.jm]
            for n in ("tbn", "sbn", "tbs", "sbs"):
                st.field(n)[:, :tile.im] = one.field(n)[:, tile.i_off:tile.i_off + tile.im]
            st.con[...] = one.con
            want = lateral_records_z(st, raw_l)
            stream = None
            if lib is None:
                import torch
                torch.cuda.set_device(0)
                ts = torch.cuda.Stream()
                torch.cuda.set_stream(ts)
                stream = ts.cuda_stream
            g = PomGpu(st, device=0, stream=stream, libpath=lib)
            move, ordered = mover(board, tile, g)
            g.set_transport(tile, move, agree=lambda mine: board.allmin(r, mine), stream_ordered=ordered)
            assert g.set_wide_external(True, min(t.im for t in tl), min(t.jm for t in tl))
            if r % 2:
                g.switch("IO_CHUNK_KB", 1)
            g.set_z_inputs(lbry=True)
            g.set_forcing_files(lbry=lbry, im_global=IMg, jm_global=JMg)
            rounds = g.exchange_rounds()
            g.set_con(iint=1)
            g.call("lateral_bc")                              # records 1 and 2 into the b and f lines
            assert g.exchange_rounds() == rounds, "lateral_bc posted a message round"
            g.download()
            for name, _, _, at in ZVARS:
                fld = ("t" if name.startswith("temp") else "s") + "b" + name.split(".")[1][0]
                for rec, sfx in ((0, "b"), (1, "f")):
                    assert same_bits(st.field(fld + sfx), want[rec][at]), (r, fld + sfx)
            g.set_con(iint=0)
            board.barrier.wait()
            g.run(TILE_STEPS)
            g.download()
            assert int(st.error_status) == 0
            g.close()
            out[r] = (st, want)
        except Exception:                                   # a dead rank must not leave the others at the barrier
            import traceback
            errs.append(traceback.format_exc())
            board.barrier.abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs[0]
    # the ghost end of the south-west tile's east line is not what it would be without the window point
    t0, w0 = tl[0], out[0][1]
    assert t0.n_north != -1 and w0[0][4][:, t0.jm - 1].any() and not same_bits(w0[0][4][:, t0.jm - 1], w0[0][4][:, t0.jm - 2])
    s = one.copy()
    g = PomGpu(s, libpath=lib)
    g.set_z_inputs(lbry=True)
    g.set_forcing_files(lbry=lbry)
    g.run(TILE_STEPS)
    g.download()
    g.close()
    bad = []
    for r in range(4):
        tile, st = tl[r], out[r][0]
        io, jo, im, jm = tile.i_off, tile.j_off, tile.im, tile.jm
        sl_j = slice(0 if jo == 0 else 1, jm if jo + jm == JMg else jm - 1)       # the cells the tile owns
        sl_i = slice(0 if io == 0 else 1, im if io + im == IMg else im - 1)
        for n in BLK2D + BLK3D:
            if n in ffc.SCRATCH:
                continue
            if not same_bits(s.field(n)[..., jo:jo + jm, io:io + im][..., sl_j, sl_i], st.field(n)[..., :jm, :im][..., sl_j, sl_i]):
                bad.append((r, n))
    assert not bad, bad


# ---- 4: the setting off -------------------------------------------------------------------------------------------------------------------
def setting_off(lib, tmp, steps=11):
    """default and explicit 0: a sigma lbry file gives the existing expectation; a z-level lbry file is refused for its level count"""
    a, raw_s, raw_l = ffc.start("seamount", ffc.BASE, steps)
    init = a.copy()
    sfrc, lbry = ffc.files(tmp, raw_s, raw_l)
    OracleTile(a).run(steps)
    for explicit in (False, True):
        b = init.copy()
        g = PomGpu(b, libpath=lib)
        if explicit:
            g.set_z_inputs(lbry=False)
        g.set_forcing_files(sfrc=sfrc, lbry=lbry)
        g.run(steps)
        g.download()
        assert not diff(a, b), (explicit, diff(a, b))
        g.close()
    b = init.copy()
    g = PomGpu(b, libpath=lib)
    zfile = write_lbry_z(tmp / "z.lbry.nc", raw_lbry_z(init, 2))
    with pytest.raises(PomGpuError):
        g.set_forcing_files(lbry=zfile)
    assert "variable temp.east has the dimension lengths (unlimited, 7, 49), wanted (records, 21, 49)" in status(g)[1]
    g.close()


# ---- 5: refusals on a foreign, stepped state ------------------------------------------------------------------------------------------------
def refusals(lib, tmp, size=(8, 8, 6)):
    """every new refusal names file and cause and leaves mirrors, slots, bdry and blkcon as they were (but error_status = 1)"""
    im, jm, kb = size
    a, raw_s, raw_sig = ffc.start("seamount", ffc.BASE, 11, size=size)
    raw = raw_lbry_z(a, 3)
    b = a.copy()
    g = PomGpu(b, libpath=lib)
    g.run(2)
    g.download()
    before = b.copy()
    g.set_z_inputs(lbry=True)
    count = [0]

    def refused(cause, tag, call=None, **kw):
        count[0] += 1
        p = write_lbry_z(tmp / f"bad{tag}.lbry.nc", kw.pop("raw", raw), **kw)
        with pytest.raises(PomGpuError) as e:
            (call or (lambda: g.set_forcing_files(lbry=p)))()
        es, msg = status(g)
        assert es == 1 and cause in msg and os.path.basename(p) in msg, (cause, msg)
        assert "status -1" in str(e.value)
        g.set_con(error_status=0)
        g.download()
        assert not diff(before, b), (cause, diff(before, b))

    refused("variable z (the z levels) is absent", "noz", drop=("z",))
    refused("variable z has 2 dimensions", "z2d", zdims=("z", "y"))
    refused("variable z has NetCDF type 4", "zint", ztype="i")
    z = raw["z"].copy()
    z[3] = z[2]
    refused("variable z is not finite and strictly increasing at level 4", "tie", zvalues=z)
    z = raw["z"].copy()
    z[5] = np.nan
    refused("variable z is not finite and strictly increasing at level 6", "nan", zvalues=z)
    refused("variable z is not finite and strictly increasing at level 2", "down", zvalues=raw["z"][::-1])
    refused("variable z holds 1 z levels, wanted 2..300", "one", zvalues=raw["z"][:1])
    refused("variable z holds 301 z levels, wanted 2..300", "many", zvalues=np.arange(1.0, 302.0))
    for n, (name, _, _, _) in enumerate(ZVARS):               # a level count of any of the four variables that differs from z
        along = jm if name.endswith("east") else im
        refused(f"variable {name} has the dimension lengths (unlimited, {KS_LBRY + 1}, {along}), wanted (records, {KS_LBRY}, {along})", f"lev{n}", levels_of={name: KS_LBRY + 1})
    refused(f"variable salt.south has the dimension lengths (unlimited, {kb}, {im}), wanted (records, {KS_LBRY}, {im})", "sigma_s", levels_of={"salt.south": kb})
    refused(f"variable u.east has the dimension lengths (unlimited, {KS_LBRY}, {jm}), wanted (records, {kb}, {jm})", "zu", levels_of={"u.east": KS_LBRY})   # u, v stay on sigma levels
    count[0] += 1
    sig = fx.write_lbry(tmp / "sigma.lbry.nc", raw_sig)        # a sigma-level file under the setting: no z
    with pytest.raises(PomGpuError):
        g.set_forcing_files(lbry=sig)
    assert "variable z (the z levels) is absent" in status(g)[1] and "sigma.lbry.nc" in status(g)[1]
    g.set_con(error_status=0)
    g.download()
    assert not diff(before, b) and count[0] == 15
    # nothing was registered: the setting is still free; a registered file pins it
    g.set_z_inputs(lbry=False)
    g.set_z_inputs(lbry=True)
    good = write_lbry_z(tmp / "good.lbry.nc", raw)
    g.set_forcing_files(lbry=good)
    with pytest.raises(PomGpuError):
        g.set_z_inputs(lbry=False)
    assert "an lbry file is registered" in status(g)[1] and "z-level" in status(g)[1]
    g.set_con(error_status=0)
    g.set_z_inputs(init=True, clim=True, lbry=True)            # the same value, and the other two settings, stay free
    g.set_z_inputs(lbry=True)
    g.download()
    assert not diff(before, b), diff(before, b)
    # a second registration with a refused file keeps the first one in use: the context steps on with the good file's records
    with pytest.raises(PomGpuError):
        g.set_forcing_files(lbry=write_lbry_z(tmp / "late.lbry.nc", raw, drop=("z",)))
    g.set_con(error_status=0)
    g.close()
    h = PomGpu(before.copy(), libpath=lib)                     # and the other way round: a sigma file pins the setting at 0
    h.set_forcing_files(lbry=sig)
    with pytest.raises(PomGpuError):
        h.set_z_inputs(lbry=True)
    assert "an lbry file is registered" in status(h)[1] and "sigma-level" in status(h)[1]
    h.close()


def tile_window_must_fit(lib, tmp, size=(20, 17, 6)):
    """a tile that claims a north neighbour at the grid's last row: the window point of its east lines does not exist"""
    a, _, _ = ffc.start("seamount", ffc.BASE, 11, size=size)
    raw = raw_lbry_z(a, 3)
    p = write_lbry_z(tmp / "fit.lbry.nc", raw)
    for nb in ("n_north", "n_west"):
        b = a.copy()
        setattr(b, nb, 1)
        g = PomGpu(b, libpath=lib)
        g.run(2)
        g.download()
        before = b.copy()
        g.set_z_inputs(lbry=True)
        with pytest.raises(PomGpuError):
            g.set_forcing_files(lbry=p)
        es, msg = status(g)
        assert es == 1 and "with its window points towards every neighbour does not fit the global grid" in msg and "fit.lbry.nc" in msg, msg
        g.set_con(error_status=0)
        g.download()
        assert not diff(before, b), diff(before, b)
        g.set_z_inputs(lbry=False)                            # nothing was registered
        g.close()


# ---- 6: the fp32 builds ---------------------------------------------------------------------------------------------------------------------
def f32_record_equals_fp64(lib64, lib32, tmp, size=(20, 17, 6)):
    """the lines are doubles in every build: after lateral_bc's first call the b and f lines of tbe sbe tbs sbs hold the fp64 records 1 and 2"""
    a, _, _ = ffc.start("archipelago", ffc.BASE, 1, size=size)
    raw = raw_lbry_z(a, 2)
    want = lateral_records_z(a, raw)
    p = write_lbry_z(tmp / "f32.lbry.nc", raw)
    got = []
    for lib in (lib64, lib32):
        b = a.copy()
        g = PomGpu(b, libpath=lib)
        g.set_z_inputs(lbry=True)
        g.set_forcing_files(lbry=p)
        g.set_con(iint=1)
        g.call("lateral_bc")
        g.download()
        g.close()
        got.append(b)
    for fld, at in (("tbe", 4), ("sbe", 5), ("tbs", 12), ("sbs", 13)):
        for rec, sfx in ((0, "b"), (1, "f")):
            assert same_bits(got[0].field(fld + sfx), want[rec][at]) and same_bits(got[1].field(fld + sfx), want[rec][at]), fld + sfx
        assert not same_bits(want[0][at], want[0][at].astype(np.float32).astype(np.float64))
