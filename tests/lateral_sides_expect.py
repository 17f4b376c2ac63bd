"""TEST HELPER shared by tests/lateral_sides_checks.py (and through it the tests of pomgpu_set_lateral_sides): what a lateral reader that
feeds any of the four open boundaries delivers, built on the CPU WITHOUT the code under test.

It extends tests/forcing_expect.py's raw_lbry / write_file / lateral_records and tests/ztosig_line_files_checks.py's raw_lbry_z /
write_lbry_z / lateral_records_z to a mask of sides (east 1, south 2, west 4, north 8 -- bit n is the edge number of pomgpu_ztosig_line):
  a side that is ON   its elevation line is the tile's piece of zeta.<side> over 1:jm / 1:im (untouched beyond), its four (., kb) arrays the
                      tile's pieces of temp salt u v, zero beyond jm / im (read_boundary_conditions_pnetcdf, io_pnetcdf.F:3426-3604, and its
                      commented look-ups for west and north, :3458-3463, :3474-3479, :3491-3498)
  a side that is OFF  t s are the line of tclim sclim next to it -- i = 1, i = im, j = 1, j = jm of the TILE (:3606-3614; east and south:
                      the commented :3607-3608, :3612-3613) --, u v zero, the elevation line as the state holds it
The east / south numbers are forcing_expect's own (same seed), so a four-sided file holds the two-sided file's .east / .south variables."""
import numpy as np
from scipy.io import netcdf_file

import forcing_expect as fx
import ztosig_line_expect as ZL
import ztosig_line_files_checks as zlf

EAST, SOUTH, WEST, NORTH = 1, 2, 4, 8
SIDES = ("east", "south", "west", "north")                    # bit n of the mask; n is the edge number of the line form of ztosig
LETTER = {"east": "e", "south": "s", "west": "w", "north": "n"}
ORDER16 = ("tbw", "sbw", "ubw", "vbw", "tbe", "sbe", "ube", "vbe", "tbn", "sbn", "vbn", "ubn", "tbs", "sbs", "vbs", "ubs")   # extpom_amd.cases.LATERAL_ORDER
ELEV = {"west": 16, "east": 17, "north": 18, "south": 19}     # the elevation lines' places in LATERAL_ORDER
VARS = ("zeta", "u", "v", "temp", "salt")


def on(mask, side):
    return bool(mask >> SIDES.index(side) & 1)


def along_j(side):
    return side in ("east", "west")


def names(mask):
    """the variables a file of the ON sides holds, <var>.<side>"""
    return tuple(f"{v}.{s}" for s in SIDES if on(mask, s) for v in VARS)


def place(side, var):
    """where temp / salt / u / v of a side lies in LATERAL_ORDER"""
    return ORDER16.index({"temp": "t", "salt": "s", "u": "u", "v": "v"}[var] + "b" + LETTER[side])


# ---- raw fields of the GLOBAL grid --------------------------------------------------------------------------------------------------
def raw_lbry(g, nrec, seed=12):
    """forcing_expect.raw_lbry (its .east / .south numbers unchanged) with the .west and .north variables beside them, float32 numbers"""
    out = fx.raw_lbry(g, nrec, seed=seed)
    rng = np.random.default_rng(seed + 100)
    kb, jm, im = g.kb, g.jm, g.im
    out["zeta.west"] = fx.f32(0.02 * rng.standard_normal((nrec, jm)))
    out["zeta.north"] = fx.f32(0.02 * rng.standard_normal((nrec, im)))
    for side, n in (("west", jm), ("north", im)):
        t0 = g.tbw[:, :jm] if side == "west" else g.tbn[:, :im]
        s0 = g.sbw[:, :jm] if side == "west" else g.sbn[:, :im]
        out["u." + side] = fx.f32(0.05 * rng.standard_normal((nrec, kb, n)))
        out["v." + side] = fx.f32(0.05 * rng.standard_normal((nrec, kb, n)))
        out["temp." + side] = fx.f32(t0[None] + 0.05 * rng.standard_normal((nrec, kb, n)))
        out["salt." + side] = fx.f32(s0[None] + 0.01 * rng.standard_normal((nrec, kb, n)))
    return out


def zvars(mask):
    """(name, edge, S-like, place in LATERAL_ORDER) of the z-level variables of the ON sides"""
    return tuple((f"{v}.{s}", SIDES.index(s), v == "salt", place(s, v)) for s in SIDES if on(mask, s) for v in ("temp", "salt"))


def raw_lbry_z(g, nrec, ks=zlf.KS_LBRY, kind="d", seed=14):
    """raw_lbry with temp / salt of all four sides on ks z levels: ztosig_line_files_checks.raw_lbry_z's .east / .south lines and `z`, and
    .west / .north lines made the same way for their own depth lines (h(2,j), h(i,jmm1))"""
    raw = raw_lbry(g, nrec)
    two = zlf.raw_lbry_z(g, nrec, ks=ks, kind=kind, seed=seed)
    for name, _, _, _ in zlf.ZVARS:
        raw[name] = two[name]
    raw["z"] = two["z"]
    rng = np.random.default_rng(seed + 100)
    zs = zlf.levels(ks, float(g.h.max()))
    hh = g.h[:g.jm, :g.im]
    for name, edge, salt, _ in zvars(WEST | NORTH):
        hl = ZL.depth_line(hh, edge)
        lines = []
        for r in range(nrec):
            _, ln = ZL.random_line(zs, hl, rng, salt)
            ln[0, 1], ln[0, -2] = 0.0, 0.005
            lines.append(ln)
        a = np.stack(lines)
        raw[name] = fx.f32(a) if kind == "f" else a
    return raw


# ---- the files ------------------------------------------------------------------------------------------------------------------------
def write_lbry(path, raw, mask, **kw):
    """a sigma-level lbry file that holds the variables of the ON sides ONLY (forcing_expect.write_file's layouts and breakages)"""
    return fx.write_file(path, raw, names(mask), **kw)


def write_lbry_z(path, raw, mask, kind="d", version=2, drop=(), levels_of=None, length_of=None):
    """a z-level lbry file of the ON sides: `z`, temp / salt as (time, z, y | x), zeta u v as ever.  drop / levels_of ({name: level count})
    / length_of ({name: line length}) break the file on purpose"""
    path = str(path)
    z = raw["z"]
    with netcdf_file(path, "w", version=version) as nc:
        nc.createDimension("time", None)
        made = {}

        def dim(hint, n):
            if (hint, n) not in made:
                made[(hint, n)] = f"{hint}{n}"
                nc.createDimension(made[(hint, n)], n)
            return made[(hint, n)]

        if "z" not in drop:
            nc.createVariable("z", kind, (dim("z", len(z)),))[:] = z
        for n in names(mask):
            if n in drop:
                continue
            a = raw[n]
            if levels_of and n in levels_of:
                a = np.resize(a, (a.shape[0], levels_of[n], a.shape[2]))
            if length_of and n in length_of:
                a = np.resize(a, a.shape[:-1] + (length_of[n],))
            hint = "y" if along_j(n.split(".")[1]) else "x"
            dims = ("time", dim(hint, a.shape[-1])) if a.ndim == 2 else ("time", dim("z" if a.shape[1] == len(z) else "s", a.shape[1]), dim(hint, a.shape[-1]))
            nc.createVariable(n, kind, dims)[:] = a
    return path


# ---- what the reader delivers to one tile -----------------------------------------------------------------------------------------------
def clim_line(st, a, side):
    """the line of tclim / sclim (kb, jm_local, im_local) next to a side of the TILE: (kb, jm) or (kb, im)"""
    im, jm = st.im, st.jm
    return {"west": a[:, :jm, 0], "east": a[:, :jm, im - 1], "south": a[:, 0, :im], "north": a[:, jm - 1, :im]}[side]


def lateral_records(st, raw, mask, nrec=None, round32=False):
    """st.lateral_records (the 20 arrays of extpom_amd.cases.LATERAL_ORDER) under a mask of sides; round32: tclim, sclim as the fp32-storage
    builds keep them"""
    some = next(n for n in names(mask))
    nrec = raw[some].shape[0] if nrec is None else nrec
    tclim, sclim = (fx.f32(st.tclim), fx.f32(st.sclim)) if round32 else (st.tclim, st.sclim)
    out = []
    for r in range(nrec):
        rec = [np.zeros_like(st.field(n)) for n in ORDER16] + [st.elw.copy(), st.ele.copy(), st.eln.copy(), st.els.copy()]
        for side in SIDES:
            off, n = (st.j_off, st.jm) if along_j(side) else (st.i_off, st.im)
            if on(mask, side):
                for var in ("temp", "salt", "u", "v"):
                    rec[place(side, var)][:, :n] = raw[f"{var}.{side}"][r][:, off:off + n]
                rec[ELEV[side]][:n] = raw[f"zeta.{side}"][r][off:off + n]
            else:
                rec[place(side, "temp")][:, :n] = clim_line(st, tclim, side)
                rec[place(side, "salt")][:, :n] = clim_line(st, sclim, side)
        out.append([np.ascontiguousarray(a) for a in rec])
    return out


def lateral_records_z(st, raw, mask, nrec=None, round32=False):
    """lateral_records with temp / salt of every ON side mapped from its z-level line by tests/ztosig_line_expect.py: the tile's piece of the
    line with one window point towards every neighbour, the tile's own depth line for that edge, a copied end only where the tile has no
    neighbour; zero beyond jm / im"""
    some = next(n for n in names(mask))
    nrec = raw[some].shape[0] if nrec is None else nrec
    sig = dict(raw)
    for name, _, _, _ in zvars(mask):
        sig[name] = np.zeros((raw[name].shape[0], st.kb, raw[name].shape[2]))
    recs = lateral_records(st, sig, mask, nrec, round32=round32)
    hh = st.h[:st.jm, :st.im]
    for r, rec in enumerate(recs):
        for name, edge, _, at in zvars(mask):
            aj = ZL.along_j(edge)
            off, n = (st.j_off, st.jm) if aj else (st.i_off, st.im)
            lo, hi = (st.n_south, st.n_north) if aj else (st.n_west, st.n_east)
            t = ZL.ztosig_line(raw["z"], ZL.window_of(raw[name][r], off, n), st.zz[:st.kb], ZL.depth_line(hh, edge), edge, lo == -1, hi == -1)
            out = np.zeros_like(rec[at])
            out[:, :n] = t
            rec[at] = out
    return recs
