"""TEST HELPER shared by tests/water_checks.py (and through it tests/test_water_emulated.py, tests/test_gpu_water.py): what the reference's
`water` (bounds_forcing.f:986-1020) and read_water_pnetcdf (io_pnetcdf.F:3227-3272) would deliver, built on the CPU WITHOUT the code under
test, and `surface` (bounds_forcing.f:963-983) with its line 979 uncommented.

Three parts: (1) seeded raw fields of the global grid, every value representable in float32 so that an NC_FLOAT and an NC_DOUBLE file hold
the same numbers; (2) the writer of <prefix>.water.NNNN.nc with scipy.io.netcdf_file in every form the library accepts and some it must
refuse; (3) a numpy restatement, statement for statement, of `water`'s schedule and interpolation.  numpy's float64 operations are IEEE
and uncontracted, as the flang build's are.  The reference's own `water_` cannot be the bar: read_water_pnetcdf_ is a trap in
oracle/ref_traps.c."""
import numpy as np
from scipy.io import netcdf_file

from forcing_expect import f32, window

TWATER = 1.                                                   # "twater=1." (days)


def name(prefix, n):
    """'(a,''in/'',a,''.water.'',i4.4,''.nc'')' with prefix = <wrk_pth>in/<netcdf_file>"""
    return "%s.water.%04d.nc" % (prefix, n)


# ---- (1) raw fields of the GLOBAL grid -----------------------------------------------------------------------------------------------
def raw_water(g, numbers, seed=14):
    """{n: (jm, im)}: a fresh-water flux in m/s (evaporation minus precipitation, a few mm/day... scaled up so that three steps move S
    well beyond rounding); no mask applied"""
    rng = np.random.default_rng(seed)
    return {n: f32(2.e-6 * rng.standard_normal((g.jm, g.im)) + 1.e-6 * (n + 1)) for n in numbers}


# ---- (2) the files -------------------------------------------------------------------------------------------------------------------
def write_water(prefix, n, field, version=2, dtype="d", odd=False, drop=False, transpose=False, extra_col=False):
    """one record's file.  version: 1 = CDF-1, 2 = CDF-2; dtype "d" / "f"; odd: `w` between other variables (a record variable among
    them) with attributes and other dimension names; drop / transpose / extra_col break the file on purpose"""
    path = name(prefix, n)
    a = np.asarray(field)
    if transpose:
        a = np.ascontiguousarray(a.T)
    if extra_col:
        a = np.concatenate([a, a[:, -1:]], axis=1)
    with netcdf_file(path, "w", version=version) as f:
        if odd:
            f.history = "written by a test"
            f.createDimension("rec", None)
            f.createDimension("spare", 3)
            x = f.createVariable("extra_first", "d", ("spare",))
            x[:] = [1.0, 2.0, 3.0]
            r = f.createVariable("extra_record", "h", ("rec", "spare"))
            r[:] = np.arange(6, dtype=np.int16).reshape(2, 3)
        f.createDimension("eta" if odd else "y", a.shape[0])
        f.createDimension("xi" if odd else "x", a.shape[1])
        if not drop:
            v = f.createVariable("w", dtype, ("eta", "xi") if odd else ("y", "x"))
            v[:] = a
            if odd:
                v.units = "m s-1"
        else:
            v = f.createVariable("water", dtype, ("y", "x"))
            v[:] = a
        if odd:
            e = f.createVariable("extra_last", "i", ("spare",))
            e[:] = [7, 8, 9]
    return path


def write_all(prefix, raw, **kw):
    return [write_water(prefix, n, a, **kw) for n, a in sorted(raw.items())]


# ---- (3) the schedule and the interpolation ------------------------------------------------------------------------------------------
def records(st, raw):
    """st.water_records: what read_water_pnetcdf(n, wat) delivers to this tile -- its window, nothing converted, nothing tapered"""
    return {n: np.ascontiguousarray(window(st, a)) for n, a in raw.items()}


def get_time(st, iint):
    """advance.f:62-75: time=dti*float(iint)/86400.d0+time0"""
    return float(st.dti) * float(np.float32(iint)) / 86400. + float(st.time0)


def iwater_of(st):
    return int(TWATER * 86400. / float(st.dti))


def water(st, iint, recs):
    """`water` at step iint on st's wssurfb, wssurff, wssurf (in place), records from recs (KeyError: the reader would have stopped).
    Returns (time, fnew, the record numbers read)."""
    im, jm = st.im, st.jm
    A = (slice(0, jm), slice(0, im))
    iwater = iwater_of(st)
    time = get_time(st, iint)
    read = []
    if iint == 1:                                             # :998
        st.wssurff[A] = recs[iint // iwater]
        read.append(iint // iwater)
    if iint == 1 or iint % iwater == 0:                       # :1000-1007
        st.wssurfb[A] = st.wssurff[A]
        st.wssurff[A] = recs[(iint + iwater) // iwater]
        read.append((iint + iwater) // iwater)
    ntime = int(time / TWATER)                                # :1010-1012
    fnew = time / TWATER - ntime
    fold = 1. - fnew
    st.wssurf[A] = fold * st.wssurfb[A] + fnew * st.wssurff[A]
    return time, fnew, read


def surface_sss(st, iint, sss_records):
    """bounds_forcing.f:976-980 with :979 uncommented: ssurf(1:im,1:jm) = sss of record (iint+cont_bry)/isrf+1 (1-based list)"""
    cb = int(st.cont_bry)
    isrf = int(.125 * 86400. / float(st.dti))
    if iint == 1 or (iint + cb) % isrf == 0:
        st.ssurf[:st.jm, :st.im] = sss_records[(iint + cb) // isrf]   # record n is list item n - 1
        return (iint + cb) // isrf + 1
    return None
