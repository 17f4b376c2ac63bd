"""TEST HELPER: the three scalar device functions that restate host arithmetic, run through pomgpu_math_probe as the kernels run them.

  divi()         pomgpu_internal.hpp   the correctly rounded quotient from a stored reciprocal      against numpy a / b (IEEE)
  gpow15()       k_adv.hip             glibc 2.35's pow(x, 1.5)                                     against libm pow, and an exact x^1.5
  proft_rad_q()  dd_exp.h              proft's short-wave term, REAL(16) rounded once               against tests/golden/device_math_rad_q.npz

Shared by tests/test_device_math_emulated.py (host build of the kernel sources) and tests/test_gpu_device_math.py (the device): every
check takes the library to load.  Every comparison is on the 64-bit patterns, NaN compared as NaN-ness.  Whole routines on model
fields reach a part of these functions' domains (salinity 30..40 reads well under half of the 128 log-table rows, no radiation term
is subnormal, no numerator is near divi's floor); here the operands are the edges.

What the divi check guards: the reciprocal, the FMAs being real FMAs, denormal handling, the select that keeps a zero numerator's sign,
the compiler flags.  It does NOT show that the second correction step is needed: a divi with one step gives the same bits on every
operand pair below.  Under POMGPU_EMU divi is the plain quotient, so the host build checks only the path to the entry."""
import ctypes
import functools
import importlib.util
import math
import os

import numpy as np

from extpom_amd.cases import make_case
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "device_math_rad_q.npz")
U64 = np.uint64


def golden_maker():
    spec = importlib.util.spec_from_file_location("make_golden_device_math", os.path.join(HERE, "golden", "make_golden_device_math.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(U64)


def not_same_bits(got, want):
    """indices where the 64-bit patterns differ; a NaN equals any NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape
    nan = np.isnan(want)
    return np.flatnonzero((np.isnan(got) != nan) | (~nan & (bits(got) != bits(want))))


def ulps_apart(got, want):
    """distance in units of the last place between non-negative doubles (inf is the neighbour of DBL_MAX); NaN against NaN is 0"""
    nan = np.isnan(want)
    d = np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64))
    d[nan] = np.where(np.isnan(got[nan]), 0, np.iinfo(np.int64).max)
    return d


def show(k, *cols):
    return [tuple(float(c[q]).hex() for c in cols) for q in k[:5]]


_CTX = {}


def context(lib):
    """one small context per library for the probes (the probe touches no mirror)"""
    if lib not in _CTX:
        st = make_case("seamount", 8, 8, 6, dte=6.0, isplit=30)
        _CTX[lib] = PomGpu(st, libpath=lib)
    return _CTX[lib]


# ---- the probe entry itself -----------------------------------------------------------------------------------------------------------
def probe_refusals(lib):
    """an unknown op, a wrong number of inputs, n < 1, n > 2^22 and null pointers are refused with a text and nothing runs; the context
    goes on answering afterwards"""
    g = context(lib)
    one = np.ones(4)
    p = lambda *arrs: (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    out = np.full(4, -7.)
    cases = [((4, 4, p(one), 1, g._p(out)), "op = 4"), ((-1, 4, p(one), 1, g._p(out)), "op = -1"),
             ((0, 4, p(one), 1, g._p(out)), "takes 2"), ((2, 4, p(one, one), 2, g._p(out)), "takes 1"), ((3, 4, p(one, one, one, one), 4, g._p(out)), "takes 5"),
             ((2, 0, p(one), 1, g._p(out)), "n = 0"), ((2, -3, p(one), 1, g._p(out)), "n = -3"), ((2, (1 << 22) + 1, p(one), 1, g._p(out)), "outside 1..2^22"),
             ((2, 4, None, 1, g._p(out)), "must be given"), ((2, 4, p(one), 1, None), "must be given"),
             ((0, 4, (ctypes.c_void_p * 2)(one.ctypes.data, None), 2, g._p(out)), "array 1 is NULL")]
    for args, text in cases:
        rc = g.L.pomgpu_math_probe(g.h, *args)
        assert rc == -1, (args[:2], rc)                       # POMGPU_EINVAL
        assert text in g.L.pomgpu_last_error(g.h).decode(), (text, g.L.pomgpu_last_error(g.h).decode())
    assert np.all(out == -7.)
    try:
        g.math_probe("DIVI", one, np.ones(5))
    except ValueError:
        pass
    else:
        raise AssertionError("arrays of two lengths were taken")
    x = np.array([4., 9., 2.25, 1.])
    assert not not_same_bits(g.math_probe("GPOW15", x), np.array([8., 27., 3.375, 1.])).size
    # one lane, a partial block, more than one block with a partial last one, many blocks
    for n in (1, 255, 257, (1 << 19) - 3):
        a = np.arange(1, n + 1, dtype=np.float64)
        assert not not_same_bits(g.math_probe("DIVI", a, np.full(n, 4.)), a / 4.).size, n


# ---- gpow15 ---------------------------------------------------------------------------------------------------------------------------
LOG_OFF = 0x3fe6955500000000
UNDER_CUT = math.exp(-512. / 1.5)                             # 2^-492.4: below, exp_inline takes specialcase() (1.5 ln x < -512)
SUBNORMAL_CUT = 2. ** (-1022. / 1.5)                          # 2^-681.3: below, x^1.5 is subnormal
# 1 / UNDER_CUT = 2^492.4: above, specialcase() with k > 0; [2^-491, 2^491) is where gpow15 takes the fast path without glibc's tests


@functools.lru_cache(None)
def libm_pow():
    libm = ctypes.CDLL("libm.so.6")
    libm.pow.restype = ctypes.c_double
    libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]
    return libm.pow


def largest_finite_arg():
    """the largest x whose x^1.5 libm keeps finite (about 2^682.67), by bisection on the patterns"""
    pw = libm_pow()
    lo, hi = int(bits(np.array([2. ** 682]))[0]), int(bits(np.array([2. ** 683]))[0])
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if math.isfinite(pw(np.array([mid], U64).view(np.float64)[0], 1.5)):
            lo = mid
        else:
            hi = mid
    return np.array([lo], U64).view(np.float64)[0]


def neighbours(x, n=100):
    c = int(bits(np.array([x]))[0])
    return np.arange(c - n, c + n + 1, dtype=U64).view(np.float64)


@functools.lru_cache(None)
def pow_inputs():
    """{name: x}: every row of both tables, every binade, dens' own range, the values where the algorithm changes path"""
    g = np.random.default_rng(15)
    half, two = int(bits(np.array([.5]))[0]), int(bits(np.array([2.]))[0])
    tables = g.integers(half, two, 1 << 16, dtype=np.uint64).view(np.float64)          # [0.5, 2) with random low bits
    e = np.repeat(np.arange(-1074, 1024), 64)
    binades = np.ldexp(1. + g.random(e.size), e)               # subnormal binades keep the bits they have; 2^-1074 * 1.x may round to 2^-1073
    assert binades.min() > 0. and np.isfinite(binades).all()
    physical = 50. * g.random(1 << 17)
    dbl_max = np.finfo(np.float64).max
    special = np.concatenate([[0., 5e-324, 2. ** -1022, 1., np.nextafter(1., 0.), np.nextafter(1., 2.), dbl_max, np.inf, np.nan],
                              neighbours(UNDER_CUT), neighbours(2. ** -681), neighbours(SUBNORMAL_CUT), neighbours(largest_finite_arg()),
                              neighbours(1. / UNDER_CUT), neighbours(2. ** -491), neighbours(2. ** 491)])
    out = {"tables": tables, "binades": binades, "physical": physical, "special": special}
    assert sum(v.size for v in out.values()) <= 1 << 19
    return out


def table_rows(x):
    """(row of GPOW_LOGTAB, row of GEXP_TAB) gpow15 reads for normal x: the integer steps are gpow15's; the exponent's argument
    1.5 ln x comes from numpy's log here, from the table there, so a row may be the neighbour's at a rounding boundary"""
    tmp = bits(x) - U64(LOG_OFF)
    i = ((tmp >> U64(45)) & U64(127)).astype(np.int64)
    kd = np.rint(1.5 * np.log(x) * (128. / math.log(2.)))
    return i, kd.astype(np.int64) & 127


def pow15_exact(x):
    """the correctly rounded x^1.5 of a finite x > 0 without any libm: x = m 2^e, x^3 = m^3 2^(3e), an integer square root with a
    sticky bit, one rounding (ties to even) to the 53 bits of a normal or the grid of 2^-1074 of a subnormal result"""
    fm, fe = math.frexp(x)
    m, e = int(fm * (1 << 53)), fe - 53
    M, E = m ** 3, 3 * e
    if E & 1:
        M, E = M << 1, E - 1
    sh = max(0, 132 - M.bit_length())
    sh += sh & 1
    M, E = M << sh, E - sh
    r = math.isqrt(M)
    sticky = r * r != M
    q = E // 2                                                # the value is (r + [0, 1)) 2^q, r of 66 bits or more
    lsb = max(r.bit_length() - 1 + q - 52, -1074)             # exponent of the result's last place
    drop = lsb - q
    keep, rem, halfway = r >> drop, r & ((1 << drop) - 1), 1 << (drop - 1)
    if rem > halfway or (rem == halfway and (sticky or keep & 1)):
        keep += 1
    try:
        return math.ldexp(keep, lsb)
    except OverflowError:
        return math.inf


@functools.lru_cache(None)
def pow_references():
    """{name: (libm pow(x, 1.5), the exact x^1.5)}, computed once"""
    pw = libm_pow()
    out = {}
    for name, x in pow_inputs().items():
        a = np.array([pw(v, 1.5) for v in x.tolist()])
        b = np.array([v * v if (v == 0. or math.isinf(v) or v != v) else pow15_exact(v) for v in x.tolist()])
        out[name] = (a, b)
    return out


def pow_inputs_reach_every_table_row():
    x = pow_inputs()["tables"]
    i, j = table_rows(x)
    assert np.bincount(i, minlength=128).min() >= 100 and np.bincount(j, minlength=128).min() >= 100


def pow_libm_is_within_one_ulp_of_exact(name):
    """a check on the exact reference: glibc's pow claims 0.52 ulp"""
    a, b = pow_references()[name]
    d = ulps_apart(a, b)
    assert d.max() <= 1, (name, int(d.max()), show(np.flatnonzero(d > 1), pow_inputs()[name], a, b))


def pow_bits(lib, name):
    """gpow15 is libm's pow(x, 1.5) bit for bit, and within one ulp of the exact value"""
    x = pow_inputs()[name]
    a, b = pow_references()[name]
    got = context(lib).math_probe("GPOW15", x)
    d = ulps_apart(got, b)
    print(f"gpow15 {name}: {x.size} arguments, {not_same_bits(got, a).size} differ from libm, largest distance to the exact value {int(d.max())} ulp")
    k = not_same_bits(got, a)
    assert not k.size, (name, k.size, show(k, x, got, a))
    assert d.max() <= 1, (name, int(d.max()), show(np.flatnonzero(d > 1), x, got, b))


# ---- dens through its own entry -----------------------------------------------------------------------------------------------------
SALT = np.array([0., 1e-320, 1e-300, 1e-250, 1e-160, 1e-100, 1., 35., 1e100, 1e150])


def dens_on_extreme_salinity(lib):
    """rho of pomgpu_dens is the oracle's bit for bit when s holds +-{0 ... 1e150} on water and on land: a garbage power times
    fsm = 0 would leave -0 where the reference leaves +0.  No magnitude above 1e150: sr * sr stays finite, no NaN payload compared"""
    a = make_case("archipelago", 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    assert a.sbias == 0.
    vals = np.concatenate([SALT, -SALT])
    s = a.field("s")
    s[...] = vals[np.arange(s.size) % vals.size].reshape(s.shape)
    wet = np.broadcast_to(a.field("fsm") != 0., s.shape)[: a.kb - 1, : a.jm, : a.im]
    for v in vals:
        here = bits(s[: a.kb - 1, : a.jm, : a.im]) == bits(np.array([v]))[0]
        assert (here & wet).any() and (here & ~wet).any(), v
    a.field("rho")[...] = 7.
    b = a.copy()
    g = PomGpu(b, libpath=lib)
    g.call("dens", "s", "t", "rho")
    g.download()
    g.close()
    o = OracleTile(a)
    o.call("dens", o.a3("s"), o.a3("t"), o.a3("rho"))
    x, y = b.field("rho"), a.field("rho")
    assert np.isfinite(y[: a.kb - 1, : a.jm, : a.im]).all()
    land = y[: a.kb - 1, : a.jm, : a.im][~wet]
    assert (land == 0.).all() and np.signbit(land).any() and (~np.signbit(land)).any()     # both zeros occur on land: the sign is compared
    k = not_same_bits(x.ravel(), y.ravel())
    assert not k.size, (k.size, show(k, s.ravel(), x.ravel(), y.ravel()))


# ---- proft_rad_q ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def rad_fixture():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in ("in", "ntp", "fam", "bits")}


def rad_fixture_is_current():
    """the stored fixture is what the generator makes today: same inputs, same REAL(16) values, the host header in agreement"""
    mk = golden_maker()
    new, old = mk.generate(), rad_fixture()
    for k in ("in", "ntp", "fam", "bits"):
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
        assert np.array_equal(new[k].view(np.uint8), old[k].view(np.uint8)), k


def rad_fixture_holds_what_it_should():
    mk, f = golden_maker(), rad_fixture()
    arr, fam = f["in"], f["fam"]
    count = np.bincount(fam, minlength=len(mk.FAMILIES))
    assert (count[:6] == 4096).all() and (count > 0).all() and os.path.getsize(FIXTURE) < (1 << 20)
    assert np.all((np.abs(arr[:, 0]) >= 1e-6) & (np.abs(arr[:, 0]) <= 1.))
    want = f["bits"].view(np.float64)
    sub = np.abs(want[fam == mk.FAM["SUBNORMAL"]])
    assert ((sub > 0.) & (sub < 2. ** -1022)).sum() > 1000                                # the single-rounding branch
    last = np.abs(want[fam == mk.FAM["LAST_SUBNORMALS"]])
    assert set(np.unique(last / 5e-324)) >= {0., 1.}                                      # the two sides of half the smallest subnormal
    k1, k2 = np.rint(arr[:, 1] / mk.LN2), np.rint(arr[:, 2] / mk.LN2)
    gap = -np.abs(k1 - k2)[fam == mk.FAM["GAPS"]]
    assert (gap < -240).sum() > 100 and ((gap >= -240) & (gap > -244)).sum() > 100 and ((gap > -54) & (gap < -40)).sum() > 100
    assert np.isnan(arr[fam == mk.FAM["NAN_X1"], 1]).all()
    assert (arr[fam == mk.FAM["PLAIN"], 1:].max(axis=1) > 700.).all() and np.nan_to_num(arr[fam != mk.FAM["PLAIN"], 1:], nan=0.).max() <= 700.


def rad_q_bits(lib):
    """proft_rad_q is the REAL(16) expression rounded once, bit for bit; above 700 it is the plain fp64 formula (2 ulp: the
    device's exp is not the host's)"""
    mk, f = golden_maker(), rad_fixture()
    ops = mk.operands(f["in"], f["ntp"])
    got = context(lib).math_probe("RAD_Q", *ops)
    plain = f["fam"] == mk.FAM["PLAIN"]
    want = f["bits"].view(np.float64)
    for k, name in enumerate(mk.FAMILIES):
        if name != "PLAIN":
            print(f"proft_rad_q {name}: {(f['fam'] == k).sum()} arguments, {not_same_bits(got[f['fam'] == k], want[f['fam'] == k]).size} differ")
    sw, r, omr, x1, x2 = (o[plain] for o in ops)
    with np.errstate(over="ignore"):
        formula = sw * (r * np.exp(x1) + omr * np.exp(x2))
    assert np.isfinite(formula).all()
    d = np.abs(bits(got[plain]).astype(np.int64) - bits(formula).astype(np.int64))
    print(f"proft_rad_q PLAIN: {plain.sum()} arguments, largest distance to the fp64 formula {int(d.max())} ulp")
    k = not_same_bits(got[~plain], want[~plain])
    assert not k.size, (k.size, [mk.FAMILIES[q] for q in np.unique(f["fam"][~plain][k])], show(k, ops[3][~plain], ops[4][~plain], got[~plain], want[~plain]))
    assert d.max() <= 2, int(d.max())


# ---- divi -----------------------------------------------------------------------------------------------------------------------------
MANTISSAS = ["random", "below_two", "above_one", "bits20"]
N_DIVI = 1 << 18


def mantissa(g, kind, n, p):
    """n significands in [1, 2) of p bits: random; all ones to within 64 units of the last place below 2; within 64 above 1; 20
    significant bits"""
    u = 2. ** (1 - p)
    if kind == "random":
        return 1. + g.integers(0, 1 << (p - 1), n).astype(np.float64) * u
    if kind == "below_two":
        return 2. - g.integers(1, 65, n).astype(np.float64) * u
    if kind == "above_one":
        return 1. + g.integers(0, 65, n).astype(np.float64) * u
    return 1. + g.integers(0, 1 << 19, n).astype(np.float64) * 2. ** -19


def sign(g, n):
    return np.where(g.random(n) < .5, -1., 1.)


@functools.lru_cache(None)
def divi_operands(p):
    """(a, b) as float64, N_DIVI pairs for the precision p = 53 or 24.  b: every mantissa family, |b| in 2^+-100 (2^+-20).  a: free (every
    family, |a| in 2^+-900 (2^+-60)); RN(b q) for a constructed q of every family, displaced by -2 .. +2 units of its last place; +-0"""
    g = np.random.default_rng(53 + p)
    ft = np.float64 if p == 53 else np.float32
    eb, ea = (100, 899) if p == 53 else (20, 59)
    A, B = [], []
    for fb in MANTISSAS:
        for fa in MANTISSAS:
            n = 4096                                          # free numerators
            B.append(sign(g, n) * np.ldexp(mantissa(g, fb, n, p), g.integers(-eb, eb, n)))
            A.append(sign(g, n) * np.ldexp(mantissa(g, fa, n, p), g.integers(-ea, ea + 1, n)))
            n = 2048 * 5                                      # a = RN(b q) and its neighbours
            b = (sign(g, n) * np.ldexp(mantissa(g, fb, n, p), g.integers(-eb, eb, n))).astype(ft)
            e = g.integers(-ea + 1, ea - 1, n)                # the exponent of a, to within the carry of the product
            q = (sign(g, n) * mantissa(g, fa, n, p)).astype(ft)
            a = (b * q).astype(ft)                            # one rounding in the type (the product of two floats is exact in fp64)
            a = np.ldexp(a, (e - np.frexp(a)[1]).astype(np.int32)).astype(ft)
            d = np.tile(np.arange(-2, 3), n // 5)
            ai = a.view(np.int64 if p == 53 else np.int32)
            a = (ai + d.astype(ai.dtype)).view(ft)            # d units of the last place further from zero
            B.append(b.astype(np.float64))
            A.append(a.astype(np.float64))
        n = 8192                                              # zero numerators of both signs over divisors of both signs
        B.append(np.tile([1., 1., -1., -1.], n // 4) * np.ldexp(mantissa(g, fb, n, p), g.integers(-eb, eb, n)))
        A.append(np.tile([0., -0., 0., -0.], n // 4))
    a, b = np.concatenate(A), np.concatenate(B)
    assert a.size == N_DIVI and np.isfinite(a).all() and np.isfinite(b).all()
    assert np.array_equal(a.astype(ft).astype(np.float64), a) and np.array_equal(b.astype(ft).astype(np.float64), b)
    lo, hi = (2. ** -100, 2. ** 100) if p == 53 else (2. ** -20, 2. ** 20)
    assert (np.abs(b) >= lo).all() and (np.abs(b) <= hi).all()
    lo, hi = (2. ** -900, 2. ** 900) if p == 53 else (2. ** -60, 2. ** 60)
    assert ((a == 0.) | ((np.abs(a) >= lo) & (np.abs(a) <= hi))).all()
    return a, b


FLOOR_LO, FLOOR_HI = 2. ** -968, 2. ** -960                  # the documented floor of divi's numerators (pomgpu_internal.hpp)


@functools.lru_cache(None)
def divi_floor_operands():
    """|a| in [2^-968, 2^-960] over b in [1, 2): the residual a - b q is a multiple of 2^-1073 or more and still exact"""
    g = np.random.default_rng(968)
    n = 1 << 16
    A, B = [], []
    for fb in MANTISSAS:
        for fa in MANTISSAS:
            B.append(sign(g, n // 16) * mantissa(g, fb, n // 16, 53))
            A.append(sign(g, n // 16) * np.ldexp(mantissa(g, fa, n // 16, 53), g.integers(-968, -960, n // 16)))
    a, b = np.concatenate(A), np.concatenate(B)
    a[:4] = [FLOOR_LO, -FLOOR_LO, FLOOR_HI, np.nextafter(FLOOR_LO, 1.)]
    assert (np.abs(a) >= FLOOR_LO).all() and (np.abs(a) <= FLOOR_HI).all()
    return a, b


def divi_bits(lib, op):
    p = 53 if op == "DIVI" else 24
    a, b = divi_operands(p)
    with np.errstate(all="ignore"):
        want = a / b if p == 53 else (a.astype(np.float32) / b.astype(np.float32)).astype(np.float64)
    assert np.isfinite(want).all() and (want[a == 0.] == 0.).all() and np.signbit(want[a == 0.]).sum() * 2 == (a == 0.).sum()
    if p == 24:
        assert (np.abs(want[a != 0.]) >= 2. ** -126).all()
    got = context(lib).math_probe(op, a, b)
    k = not_same_bits(got, want)
    print(f"{op}: {a.size} pairs, {k.size} quotients differ from a / b")
    assert not k.size, (op, k.size, show(k, a, b, got, want))


def divi_floor_bits(lib):
    a, b = divi_floor_operands()
    got = context(lib).math_probe("DIVI", a, b)
    k = not_same_bits(got, a / b)
    print(f"DIVI at the floor: {a.size} pairs, {k.size} quotients differ from a / b")
    assert not k.size, (k.size, show(k, a, b, got, a / b))
