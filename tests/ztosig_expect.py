"""TEST HELPER shared by the ztosig tests: the reference's ztosig with splinc / splint (initialize.f:547-667) restated in numpy WITHOUT
the code under test, vectorised over the columns, and the generator of the inputs every ztosig test uses.

The restatement follows the reference line by line: `a**3` is a*a*a, `h**2` is h*h, the literals 0.01, 1.0, 2., 6., 3. and the implicit
REAL(4) `qn` are single-precision constants, and `amax1` is the REAL(4) intrinsic: the neighbour maximum reaches tin(k) rounded to
single precision (:567-569).  tests/test_ztosig_vs_reference.py holds it to the reference's own compiled ztosig_, bit for bit.

Arrays are in the model's numpy order: src (ks, jm, im), h (jm, im), the result (kb, jm, im)."""
import hashlib

import numpy as np

MISSING = np.float64(np.float32(0.01))                       # "tin(k).lt.0.01": the REAL(4) literal, widened for the comparison
SHAPES = [(8, 8, 2, 6), (8, 8, 5, 6), (20, 17, 5, 6), (65, 49, 33, 21), (66, 50, 33, 21), (64, 48, 70, 50)]   # (im, jm, ks, kb)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()[:16]


def neighbour_max(src):
    """amax1 over the four RAW neighbours of every interior column, rounded to single: (ks, jm-2, im-2)"""
    m = np.maximum(np.maximum(src[:, 1:-1, :-2], src[:, 1:-1, 2:]), np.maximum(src[:, :-2, 1:-1], src[:, 2:, 1:-1]))
    with np.errstate(over="ignore"):
        return m.astype(np.float32).astype(np.float64)


def fill_in(zs, src, h):
    """tin of every interior column (:564-572): (ks, jm-2, im-2)"""
    ks = len(zs)
    c, hh, tmax = src[:, 1:-1, 1:-1], h[1:-1, 1:-1], neighbour_max(src)
    tin = np.empty_like(c)
    for k in range(ks):
        v = np.where((zs[k] <= hh) & (c[k] < MISSING), tmax[k], c[k])
        if k:
            v = np.where(v < MISSING, tin[k - 1], v)
        tin[k] = v
    return tin


def splinc(x, y, xnew):
    """splinc(x, y, n, 2.d30, 2.d30, xnew, ynew, m) (:598-638) for many columns: x (n), y (n, ...), xnew (m, ...) -> ynew (m, ...)"""
    n = len(x)
    y2, u = np.zeros_like(y), np.zeros_like(y)
    for i in range(1, n - 1):
        sig = (x[i] - x[i - 1]) / (x[i + 1] - x[i - 1])
        p = sig * y2[i - 1] + 2.0
        y2[i] = (sig - 1.0) / p
        u[i] = (6.0 * ((y[i + 1] - y[i]) / (x[i + 1] - x[i]) - (y[i] - y[i - 1]) / (x[i] - x[i - 1])) / (x[i + 1] - x[i - 1]) - sig * u[i - 1]) / p
    qn, un = 0.0, 0.0
    y2[n - 1] = (un - qn * u[n - 2]) / (qn * y2[n - 2] + 1.0)
    for k in range(n - 2, -1, -1):
        y2[k] = y2[k] * y2[k + 1] + u[k]
    out = np.empty_like(xnew)
    for m in range(len(xnew)):                                # splint (:641-667): the bisection ends at the last klo with xa(klo) <= x
        xv = xnew[m]
        klo = np.clip(np.searchsorted(x, xv, side="right") - 1, 0, n - 2)
        khi = klo + 1
        hh = x[khi] - x[klo]
        a, b = (x[khi] - xv) / hh, (xv - x[klo]) / hh
        ylo, yhi = np.take_along_axis(y, klo[None], 0)[0], np.take_along_axis(y, khi[None], 0)[0]
        y2lo, y2hi = np.take_along_axis(y2, klo[None], 0)[0], np.take_along_axis(y2, khi[None], 0)[0]
        out[m] = a * ylo + b * yhi + ((a * a * a - a) * y2lo + (b * b * b - b) * y2hi) * (hh * hh) / 6.0
    return out


def ztosig(zs, src, zz, h, west=True, east=True, south=True, north=True):
    """the whole routine on one (im, jm) array; west .. north: that edge is physical (n_west == -1 ...).  Without a neighbour's data the
    ghost lines of the other edges keep the zero of `t = 0.` -- a tile's expectation is the single tile's result on its window instead."""
    zs, src, zz, h = (np.ascontiguousarray(a, dtype=np.float64) for a in (zs, src, zz, h))
    kb = len(zz)
    t = np.zeros((kb,) + h.shape)
    hh = h[1:-1, 1:-1]
    zzh = -zz[:, None, None] * hh[None]
    with np.errstate(all="ignore"):
        t[:, 1:-1, 1:-1] = np.where(hh[None] > 1.0, splinc(zs, fill_in(zs, src, h), zzh), 0.0)
    if west:
        t[:, :, 0] = t[:, :, 1]
    if east:
        t[:, :, -1] = t[:, :, -2]
    if south:
        t[:, 0, :] = t[:, 1, :]
    if north:
        t[:, -1, :] = t[:, -2, :]
    return t


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(im, jm, ks, kb, seed=0, salt=False, grid=None, zmax=1000.0):
    """(zs, src, zz, h) with everything the checks want to see (assert_inputs_are_demanding): a temperature-like (salt: salinity-like)
    profile with a quarter of the values missing, zeros below the bottom, and special columns at fixed interior places.  grid = (zz, h): a
    source for a given grid (the file-based checks), whose h and zz are returned as they came"""
    rng = np.random.default_rng(1000 * seed + 7 * im + 3 * jm + ks + (500 if salt else 0))
    zs = 5.0 + np.round((zmax - 5.0) * (np.arange(ks) / (ks - 1.0)) ** 1.5 * 8.0) / 8.0
    if grid is None:
        z = -np.arange(kb) / (kb - 1.0)
        zz = np.empty(kb)
        zz[:-1] = 0.5 * (z[:-1] + z[1:])
        zz[-1] = 2.0 * zz[-2] - zz[-3]
        h = 20.0 + 1380.0 * rng.random((jm, im)) ** 2
        h[rng.random((jm, im)) < 0.06] = 0.75
        h[2, 2], h[2, 3], h[4, 2], h[5, 5], h[1, 1] = 1.0, 0.5, 20.0, 1400.0, 1200.0
        h[1, -2], h[-2, 1], h[-2, -2] = 300.0, 500.0, 800.0     # the columns the corners copy
        hit = [(zs[m] / -zz[k]) for m in range(ks) for k in range(kb) if -zz[k] * (zs[m] / -zz[k]) == zs[m] and zs[m] / -zz[k] > 1.0]
        h[4, 4] = hit[len(hit) // 2]
        h[5, 3] = zs[1]                                       # a bottom exactly on a z level: "zs(k).le.h"
    else:
        zz, h = grid
    prof = (34.0 + 1.5 * (1.0 - np.exp(-zs / 400.0))) if salt else (2.0 + 22.0 * np.exp(-zs / 300.0))
    src = prof[:, None, None] * (1.0 + 0.05 * rng.standard_normal((ks, jm, im)))
    src[zs[:, None, None] > h[None]] = 0.0                    # below the bottom
    deep = rng.random((jm, im)) < 0.3
    src[-1, deep] = prof[-1] * 1.01                           # ... but not everywhere: data below h that is not missing
    miss = rng.random((ks, jm, im)) < 0.25
    src[miss] = rng.choice([0.0, 0.005, -1.0], size=int(miss.sum()))
    src[:, 3, 3] = 0.0                                        # an all-missing column whose level 1 has no valid neighbour
    for j, i in ((3, 2), (3, 4), (2, 3), (4, 3)):
        src[0, j, i] = 0.0
    src[0, 5, 5] = 0.0                                        # a missing level 1 with valid neighbours
    for j, i in ((5, 4), (5, 6), (4, 5), (6, 5)):
        src[0, j, i] = prof[0] * (1.0 + 0.01 * (i + j) / 3.0)
    src[1, 5, 3] = 0.0                                        # missing where zs(k) == h (the generated h), with valid neighbours
    for j, i in ((5, 2), (5, 4), (4, 3), (6, 3)):
        src[1, j, i] = prof[1] * (1.0 + 0.01 * (i + j) / 5.0)
    src[1, 5, 5] = 0.0099999999                               # between the REAL(4) 0.01 and the double 0.01: not missing
    src[:, 1, 1] = prof                                       # a complete column
    if ks >= 5:
        src[1:4, 1, 1] = 0.0                                  # ... with a run of missing levels that h covers
        for j, i in ((1, 0), (1, 2), (0, 1), (2, 1)):
            src[2:4, j, i] = 0.0                              # the run's tail has no valid neighbour: the copy-down chain
    return zs, src, zz, h


def assert_inputs_are_demanding(zs, src, zz, h):
    """what the issue wants the inputs to hold, asserted on the arrays themselves"""
    ks = len(zs)
    c, hh = src[:, 1:-1, 1:-1], h[1:-1, 1:-1]
    wet = (hh > 1.0)[None]
    m = c < MISSING
    cover = zs[:, None, None] <= hh[None]
    m4 = np.maximum(np.maximum(src[:, 1:-1, :-2], src[:, 1:-1, 2:]), np.maximum(src[:, :-2, 1:-1], src[:, 2:, 1:-1]))
    tmax = neighbour_max(src)
    assert (hh <= 1.0).any() and (hh == 1.0).any() and (hh < 1.0).any(), "h <= 1"
    assert (m & cover & wet & (tmax >= MISSING)).any(), "a missing value with a valid neighbour"
    assert (m & cover & wet & (tmax < MISSING)).any(), "a missing value without a valid neighbour"
    assert (m[0] & wet[0]).any(), "a missing level 1"
    assert (m.all(axis=0) & wet[0]).any(), "an all-missing column"
    assert (m & ~cover & wet).any(), "a missing value below h"
    assert (m & wet & (tmax >= MISSING) & (zs[:, None, None] == hh[None])).any(), "a missing value where zs(k) == h"
    assert ((c >= MISSING) & (c < 0.01) & cover & wet).any(), "a value between the single-precision 0.01 and the double one"
    assert (~m & ~cover & wet).any(), "data below h"
    assert (m & cover & wet & (tmax != m4) & (tmax >= MISSING)).any(), "a neighbour maximum that is no single-precision number"
    if ks >= 3:
        tin = fill_in(zs, src, h)
        chain = np.zeros_like(m)
        chain[1:] = m[1:] & ((tmax[1:] < MISSING) | ~cover[1:])
        assert (chain[1:] & chain[:-1] & wet & (tin[1:] >= MISSING)).any(), "a run of missing levels filled from above"
    x = -zz[:, None, None] * hh[None]
    assert zs[0] > 0.0 and (np.diff(zs) > 0).all()
    assert ((x < zs[0]) & wet).any() and ((x > zs[-1]) & wet).any(), "sigma points above zs(1) and below zs(ks)"
    assert (np.isin(x, zs) & wet).any(), "a sigma point on a z level"


def assert_result_is_demanding(t):
    """distinct values on all four edges and corners, a non-zero level kb"""
    kb = t.shape[0]
    e = [t[:, :, 0], t[:, :, -1], t[:, 0, :], t[:, -1, :]]
    assert all(a.any() for a in e) and t[kb - 1].any()
    corners = [t[0, 0, 0], t[0, 0, -1], t[0, -1, 0], t[0, -1, -1]]
    assert len(set(corners)) == 4 and all(corners), corners
    assert not np.array_equal(e[0][:, 1:-1], e[1][:, 1:-1]) and not np.array_equal(e[2][:, 1:-1], e[3][:, 1:-1])
    assert np.isfinite(t).all()
