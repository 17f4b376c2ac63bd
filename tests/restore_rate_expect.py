"""TEST HELPER shared by the restore-rate tests: the generator of sponge-like rates, what the library is to make of a rate file -- ztosig of
tests/ztosig_expect.py (held to the reference's compiled ztosig_) on the file's GLOBAL field -- and restore_interior
(bounds_forcing.f:1023-1121) restated in numpy WITHOUT the code under test, with the rate calls the reference keeps commented
(:1049-1051, :1076-1079) restored: after "taurstrf = 1./trst" the rate that goes with T/S record n lands on taurstrf(1:im,1:jm,1:kb).
tests/test_restore_rate_emulated.py holds the restatement to the oracle's pomo_restore_interior where the rate is uniformly 1/30.

Arrays are in the model's numpy order: a rate on z levels (ks, jm, im), a mapped rate (kb, jm, im)."""
import numpy as np

import ztosig_expect as Z
from ztosig_expect import MISSING, digest, same_bits          # noqa: F401

TRST = 30.0
# (im, jm, ks, kb) of the inputs the reference's ztosig_ is pinned on (tests/golden/restore_rate.json); the last one is the map-only input
# with a negative mapped value
SHAPES = [(8, 8, 2, 6), (8, 8, 5, 6), (20, 17, 5, 6), (65, 49, 33, 21)]
EFOLD = 0.15                                                 # of the grid


def levels(ks, zmax):
    return 5.0 + np.round((zmax - 5.0) * (np.arange(ks) / (ks - 1.0)) ** 1.5 * 8.0) / 8.0


def sponge(im, jm, zs, record=0, steep=False):
    """a plain exponential sponge on the levels zs: strongest on the four edges (each with its own strength, so the corners differ), e-folding
    EFOLD of the grid, zero beyond three e-foldings; linear in depth, so that the natural spline has nothing to undershoot on -- steep: gone
    below the upper levels instead, which it does undershoot on.  Records differ by a factor.  At fixed interior places (as
    ztosig_expect.make_inputs plants its special columns): an all-small column whose level 1 has no valid neighbour, and an exact 1/30."""
    x, y = np.arange(im) / (im - 1.0), np.arange(jm) / (jm - 1.0)

    def side(d, amp):
        e = amp * np.exp(-d / EFOLD)
        e[d > 3.0 * EFOLD] = 0.0
        return e

    r2 = (side(x, 0.15) + side(1.0 - x, 0.12))[None, :] + (side(y, 0.09) + side(1.0 - y, 0.075))[:, None]
    if steep:
        upper = (zs <= zs[len(zs) // 4])[:, None, None]         # ... and a small valid rate below: a step the fill-in leaves alone
        r = np.where(upper, 8.0 * r2[None], 0.0125 * (r2 > 0.0)[None])
    else:
        r = (1.0 - 0.5 * zs / zs[-1])[:, None, None] * r2[None]
    r = r * (1.0 + 0.125 * record)
    r[:, 3, 3] = 0.0
    for j, i in ((3, 2), (3, 4), (2, 3), (4, 3)):
        r[0, j, i] = 0.0
    r[0, 5, 5] = 1.0 / TRST
    return r


def make_rate(im, jm, ks, kb, grid=None, record=0, steep=False):
    """(zs, rate, zz, h): a sponge for a given grid = (zz, h) (default: ztosig_expect.make_inputs's own); the levels reach below the deepest
    column, so nothing but level kb is extrapolated"""
    if grid is None:
        _, _, zz, h = Z.make_inputs(im, jm, ks, kb)
    else:
        zz, h = grid
    zs = levels(ks, 1.0625 * float(np.max(h)))
    return zs, sponge(im, jm, zs, record, steep), zz, h


def assert_rates_are_demanding(zs, rate, h, natural=False):
    """what the issue wants the rate inputs to hold, asserted on the arrays themselves; natural: the sponge has them away from the planted
    places too (its edge, and the middle its three e-foldings do not reach)"""
    c, hh = rate[:, 1:-1, 1:-1], h[1:-1, 1:-1]
    wet, cover, m, tmax = (hh > 1.0)[None], zs[:, None, None] <= hh[None], c < MISSING, Z.neighbour_max(rate)
    a, b, col = m & cover & wet & (tmax >= MISSING), m & cover & wet & (tmax < MISSING), m.all(axis=0) & wet[0]
    assert a.any(), "a covered value below MISSING with a valid neighbour"
    assert b.any(), "a covered value below MISSING without a valid neighbour"
    assert col.any(), "an all-small column"
    assert (rate == 1.0 / TRST).any() or (rate == np.float64(np.float32(1.0 / TRST))).any(), "an exact 1/30 (an NC_FLOAT file holds it rounded)"
    assert (c >= MISSING).any() and (rate >= 0.0).all()
    if natural:
        for q in (a, b):
            q = q.copy()
            q[:, 1:4, 1:4] = False                              # the planted places: (3,3) and its neighbours, interior indices 1..3
            assert q.any()
        col = col.copy()
        col[2, 2] = False
        assert col.any()


def assert_mapped_is_demanding(t):
    kb = t.shape[0]
    assert t[kb - 1].any(), "a non-zero level kb"
    corners = [t[0, 0, 0], t[0, 0, -1], t[0, -1, 0], t[0, -1, -1]]
    assert len(set(corners)) == 4 and all(corners), corners
    assert np.isfinite(t).all()


def mapped(zs, rate, zz, h):
    """what a rate file's record becomes: ztosig on the global field, all kb levels"""
    return Z.ztosig(zs, rate, zz, h)


def cut(tile, a):
    return np.ascontiguousarray(a[..., tile.j_off:tile.j_off + tile.jm, tile.i_off:tile.i_off + tile.im])


# ---- restore_interior with the rate calls restored ------------------------------------------------------------------------------------
def restore_interior(st, ts_records, rate_of=None):
    """one call of restore_interior on the PomState st (in place) for its iint, time, dti, iend.  ts_records[n-1] = (tr, sr) of record n,
    (kb, jm, im); rate_of(n): the rate that goes with record n, (kb, jm, im) on the sigma levels, or None for the reference's 1/trst"""
    im, jm, kb = st.im, st.jm, st.kb
    F = st.field
    dti, time, iint, iend = float(st.dti), float(st.time), int(st.iint), int(st.iend)
    irst = int(TRST * 86400.0 / dti)
    ntime = int(time / TRST)

    def load(n):
        tr, sr = ts_records[n - 1]
        F("trstrf")[:, :jm, :im] = tr                           # :1041-1042, :1062-1063
        F("srstrf")[:, :jm, :im] = sr
        F("taurstrf")[...] = 1.0 / TRST                         # :1043, :1065: the whole array
        r = rate_of(n) if rate_of is not None else None
        if r is not None:
            F("taurstrf")[:, :jm, :im] = r                      # :1049-1051, :1076-1079: read_restore_tau_interior + ztosig onto taurstrf

    if iint == 2:
        load(iint // irst + 1)
    if iint == 2 or iint % irst == 0:
        for n in ("trstr", "srstr", "taurstr"):
            F(n + "b")[:kb - 1, :jm, :im] = F(n + "f")[:kb - 1, :jm, :im]
        if iint != iend:
            load((iint + irst) // irst + 1)
    fnew = time / TRST - ntime
    fold = 1.0 - fnew
    I = (slice(0, kb - 1), slice(0, jm), slice(0, im))
    for n in ("trstr", "srstr", "taurstr"):
        F(n)[I] = fold * F(n + "b")[I] + fnew * F(n + "f")[I]
    c = 2.0 * dti / 86400.0
    for n, r in (("t", "trstr"), ("tb", "trstr"), ("s", "srstr"), ("sb", "srstr")):
        F(n)[I] = F(n)[I] + c * F("taurstr")[I] * (F(r)[I] - F(n)[I])
    for n in ("t", "tb", "s", "sb"):
        F(n)[:kb - 1] = F(n)[:kb - 1] * F("fsm")[None]
