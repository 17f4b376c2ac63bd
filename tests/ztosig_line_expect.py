"""TEST HELPER shared by the tests of the line form of ztosig (pomgpu_ztosig_line, pomgpu_set_z_lateral): the reference's commented blocks
behind read_boundary_conditions_pnetcdf (bounds_forcing.f:636-716) restated in numpy WITHOUT the code under test, and the generator of the
inputs every such test uses.

The block spreads a line across the tile -- ts1(i,j,k) = t_e(j,k), hs(i,j) = h(imm1,j) --, calls ztosig and keeps ts2(im/2, j, k).  Here
the line is mapped as a line: each point is one ztosig column (tests/ztosig_expect.py's splinc, the fill-in restated for a source that
does not vary across the line).  tests/test_ztosig_line_vs_reference.py builds the replicated 3-D source as the block does, calls the
reference's own compiled ztosig_ and holds this restatement to the sampled column / row, bit for bit.

Arrays are in the model's numpy order: a line source is (ks, n) or, with its two window points, (ks, n + 2); the result is (kb, n)."""
import numpy as np

import ztosig_expect as Z
from ztosig_expect import MISSING, digest, same_bits  # noqa: F401

EDGES = ("east", "south", "west", "north")                    # the edge argument of pomgpu_ztosig_line: 0 .. 3
SHAPES = [(8, 8, 2, 6), (8, 8, 5, 6), (20, 17, 5, 6), (65, 49, 33, 21), (64, 48, 70, 50)]   # (im, jm, ks, kb)


def along_j(edge):
    return edge in (0, 2)


def depth_line(h, edge):
    """hs of the block, as a line: h(imm1,j), h(i,2), h(2,j), h(i,jmm1) of h (jm, im)"""
    return np.array((h[:, -2], h[1, :], h[:, 1], h[-2, :])[edge], dtype=np.float64)


def neighbour_max(own, prev, nxt, edge):
    """amax1(tb(i-1,j,k), tb(i+1,j,k), tb(i,j-1,k), tb(i,j+1,k)) of the replicated source, rounded to single: along j the first two are
    the point's own raw value, along i the last two"""
    m = np.maximum(np.maximum(own, own), np.maximum(prev, nxt)) if along_j(edge) else np.maximum(np.maximum(prev, nxt), np.maximum(own, own))
    with np.errstate(over="ignore"):
        return m.astype(np.float32).astype(np.float64)


def fill_in(zs, srcw, hl, edge):
    """tin of every line point (initialize.f:564-572) from the RAW source with its window points: srcw (ks, n + 2) -> (ks, n)"""
    own, tmax = srcw[:, 1:-1], neighbour_max(srcw[:, 1:-1], srcw[:, :-2], srcw[:, 2:], edge)
    tin = np.empty_like(own)
    for k in range(len(zs)):
        v = np.where((zs[k] <= hl) & (own[k] < MISSING), tmax[k], own[k])
        if k:
            v = np.where(v < MISSING, tin[k - 1], v)
        tin[k] = v
    return tin


def ztosig_line(zs, srcw, zz, hl, edge, lo_physical=True, hi_physical=True):
    """one line: srcw (ks, n + 2) with the window points beyond both ends (ignored at a physical end), hl (n) -> (kb, n).  A physical
    end takes the finished value of the point next to it (initialize.f:589-592); an end towards a neighbour is the owner's column, formed
    from the window point (what the exchange of :586 brings)"""
    zs, srcw, zz, hl = (np.ascontiguousarray(a, dtype=np.float64) for a in (zs, srcw, zz, hl))
    zzh = -zz[:, None] * hl[None]
    with np.errstate(all="ignore"):
        t = np.where(hl[None] > 1.0, Z.splinc(zs, fill_in(zs, srcw, hl, edge), zzh), 0.0)
    if lo_physical:
        t[:, 0] = t[:, 1]
    if hi_physical:
        t[:, -1] = t[:, -2]
    return t


def with_window(line, lo=7.75, hi=7.75):
    """(ks, n) -> (ks, n + 2): a line with two window points that a physical end must not read (a valid-looking value that would win every maximum)"""
    ks = line.shape[0]
    return np.concatenate([np.full((ks, 1), lo * 1000.0), line, np.full((ks, 1), hi * 1000.0)], axis=1)


def window_of(gline, first, n):
    """the points first .. first+n-1 (0-based) of a global line with one more point on either side; beyond the global line: with_window's value"""
    return with_window(gline)[:, first:first + n + 2].copy()


def random_line(zs, hl, rng, salt=False):
    """(profile, a line (ks, n) for the depths hl): a temperature-like (salt: salinity-like) profile with noise, zeros below the bottom but
    not everywhere, a quarter of the values missing"""
    ks, n = len(zs), len(hl)
    prof = (34.0 + 1.5 * (1.0 - np.exp(-zs / 400.0))) if salt else (2.0 + 22.0 * np.exp(-zs / 300.0))
    src = prof[:, None] * (1.0 + 0.05 * rng.standard_normal((ks, n)))
    src[zs[:, None] > hl[None]] = 0.0                         # below the bottom
    src[-1, rng.random(n) < 0.3] = prof[-1] * 1.01            # ... but not everywhere: data below hl that is not missing
    miss = rng.random((ks, n)) < 0.25
    src[miss] = rng.choice([0.0, 0.005, -1.0], size=int(miss.sum()))
    return prof, src


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(im, jm, ks, kb, edge, salt=False, seed=0):
    """(zs, line, zz, h): the levels, the z-level line (ks, n) of the whole edge, the sigma levels and a depth array (jm, im) whose line
    for `edge` (depth_line) holds the special points at fixed places; n = jm (east, west) or im"""
    rng = np.random.default_rng(1000 * seed + 7 * im + 3 * jm + ks + 10000 * (edge + 1) + (500 if salt else 0))
    n = jm if along_j(edge) else im
    zs = 5.0 + np.round((1000.0 - 5.0) * (np.arange(ks) / (ks - 1.0)) ** 1.5 * 8.0) / 8.0
    z = -np.arange(kb) / (kb - 1.0)
    zz = np.empty(kb)
    zz[:-1] = 0.5 * (z[:-1] + z[1:])
    zz[-1] = 2.0 * zz[-2] - zz[-3]
    h = 20.0 + 1380.0 * rng.random((jm, im)) ** 2
    h[rng.random((jm, im)) < 0.06] = 0.75
    hl = 20.0 + 1380.0 * rng.random(n) ** 2
    hl[rng.random(n) < 0.08] = 0.75
    hit = [(zs[m] / -zz[k]) for m in range(ks) for k in range(kb) if -zz[k] * (zs[m] / -zz[k]) == zs[m] and zs[m] / -zz[k] > zs[0]]
    hl[[0, 1, 2, 3, 4, 5, n - 2, n - 1]] = 300.0, 1200.0, 1.0, 0.5, hit[len(hit) // 2], zs[1], 30.0, 1400.0
    if along_j(edge):                                         # the block's hs: h(imm1,j) / h(2,j)
        h[:, -2 if edge == 0 else 1] = hl
    else:                                                     # h(i,2) / h(i,jmm1)
        h[1 if edge == 1 else -2, :] = hl
    prof, src = random_line(zs, hl, rng, salt)
    src[:, 0], src[:, n - 1] = prof * 1.02, prof * 0.97       # distinct, complete ends
    src[:, 2] = prof * 1.01
    src[0, 1] = 0.0                                           # point 2: a missing level 1 with both line neighbours valid (the copied end shows it)
    src[0, 3:6] = 0.0                                         # point 5: a missing level 1 without a valid neighbour
    src[0, n - 2], src[0, n - 3] = 0.0, 0.005                 # point n-1: missing with ONE valid neighbour, the end point
    src[-1, n - 2] = 0.0                                      # ... and missing below its shallow bottom
    if ks >= 5:
        src[1:4, 1] = 0.0                                     # a run of missing levels at point 2 ...
        src[2:4, 0], src[2:4, 2] = 0.0, -1.0                  # ... whose tail has no valid neighbour: the copy-down chain
    src[1 if ks < 5 else 4, 1] = 0.0099999999                 # between the REAL(4) 0.01 and the double 0.01: not missing (hl(2) covers the level)
    return zs, src, zz, h


def assert_inputs_are_demanding(zs, line, zz, hl, edge):
    """what the issue wants the inputs to hold, asserted on the arrays themselves (the whole edge's line, both ends physical)"""
    ks, n = line.shape
    w = with_window(line, -1.0, -1.0)                         # the ends copy their neighbours: their own fill-in is never used
    own, prev, nxt = w[:, 1:-1], w[:, :-2], w[:, 2:]
    wet = (hl > 1.0)[None]
    m = own < MISSING
    cover = zs[:, None] <= hl[None]
    tmax = neighbour_max(own, prev, nxt, edge)
    need = m & cover & wet
    inner = np.zeros((1, n), bool)
    inner[0, 1:-1] = True
    assert (hl == 1.0).any() and (hl < 1.0).any(), "hl <= 1"
    assert (need & inner & (prev >= MISSING) & (nxt >= MISSING)).any(), "a missing value with both line neighbours valid"
    assert (need & inner & ((prev >= MISSING) != (nxt >= MISSING))).any(), "a missing value with one line neighbour valid"
    assert (need & inner & (tmax < MISSING)).any(), "a missing value without a valid neighbour"
    assert (m[0] & wet[0] & inner[0]).any() and (need[0] & inner[0] & (tmax[0] < MISSING)).any(), "a missing level 1, one of them staying missing"
    assert (m & ~cover & wet).any(), "a missing value below hl"
    assert (~m & ~cover & wet).any(), "data below hl"
    assert ((own >= MISSING) & (own < 0.01) & cover & wet).any(), "a value between the single-precision 0.01 and the double one"
    assert (need & inner & (tmax >= MISSING) & (tmax != np.maximum(own, np.maximum(prev, nxt)))).any(), "a neighbour maximum that is no single-precision number"
    assert need[:, 1].any() and need[:, n - 2].any(), "a missing value at point 2 and at point n-1"
    if ks >= 3:
        chain = m & ((tmax < MISSING) | ~cover)
        tin = fill_in(zs, w, hl, edge)
        assert (chain[1:] & chain[:-1] & wet & (tin[1:] >= MISSING)).any(), "a run of missing levels filled from above"
    x = -zz[:, None] * hl[None]
    assert zs[0] > 0.0 and (np.diff(zs) > 0).all()
    assert ((x < zs[0]) & wet).any() and ((x > zs[-1]) & wet).any(), "sigma points above zs(1) and below zs(ks)"
    assert (np.isin(x, zs) & wet).any(), "a sigma point on a z level"
    assert (zs[1] == hl).any(), "a bottom on a z level"


def assert_result_is_demanding(t):
    """distinct, non-zero values at both ends (copies of points 2 and n-1), a non-zero level kb, zeros where hl <= 1"""
    assert np.isfinite(t).all() and t[-1].any() and t[0, 0] != 0.0 and t[0, -1] != 0.0 and t[0, 0] != t[0, -1]
    assert same_bits(t[:, 0], t[:, 1]) and same_bits(t[:, -1], t[:, -2]) and not t[:, 2].any()
