"""TEST HELPER: what the library is to make of Lagrangian floats (include/pomgpu.h "Lagrangian floats"), WITHOUT the code under test.

numpy fp64, vectorised over the floats, one IEEE operation per statement and in the association the header states; the library is built
with -ffp-contract=off, so the bar is bits.  Arrays are in the model's numpy order (kb, jm, im); indices below are the header's 1-based
ones and lose 1 where they meet numpy.  A float set is a dict x y sig (float64) status kind id (int32).

Two things are formulated on purpose otherwise than the kernels do them, so that an agreement means something: the level search counts
the levels at or above sig (the kernels keep the last one that is), and the index limits are np.clip on integers (the kernels compare).

Where the header leaves a choice this file makes it, and the library follows:
  * the finiteness of sn is that of the sum sig + dti * c2, before reflection and limits (fmax / fmin would turn a NaN into -1);
  * `book`, the bookkeeping of which branches were taken, counts occurrences: it is what the tests' coverage conditions are asserted on,
    never a measurement of the code under test.  i_low / i_high / j_low / j_high: an index that a limit changed, at that end of that axis
    -- the corners of u's and v's cells and the i - 1 (j - 1) of the metric under u (v)."""
import numpy as np

ACTIVE, EXITED, LOST = 0, 1, 2
SAMPLES = ("lon", "lat", "depth", "t", "s")
BRANCHES = ("interior_move", "land_rejection", "exit_west", "exit_east", "exit_south", "exit_north", "reflect_surface", "reflect_bottom",
            "above_zz1", "below_zzkbm1", "kind0", "kind1", "i_low", "i_high", "j_low", "j_high")


def new_book():
    return {b: 0 for b in BRANCHES}


def note(book, key, mask):
    if book is not None:
        book[key] += int(np.count_nonzero(mask))


def L(p, q, f):
    d = q - p
    m = f * d
    return p + m


def axis(xs, n, book=None, name=None):
    """one axis of a field point's cell: indices i0, i1 (1-based, limited to 1..n) and the fraction"""
    xs = np.fmax(xs, 0.0)
    xs = np.fmin(xs, float(n + 1))
    fl = np.floor(xs)
    f = xs - fl
    a = fl.astype(np.int64)
    if name:
        note(book, name + "_low", a < 1)
        note(book, name + "_high", a + 1 > n)
    return np.clip(a, 1, n), np.clip(a + 1, 1, n), f


def cell(x, n):
    """the containing cell along one axis, limited to 1..n"""
    xs = x + 0.5
    xs = np.fmax(xs, 0.0)
    xs = np.fmin(xs, float(n + 1))
    return np.clip(np.floor(xs).astype(np.int64), 1, n)


def levels_zz(a, sig, book=None):
    """u v t s: (k, k2, fz, alone) with level k alone at or above zz(1) and at or below zz(kbm1)"""
    zz = np.asarray(a.zz).reshape(-1)
    kbm1 = a.kb - 1
    top = sig >= zz[0]
    bot = ~top & (sig <= zz[kbm1 - 1])
    note(book, "above_zz1", top)
    note(book, "below_zzkbm1", bot)
    k = np.maximum((zz[None, :kbm1 - 1] >= sig[:, None]).sum(axis=1), 1)          # levels 1..kbm1-1 at or above sig
    num = zz[k - 1] - sig
    den = zz[k - 1] - zz[k]
    fz = num / den
    alone = top | bot
    ka = np.where(top, 1, np.where(bot, kbm1, k))
    return ka, np.where(alone, ka, k + 1), fz, alone


def levels_z(a, sig):
    """w: the k in 1..kbm1 with z(k) >= sig > z(k+1)"""
    z = np.asarray(a.z).reshape(-1)
    kbm1 = a.kb - 1
    k = np.maximum((z[None, :kbm1] >= sig[:, None]).sum(axis=1), 1)
    num = z[k - 1] - sig
    den = z[k - 1] - z[k]
    return k, k + 1, num / den


def bil(f2, i0, i1, j0, j1, fx, fy):
    """L in i, then in j, of a 2-D gatherer f2(i, j)"""
    south = L(f2(i0, j0), f2(i1, j0), fx)
    north = L(f2(i0, j1), f2(i1, j1), fx)
    return L(south, north, fy)


def velocity(a, x, y, sig, book=None):
    """V(x, y, sig) = (U / DXU, V / DYV, W / D) in cells, cells and sigma per second"""
    im, jm = a.im, a.jm
    ui0, ui1, ufx = axis(x + 0.5, im, book, "i")
    uj0, uj1, ufy = axis(y, jm)
    vi0, vi1, vfx = axis(x, im)
    vj0, vj1, vfy = axis(y + 0.5, jm, book, "j")
    k, k2, fz, alone = levels_zz(a, sig, book)
    kw, kw2, fzw = levels_z(a, sig)

    def on_zz(f3, i0, i1, j0, j1, fx, fy):
        up = bil(lambda i, j: f3[k - 1, j - 1, i - 1], i0, i1, j0, j1, fx, fy)
        dn = bil(lambda i, j: f3[k2 - 1, j - 1, i - 1], i0, i1, j0, j1, fx, fy)
        return np.where(alone, up, L(up, dn, fz))

    U = on_zz(a.u, ui0, ui1, uj0, uj1, ufx, ufy)
    V = on_zz(a.v, vi0, vi1, vj0, vj1, vfx, vfy)
    wup = bil(lambda i, j: a.w[kw - 1, j - 1, i - 1], vi0, vi1, uj0, uj1, vfx, ufy)
    wdn = bil(lambda i, j: a.w[kw2 - 1, j - 1, i - 1], vi0, vi1, uj0, uj1, vfx, ufy)
    W = L(wup, wdn, fzw)

    def dxu(i, j):
        note(book, "i_low", i - 1 < 1)
        s = a.dx[j - 1, i - 1] + a.dx[j - 1, np.maximum(i - 1, 1) - 1]
        return 0.5 * s

    def dyv(i, j):
        note(book, "j_low", j - 1 < 1)
        s = a.dy[j - 1, i - 1] + a.dy[np.maximum(j - 1, 1) - 1, i - 1]
        return 0.5 * s

    DXU = bil(dxu, ui0, ui1, uj0, uj1, ufx, ufy)
    DYV = bil(dyv, vi0, vi1, vj0, vj1, vfx, vfy)
    D = bil(lambda i, j: a.dt[j - 1, i - 1], vi0, vi1, uj0, uj1, vfx, ufy)
    return U / DXU, V / DYV, W / D


def classify(a, x, y, s):
    """0 not finite, 1 outside 2..im-1 x 2..jm-1, 2 on land, 3 in the water; and the containing cell's doubles"""
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(s)
    xc = np.floor(x + 0.5)
    yc = np.floor(y + 0.5)
    inside = fin & (xc >= 2.0) & (xc <= float(a.im - 1)) & (yc >= 2.0) & (yc <= float(a.jm - 1))
    ic = np.where(inside, xc, 2.0).astype(np.int64)
    jc = np.where(inside, yc, 2.0).astype(np.int64)
    land = a.fsm[jc - 1, ic - 1] == 0.0
    where = np.where(~fin, 0, np.where(~inside, 1, np.where(land, 2, 3)))
    return where, xc, yc


def admit(a, x, y, sig, stored=None):
    """the status upload gives: not finite or on land LOST, outside EXITED; a stored status other than ACTIVE is kept"""
    with np.errstate(all="ignore"):
        where, _, _ = classify(a, x, y, sig)
    st = np.where(where == 3, ACTIVE, np.where(where == 1, EXITED, LOST)).astype(np.int32)
    if stored is not None:
        st = np.where(np.asarray(stored) != ACTIVE, stored, st).astype(np.int32)
    return st


def new_floats(a, x, y, sig, kind=None, ids=None):
    x, y, sig = (np.array(v, dtype=np.float64).ravel() for v in (x, y, sig))
    n = x.size
    return dict(x=x, y=y, sig=sig, status=admit(a, x, y, sig), kind=np.zeros(n, np.int32) if kind is None else np.array(kind, dtype=np.int32).ravel(),
                id=np.arange(n, dtype=np.int32) if ids is None else np.array(ids, dtype=np.int32).ravel())


def step(a, F, book=None):
    """one midpoint step of length dti with the fields of state a frozen; F is changed in place"""
    act = np.flatnonzero(F["status"] == ACTIVE)
    if not act.size:
        return F
    x, y, sig, keeps = F["x"][act], F["y"][act], F["sig"][act], F["kind"][act] == 1
    note(book, "kind0", ~keeps)
    note(book, "kind1", keeps)
    dti = float(a.dti)
    hm = 0.5 * dti
    with np.errstate(all="ignore"):
        a1, b1, c1 = velocity(a, x, y, sig, book)
        xm = x + hm * a1
        ym = y + hm * b1
        sm = np.where(keeps, sig, sig + hm * c1)
        sm = np.fmax(sm, -1.0)
        sm = np.fmin(sm, 0.0)
        a2, b2, c2 = velocity(a, xm, ym, sm, book)
        xn = x + dti * a2
        yn = y + dti * b2
        sraw = np.where(keeps, sig, sig + dti * c2)
        up = sraw > 0.0
        sn = np.where(up, -sraw, sraw)
        down = sn < -1.0
        sn = np.where(down, -2.0 - sn, sn)
        sn = np.fmax(sn, -1.0)
        sn = np.fmin(sn, 0.0)
        where, xc, yc = classify(a, xn, yn, sraw)
    ok = where != 0
    note(book, "reflect_surface", ok & up)
    note(book, "reflect_bottom", ok & down)
    note(book, "exit_west", (where == 1) & (xc < 2.0))
    note(book, "exit_east", (where == 1) & (xc > float(a.im - 1)))
    note(book, "exit_south", (where == 1) & (yc < 2.0))
    note(book, "exit_north", (where == 1) & (yc > float(a.jm - 1)))
    note(book, "land_rejection", where == 2)
    note(book, "interior_move", where == 3)
    status = F["status"][act]
    status[where == 0] = LOST                                   # position kept
    status[where == 1] = EXITED                                 # this is where it left
    moved = (where == 1) | (where == 3)
    F["x"][act] = np.where(moved, xn, x)
    F["y"][act] = np.where(moved, yn, y)
    F["sig"][act] = np.where(ok, sn, sig)                       # land: x, y kept, sig = sn
    F["status"][act] = status
    return F


def sample(a, F):
    """lon lat depth t s of every float, whatever its status"""
    x, y, sig = F["x"], F["y"], F["sig"]
    with np.errstate(all="ignore"):
        i0, i1, fx = axis(x, a.im)
        j0, j1, fy = axis(y, a.jm)
        lon = bil(lambda i, j: a.east_e[j - 1, i - 1], i0, i1, j0, j1, fx, fy)
        lat = bil(lambda i, j: a.north_e[j - 1, i - 1], i0, i1, j0, j1, fx, fy)
        ic, jc = cell(x, a.im), cell(y, a.jm)
        depth = a.et[jc - 1, ic - 1] + sig * a.dt[jc - 1, ic - 1]
        k, k2, fz, alone = levels_zz(a, sig)
        t = np.where(alone, a.t[k - 1, jc - 1, ic - 1], L(a.t[k - 1, jc - 1, ic - 1], a.t[k2 - 1, jc - 1, ic - 1], fz))
        s = np.where(alone, a.s[k - 1, jc - 1, ic - 1], L(a.s[k - 1, jc - 1, ic - 1], a.s[k2 - 1, jc - 1, ic - 1], fz))
    return dict(lon=lon, lat=lat, depth=depth, t=t, s=s)


def body_runs(a):
    """does the step that is about to run with a.iint already raised run mode_internal's 3-D part (advance.f:362)?"""
    return (int(a.iint) != 1 or float(a.time0) != 0.0) and int(a.mode) != 2
