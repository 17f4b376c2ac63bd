"""TEST HELPER: the checks of the Lagrangian floats (include/pomgpu.h "Lagrangian floats"), each taking the library to load.

Shared by tests/test_floats_emulated.py (host build of the kernel sources) and tests/test_gpu_floats.py (the device).  The bar is
tests/float_expect.py, bit for bit on all six arrays of the float state and the five sampled values; the checks of section 2 do not go
through it.  Coverage conditions are asserted on the expectation's own bookkeeping (X.new_book), never on the code under test."""
import json
import os

import numpy as np

import float_expect as X
from uv_tail_fused_checks import diff, start
from extpom_amd.lib import PomGpuError
from extpom_amd.model import PomGpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["archipelago", "seamount"]
SIZES = [(8, 8, 6), (20, 17, 6), (65, 49, 21)]
COUNTS = [1, 63, 64, 65, 257, 70001]                          # the wave, block and grid edges of one lane per float, 256 lanes a block
# (cells a step along i and j, sigma a step): a few tenths of a cell, and several cells -- finite, so that the index limits act
SPEEDS = {"weak": (0.3, 0.15), "strong": (4.0, 0.9)}
KEYS = ("x", "y", "sig", "status", "kind", "id")
KW = dict(title="floats", time_start="2000-01-01 00:00:00 +00:00")


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def wrong(dev, want, keys=KEYS):
    """the arrays that differ in a bit"""
    return [k for k in keys if dev[k].shape != want[k].shape or dev[k].dtype != want[k].dtype or not np.array_equal(bits(dev[k]), bits(want[k]))]


def copy(F):
    return {k: v.copy() for k, v in F.items()}


def refused(fn, *words):
    try:
        fn()
    except PomGpuError as e:
        assert all(w in str(e) for w in words), str(e)
        return
    raise AssertionError("not refused")


# ---- hand-made fields and seeds -------------------------------------------------------------------------------------------------------------
def hand_made(b, speed="weak", seed=3):
    """u v w of state b replaced by finite pseudo-random fields of SPEEDS[speed] cells (sigma) a step; a state with no land inside
    2..im-1 x 2..jm-1 (seamount) gets one hand-made land cell, so that every case can reject a float"""
    cells, csig = SPEEDS[speed]
    r = np.random.default_rng(seed)
    shp = (b.kb, b.jm_local, b.im_local)
    dti = float(b.dti)
    assert (b.dt[:b.jm, :b.im] > 0.).all() and dti > 0.
    b.u[...] = cells * (b.dx[None] / dti) * (2.0 * r.random(shp) - 1.0)
    b.v[...] = cells * (b.dy[None] / dti) * (2.0 * r.random(shp) - 1.0)
    b.w[...] = csig * (b.dt[None] / dti) * (2.0 * r.random(shp) - 1.0)
    if (b.fsm[1:b.jm - 1, 1:b.im - 1] != 0.).all():
        b.fsm[b.jm // 2 - 1, b.im // 2] = 0.0
    return b


def seeds(b, per_axis=None):
    """a lattice over the whole grid at five depths, kinds alternating, and four floats beside every land cell and along every side"""
    im, jm = b.im, b.jm
    n = per_axis or min(2 * max(im, jm) - 3, 40)
    gx, gy, gs = np.meshgrid(np.linspace(1.51, im - 0.51, n), np.linspace(1.51, jm - 0.51, n), np.array([0.0, -0.02, -0.5, -0.97, -1.0]), indexing="ij")
    x, y, s = [gx.ravel()], [gy.ravel()], [gs.ravel()]
    land = np.argwhere(b.fsm[:jm, :im] == 0.0) + 1            # (j, i), 1-based
    for dxo, dyo in ((0.55, 0.0), (-0.55, 0.0), (0.0, 0.55), (0.0, -0.55), (0.0, 0.0)):   # (the last: on the land cell, LOST on admission)
        x.append(land[:, 1] + dxo); y.append(land[:, 0] + dyo); s.append(np.full(len(land), -0.3))
    t = np.linspace(1.6, max(im, jm) - 0.6, 2 * max(im, jm))
    for xs, ys in ((np.full_like(t, 1.52), t), (np.full_like(t, im - 0.52), t), (t, np.full_like(t, 1.52)), (t, np.full_like(t, jm - 0.52))):
        x.append(xs); y.append(ys); s.append(np.full_like(t, -0.6))
    x, y, s = np.concatenate(x), np.concatenate(y), np.concatenate(s)
    kind = (np.arange(x.size) % 2).astype(np.int32)
    kind[s == 0.0] = 1                                        # surface drifters
    ids = (7 * np.arange(x.size) + 11).astype(np.int32)       # the caller's numbering, carried and never read
    return x, y, s, kind, ids


def scattered(b, n, seed=5):
    """n floats anywhere in the grid and a little beyond, any depth"""
    r = np.random.default_rng(seed)
    x = 0.5 + (b.im + 0.5) * r.random(n)
    y = 0.5 + (b.jm + 0.5) * r.random(n)
    s = -r.random(n)
    return x, y, s, (r.random(n) < 0.5).astype(np.int32), r.permutation(n).astype(np.int32)


def put(g, b, seed):
    """the seed registered in context g, and the expectation's float set on state b"""
    x, y, s, kind, ids = seed
    g.set_floats(x, y, s, kind, ids)
    return X.new_floats(b, x, y, s, kind, ids)


# ---- 1: float_step alone against the expectation ----------------------------------------------------------------------------------------------
def step_alone(lib, case, size, speed, steps=3, need_branches=False):
    _, b = start(case, None, size)
    hand_made(b, speed)
    g = PomGpu(b, libpath=lib)
    F = put(g, b, seeds(b))
    assert g.float_count() == F["x"].size
    assert not wrong(g.floats(), F), ("admission", wrong(g.floats(), F))
    assert {X.ACTIVE, X.LOST} <= set(F["status"].tolist())
    book = X.new_book()
    for n in range(steps):
        g.float_step()
        X.step(b, F, book)
        assert not wrong(g.floats(), F), (f"step {n + 1}", wrong(g.floats(), F))
    assert not wrong(g.float_sample(), X.sample(b, F), X.SAMPLES), wrong(g.float_sample(), X.sample(b, F), X.SAMPLES)
    if need_branches:
        assert all(book[k] > 0 for k in X.BRANCHES), {k: v for k, v in book.items() if not v}
    g.close()
    return book


def counts(lib, n, steps=2):
    _, b = start("archipelago", None, (20, 17, 6))
    hand_made(b, "strong", seed=9)
    g = PomGpu(b, libpath=lib)
    F = put(g, b, scattered(b, n))
    for _ in range(steps):
        g.float_step()
        X.step(b, F)
    assert g.float_count() == n and not wrong(g.floats(), F), wrong(g.floats(), F)
    assert not wrong(g.float_sample(), X.sample(b, F), X.SAMPLES)
    g.close()


def not_finite(lib):
    """host build only: NaN and infinity in u and in positions give LOST with the position kept, and address nothing outside the arrays"""
    _, b = start("archipelago", None, (20, 17, 6))
    hand_made(b, "weak")
    b.u[:, 8:11, 5:9] = np.nan
    b.u[:, 3:5, 12:15] = np.inf
    b.w[:, 12:14, 3:6] = -np.inf
    g = PomGpu(b, libpath=lib)
    x, y, s, kind, ids = seeds(b)
    x[3], y[5], s[7], x[9], y[11], s[13] = np.nan, np.nan, np.nan, np.inf, -np.inf, np.inf
    F = put(g, b, (x, y, s, kind, ids))
    assert not wrong(g.floats(), F) and (F["status"][[3, 5, 7, 9, 11, 13]] == X.LOST).all()
    nlost = 0
    for _ in range(2):
        before = copy(F)
        g.float_step()
        X.step(b, F)
        got = g.floats()
        assert not wrong(got, F), wrong(got, F)
        lost = (got["status"] == X.LOST) & (before["status"] == X.ACTIVE)
        nlost += int(lost.sum())
        assert not wrong({k: got[k][lost] for k in ("x", "y", "sig")}, {k: before[k][lost] for k in ("x", "y", "sig")}, ("x", "y", "sig"))   # position kept
    assert nlost > 0
    assert not wrong(g.float_sample(), X.sample(b, F), X.SAMPLES)
    g.close()


# ---- 2: checks that do not go through float_expect.py ----------------------------------------------------------------------------------------
def uniform_grid(size=(20, 17, 6), d=8000.0):
    _, b = start("seamount", None, size)
    b.dx[...] = d
    b.dy[...] = d
    b.u[...] = 0.0
    b.v[...] = 0.0
    b.w[...] = 0.0
    return b


def zero_flow(lib):
    b = uniform_grid()
    g = PomGpu(b, libpath=lib)
    F = put(g, b, seeds(b))
    for _ in range(3):
        g.float_step()
    assert not wrong(g.floats(), F), wrong(g.floats(), F)      # nobody moves, nobody changes status
    g.close()


def uniform_flow(lib, steps=10):
    """all dx equal, u = U, v = w = 0: every L is exact, so x follows x = x + dti * (U / dx) bit for bit and y, sig are untouched"""
    b = uniform_grid()
    U, d, dti = 16.25, 8000.0, float(b.dti)                   # 0.37 cells a step
    b.u[...] = U
    g = PomGpu(b, libpath=lib)
    r = np.random.default_rng(2)
    n = 300
    x, y, s = 2.0 + 3.0 * r.random(n), 3.0 + 11.0 * r.random(n), -r.random(n)
    g.set_floats(x, y, s, kind=(np.arange(n) % 2))
    for _ in range(steps):
        g.float_step()
        x = x + dti * (U / d)
    got = g.floats()
    assert (got["status"] == X.ACTIVE).all()
    assert not wrong(got, dict(x=x, y=y, sig=s), ("x", "y", "sig")), wrong(got, dict(x=x, y=y, sig=s), ("x", "y", "sig"))
    g.close()


def solid_body(lib, steps=10, tol=1.0e-11):
    """u = -Om (y_u - yc) dx at u's point (i - 0.5, j), v = Om (x_v - xc) dy at v's point (i, j - 0.5), uniform grid: the fields are linear,
    so the midpoint step is X <- (I + hA + h^2 A^2 / 2) X in closed form.  Fewer than 100 roundings a step of at most 2^-53 * 32 each give
    3.6e-13 cells a step; a staggering wrong by half a cell is off by 0.5 * Om * dti a step, 0.005 cells here"""
    b = uniform_grid()
    d, dti = 8000.0, float(b.dti)
    hOm = 0.01
    Om = hOm / dti
    xc, yc = 10.5, 9.0
    jj = np.arange(1, b.jm_local + 1, dtype=np.float64)[None, :, None]
    ii = np.arange(1, b.im_local + 1, dtype=np.float64)[None, None, :]
    b.u[...] = -Om * (jj - yc) * d + 0.0 * ii
    b.v[...] = Om * (ii - xc) * d + 0.0 * jj
    g = PomGpu(b, libpath=lib)
    r = np.random.default_rng(4)
    n = 200
    rad, ang = 0.5 + 4.5 * r.random(n), 2.0 * np.pi * r.random(n)
    x, y, s = xc + rad * np.cos(ang), yc + rad * np.sin(ang), -r.random(n)
    g.set_floats(x, y, s, kind=np.ones(n, np.int32))
    px, py = x - xc, y - yc
    for _ in range(steps):
        g.float_step()
        px, py = (1.0 - 0.5 * hOm * hOm) * px - hOm * py, hOm * px + (1.0 - 0.5 * hOm * hOm) * py
    got = g.floats()
    assert (got["status"] == X.ACTIVE).all()
    err = max(np.abs(got["x"] - (xc + px)).max(), np.abs(got["y"] - (yc + py)).max())
    assert err <= tol and 0.5 * hOm > 1.0e6 * tol, err
    assert np.array_equal(bits(got["sig"]), bits(s))
    g.close()


def permutation(lib):
    _, b = start("archipelago", None, (20, 17, 6))
    hand_made(b, "strong")
    seed = seeds(b)
    p = np.random.default_rng(8).permutation(seed[0].size)
    g = PomGpu(b, libpath=lib)
    g.set_floats(*seed)
    for _ in range(3):
        g.float_step()
    one = g.floats()
    g.set_floats(*[a[p] for a in seed])
    for _ in range(3):
        g.float_step()
    two = g.floats()
    assert not wrong(two, {k: v[p] for k, v in one.items()})
    g.close()


def one_among_many(lib):
    _, b = start("archipelago", None, (20, 17, 6))
    hand_made(b, "weak")
    many = scattered(b, 70001, seed=12)
    F0 = X.new_floats(b, *many)
    pick = int(np.flatnonzero(F0["status"] == X.ACTIVE)[1234])
    g = PomGpu(b, libpath=lib)
    g.set_floats(*many)
    for _ in range(3):
        g.float_step()
    among = {k: v[pick:pick + 1] for k, v in g.floats().items()}
    g.set_floats(*[a[pick:pick + 1] for a in many])
    for _ in range(3):
        g.float_step()
    assert not wrong(g.floats(), among), wrong(g.floats(), among)
    g.close()


def two_contexts(lib):
    _, b = start("archipelago", None, (20, 17, 6))
    hand_made(b, "strong")
    out = []
    for _ in range(2):
        g = PomGpu(b.copy(), libpath=lib)
        g.set_floats(*seeds(b))
        for _ in range(3):
            g.float_step()
        out.append((g.floats(), g.float_sample()))
        g.close()
    assert not wrong(out[0][0], out[1][0]) and not wrong(out[0][1], out[1][1], X.SAMPLES)


# ---- 3: in the step -----------------------------------------------------------------------------------------------------------------------------
def in_step(lib, case, mode, size=(20, 17, 6), steps=4):
    """run(steps) with floats == run(1), download, the expectation's step on what was downloaded, repeated; from the initial state, whose first
    step skips the 3-D body and rests the floats"""
    _, b = start(case, dict(mode=mode), size)
    c = b.copy()
    g, h = PomGpu(b, libpath=lib), PomGpu(c, libpath=lib)
    seed = seeds(b)
    F = put(g, b, seed)
    g.run(steps)
    moved = 0
    for _ in range(steps):
        h.run(1)
        h.download()
        if X.body_runs(c):
            X.step(c, F)
            moved += 1
    assert moved == steps - 1
    got = g.floats()
    assert not wrong(got, F), wrong(got, F)
    x0 = seed[0][F["status"] == X.ACTIVE]
    assert x0.size and not np.array_equal(F["x"][F["status"] == X.ACTIVE], x0)     # the flow did move them
    g.download()
    assert not diff(b, c, skip=()), diff(b, c, skip=())
    assert not wrong(g.float_sample(), X.sample(c, F), X.SAMPLES)
    g.close()
    h.close()


def no_interference(lib, size=(65, 49, 21)):
    """every array of the state after run(5) with floats equals the run without them"""
    _, b = start("archipelago", None, size, warm=1)
    c = b.copy()
    g, h = PomGpu(b, libpath=lib), PomGpu(c, libpath=lib)
    g.set_floats(*seeds(b))
    g.run(5)
    h.run(5)
    g.download()
    h.download()
    assert not diff(b, c, skip=()), diff(b, c, skip=())
    assert int(b.error_status) == 0
    g.close()
    h.close()


def launch_counts(lib, size=(65, 49, 21)):
    _, b = start("seamount", None, size)
    g = PomGpu(b, libpath=lib)
    g.run(2)
    g.prof_begin()
    g.run(5)
    off = {k: n for k, (n, _) in g.prof_end().items()}
    g.set_floats(*seeds(b))
    g.prof_begin()
    g.run(5)
    on = {k: n for k, (n, _) in g.prof_end().items()}
    assert "k_float_step" not in off and on.pop("k_float_step") == 5, (off, on)
    assert on == off, {k: (off.get(k), on.get(k)) for k in set(on) | set(off) if off.get(k) != on.get(k)}
    assert off["k_profq"] == 5 and not any(k.startswith(("k_realvertvl", "k_restore_fields")) for k in on), on   # nothing lazy formed
    g.set_floats([], [], [])
    assert g.float_count() == 0
    g.prof_begin()
    g.run(5)
    again = {k: n for k, (n, _) in g.prof_end().items()}
    assert again == off, {k: (off.get(k), again.get(k)) for k in set(again) | set(off) if off.get(k) != again.get(k)}
    g.close()


def mode_2_rests(lib):
    _, b = start("seamount", dict(mode=2), (20, 17, 6))
    g = PomGpu(b, libpath=lib)
    F = put(g, b, seeds(b))
    g.prof_begin()
    g.run(3)
    assert "k_float_step" not in g.prof_end()
    assert not wrong(g.floats(), F)
    g.close()


def never_on_land(lib, size=(65, 49, 21), steps=20):
    _, b = start("archipelago", None, size)
    g = PomGpu(b, libpath=lib)
    g.set_floats(*seeds(b))
    g.run(steps)
    F = g.floats()
    act = F["status"] == X.ACTIVE
    ic, jc = np.floor(F["x"][act] + 0.5).astype(int), np.floor(F["y"][act] + 0.5).astype(int)
    assert act.any() and (b.fsm[jc - 1, ic - 1] != 0.0).all()
    assert (ic >= 2).all() and (ic <= b.im - 1).all() and (jc >= 2).all() and (jc <= b.jm - 1).all()
    g.close()


# ---- 4: files ----------------------------------------------------------------------------------------------------------------------------------
def check_header(path, n, title=KW["title"], time_start=KW["time_start"]):
    """the whole header against tests/golden/float_file_schema.json"""
    from scipy.io import netcdf_file
    want = json.load(open(os.path.join(HERE, "golden", "float_file_schema.json")))
    fill = lambda t: t.replace("{title}", title).replace("{time_start}", time_start)
    with netcdf_file(str(path), "r", mmap=False) as f:
        assert f.version_byte == want["version_byte"], f.version_byte
        got_g = [[k, v.decode() if isinstance(v, bytes) else v] for k, v in f._attributes.items()]
        assert got_g == [[k, fill(v)] for k, v in want["global_atts"]], got_g
        assert [[k, v] for k, v in f.dimensions.items()] == [["nfloat", n]], f.dimensions
        assert list(f.variables) == [v["name"] for v in want["vars"]], list(f.variables)
        for v in want["vars"]:
            q = f.variables[v["name"]]
            assert list(q.dimensions) == v["dims"], (v["name"], q.dimensions)
            assert q.typecode() == v["type"] and q.data.dtype.str == {"d": ">f8", "i": ">i4"}[v["type"]], (v["name"], q.typecode())
            got_a = [[k, a.decode() if isinstance(a, bytes) else a] for k, a in q._attributes.items()]
            assert got_a == [[k, fill(t)] for k, t in v["atts"]], (v["name"], got_a)


def file_shows_the_floats(lib, tmp):
    """the file opens with scipy.io.netcdf_file and shows the downloaded arrays, the samples, iint and time"""
    from scipy.io import netcdf_file
    _, b = start("archipelago", None, (20, 17, 6))
    g = PomGpu(b, libpath=lib)
    g.set_floats(*seeds(b))
    g.run(3)
    path = os.path.join(str(tmp), "a.floats.nc")
    g.write_file("floats", path, **KW)
    F, S = g.floats(), g.float_sample()
    g.get_con()
    check_header(path, F["x"].size)
    with netcdf_file(path, "r", mmap=False) as f:
        for k in KEYS:
            assert np.array_equal(bits(np.array(f.variables[k].data, dtype=F[k].dtype)), bits(F[k])), k
        for k in X.SAMPLES:
            assert np.array_equal(bits(np.array(f.variables[k].data, dtype=np.float64)), bits(S[k])), k
        assert float(f.variables["iint"].data) == 3.0 and float(f.variables["time"].data) == float(b.time)
    g.close()


def checkpoint(lib, tmp, steps=3, more=2):
    """write, read_floats in a fresh context started from the downloaded state, `more` steps: the uninterrupted run's floats"""
    _, b = start("archipelago", None, (20, 17, 6))
    g = PomGpu(b, libpath=lib)
    g.set_floats(*seeds(b))
    g.run(steps)
    path = os.path.join(str(tmp), "ck.floats.nc")
    g.write_file("floats", path, **KW)
    g.download()
    c = b.copy()
    at_write = g.floats()
    g.run(more)
    h = PomGpu(c, libpath=lib)
    t, ii = h.read_floats(path)
    assert ii == float(steps) and t == float(c.time)
    assert not wrong(h.floats(), at_write), wrong(h.floats(), at_write)       # EXITED and LOST included: the stored status is kept
    assert set(at_write["status"].tolist()) >= {X.ACTIVE, X.LOST}
    h.run(more)
    assert not wrong(h.floats(), g.floats()), wrong(h.floats(), g.floats())
    assert not np.array_equal(g.floats()["x"], at_write["x"])
    g.close()
    h.close()


def hand_file(path, arrays, scalars=None, record=False, types=None):
    """a CDF-2 file an outside tool would write: 1-D variables, one dimension per distinct length (`record`: the unlimited one for all)"""
    from scipy.io import netcdf_file
    with netcdf_file(str(path), "w", version=2) as f:
        if record:
            f.createDimension("nfloat", None)
        for name, x in (scalars or {}).items():
            v = f.createVariable(name, "d", ())
            v[...] = float(x)
        for name, x in arrays.items():
            dim = "nfloat" if record else "n%d" % len(x)
            if dim not in f.dimensions:
                f.createDimension(dim, len(x))
            v = f.createVariable(name, (types or {}).get(name, "i" if np.asarray(x).dtype.kind == "i" else "d"), (dim,))
            v[:] = x
    return path


def initial_file(lib, tmp):
    """x y sig alone: an initial file any tool can write; kind 0, id 0..n-1, the admission's status"""
    _, b = start("archipelago", None, (20, 17, 6))
    x, y, s, _, _ = seeds(b)
    path = hand_file(os.path.join(str(tmp), "init.floats.nc"), dict(sig=s, y=y, x=x))
    g = PomGpu(b, libpath=lib)
    assert g.read_floats(path) == (0.0, 0.0)
    assert not wrong(g.floats(), X.new_floats(b, x, y, s))
    g.close()


def file_refusals(lib, tmp):
    """every refusal leaves a foreign float set and the state as they were"""
    _, b = start("archipelago", None, (20, 17, 6))
    c = b.copy()
    g = PomGpu(b, libpath=lib)
    F = put(g, b, scattered(b, 50))
    x, y, s, kind, ids = seeds(b)
    n = x.size
    p = lambda name: os.path.join(str(tmp), name)
    refused(lambda: g.read_floats(p("absent.nc")), "cannot open")
    refused(lambda: g.read_floats(hand_file(p("noy.nc"), dict(x=x, sig=s))), "variable y is absent")
    refused(lambda: g.read_floats(hand_file(p("nox.nc"), dict(y=y, sig=s))), "variable x is absent")
    refused(lambda: g.read_floats(hand_file(p("f32.nc"), dict(x=x, y=y, sig=s), types=dict(sig="f"))), "variable sig has NetCDF type 5")
    refused(lambda: g.read_floats(hand_file(p("len.nc"), dict(x=x, y=y[:3], sig=s))), "variable y has the dimension lengths (3)")
    refused(lambda: g.read_floats(hand_file(p("rec.nc"), dict(x=x, y=y, sig=s), record=True)), "record variable")
    refused(lambda: g.read_floats(hand_file(p("kind.nc"), dict(x=x, y=y, sig=s, kind=kind.astype(np.float64)))), "variable kind has NetCDF type 6")
    refused(lambda: g.read_floats(hand_file(p("time.nc"), dict(x=x, y=y, sig=s, time=np.zeros(n)))), "variable time has the dimension lengths")
    good = hand_file(p("good.nc"), dict(x=x, y=y, sig=s, kind=kind, id=ids), scalars=dict(time=1.5, iint=7))
    raw = open(good, "rb").read()
    open(p("short.nc"), "wb").write(raw[:len(raw) - 4 * n - 8])
    refused(lambda: g.read_floats(p("short.nc")), "reaches beyond the file")
    open(p("hdr.nc"), "wb").write(raw[:40])
    refused(lambda: g.read_floats(p("hdr.nc")), "ends inside its header")
    open(p("cdf5.nc"), "wb").write(b"CDF\x05" + raw[4:])
    refused(lambda: g.read_floats(p("cdf5.nc")), "CDF version 5")
    open(p("hdf.nc"), "wb").write(b"\x89HDF\r\n\x1a\n" + raw[8:])
    refused(lambda: g.read_floats(p("hdf.nc")), "HDF5")
    refused(lambda: g.write_file("floats", os.path.join(str(tmp), "no", "such", "dir.nc")), "cannot open")
    assert g.float_count() == 50 and not wrong(g.floats(), F)
    g.download()
    assert not diff(b, c, skip=())
    assert g.read_floats(good) == (1.5, 7.0)                  # and the good one is taken, time and iint applied to nothing
    assert not wrong(g.floats(), X.new_floats(b, x, y, s, kind, ids))
    g.get_con()
    assert int(b.iint) == int(c.iint) and float(b.time) == float(c.time)
    g.close()


# ---- 5: hosts ----------------------------------------------------------------------------------------------------------------------------------
def refusals(lib):
    _, b = start("archipelago", None, (20, 17, 6))
    g = PomGpu(b, libpath=lib)
    one = np.array([5.0])
    refused(lambda: g.float_step(), "no floats are registered")
    refused(lambda: g.float_sample(), "no floats are registered")
    refused(lambda: g.write_file("floats", "/nonexistent/x.nc"), "no floats are registered")
    refused(lambda: g._chk(g.L.pomgpu_float_upload(g.h, -1, g._p(one), g._p(one), g._p(one), None, None), "float_upload"), "0..67108864")
    refused(lambda: g._chk(g.L.pomgpu_float_upload(g.h, (1 << 26) + 1, g._p(one), g._p(one), g._p(one), None, None), "float_upload"), "0..67108864")
    refused(lambda: g._chk(g.L.pomgpu_float_upload(g.h, 1, g._p(one), None, g._p(one), None, None), "float_upload"), "no host array")
    assert g.float_count() == 0 and g.floats()["x"].size == 0
    F = put(g, b, scattered(b, 65))
    refused(lambda: g._chk(g.L.pomgpu_float_upload(g.h, 1, None, g._p(one), g._p(one), None, None), "float_upload"), "no host array")
    refused(lambda: g._chk(g.L.pomgpu_float_upload(g.h, -5, g._p(one), g._p(one), g._p(one), None, None), "float_upload"), "0..67108864")
    refused(lambda: g.tune_placement(), "floats are registered")
    assert g.float_count() == 65 and not wrong(g.floats(), F)  # the refused calls changed nothing
    g._chk(g.L.pomgpu_float_download(g.h, None, None, None, None, None, None), "float_download")   # any pointer may be NULL
    g.set_con(error_status=0)
    g.run(2)
    g.set_floats([], [], [])                                  # n = 0 frees
    assert g.float_count() == 0
    g.tune_placement()                                        # accepted again
    g.close()


def tile_refuses(lib):
    """a context with a neighbour in pomgpu_dims refuses floats and says why"""
    from extpom_amd import decomp
    from extpom_amd.cases import make_case
    iml, jml = decomp.local_size(65, 49, 2, 1)
    tile = decomp.make_tile(0, 65, 49, iml, jml, n_proc=2)
    st = make_case("seamount", 65, 49, 6, tile=tile, dte=6.0, isplit=30)
    g = PomGpu(st, libpath=lib)
    refused(lambda: g.set_floats([5.0], [5.0], [-0.5]), "tile with neighbours", "single tile")
    refused(lambda: g.read_floats("/nonexistent/x.nc"), "cannot open")
    assert g.float_count() == 0
    g.close()


def fp32_builds_refuse(lib):
    _, b = start("seamount", None, (9, 8, 5))
    g = PomGpu(b, libpath=lib)
    for fn in (lambda: g.set_floats([5.0], [5.0], [-0.5]), g.float_step, g.float_sample, lambda: g.read_floats("x.nc"), lambda: g.write_file("floats", "x.nc")):
        refused(fn, "fp32-storage variant")
    assert g.float_count() == 0
    g.close()
