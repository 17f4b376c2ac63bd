"""TEST HELPER: the checks of the passive tracers (include/pomgpu.h "passive tracers"), each taking the library to load.

Shared by tests/test_tracers_emulated.py (host build of the kernel sources) and tests/test_gpu_tracers.py (the device).  The bar is
tests/tracer_expect.py -- the CPU oracle with the tracer stage inserted -- bit for bit on 64-bit patterns over levels 1..kbm1 of every
owned cell; level kb must be finite."""
import ctypes

import numpy as np

import tracer_expect as X
from uv_tail_fused_checks import ISPLIT, SCRATCH, diff, same_bits, start  # noqa: F401
from extpom_amd.model import PomGpu
from extpom_amd.lib import PomGpuError

CASES = ["archipelago", "seamount"]
SIZES = [(65, 49, 21), (20, 17, 6), (9, 8, 5)]
ADV = [(2, 1), (2, 2), (1, 1)]
# open sides on which the oracle's flow takes one branch of bcond(4) alone within the steps of the independent check: seamount's flow is a
# uniform eastward current, its east side has no inflow cell and its west side no outflow cell (its south and north sides are land);
# archipelago takes both branches on all four.  A side named here is still required to take the branch it names
ONE_BRANCH = {("seamount", "east"): "outflow", ("seamount", "west"): "inflow"}
ARRAYS = ("trb", "tr", "clim", "wsurf", "surf", "be", "bw", "bn", "bs")


def put(g, n, t):
    for name in ARRAYS:
        g.tracer_upload(n, name, t[name])
    if t["q"] is not None:
        g.tracer_upload(n, "source", t["q"])
    g.set_tracer(n, nbc=t["nbc"], decay=t["lam"])


def eq(dev, want, kb, what=""):
    assert np.isfinite(dev[kb - 1]).all(), f"{what}: level kb is not finite"
    assert same_bits(dev[:kb - 1], want[:kb - 1]), f"{what}: {int(np.count_nonzero(dev[:kb - 1] != want[:kb - 1]))} cells differ in value"


def eq_tracer(g, n, t, kb, what=""):
    eq(g.tracer_download(n, "tr"), t["tr"], kb, f"{what} tracer {n} tr")
    eq(g.tracer_download(n, "trb"), t["trb"], kb, f"{what} tracer {n} trb")


def independent(a, seed=7, nbc=1, source=True, clim=True, i0=0, j0=0, gshape=None):
    """a tracer unrelated to T and S, a function of GLOBAL indices: O(1) values with a -0.0 in trb on a wet and on a land cell, a non-zero
    trclim, a flux and a surface value, boundary values, q on a few cells with decay"""
    kb, jm, im = a.kb, a.jm_local, a.im_local
    JM, IM = gshape or (jm, im)
    r = np.random.default_rng(seed)
    JMp, IMp = JM + 40, IM + 40                               # a margin: a tile's arrays may reach beyond the grid (jm_local > jm)
    G3 = lambda s: s * r.random((kb, JMp, IMp))
    cut3 = lambda x: np.ascontiguousarray(x[:, j0:j0 + jm, i0:i0 + im])
    cut2 = lambda x: np.ascontiguousarray(x[j0:j0 + jm, i0:i0 + im])
    trb = 1.0 + G3(0.5)
    tr = trb + G3(1.0e-3)
    trb[0, JM // 2, IM // 2] = -0.0
    trb[1, JM // 3, IM // 3] = -0.0
    cl = G3(0.25) if clim else np.zeros((kb, JMp, IMp))
    wsurf = 1.0e-6 * (r.random((JMp, IMp)) - 0.5)
    surf = 1.0 + 0.5 * r.random((JMp, IMp))
    be, bw, bn, bs = 2.0 * r.random((kb, JMp)), 2.0 * r.random((kb, JMp)), 2.0 * r.random((kb, IMp)), 2.0 * r.random((kb, IMp))
    q = None
    if source:
        q = np.zeros((kb, JMp, IMp))
        for (k, j, i) in ((0, JM // 2, IM // 2), (1, JM // 3, IM // 4), (kb - 2, 2, 2), (0, JM - 1, IM - 1)):
            q[k, j, i] = 1.0e-4 * (1 + k)
        q[kb - 3, 3, 3] = -0.0
    t = X.new_tracer(a, trb=cut3(trb), tr=cut3(tr), clim=cut3(cl), wsurf=cut2(wsurf) * (a.fsm != 0.), surf=cut2(surf),
                     be=np.ascontiguousarray(be[:, j0:j0 + jm]), bw=np.ascontiguousarray(bw[:, j0:j0 + jm]),
                     bn=np.ascontiguousarray(bn[:, i0:i0 + im]), bs=np.ascontiguousarray(bs[:, i0:i0 + im]),
                     q=None if q is None else cut3(q), lam=2.0e-5 if source else 0.0, nbc=nbc)
    return t


def quiet_restore(st):
    """restore_interior's rate zero in both generations: T and S keep what the filter left (the mask and a zero's sign aside), the started
    state's way of being `without restore records` (records are loaded at iint = 2 and every 30 days only)"""
    st.taurstrb[...] = 0.0
    st.taurstrf[...] = 0.0


# ---- pins: the expectation itself (no library) ------------------------------------------------------------------------------------------
def pin_hooked_run_equals_plain_run(case, size, adv, steps=4):
    """(a) the hooked oracle run with no tracer, and with tracers, leaves every array as pomo_run does"""
    from oracle.pyoracle import OracleTile
    a, b = start(case, dict(nadv=adv[0], nitera=adv[1]), size)
    c = b.copy()
    OracleTile(a).run(steps)
    X.Stepper(b).run(steps)
    s = X.Stepper(c, [independent(c)])
    s.run(steps)
    assert s.stages == steps - 1
    # (with tracers: every array that is not scratch -- advt leaves its last vertical fluxes in zflux)
    assert not diff(a, b, skip=()) and not diff(a, c), (diff(a, b, skip=()), diff(a, c))


def pin_stage_reproduces_t_and_s(case, size, adv, steps=3):
    """(a) the stage fed with T's and S's inputs gives the oracle's t tb s sb of every step, restore_interior (which tracers do not have)
    applied on the test side: the hook's position, bcond4_one and the filter in one"""
    a, _ = start(case, dict(nadv=adv[0], nitera=adv[1]), size)
    s = X.Stepper(a, [])
    for n in range(steps):
        s.tracers = [X.twin_of(a, "s"), X.twin_of(a, "t")]
        body = n > 0
        s.run(1)
        for t, f, rstr in ((s.tracers[0], "s", a.srstr), (s.tracers[1], "t", a.trstr)):
            tr, trb = (X.restore_one(a, t["tr"], rstr), X.restore_one(a, t["trb"], rstr)) if body else (t["tr"], t["trb"])
            eq(tr, a.field(f), a.kb, f"step {n + 1} {f}")
            eq(trb, a.field(f + "b"), a.kb, f"step {n + 1} {f}b")


def pin_bcond4_one(case, size):
    """(b) bcond4_one on T and on S equals pomo_bcond(4)"""
    from oracle.pyoracle import OracleTile
    a, _ = start(case, None, size, warm=2)
    uf, vf = a.uf.copy(), a.vf.copy()
    st = {}
    X.bcond4_one(a, uf, a.t, a.tbe, a.tbw, a.tbn, a.tbs, st)
    X.bcond4_one(a, vf, a.s, a.sbe, a.sbw, a.sbn, a.sbs)
    OracleTile(a).call("bcond", ctypes.c_int(4))
    assert same_bits(uf, a.uf) and same_bits(vf, a.vf)
    assert sum(st[s][0] + st[s][1] for s in X.SIDES) > 0, st   # (a side of land cells alone, seamount's south and north, counts nothing)


# ---- the checks (library) -----------------------------------------------------------------------------------------------------------------
def twins_started(lib, case, size=(65, 49, 21), steps=5):
    """1. ntr = 3 from a started state whose restore rate is zero: tracer 1 is S's twin, tracer 2 T's, tracer 3 unrelated; after 5 unobserved
    steps tracer 1 == s / sb, tracer 2 == t / tb (the order S then T shows a kernel that reads t, s or the wrong tracer), tracer 3 and the
    twins == the expectation, and the flow is the oracle's"""
    a, b = start(case, None, size, warm=3)
    quiet_restore(a)
    quiet_restore(b)
    tr = [X.twin_of(a, "s"), X.twin_of(a, "t"), independent(a)]
    g = PomGpu(b, libpath=lib)
    g.set_tracers(3)
    for n, t in enumerate(tr, 1):
        put(g, n, t)
    X.Stepper(a, tr).run(steps)
    g.run(steps)
    g.download()
    assert not diff(a, b), diff(a, b)
    for n in (1, 2, 3):
        eq_tracer(g, n, tr[n - 1], a.kb, "expectation:")
    for n, f in ((1, "s"), (2, "t")):
        # the mask restore_interior multiplies T and S with (the rate is zero) is the one thing the twins lack
        eq(X.restore_one(b, g.tracer_download(n, "tr"), b.field(f + "rstr")), b.field(f), a.kb, f"tracer {n} tr against {f}")
        eq(X.restore_one(b, g.tracer_download(n, "trb"), b.field(f + "rstr")), b.field(f + "b"), a.kb, f"tracer {n} trb against {f}b")
    g.close()


def twins_cold(lib, case, size=(65, 49, 21), steps=6):
    """1. from iint = 1, time0 = 0: restore_interior loads its record at iint = 2 and relaxes T and S from then on, which a tracer does not
    do; so the twins are held step by step -- after every step restore_one of tracer 1 == s / sb and of tracer 2 == t / tb, and the twins
    take the restored bits on for the next step"""
    a, b = start(case, None, size)
    tr = [X.twin_of(a, "s"), X.twin_of(a, "t"), independent(a, source=False)]
    g = PomGpu(b, libpath=lib)
    g.set_tracers(3)
    for n, t in enumerate(tr, 1):
        put(g, n, t)
    s = X.Stepper(a, tr)
    for step in range(steps):
        s.run(1)
        g.run(1)
        g.download()
        assert not diff(a, b), diff(a, b)
        for n in (1, 2, 3):
            eq_tracer(g, n, tr[n - 1], a.kb, f"step {step + 1} expectation:")
        for n, f in ((1, "s"), (2, "t")):
            for arr, fld in (("tr", f), ("trb", f + "b")):
                dev = g.tracer_download(n, arr)
                got = X.restore_one(b, dev, b.field(f + "rstr")) if step else dev
                eq(got, b.field(fld), a.kb, f"step {step + 1} tracer {n} {arr} against {fld}")
                tr[n - 1][arr][...] = b.field(fld)
                g.tracer_upload(n, arr, b.field(fld))
    g.close()


def against_expectation(lib, case, size, adv=(2, 1), nbc=1, steps=4, nml=None, ntr=1, switch=None, need_branches=True):
    """2. independent tracers against the expectation: a non-zero flux or a surface value, trclim, q with decay, boundary values, -0.0"""
    kw = dict(nadv=adv[0], nitera=adv[1])
    kw.update(nml or {})
    a, b = start(case, kw, size, warm=2)
    tr = [independent(a, seed=7 + n, nbc=nbc if n == 0 else (3 if nbc == 1 else 1), source=n != 1, clim=n != 2) for n in range(ntr)]
    assert np.any(tr[0]["clim"] != 0.) and np.any(tr[0]["q"] != 0.) and np.any(np.signbit(tr[0]["trb"]))
    start_bits = [t["tr"].copy() for t in tr]
    g = PomGpu(b, libpath=lib)
    if switch:
        g.switch(switch, 1)
    g.set_tracers(ntr)
    for n, t in enumerate(tr, 1):
        put(g, n, t)
    s = X.Stepper(a, tr)
    s.run(steps)
    g.run(steps)
    g.download()
    assert not diff(a, b), diff(a, b)
    for n in range(1, ntr + 1):
        eq_tracer(g, n, tr[n - 1], a.kb)
        assert not same_bits(tr[n - 1]["tr"], start_bits[n - 1])
    if need_branches:
        for side in X.SIDES:
            infl, outf = s.stats[side]
            if infl + outf == 0:                              # not an open side: land cells alone (seamount's south and north)
                assert case == "seamount" and side in ("south", "north"), (case, side)
                continue
            lone = ONE_BRANCH.get((case, side))
            assert (infl > 0 or lone == "outflow") and (outf > 0 or lone == "inflow"), (case, side, s.stats)
    g.close()
    return a, b


def mode4(lib, case, size=(65, 49, 21), steps=4):
    """3. mode = 4: T and S stand still, the tracer moves and equals the expectation"""
    a, b = against_expectation(lib, case, size, nml=dict(mode=4), steps=steps, need_branches=False)
    a0, _ = start(case, dict(mode=4), size, warm=2)
    for f in ("t", "tb", "s", "sb"):
        assert same_bits(b.field(f), a0.field(f)), f


def velocity(g):
    return g.check_velocity()


def no_interference(lib, case="archipelago", size=(65, 49, 21), steps=4):
    """4. with ntr = 3 every array of blk2d, blk3d, bdry that is not scratch and check_velocity's result equal the run without tracers on the
    same library; after set_tracers(0) a further run equals the run that never had any"""
    _, b = start(case, None, size, warm=2)
    c = b.copy()
    g0, g1 = PomGpu(b, libpath=lib), PomGpu(c, libpath=lib)
    g1.set_tracers(3)
    for n in (1, 2, 3):
        put(g1, n, independent(c, seed=20 + n, nbc=1 if n != 2 else 3))
    for part in (0, 1):
        g0.run(steps)
        g1.run(steps)
        v0, v1 = velocity(g0), velocity(g1)
        g0.download()
        g1.download()
        assert not diff(b, c), diff(b, c)
        assert same_bits(b.bdry, c.bdry) and v0 == v1, (v0, v1)
        if part == 0:
            assert not same_bits(g1.tracer_download(1, "tr")[:-1], independent(c, seed=21)["tr"][:-1])   # the tracers did move
            g1.set_tracers(0)
            assert g1.tracer_count() == 0
    g0.close()
    g1.close()


def step_forms(lib, case="archipelago", size=(65, 49, 21)):
    """5. run(4), four run(1) and four advance() leave the same tracer bits"""
    out = []
    for form in ("run4", "run1", "advance"):
        _, b = start(case, None, size, warm=2)
        g = PomGpu(b, libpath=lib)
        g.set_tracers(2)
        put(g, 1, independent(b, seed=31))
        put(g, 2, independent(b, seed=32, nbc=3))
        first = int(b.iint) + 1
        if form == "run4":
            g.run(4)
        elif form == "run1":
            for _ in range(4):
                g.run(1)
        else:
            for n in range(first, first + 4):
                g.set_con(iint=n)
                g.advance()
        out.append([g.tracer_download(n, arr) for n in (1, 2) for arr in ("tr", "trb")])
        g.close()
    for o in out[1:]:
        assert all(same_bits(x, y) for x, y in zip(out[0], o))
    assert np.isfinite(out[0][0]).all()


def refusals(lib):
    """7. every refusal in words, ntr = 1 and ntr = 8 accepted, the state untouched by a refused call"""
    _, b = start("seamount", None, (9, 8, 5), warm=1)
    g = PomGpu(b, libpath=lib)

    def refused(fn, *words):
        try:
            fn()
        except PomGpuError as e:
            assert all(w in str(e) for w in words), str(e)
            return
        raise AssertionError("not refused")

    dummy = np.zeros(g.tracer_shape("tr"))
    refused(lambda: g.tracer_upload(1, "tr", dummy), "no tracers are registered")
    refused(lambda: g.tracer_download(1, "tr"), "no tracers are registered")
    refused(lambda: g.set_tracers(9), "0..8")
    refused(lambda: g.set_tracers(-1), "0..8")
    assert g.tracer_count() == 0
    g.set_tracers(8)
    assert g.tracer_count() == 8
    g.set_tracers(1)
    assert g.tracer_count() == 1
    t = independent(b, seed=41)
    put(g, 1, t)
    refused(lambda: g.set_tracers(9), "0..8")
    refused(lambda: g.tracer_upload(2, "tr", dummy), "1..1 are registered")
    refused(lambda: g.tracer_upload(0, "tr", dummy), "1..1 are registered")
    refused(lambda: g._chk(g.L.pomgpu_tracer_upload(g.h, 1, 10, g._p(dummy)), "tracer_upload"), "names no tracer array")
    refused(lambda: g._chk(g.L.pomgpu_tracer_download(g.h, 1, -1, g._p(dummy)), "tracer_download"), "names no tracer array")
    refused(lambda: g.set_tracer(1, nbc=2), "short-wave")
    refused(lambda: g.set_tracer(1, nbc=4), "short-wave")
    refused(lambda: g.tune_placement(), "tracers are registered")
    assert g.tracer_count() == 1
    for name in ARRAYS:                                       # the state is untouched by the refused calls
        assert same_bits(g.tracer_download(1, name), t[name]), name
    assert same_bits(g.tracer_download(1, "source"), t["q"])
    g.tracer_upload(1, "source", None)
    assert not g.tracer_download(1, "source").any()
    g.set_con(error_status=0)                                 # (a refusal raises the reference's error flag, as every refusal of the library does)
    g.run(2)
    g.set_tracers(0)
    g.tune_placement()                                        # accepted again
    g.close()


def fp32_builds_refuse(lib):
    _, b = start("seamount", None, (9, 8, 5))
    g = PomGpu(b, libpath=lib)
    try:
        g.set_tracers(1)
    except PomGpuError as e:
        assert "fp32-storage variant" in str(e), str(e)
    else:
        raise AssertionError("not refused")
    assert g.tracer_count() == 0
    g.close()


# ---- 6: tiles --------------------------------------------------------------------------------------------------------------------------------
TILE_GRID, TILE_KB, TILE_ISPLIT, TILE_STEPS = (65, 49), 21, 10, 4


def added_rounds(steps, ntr, adv=(2, 1)):
    """message rounds the tracers add under the library's own exchange, all on the kernels' stream (tracer_stage, pomgpu_api.hip): per step
    that runs the 3-D body (every step but iint = 1) ONE round that carries trf of all tracers -- solver.f:728 and advance.f:436 of every
    tracer merged, as for T and S -- with the one-pass advection and with advt1 (which has no exchange of its own); nitera > 1 adds
    smol_adif's nitera rounds and :728 per tracer"""
    per_tracer = adv[1] + 1 if adv[0] == 2 and adv[1] > 1 else 0
    return (steps - 1) * (1 + ntr * per_tracer) if ntr else 0


def run_tiles(lib, case, nx, ny, ntr, adv=(2, 1)):
    """nx x ny tiles under the library's exchange (the wide-halo external mode where the tiles are wide enough), one host thread each;
    {rank: (tile, tracer arrays, state, (rounds, side rounds))}"""
    import threading
    from extpom_amd import decomp
    from extpom_amd.cases import finish_initial, make_case
    from forcing_files_checks import Board, device_mover, host_mover
    mover = host_mover if lib is not None else device_mover
    IMg, JMg = TILE_GRID
    world = nx * ny
    iml, jml = decomp.local_size(IMg, JMg, nx, ny)
    tiles = [decomp.make_tile(r, IMg, JMg, iml, jml, n_proc=world) for r in range(world)]
    board, out, errs = Board(world), {}, []

    def rank(r):
        try:
            tile = tiles[r]
            st = make_case(case, IMg, JMg, TILE_KB, tile=tile, dte=6.0, isplit=TILE_ISPLIT, nadv=adv[0], nitera=adv[1])
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
            g.set_wide_external(True, min(t.im for t in tiles), min(t.jm for t in tiles))

            def dens(s, a, b, c):
                g.upload(s); g.call("dens", a, b, c); g.download(s)

            def baropg(s):
                g.upload(s); g.call("baropg_mcc" if int(s.npg) == 2 else "baropg"); g.download(s)

            finish_initial(st, dens, baropg)
            g.upload(st)
            board.barrier.wait()
            r0, s0 = g.exchange_rounds(), g.exchange_rounds_side()
            g.set_tracers(ntr)
            for n in range(1, ntr + 1):
                put(g, n, independent(st, seed=50 + n, nbc=1 if n != 2 else 3, i0=tile.i_off, j0=tile.j_off, gshape=(JMg, IMg)))
            g.run(TILE_STEPS)
            rounds = (g.exchange_rounds() - r0, g.exchange_rounds_side() - s0)
            arrs = {(n, k): g.tracer_download(n, k) for n in range(1, ntr + 1) for k in ("tr", "trb")}
            g.download()
            assert int(st.error_status) == 0
            g.close()
            out[r] = (tile, arrs, st, rounds)
        except Exception:                                     # a dead rank must not leave the others at the barrier
            import traceback
            errs.append(traceback.format_exc())
            board.barrier.abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs[0]
    return out


def tiles(lib, nx, ny, case="archipelago", ntr=3, adv=(2, 1)):
    """6. tracer arrays on owned cells equal the single tile's; the tracers add added_rounds() message rounds on the kernels' stream and none
    on the side stream; the flow is the flow without tracers"""
    from extpom_amd.cases import make_case
    from oracle.pyoracle import oracle_finish_initial
    IMg, JMg = TILE_GRID
    one = make_case(case, IMg, JMg, TILE_KB, dte=6.0, isplit=TILE_ISPLIT, nadv=adv[0], nitera=adv[1])
    oracle_finish_initial(one)
    g = PomGpu(one, libpath=lib)
    g.set_tracers(ntr)
    for n in range(1, ntr + 1):
        put(g, n, independent(one, seed=50 + n, nbc=1 if n != 2 else 3))
    g.run(TILE_STEPS)
    single = {(n, k): g.tracer_download(n, k) for n in range(1, ntr + 1) for k in ("tr", "trb")}
    g.close()
    on, off = run_tiles(lib, case, nx, ny, ntr, adv), run_tiles(lib, case, nx, ny, 0, adv)
    bad = []
    kbm1 = TILE_KB - 1
    for r, (tile, arrs, st, rounds) in on.items():
        io, jo, im, jm = tile.i_off, tile.j_off, tile.im, tile.jm
        sl_j = slice(0 if jo == 0 else 1, jm if jo + jm == JMg else jm - 1)       # the cells the tile owns
        sl_i = slice(0 if io == 0 else 1, im if io + im == IMg else im - 1)
        for key, x in arrs.items():
            ref = single[key][:kbm1, jo:jo + jm, io:io + im][:, sl_j, sl_i]
            if not same_bits(ref, x[:kbm1, :jm, :im][:, sl_j, sl_i]) or not np.isfinite(x).all():
                bad.append((r, key))
        assert rounds[0] == off[r][3][0] + added_rounds(TILE_STEPS, ntr, adv) and rounds[1] == off[r][3][1], (r, rounds, off[r][3])
        assert not diff(st, off[r][2]), (r, diff(st, off[r][2]))
    assert not bad, bad
    assert not same_bits(single[(1, "tr")], independent(one, seed=51)["tr"])
