"""TEST HELPER: what the library is to make of passive tracers (include/pomgpu.h "passive tracers"), WITHOUT the code under test.

The CPU oracle steps the flow (pomo_run); the tracer stage is inserted where the library runs it.  pomo_mode_internal is one call, so the
stage runs inside the oracle's own exchange hook: on one tile the hook is a no-op, and the first exchange behind advance.f:454 is that of
uf at :466.  Between :454 and :466 the reference runs advu, advv, profu, profv and bcondorl(3), which write uf, vf, wubot, wvbot and
nothing the stage reads (u v w aam kh etb etf dt and the grid): the state the stage sees at :466 is the state it would see in front of
:459.  The stage itself is the oracle's pomo_advt1 / pomo_advt2 / pomo_proft on the tracer's own arrays -- they take the field as an
argument -- plus three restatements in numpy: the source term, bcond(4) for one field (bcond4_one) and the filter.

What is restated is pinned before it is trusted (tests/test_tracers_emulated.py, the tests named pin_*):
  (a) the hooked run with no tracer equals pomo_run on every array, and the stage fed with T's and S's own inputs reproduces the oracle's
      t, tb, s, sb up to restore_interior, which the tracers do not have and the test applies (restore_one): position, bcond4_one and the
      filter at once.  Not with nitera > 1: there smol_adif reads the edge lines of the work array, which advt2 never writes -- for T
      they hold what profq left in uf, for a tracer what its own last step left;
  (b) bcond4_one on T and on S equals pomo_bcond(4).

Arrays are in the model's numpy order (kb, jm, im); a tracer is a dict with trb tr clim wsurf surf be bw bn bs (arrays), q (array or None),
lam, nbc."""
import ctypes

import numpy as np

from oracle.pyoracle import OracleTile

SIDES = ("east", "west", "south", "north")


def p(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return ctypes.c_void_p(a.ctypes.data)


def new_tracer(a, **kw):
    """a tracer with the library's defaults on the grid of state a; keywords replace arrays / lam / nbc"""
    kb, jm, im = a.kb, a.jm_local, a.im_local
    t = dict(trb=np.zeros((kb, jm, im)), tr=np.zeros((kb, jm, im)), clim=np.zeros((kb, jm, im)), wsurf=np.zeros((jm, im)),
             surf=np.zeros((jm, im)), be=np.zeros((kb, jm)), bw=np.zeros((kb, jm)), bn=np.zeros((kb, im)), bs=np.zeros((kb, im)),
             q=None, lam=0.0, nbc=1)
    for k, v in kw.items():
        assert k in t, k
        t[k] = v if np.isscalar(v) or v is None else np.ascontiguousarray(v, dtype=np.float64).copy()
    return t


def twin_of(a, which):
    """the tracer that is T's ("t") or S's ("s") twin in state a: its arrays hold that field's bits"""
    f = which
    return new_tracer(a, trb=a.field(f + "b"), tr=a.field(f), clim=a.field(f + "clim"), wsurf=a.field("w" + f + "surf"),
                      surf=a.field(f + "surf"), be=a.field(f + "be"), bw=a.field(f + "bw"), bn=a.field(f + "bn"), bs=a.field(f + "bs"),
                      nbc=int(a.nbct if f == "t" else a.nbcs))


def bcond4_one(a, ff, f, be, bw, bn, bs, stats=None):
    """bcond(4)'s lines for T (bounds_forcing.f:155-231) with ff for uf, f for t, be bw bn bs for tbe tbw tbn tbs, on one tile whose four
    edges are open, then its mask.  stats: per side, [inflow cells, outflow cells] over the wet edge cells"""
    im, jm, kbm1 = a.im, a.jm, a.kb - 1
    dti, zz, u, v, w, dt, dx, dy, fsm = a.dti, np.asarray(a.zz).reshape(-1), a.u, a.v, a.w, a.dt, a.dx, a.dy, a.fsm

    def note(side, infl, wet):
        if stats is not None:
            s = stats.setdefault(side, [0, 0])
            s[0] += int(np.count_nonzero(infl & wet))
            s[1] += int(np.count_nonzero(~infl & wet))

    for k in range(kbm1):
        vert = k != 0 and k != kbm1 - 1
        # east, then west, inside the reference's j loop; south, then north, inside its i loop: at a corner south / north wins
        u1 = 2. * u[k, :, im - 1] * dti / (dx[:, im - 1] + dx[:, im - 2])
        infl = u1 <= 0.
        vin = f[k, :, im - 1] - u1 * (be[k, :] - f[k, :, im - 1])
        vout = f[k, :, im - 1] - u1 * (f[k, :, im - 1] - f[k, :, im - 2])
        if vert:
            wm = .5 * (w[k, :, im - 2] + w[k + 1, :, im - 2]) * dti / ((zz[k - 1] - zz[k + 1]) * dt[:, im - 2])
            vout = vout - wm * (f[k - 1, :, im - 2] - f[k + 1, :, im - 2])
        ff[k, :, im - 1] = np.where(infl, vin, vout)
        note("east", infl, fsm[:, im - 1] != 0.)
        u1 = 2. * u[k, :, 1] * dti / (dx[:, 0] + dx[:, 1])
        infl = u1 >= 0.
        vin = f[k, :, 0] - u1 * (f[k, :, 0] - bw[k, :])
        vout = f[k, :, 0] - u1 * (f[k, :, 1] - f[k, :, 0])
        if vert:
            wm = .5 * (w[k, :, 1] + w[k + 1, :, 1]) * dti / ((zz[k - 1] - zz[k + 1]) * dt[:, 1])
            vout = vout - wm * (f[k - 1, :, 1] - f[k + 1, :, 1])
        ff[k, :, 0] = np.where(infl, vin, vout)
        note("west", infl, fsm[:, 0] != 0.)
        u1 = 2. * v[k, 1, :] * dti / (dy[0, :] + dy[1, :])
        infl = u1 >= 0.
        vin = f[k, 0, :] - u1 * (f[k, 0, :] - bs[k, :])
        vout = f[k, 0, :] - u1 * (f[k, 1, :] - f[k, 0, :])
        if vert:
            wm = .5 * (w[k, 1, :] + w[k + 1, 1, :]) * dti / ((zz[k - 1] - zz[k + 1]) * dt[1, :])
            vout = vout - wm * (f[k - 1, 1, :] - f[k + 1, 1, :])
        ff[k, 0, :] = np.where(infl, vin, vout)
        note("south", infl, fsm[0, :] != 0.)
        u1 = 2. * v[k, jm - 1, :] * dti / (dy[jm - 1, :] + dy[jm - 2, :])
        infl = u1 <= 0.
        vin = f[k, jm - 1, :] - u1 * (bn[k, :] - f[k, jm - 1, :])
        vout = f[k, jm - 1, :] - u1 * (f[k, jm - 1, :] - f[k, jm - 2, :])
        if vert:
            wm = .5 * (w[k, jm - 2, :] + w[k + 1, jm - 2, :]) * dti / ((zz[k - 1] - zz[k + 1]) * dt[jm - 2, :])
            vout = vout - wm * (f[k - 1, jm - 2, :] - f[k + 1, jm - 2, :])
        ff[k, jm - 1, :] = np.where(infl, vin, vout)
        note("north", infl, fsm[jm - 1, :] != 0.)
    ff[:kbm1] = ff[:kbm1] * fsm[None]


def restore_one(a, x, rstr):
    """restore_interior's lines for one field (bounds_forcing.f:1099-1120) with the taurstr and trstr / srstr state a holds: what T and S
    get behind the filter and the tracers do not"""
    kbm1 = a.kb - 1
    y = x.copy()
    y[:kbm1] = x[:kbm1] + 2. * a.dti / 86400. * a.taurstr[:kbm1] * (rstr[:kbm1] - x[:kbm1])
    y[:kbm1] = y[:kbm1] * a.fsm[None]
    return y


class Stepper:
    """the oracle on state a, stepping `tracers` (a list of dicts, changed in place) along with the flow"""

    def __init__(self, a, tracers=()):
        assert a.im == a.im_local and a.jm == a.jm_local and min(a.n_west, a.n_east, a.n_south, a.n_north) == -1 == max(
            a.n_west, a.n_east, a.n_south, a.n_north), "one tile, four open edges"
        self.a, self.tracers, self.stats, self.stages = a, list(tracers), {}, 0
        self._busy = False
        self._uf = a.field("uf").ctypes.data
        self._seen = 0
        self.ot = OracleTile(a, exch3d=self._hook)

    def _hook(self, arr):
        if self._busy or arr.ctypes.data != self._uf or arr.shape[0] != self.a.kb - 1:
            return
        self._seen += 1
        if self._seen == self._at:                            # advance.f:466
            self._busy = True
            try:
                self.stage()
            finally:
                self._busy = False

    def stage(self):
        a, ot = self.a, self.ot
        kbm1 = a.kb - 1
        self.stages += 1
        for t in self.tracers:
            # the work array is the tracer's own and lives on: advt2 with nitera > 1 reads its edge lines, which it never writes, in
            # smol_adif (for T they hold what uf last held); level kb stays +0.0
            trf = t.setdefault("trf", np.zeros_like(t["trb"]))
            ot.call("advt1" if int(a.nadv) == 1 else "advt2", p(t["trb"]), p(t["tr"]), p(t["clim"]), p(trf))
            if t["q"] is not None or t["lam"] != 0.:
                q = t["q"] if t["q"] is not None else np.zeros_like(trf)
                x = t["lam"] * t["trb"][:kbm1]
                x = q[:kbm1] - x
                x = a.dti2 * x
                trf[:kbm1] = trf[:kbm1] + x
            ot.call("proft", p(trf), p(t["wsurf"]), p(t["surf"]), ctypes.c_int(int(t["nbc"])))
            bcond4_one(a, trf, t["tr"], t["be"], t["bw"], t["bn"], t["bs"], self.stats)
            new = t["tr"] + .5 * a.smoth * (trf + t["trb"] - 2. * t["tr"])
            t["trb"][...] = new
            t["tr"][...] = trf
            assert not trf[kbm1].any() and not np.signbit(trf[kbm1]).any()

    def run(self, nsteps):
        a = self.a
        for _ in range(nsteps):
            body = (int(a.iint) + 1 != 1 or a.time0 != 0.) and int(a.mode) != 2
            # exchanges of (uf, kbm1 levels) in front of :466: none in mode 4; else advt's own for T (advt2: nitera + 1) and :436
            before = 0 if int(a.mode) == 4 else (1 if int(a.nadv) == 1 else int(a.nitera) + 2)
            self._seen, self._at = 0, (before + 1 if body else -1)
            n0 = self.stages
            self.ot.run(1)
            assert self.stages == n0 + (1 if body else 0), "the tracer stage runs once per step that runs the 3-D body"
        return a
