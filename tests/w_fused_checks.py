"""TEST HELPER: w formed inside the q2 / q2l advection march on one tile (k_advq_col<2, true>), no vertvl launch in mode_internal.

Shared by tests/test_w_fused_emulated.py (host build of the kernel sources, a serial grid) and tests/test_gpu_w_fused.py (the
device): every check takes the library to load.  The bar is the CPU oracle, bit for bit on 64-bit patterns, over every COMMON array
that is not scratch -- w included -- after steps that follow each other unobserved (run(2), run(1), run(3), one download), and the
library's own event profile says which kernels ran."""
import numpy as np

import off_default
from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial

SCRATCH = {"tps", "fluxua", "fluxva", "zflux"}
CASES = ["archipelago", "seamount", "island"]
NAMELISTS = {"default": dict(), "mode4": dict(mode=4), "nadv1": dict(nadv=1), "npg2": dict(npg=2), "off_default": "off_default"}
# (im, jm, kb): a wavefront's 62-column edge inside the interior (65, 66), a flat tile, a last workgroup of one row, one interior column
# per side, the benchmark's kb, a kb beyond the register kernels' (this kernel is a loop kernel and stays fused there)
SIZES = [(65, 49, 21), (66, 50, 21), (128, 12, 21), (20, 17, 6), (8, 8, 6), (20, 14, 50), (20, 14, 65)]
# switches under which mode_internal keeps the vertvl launch: (q2 / q2l kernel of the profile, its launches per body step)
KEEP = {"W_NOFUSE": ("k_advq2_col", 1), "ADVQ_SINGLE": ("k_advq_col", 2), "ADVQ_EXCHANGE": ("k_advq2_col", 1)}
ISPLIT = 30
VERTVL, ADVQ2 = "k_vertvl", "k_advq2_col"


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


def diff(a, b, skip=SCRATCH):
    return [n for n in BLK2D + BLK3D if n not in skip and not same_bits(a.field(n), b.field(n))]


def start(case, nml=None, size=(65, 49, 21), warm=0):
    """(oracle's state, the library's copy) at the initial state (the next step, iint = 1, skips the 3-D body) or `warm` steps in"""
    if nml == "off_default":
        a = off_default.off_default_case(case, *size, oracle_finish_initial)
    else:
        a = make_case(case, *size, dte=6.0, isplit=ISPLIT, **(nml or {}))
        oracle_finish_initial(a)
    if warm:
        OracleTile(a).run(warm)
    return a, a.copy()


def launches(prof, name):
    return prof.get(name, (0, 0.0))[0]


def interior(x):
    return x[..., 1:-1, 1:-1]


def exercises(a):
    """what the oracle's state must hold for the comparison to guard the fused march: a w that is not zero, at the surface too (a
    surface volume flux), and an interior land column (the mask of bcondorl(5) does something)"""
    kb = a.kb
    return {"w": bool(np.any(interior(a.w) != 0.)), "w_surface": bool(np.any(interior(a.w[0]) != 0.)), "w_bottom": bool(np.any(interior(a.w[kb - 1]) != 0.)),
            "vfluxf": bool(np.any(interior(a.vfluxf) != 0.)), "land_inside": bool(np.any(interior(a.fsm) == 0.)),
            "q2": bool(np.any(interior(a.q2[1:kb - 1]) != 0.))}


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def unobserved_steps(lib, case, nml, size, switch=None, calls=(2, 1, 3), need=()):
    """run(2), run(1), run(3) and one download at the end; per step that runs the 3-D body (all but iint = 1): one k_advq2_col and no
    k_vertvl -- or, under a switch of KEEP, the pair"""
    a, b = start(case, nml, size)
    g = PomGpu(b, libpath=lib)
    if switch:
        g.switch(switch, 1)
    g.prof_begin()
    for n in calls:
        g.run(n)
    prof = g.prof_end()
    body = sum(calls) - 1
    if switch:
        name, per = KEEP[switch]
        assert launches(prof, VERTVL) == body and launches(prof, name) == per * body, prof
    else:
        assert launches(prof, VERTVL) == 0 and launches(prof, ADVQ2) == body and launches(prof, "k_advq_col") == 0, prof
    OracleTile(a).run(sum(calls))
    g.download()
    assert a.iint == b.iint and not diff(a, b), diff(a, b)
    ex = exercises(a)
    assert all(ex[k] for k in need), ex
    g.close()


def land_forced(lib, size=(65, 49, 21), switch=None):
    """a surface volume flux that is NOT masked, uploaded over the case's own: on an interior land column the running sum starts off
    zero, the stored w is zero on levels 1..kbm1 (the mask) and the sum itself at level kb (no mask there) -- and q2, q2l are not
    zero on land in the first step that runs the body.  And a w that is not zero anywhere, so that on the rim (where vertvl forms
    nothing) the mask alone has land columns to clear"""
    a, b = start("archipelago", None, size)
    for st in (a, b):
        st.vfluxf[...] = 1.0e-7 + 1.0e-8 * np.cos(np.arange(st.vfluxf.size, dtype=np.float64)).reshape(st.vfluxf.shape)
        st.vfluxb[...] = 0.5 * st.vfluxf
        st.w[...] = 1.0e-5 * (1.5 + np.sin(np.arange(st.w.size, dtype=np.float64))).reshape(st.w.shape)
    land = interior(a.fsm) == 0.
    assert land.any() and np.all(interior(a.q2)[:, land] != 0.)
    rim = np.ones(a.fsm.shape, dtype=bool)
    rim[1:-1, 1:-1] = False
    rim_land = rim & (a.fsm == 0.)
    assert rim_land.any() and (rim & (a.fsm != 0.)).any()
    g = PomGpu(b, libpath=lib)
    if switch:
        g.switch(switch, 1)
    ot = OracleTile(a)
    for n, body in ((2, 1), (2, 2)):                          # the first body step alone (q2 on land still as initialised), then two more
        g.prof_begin()
        g.run(n)
        prof = g.prof_end()
        assert launches(prof, VERTVL) == (body if switch else 0) and launches(prof, ADVQ2) == body, prof
        ot.run(n)
        g.download()
        assert not diff(a, b), diff(a, b)
        kb = a.kb
        assert np.any(interior(a.w[kb - 1])[land] != 0.) and np.all(interior(a.w[:kb - 1])[:, land] == 0.)
        assert np.all(a.w[:kb - 1][:, rim_land] == 0.) and np.all(a.w[kb - 1][rim_land] != 0.) and np.all(a.w[:, rim & (a.fsm != 0.)] != 0.)
    g.close()


def switch_flipped_live(lib):
    """POMGPU_W_NOFUSE set and unset between the steps of one context: the oracle's bits, i.e. those of either side alone"""
    a, b = start("archipelago", None, warm=1)
    ot = OracleTile(a)
    g = PomGpu(b, libpath=lib)
    for n, sw in ((2, None), (1, 1), (2, None), (1, 1), (1, None)):
        g.switch("W_NOFUSE", sw)
        g.prof_begin()
        g.run(n)
        prof = g.prof_end()
        assert launches(prof, VERTVL) == (n if sw else 0) and launches(prof, ADVQ2) == n, prof
        ot.run(n)
    g.switch("W_NOFUSE", None)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def fused_equals_pair(lib, steps=6, case="archipelago", size=(65, 49, 21), fuses=True):
    """no oracle (the fp32 study builds have none): a context with POMGPU_W_NOFUSE and one without, every array, scratch included.
    fuses=False: a build without the fused kernel (the fp32-arithmetic variant keeps its stencil kernels free of fp64 arithmetic,
    tests/test_fp32_arith_variant.py) must say so in its profile -- vertvl on both sides -- and give the same bits all the same"""
    a = make_case(case, *size, dte=6.0, isplit=ISPLIT)
    oracle_finish_initial(a)
    b = a.copy()
    ga, gb = PomGpu(a, libpath=lib), PomGpu(b, libpath=lib)
    ga.switch("W_NOFUSE", 1)
    ga.prof_begin()
    gb.prof_begin()
    ga.run(steps)
    gb.run(steps)
    pa, pb = ga.prof_end(), gb.prof_end()
    assert launches(pa, VERTVL) == steps - 1 and launches(pb, VERTVL) == (0 if fuses else steps - 1), (pa, pb)
    assert launches(pa, ADVQ2) == launches(pb, ADVQ2) == steps - 1, (pa, pb)
    ga.download()
    gb.download()
    assert not diff(a, b, skip=()), diff(a, b, skip=())
    ex = exercises(a)
    assert ex["w"] and ex["w_surface"] and ex["land_inside"] and ex["q2"], ex
    ga.close()
    gb.close()


def routine_by_routine(lib):
    """the Fortran host's call sequence (mode_internal is one call there): fused as well"""
    a, b = start("seamount", None, warm=1)
    g = PomGpu(b, libpath=lib)
    first = int(b.iint) + 1
    g.prof_begin()
    for n in range(first, first + 2):
        g.set_con(iint=n)
        g.call("get_time")
        g.get_con()
        g.call("lateral_viscosity")
        g.call("mode_interaction")
        for iext in range(1, ISPLIT + 1):
            g.set_con(iext=iext)
            g.call("mode_external")
        g.set_con(iext=ISPLIT + 1)
        g.call("mode_internal")
        g.check_velocity()
    prof = g.prof_end()
    assert launches(prof, VERTVL) == 0 and launches(prof, ADVQ2) == 2, prof
    OracleTile(a).run(2)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def stand_alone_entry_points(lib):
    """pomgpu_vertvl and pomgpu_advq keep their own kernels"""
    a, b = start("archipelago", None, warm=2)
    g = PomGpu(b, libpath=lib)
    g.prof_begin()
    g.call("vertvl")
    prof = g.prof_end()
    assert launches(prof, VERTVL) == 1 and launches(prof, ADVQ2) == 0, prof
    g.close()
