"""TEST HELPER: the depth-mean correction of u, v (advance.f:365-393) applied by every kernel that loads them, no k_int_uvmean pass in
mode_internal on one tile.

Shared by tests/test_uvmean_onload_emulated.py (host build of the kernel sources, a serial grid) and tests/test_gpu_uvmean_onload.py
(the device): every check takes the library to load.  The bar is the CPU oracle, bit for bit on 64-bit patterns, over every COMMON
array that is not scratch, after steps that follow each other unobserved (run(2), run(1), run(3), one download), and the library's
own event profile says whether the pass ran."""
import numpy as np

from uv_tail_fused_checks import CASES, ISPLIT, SCRATCH, diff, launches, read3, same_bits, start, step_by_routine, write3  # noqa: F401
from extpom_amd.cases import make_case
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial

NAMELISTS = {"default": dict(), "mode4": dict(mode=4), "npg2": dict(npg=2), "off_default": "off_default", "nadv1": dict(nadv=1)}
FALLBACK_NML = {"nadv1"}                                      # the upstream tracer advection reads u, v with kernels that do not correct: the pass stays
# (im, jm, kb): a wavefront's 62-column edge inside the interior (65, 66), a flat tile of two workgroup rows, a last workgroup of one
# row, one interior column per side, the benchmark's kb
SIZES = [(65, 49, 21), (66, 50, 21), (128, 12, 21), (20, 17, 6), (8, 8, 6), (20, 14, 50)]
SIZE_FALLBACK = (20, 14, 65)                                  # kb beyond the register kernels of the fused tail
# switches under which mode_internal keeps the pass
KEEP = ["UVMEAN_PASS", "W_NOFUSE", "UV_NOFUSE", "ADVT2_SINGLE"]
ADVQ2, ADVT2, ADVUV, TAIL, RIM = "k_advq2_col", "k_advt2x2_col", "k_advuv_col", "k_profuv_filter_reg2", "k_uv_filter_rim"


def passes(prof):
    """launches of the correction pass, whatever its shape (k_int_uvmean, k_int_uvmean_reg, k_int_uvmean_reg2)"""
    return sum(v[0] for k, v in prof.items() if k.startswith("k_int_uvmean"))


def exercises(a):
    """what the oracle's state must hold for the comparison to guard the on-load correction: with this state's transports the
    correction (u - su) + cu changes u on an interior column, on the columns 2..4 and im-2..im the fused filter leaves to the rim
    kernel, v alike on its rows; there is land inside the rim; and the two means differ"""
    kbm1 = a.kb - 1
    dz = np.asarray(a.dz).reshape(-1)[:kbm1]
    su, sv = np.zeros_like(a.dt), np.zeros_like(a.dt)
    for k in range(kbm1):
        su = su + a.u[k] * dz[k]
        sv = sv + a.v[k] * dz[k]
    cu = (a.utb[:, 1:] + a.utf[:, 1:]) / (a.dt[:, 1:] + a.dt[:, :-1])
    cv = (a.vtb[1:, :] + a.vtf[1:, :]) / (a.dt[1:, :] + a.dt[:-1, :])
    du = ((a.u[:kbm1, :, 1:] - su[:, 1:]) + cu) != a.u[:kbm1, :, 1:]              # columns 2..im
    dv = ((a.v[:kbm1, 1:, :] - sv[1:, :]) + cv) != a.v[:kbm1, 1:, :]              # rows 2..jm
    return {"u_interior": bool(du[:, 4:-4, 4:-4].any()), "v_interior": bool(dv[:, 4:-4, 4:-4].any()),
            "u_west": bool(du[:, :, 0:3].any()), "u_east": bool(du[:, :, -3:].any()),
            "v_south": bool(dv[:, 0:3, :].any()), "v_north": bool(dv[:, -3:, :].any()),
            "land_inside": bool(np.any(a.fsm[1:-1, 1:-1] == 0.)), "means_differ": bool(np.any(cu[1:, :] != cv[:, 1:]))}


ALL_NEEDS = ("u_interior", "v_interior", "u_west", "u_east", "v_south", "v_north", "land_inside", "means_differ")


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def unobserved_steps(lib, case, nml, size, switch=None, calls=(2, 1, 3), onload=True, need=()):
    """run(2), run(1), run(3) and one download at the end; per step that runs the 3-D body (all but iint = 1): no k_int_uvmean* launch
    where the on-load correction applies, one otherwise (a switch of KEEP, nadv = 1, kb = 65)"""
    a, b = start(case, nml, size)
    g = PomGpu(b, libpath=lib)
    if switch:
        g.switch(switch, 1)
    g.prof_begin()
    for n in calls:
        g.run(n)
    prof = g.prof_end()
    body = sum(calls) - 1
    assert passes(prof) == (0 if onload and not switch else body), prof
    OracleTile(a).run(sum(calls))
    g.download()
    assert a.iint == b.iint and not diff(a, b), diff(a, b)
    ex = exercises(a)
    assert all(ex[k] for k in need), ex
    g.close()


def switch_flipped_live(lib):
    """POMGPU_UVMEAN_PASS set and unset between the steps of one context: the oracle's bits, i.e. those of either side alone"""
    a, b = start("archipelago", None, warm=1)
    ot = OracleTile(a)
    g = PomGpu(b, libpath=lib)
    for n, sw in ((2, None), (1, 1), (2, None), (1, 1), (1, None)):
        g.switch("UVMEAN_PASS", sw)
        g.prof_begin()
        g.run(n)
        prof = g.prof_end()
        assert passes(prof) == (n if sw else 0), prof
        ot.run(n)
    g.switch("UVMEAN_PASS", None)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def routine_by_routine(lib, upload_u=False):
    """the Fortran host's call sequence -- lateral_viscosity there runs without the 2-D sums (sum2d = 0) and leaves the depth sums of
    u, v all the same.  upload_u: u written from outside between lateral_viscosity and mode_internal (the same bits, but the library
    cannot know): the sums are no longer valid, the pass runs, the bits are the oracle's"""
    a, b = start("seamount", None, warm=1)
    g = PomGpu(b, libpath=lib)
    first = int(b.iint) + 1

    def hook(point):
        if upload_u and point == "lateral_viscosity":
            write3(g, "u", read3(g, "u"))

    g.prof_begin()
    for n in range(first, first + 2):
        step_by_routine(g, n, hook)
    prof = g.prof_end()
    assert passes(prof) == (2 if upload_u else 0) and launches(prof, ADVQ2) == 2, prof
    OracleTile(a).run(2)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def upload_changes_u(lib):
    """a DIFFERENT u uploaded between lateral_viscosity and mode_internal: the pass runs on the new u, as in a context that never
    corrects on load"""
    a = make_case("archipelago", 65, 49, 21, dte=6.0, isplit=ISPLIT)
    oracle_finish_initial(a)
    OracleTile(a).run(1)
    b = a.copy()
    ga, gb = PomGpu(a, libpath=lib), PomGpu(b, libpath=lib)
    ga.switch("UVMEAN_PASS", 1)
    first = int(a.iint) + 1
    for g in (ga, gb):
        def hook(point, g=g):
            if point == "lateral_viscosity":
                u = read3(g, "u")
                write3(g, "u", u * 1.25 + 1.0e-3 * (u != 0.))
        g.prof_begin()
        step_by_routine(g, first, hook)
        step_by_routine(g, first + 1)
    pa, pb = ga.prof_end(), gb.prof_end()
    assert passes(pa) == 2 and passes(pb) == 1, (pa, pb)       # gb: the step with the upload falls back, the next corrects on load
    ga.download()
    gb.download()
    assert not diff(a, b, skip=()), diff(a, b, skip=())
    ga.close()
    gb.close()


def stand_alone_entry_points(lib):
    """the stand-alone entry points keep their kernels and read u, v as they are in memory: the same results with and without the
    switch, and a pomgpu_advct of its own leaves sums that the next mode_internal may use only if nothing came in between"""
    a, b = start("archipelago", None, warm=2)
    c = b.copy()
    out = []
    for st, sw in ((b, None), (c, 1)):
        g = PomGpu(st, libpath=lib)
        g.switch("UVMEAN_PASS", sw)
        g.prof_begin()
        g.call("advct")
        g.call("vertvl")
        g.call("advu")
        g.call("advv")
        g.call("bcond", 4)
        g.call("bcond", 6)
        g.call("bcondorl", 3)
        prof = g.prof_end()
        assert passes(prof) == 0 and launches(prof, "k_vertvl") == 1 and launches(prof, "k_advct_col") == 1, prof
        g.download()
        out.append(st)
        g.close()
    assert not diff(out[0], out[1], skip=()), diff(out[0], out[1], skip=())


def onload_equals_pass(lib, steps=6, case="archipelago", size=(65, 49, 21), onload=True):
    """no oracle (the fp32 study builds have none): a context with POMGPU_UVMEAN_PASS and one without, every array, scratch included.
    onload=False: a build that keeps the pass (the fp32-arithmetic variant: no fp64 arithmetic in its stencil kernels) must say so in
    its profile -- the pass on both sides -- and give the same bits all the same"""
    a = make_case(case, *size, dte=6.0, isplit=ISPLIT)
    oracle_finish_initial(a)
    b = a.copy()
    ga, gb = PomGpu(a, libpath=lib), PomGpu(b, libpath=lib)
    ga.switch("UVMEAN_PASS", 1)
    ga.prof_begin()
    gb.prof_begin()
    ga.run(steps)
    gb.run(steps)
    pa, pb = ga.prof_end(), gb.prof_end()
    assert passes(pa) == steps - 1 and passes(pb) == (0 if onload else steps - 1), (pa, pb)
    for name in (ADVQ2, ADVT2, ADVUV, TAIL, RIM):                # the profile names of the kernels stay
        assert launches(pa, name) == launches(pb, name) == steps - 1, (name, pa, pb)
    ga.download()
    gb.download()
    assert not diff(a, b, skip=()), diff(a, b, skip=())
    ex = exercises(a)
    assert all(ex[k] for k in ALL_NEEDS), ex
    ga.close()
    gb.close()
