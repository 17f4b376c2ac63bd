"""TEST HELPER: profu / profv fused with the velocity filter on one tile (k_profuv_filter_reg2), uf and vf of the interior on demand.

Shared by tests/test_uv_tail_fused_emulated.py (host build of the kernel sources, a serial grid) and tests/test_gpu_uv_tail_fused.py
(the device): every check takes the library to load.  The bar is the CPU oracle, bit for bit on 64-bit patterns, over every COMMON
array that is not scratch -- uf, vf included, which the fused kernel does not store on the interior.  The existing suites step with
run(1) + download(); here steps follow each other unobserved."""
import numpy as np

import off_default
from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D, P3
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial

SCRATCH = {"tps", "fluxua", "fluxva", "zflux"}
CASES = ["archipelago", "seamount", "island"]
NAMELISTS = {"default": dict(), "mode4": dict(mode=4), "nadv1": dict(nadv=1), "npg2": dict(npg=2), "off_default": "off_default"}
# (im, jm, kb): a wavefront's 62-column edge inside the interior (65, 66), a flat tile, one interior column at the smallest register kb,
# both sides of a template bound, the benchmark's kb, the largest register kb
SIZES_FUSED = [(65, 49, 21), (66, 50, 21), (128, 12, 21), (8, 8, 6), (20, 14, 24), (20, 14, 25), (20, 14, 50), (20, 14, 64)]
# no interior; kb on either side of the register kernels' range (6..64, whose two ends are fused above): the unfused pair / the scratch
# kernels.  9x8: the smallest grid the fused tail accepts, so nothing but kb = 5 keeps it off
SIZES_FALLBACK = [(7, 9, 6), (20, 14, 65), (9, 8, 5)]
POINTS = ["mode_internal", "check_velocity", "lateral_viscosity", "mode_external_last"]
ISPLIT = 30
FUSED, RIM, UNFUSED, COPY = "k_profuv_filter_reg2", "k_uv_filter_rim", "k_uv_filter_reg2", "k_uvf_copy"
SCRATCH_U, SCRATCH_V = "k_advu_profu", "k_advv_profv"        # advu + profu, advv + profv where kb is outside the register kernels' range


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


def read3(g, name):
    out = np.empty_like(g.st.field(name))
    g._chk(g.L.pomgpu_download_3d(g.h, P3[name], g._p(out)), "download_3d")
    return out


def write3(g, name, new):
    g._chk(g.L.pomgpu_upload_3d(g.h, P3[name], g._p(np.ascontiguousarray(new))), "upload_3d")


def launches(prof, name):
    return prof.get(name, (0, 0.0))[0]


def step_by_routine(g, n, hook=lambda point: None):
    """one internal step as the Fortran host makes it (advance.f:6-59 routine by routine)"""
    g.set_con(iint=n)
    g.call("get_time")
    g.get_con()
    g.call("lateral_viscosity")
    hook("lateral_viscosity")
    g.call("mode_interaction")
    for iext in range(1, ISPLIT + 1):
        g.set_con(iext=iext)
        g.call("mode_external")
    hook("mode_external_last")
    g.set_con(iext=ISPLIT + 1)
    g.call("mode_internal")
    hook("mode_internal")
    g.check_velocity()
    hook("check_velocity")


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def unobserved_steps(lib, case, nml, size, fused=True, calls=(2, 1, 3)):
    """run(2), run(1), run(3) and one download at the end; the profile says which tail ran (iint = 1 skips the 3-D body)"""
    a, b = start(case, nml, size)
    g = PomGpu(b, libpath=lib)
    g.prof_begin()
    for n in calls:
        g.run(n)
    prof = g.prof_end()
    body = sum(calls) - 1
    if fused:
        assert launches(prof, FUSED) == body and launches(prof, RIM) == body and launches(prof, UNFUSED) == 0, prof
    else:
        assert launches(prof, FUSED) == 0 and launches(prof, RIM) == 0, prof
    assert launches(prof, COPY) == 0, prof
    scratch = 0 if 6 <= size[2] <= 64 else body               # the scratch pair runs at exactly the kb the register kernels do not serve
    assert launches(prof, SCRATCH_U) == scratch and launches(prof, SCRATCH_V) == scratch, prof
    OracleTile(a).run(sum(calls))
    g.download()
    assert a.iint == b.iint and not diff(a, b), diff(a, b)
    assert np.any(a.uf[:a.kb - 1] != 0.) and np.any(a.vf[:a.kb - 1] != 0.)   # the comparison of uf, vf is not one of zeros
    g.close()


def routine_by_routine(lib, case, point, name):
    """uf or vf alone downloaded after one kind of call in each of three steps: the oracle's of the last completed step"""
    a, b = start(case, None, warm=2)
    ot = OracleTile(a)
    g = PomGpu(b, libpath=lib)
    first = int(b.iint) + 1
    done = {first - 1: a.field(name).copy()}
    state = {"n": first}

    def hook(p):
        if p != point:
            return
        n = state["n"]
        want = done[n if p in ("mode_internal", "check_velocity") else n - 1]
        assert same_bits(read3(g, name), want), f"{name} read after {p} of step {n}"

    for n in range(first, first + 3):
        ot.run(1)
        done[n] = a.field(name).copy()
        state["n"] = n
        step_by_routine(g, n, hook)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def writer_after_steps(lib, what, tmp_path=None):
    a, b = start("archipelago", None, warm=1)
    g = PomGpu(b, libpath=lib)
    g.run(3)                                                  # uf, vf of the interior pending
    OracleTile(a).run(3)
    if what == "u":                                           # the copy is taken from the u before the caller's
        write3(g, "u", a.u * 1.5 + 1.0e-3)
        assert same_bits(read3(g, "uf"), a.uf) and same_bits(read3(g, "vf"), a.vf)
        assert same_bits(read3(g, "u"), np.ascontiguousarray(a.u * 1.5 + 1.0e-3))
    elif what == "uf":                                        # the caller's uf wins, and stays
        write3(g, "uf", a.uf * 0. + 7.0)
        assert np.all(read3(g, "uf") == 7.0) and same_bits(read3(g, "vf"), a.vf)
        g.download()
        assert np.all(b.uf == 7.0) and diff(a, b) == ["uf"]
    elif what == "state":
        c = a.copy()
        c.uf[...] = 7.0
        c.u[...] = a.u * 1.5
        g.upload(c)
        assert np.all(read3(g, "uf") == 7.0) and same_bits(read3(g, "vf"), a.vf)
    elif what == "restart":                                   # the writer brings the mirrors up to date: two copies by it, none after
        g.prof_begin()
        g.write_file("restart", tmp_path / "restart.nc", title="archipelago", time_start="2000-01-01 00:00:00 +00:00")
        g.io_wait()
        assert launches(g.prof_end(), COPY) == 2
        g.prof_begin()
        g.download()
        assert launches(g.prof_end(), COPY) == 0
        assert not diff(a, b), diff(a, b)
    elif what == "tune":                                      # moves every 3-D array; its trial steps advance the model
        g.switch("TUNE_FORCE", 1)
        r = g.tune_placement(1, 2)
        OracleTile(a).run(2 * r["tried"])
        g.download()
        assert not diff(a, b), diff(a, b)
        g.run(2)
        OracleTile(a).run(2)
        g.download()
        assert not diff(a, b), diff(a, b)
    g.close()


def address_handed_out(lib):
    a, b = start("archipelago", None, warm=1)
    g = PomGpu(b, libpath=lib)
    g.run(2)
    g.prof_begin()
    assert g.device_ptr("t")                                  # any 3-D address: the pending copy is made, the fusion ends
    assert launches(g.prof_end(), COPY) == 2
    g.prof_begin()
    g.run(3)
    prof = g.prof_end()
    assert launches(prof, FUSED) == 0 and launches(prof, UNFUSED) == 3 and launches(prof, COPY) == 0, prof
    g.download()
    OracleTile(a).run(5)
    assert not diff(a, b), diff(a, b)
    g.close()


def switch_flipped_live(lib):
    a, b = start("archipelago", None, warm=1)
    ot = OracleTile(a)
    g = PomGpu(b, libpath=lib)
    g.run(2)                                                  # pending
    ot.run(2)
    g.switch("UV_NOFUSE", 1)
    g.prof_begin()
    g.run(1)                                                  # the unfused pair stores uf, vf: the flag is dropped, no copy
    ot.run(1)
    assert same_bits(read3(g, "uf"), a.uf)
    prof = g.prof_end()
    assert launches(prof, COPY) == 0 and launches(prof, UNFUSED) == 1 and launches(prof, FUSED) == 0, prof
    g.switch("UV_NOFUSE", None)
    g.run(2)                                                  # pending again
    ot.run(2)
    g.switch("UV_NOFUSE", 1)                                  # the switch does not stand between a pending uf and its reader
    assert same_bits(read3(g, "vf"), a.vf)
    g.run(1)
    ot.run(1)
    g.switch("UV_NOFUSE", None)
    g.run(1)
    ot.run(1)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def lazy_equals_eager(lib, steps=12, case="archipelago", size=(65, 49, 21)):
    """no oracle: a context with POMGPU_UV_NOFUSE and one without, every array, scratch included"""
    a = make_case(case, *size, dte=6.0, isplit=ISPLIT)
    oracle_finish_initial(a)
    b = a.copy()
    ga, gb = PomGpu(a, libpath=lib), PomGpu(b, libpath=lib)
    ga.switch("UV_NOFUSE", 1)
    ga.prof_begin()
    gb.prof_begin()
    ga.run(steps)
    gb.run(steps)
    pa, pb = ga.prof_end(), gb.prof_end()
    assert launches(pa, UNFUSED) == steps - 1 and launches(pa, FUSED) == 0 and launches(pb, FUSED) == steps - 1 and launches(pb, UNFUSED) == 0
    ga.download()
    gb.download()
    assert not diff(a, b, skip=()), diff(a, b, skip=())
    assert np.any(a.uf[:a.kb - 1] != 0.)
    ga.close()
    gb.close()


def launch_counts(lib):
    a, b = start("seamount", None, warm=1)
    g = PomGpu(b, libpath=lib)
    g.prof_begin()
    g.run(5)
    prof = g.prof_end()
    assert launches(prof, FUSED) == 5 and launches(prof, RIM) == 5 and launches(prof, "k_uvb_bottom") == 5, prof
    assert launches(prof, UNFUSED) == 0 and launches(prof, "k_profuv_reg2") == 0 and launches(prof, COPY) == 0, prof
    g.prof_begin()
    g.download()
    prof = g.prof_end()
    assert launches(prof, COPY) == 2, prof                    # one per component
    g.prof_begin()
    g.download()
    assert launches(g.prof_end(), COPY) == 0
    OracleTile(a).run(5)
    assert not diff(a, b), diff(a, b)
    g.close()


def deterministic(lib, steps=20):
    """the same steps twice in one context and once more in a second: identical bits.  Workgroups of the fused kernel rewrite the ub, vb
    that their neighbours' bottom friction reads -- on the device only the order of the workgroups decides what a racing read sees"""
    a = make_case("archipelago", 130, 49, 21, dte=6.0, isplit=ISPLIT)
    oracle_finish_initial(a)
    b, c = a.copy(), a.copy()
    g = PomGpu(a, libpath=lib)
    g.run(steps)
    g.download()                                              # a: the first run
    g.upload(b)                                               # the same context from the initial state again
    g.run(steps)
    g.download()
    g2 = PomGpu(c, libpath=lib)
    g2.run(steps)
    g2.download()
    assert int(a.iint) == steps and not diff(a, b, skip=()) and not diff(a, c, skip=()), (diff(a, b, skip=()), diff(a, c, skip=()))
    g.close()
    g2.close()
