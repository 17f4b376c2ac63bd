"""TEST HELPER: aam and aam2d formed inside advct's march on one tile (k_advct_col<*, true>): no k_aam_pair / k_aam and no k_vint in a step,
the new aam stored to the buffer that is not being read, a parity that says which of the two holds the current aam.

Shared by tests/test_aam_fused_emulated.py (host build of the kernel sources, a serial grid) and tests/test_gpu_aam_fused.py (the
device): every check takes the library to load.  The bar is the CPU oracle, bit for bit on 64-bit patterns, over every COMMON array
that is not scratch -- aam and aam2d included -- and the library's own event profile says which kernels ran.  aam_init is set off zero
(AAM_INIT) so that a rim cell, which keeps it for ever, shows when it is copied wrongly -- and so does a level kb read from the spare
array, which holds zeros there."""
import numpy as np

import off_default
from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D, P3
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial
from w_fused_checks import CASES, NAMELISTS, SIZES, SCRATCH, same_bits, interior   # noqa: F401

ISPLIT = 30
AAM_INIT = 137.5
ADVCT, FUSED, VINT, COPY = "k_advct_col", "advct_aam_fused", "k_vint", "k_aam_copy"
# switches under which the step still takes the fused march: every reader of aam in them is a column kernel that reads the current buffer
STILL_FUSED = ["ADVT2_SINGLE", "ADVQ_SINGLE"]


def diff(a, b, skip=SCRATCH):
    return [n for n in BLK2D + BLK3D if n not in skip and not same_bits(a.field(n), b.field(n))]


def launches(prof, name):
    return prof.get(name, (0, 0.0))[0]


def pair(prof):
    return launches(prof, "k_aam_pair") + launches(prof, "k_aam")


def counts(prof):
    return {"advct": launches(prof, ADVCT), "fused": launches(prof, FUSED), "pair": pair(prof), "vint": launches(prof, VINT), "copy": launches(prof, COPY)}


def start(case, nml=None, size=(65, 49, 21), warm=0):
    """(oracle's state, the library's copy) at the initial state or `warm` steps in; aam_init = AAM_INIT except in the off-default case,
    which has its own (50)"""
    if nml == "off_default":
        a = off_default.off_default_case(case, *size, oracle_finish_initial)
    else:
        a = make_case(case, *size, **dict(dict(dte=6.0, isplit=ISPLIT, aam_init=AAM_INIT), **(nml or {})))
        oracle_finish_initial(a)
    assert float(a.aam_init) != 0. and np.all(a.aam == float(a.aam_init))
    if warm:
        OracleTile(a).run(warm)
    return a, a.copy()


def exercises(a):
    """what the oracle's state must hold after a step for the comparison to guard the fused march"""
    kb, init = a.kb, float(a.aam_init)
    rim = np.ones(a.fsm.shape, dtype=bool)
    rim[1:-1, 1:-1] = False
    return {"aam_new": bool(np.mean(interior(a.aam[:kb - 1]) != init) > 0.9), "rim_keeps_init": bool(np.all(a.aam[:kb - 1][:, rim] == init)),
            "aam2d_varies": bool(np.unique(interior(a.aam2d)).size > a.aam2d.size // 4), "land_inside": bool(np.any(interior(a.fsm) == 0.))}


def read3(g, name):
    out = np.empty_like(g.st.field(name))
    g._chk(g.L.pomgpu_download_3d(g.h, P3[name], g._p(out)), "download_3d")
    return out


def upload3(g, name, new):
    g._chk(g.L.pomgpu_upload_3d(g.h, P3[name], g._p(np.ascontiguousarray(new))), "upload_3d")


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def unobserved_steps(lib, case, nml, size, switch=None, calls=(2, 1, 3), need=(), copies=None):
    """run(2), run(1), run(3) and one download at the end.  Per step (lateral_viscosity runs in every one, the first included): one
    k_advct_col that formed aam, no k_aam_pair, k_aam or k_vint -- or, under POMGPU_AAM_NOFUSE, the pair and k_vint once each.
    copies: the canonical copies the steps themselves may make (None: not counted)"""
    a, b = start(case, nml, size)
    g = PomGpu(b, libpath=lib)
    if switch:
        g.switch(switch, 1)
    g.prof_begin()
    for n in calls:
        g.run(n)
    prof = g.prof_end()
    steps, c = sum(calls), counts(prof)
    if switch == "AAM_NOFUSE":
        assert c == {"advct": steps, "fused": 0, "pair": steps, "vint": steps, "copy": 0}, prof
    else:
        assert c["advct"] == c["fused"] == steps and c["pair"] == 0 and c["vint"] == 0, prof
        assert copies is None or c["copy"] == copies, prof
    OracleTile(a).run(steps)
    g.download()
    assert a.iint == b.iint and not diff(a, b), diff(a, b)
    ex = exercises(a)
    assert all(ex[k] for k in need), ex
    g.close()


def both_parities(lib, mean=False):
    """run(1), run(2), run(3), run(4) of one context with a download after each: the download finds the current aam in the spare array
    after the odd calls (one canonical copy) and in the slot after the even ones (none).  After the first call -- the odd parity --
    a perturbed aam is uploaded, to the oracle alike: the next advct must read it, from the slot.
    mean: with the time-mean output on (pomgpu_set_mean_output), the means against acc = acc + x over the oracle's steps"""
    a, b = start("archipelago")
    ot = OracleTile(a)
    g = PomGpu(b, libpath=lib)
    acc, nacc = {n: np.zeros_like(a.field(n)) for n in PomGpu.MEAN_FIELDS}, 0
    if mean:
        g.set_mean_output(True)
    for n in (1, 2, 3, 4):
        g.run(n)
        for _ in range(n):
            ot.run(1)
            for f in acc:
                acc[f] = acc[f] + a.field(f)
            nacc += 1
        if n == 1:                                            # the odd parity, unobserved so far
            new = np.ascontiguousarray(a.aam * (1.25 + 0.25 * np.cos(np.arange(a.aam.size, dtype=np.float64))).reshape(a.aam.shape))
            twin = a.copy()
            OracleTile(twin).run(1)
            a.aam[...] = new
            g.prof_begin()
            upload3(g, "aam", new)
            assert launches(g.prof_end(), COPY) == 1
            assert same_bits(read3(g, "aam"), new)
            probe = a.copy()
            OracleTile(probe).run(1)
            assert not same_bits(probe.advx, twin.advx) and not same_bits(probe.q2, twin.q2)   # the perturbation reaches advct and advq
            continue
        g.prof_begin()
        g.download()
        assert launches(g.prof_end(), COPY) == n % 2, n
        assert a.iint == b.iint and not diff(a, b), (n, diff(a, b))
    if mean:
        assert g.mean_count() == nacc
        for f in acc:
            assert same_bits(g.mean(f), acc[f] / float(nacc)), f
    ex = exercises(a)                                         # (the rim carries the perturbation now)
    assert ex["aam_new"] and ex["aam2d_varies"] and ex["land_inside"], ex
    g.close()


def restart_at_the_odd_parity(lib, tmp_path):
    """write_file("restart") after three unobserved steps (the current aam is in the spare array): the file's aam is the oracle's.  One
    more step, and pomgpu_read_restart at the odd parity again: the mirrors hold the file, aam included, and two unobserved steps from
    there are the oracle's started from the same state"""
    a, b = start("archipelago")
    g = PomGpu(b, libpath=lib)
    g.run(3)
    OracleTile(a).run(3)
    path = tmp_path / "restart.nc"
    g.write_file("restart", path, title="archipelago", time_start="2000-01-01 00:00:00 +00:00")
    g.io_wait()
    g.run(1)                                                  # the writer has made the slot current: odd again
    g.prof_begin()
    g.read_restart(path)
    assert launches(g.prof_end(), COPY) == 1
    g.download()
    assert same_bits(b.aam, a.aam) and same_bits(b.aam2d, a.aam2d) and same_bits(b.u, a.u) and same_bits(b.q2, a.q2)
    a2 = b.copy()
    OracleTile(a2).run(2)
    g.run(2)
    g.download()
    assert a2.iint == b.iint and not diff(a2, b), diff(a2, b)
    g.close()


def address_handed_out(lib):
    """pomgpu_device_3d(aam) at the odd parity: the slot is made current, and the pair runs from then on"""
    a, b = start("archipelago")
    g = PomGpu(b, libpath=lib)
    g.run(1)
    g.prof_begin()
    assert g.device_ptr("aam")
    assert launches(g.prof_end(), COPY) == 1
    g.prof_begin()
    g.run(3)
    c = counts(g.prof_end())
    assert c == {"advct": 3, "fused": 0, "pair": 3, "vint": 3, "copy": 0}, c
    OracleTile(a).run(4)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def switch_flipped_live(lib):
    """POMGPU_AAM_NOFUSE set and unset between the steps of one context, at the odd parity too: the flip canonicalises"""
    a, b = start("archipelago")
    ot = OracleTile(a)
    g = PomGpu(b, libpath=lib)
    for n, sw, copy in ((1, None, 0), (2, 1, 1), (3, None, 0), (1, 1, 1), (2, None, 0), (2, 1, 0)):
        g.prof_begin()
        g.switch("AAM_NOFUSE", sw)
        g.run(n)
        c = counts(g.prof_end())
        assert c == {"advct": n, "fused": 0 if sw else n, "pair": n if sw else 0, "vint": n if sw else 0, "copy": copy}, (n, sw, c)
        ot.run(n)
    g.switch("AAM_NOFUSE", None)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def stand_alone_entry_points(lib):
    """pomgpu_advct, pomgpu_lateral_viscosity, pomgpu_mode_interaction after three unobserved fused steps (the odd parity): they read
    and write aam in its slot, with their own kernels"""
    for calls in (("advct",), ("lateral_viscosity",), ("lateral_viscosity", "mode_interaction"), ("mode_interaction",)):
        a, b = start("archipelago")
        ot = OracleTile(a)
        g = PomGpu(b, libpath=lib)
        g.run(3)
        ot.run(3)
        g.prof_begin()
        for name in calls:
            g.call(name)
            ot.call(name)
        c = counts(g.prof_end())
        assert c["fused"] == 0 and c["copy"] == 1 and c["pair"] == calls.count("lateral_viscosity") and c["vint"] == calls.count("mode_interaction"), (calls, c)
        g.download()
        assert not diff(a, b), (calls, diff(a, b))
        g.close()


def routine_by_routine(lib):
    """the Fortran host's call sequence keeps the pair (pomgpu_lateral_viscosity does not know that pomgpu_mode_interaction follows):
    per step one k_aam_pair / k_aam and one k_vint as before, and ONE canonical copy in all, where the sequence takes over from fused
    steps at the odd parity -- no copy per step"""
    a, b = start("seamount")
    g = PomGpu(b, libpath=lib)
    g.run(3)
    g.get_con()
    first = int(b.iint) + 1
    g.prof_begin()
    for n in range(first, first + 3):
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
    c = counts(g.prof_end())
    assert c == {"advct": 3, "fused": 0, "pair": 3, "vint": 3, "copy": 1}, c
    OracleTile(a).run(6)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def fused_equals_pair(lib, steps=5, case="archipelago", size=(65, 49, 21), fuses=True):
    """no oracle (the fp32 study builds have none): a context with POMGPU_AAM_NOFUSE and one without, every array, scratch included.
    fuses=False: a build without the fused kernel (the fp32-arithmetic variant keeps its stencil kernels free of fp64 arithmetic) must
    say so in its profile -- the pair on both sides -- and give the same bits all the same"""
    a = make_case(case, *size, dte=6.0, isplit=ISPLIT, aam_init=AAM_INIT)
    oracle_finish_initial(a)
    b = a.copy()
    ga, gb = PomGpu(a, libpath=lib), PomGpu(b, libpath=lib)
    ga.switch("AAM_NOFUSE", 1)
    ga.prof_begin()
    gb.prof_begin()
    ga.run(steps)
    gb.run(steps)
    ca, cb = counts(ga.prof_end()), counts(gb.prof_end())
    assert ca == {"advct": steps, "fused": 0, "pair": steps, "vint": steps, "copy": 0}, ca
    assert cb == ({"advct": steps, "fused": steps, "pair": 0, "vint": 0, "copy": 0} if fuses else ca), cb
    ga.download()
    gb.download()
    assert not diff(a, b, skip=()), diff(a, b, skip=())
    ex = exercises(a)
    assert ex["aam_new"] and ex["aam2d_varies"] and ex["land_inside"], ex
    ga.close()
    gb.close()
