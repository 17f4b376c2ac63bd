"""TEST HELPER: wr (realvertvl, solver.f:2024-2067) formed only when something reads it -- one tile, no exchange.

Shared by tests/test_wr_on_demand_emulated.py (host build of the kernel sources) and tests/test_gpu_wr_on_demand.py (the device):
every check takes the library to load.  The bar is the CPU oracle, bit for bit on 64-bit patterns; wr is compared like any other
array.  The existing suites step with run(1) + download(), which forms wr every step; here steps follow each other unobserved."""
import numpy as np

from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D, P2, P3
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial

SCRATCH = {"tps", "fluxua", "fluxva", "zflux"}
CASES = ["seamount", "basin", "archipelago"]
NAMELISTS = [dict(), dict(nadv=1), dict(mode=2), dict(mode=4), dict(npg=2)]
# where the routine-by-routine host reads wr: after each of the five kinds of call (the external mode twice: a substep in the middle
# and the last one, which has rewritten etf)
POINTS = ["lateral_viscosity", "mode_interaction", "mode_external_mid", "mode_external_last", "mode_internal", "check_velocity"]
ISPLIT = 30


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


def diff(a, b, skip=SCRATCH):
    return [n for n in BLK2D + BLK3D if n not in skip and not same_bits(a.field(n), b.field(n))]


def start(case, nml=None, warm=False, size=(65, 49, 21)):
    """(oracle's state, the library's copy): the initial state (the next step is iint = 1, which skips the 3-D body) or three steps in"""
    a = make_case(case, *size, dte=6.0, isplit=ISPLIT, **(nml or {}))
    oracle_finish_initial(a)
    if warm:
        OracleTile(a).run(3)
    return a, a.copy()


def read_wr(g):
    out = np.empty_like(g.st.field("wr"))
    g._chk(g.L.pomgpu_download_3d(g.h, P3["wr"], g._p(out)), "download_3d")
    return out


def launches(prof, prefix):
    return sum(n for name, (n, _) in prof.items() if name.startswith(prefix))


def step_by_routine(g, n, hook=lambda point: None):
    """one internal step as the Fortran host makes it (advance.f:6-59 routine by routine)"""
    g.set_con(iint=n)
    g.call("get_time")
    g.get_con()
    g.call("lateral_viscosity")
    hook("lateral_viscosity")
    g.call("mode_interaction")
    hook("mode_interaction")
    for iext in range(1, ISPLIT + 1):
        g.set_con(iext=iext)
        g.call("mode_external")
        if iext == 3:
            hook("mode_external_mid")
        if iext == ISPLIT:
            hook("mode_external_last")
    g.set_con(iext=ISPLIT + 1)
    g.call("mode_internal")
    hook("mode_internal")
    g.check_velocity()
    hook("check_velocity")


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def unobserved_steps(lib, case, nml, warm, size=(65, 49, 21), calls=(2, 1, 2)):
    a, b = start(case, nml, warm, size)
    g = PomGpu(b, libpath=lib)
    for n in calls:
        g.run(n)
    OracleTile(a).run(sum(calls))
    g.download()
    assert a.iint == b.iint and not diff(a, b), diff(a, b)
    if warm and int(a.mode) != 2:
        assert np.any(a.wr != 0.)                             # the comparison of wr is not one of zeros
    g.close()


def routine_by_routine(lib, case, warm, point):
    a, b = start(case, None, warm)
    ot = OracleTile(a)
    g = PomGpu(b, libpath=lib)
    first = int(b.iint) + 1
    done = {first - 1: a.wr.copy()}                           # wr of the last completed step, by step number
    state = {"n": first}

    def hook(p):
        if p != point:
            return
        n = state["n"]
        want = done[n if p in ("mode_internal", "check_velocity") else n - 1]
        assert same_bits(read_wr(g), want), f"wr read after {p} of step {n}"

    for n in range(first, first + 3):
        ot.run(1)
        done[n] = a.wr.copy()
        state["n"] = n
        step_by_routine(g, n, hook)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def launch_counts(lib, size=(65, 49, 21)):
    a, b = start("seamount", None, True, size)
    g = PomGpu(b, libpath=lib)
    g.prof_begin()
    g.run(5)
    prof = g.prof_end()
    assert launches(prof, "k_realvertvl") == 0, prof
    g.prof_begin()
    g.download()
    prof = g.prof_end()
    assert launches(prof, "k_realvertvl") == 1, prof
    g.switch("WR_NODEFER", 1)
    g.prof_begin()
    g.run(5)
    prof = g.prof_end()
    assert launches(prof, "k_realvertvl") == 5, prof
    g.download()
    OracleTile(a).run(10)
    assert not diff(a, b), diff(a, b)
    g.close()


def launch_counts_by_routine(lib):
    """check_velocity after every step brings none of the lazily kept arrays up to date: it reads vaf alone"""
    a, b = start("seamount", None, True)
    g = PomGpu(b, libpath=lib)
    first = int(b.iint) + 1
    g.prof_begin()
    for n in range(first, first + 3):
        step_by_routine(g, n)
    prof = g.prof_end()
    assert launches(prof, "k_realvertvl") == 0, prof
    for k in ("k_restore_fields", "k_roundtrip"):             # the full 3-D passes (k_roundtrip_level, one plane, is what deferring rho's round trip leaves)
        assert prof.get(k, (0, 0.0))[0] == 0, (k, prof)
    assert prof["k_ts_update"][0] == 3 and prof["k_profq"][0] == 3   # three full steps did run
    g.download()
    OracleTile(a).run(3)
    assert not diff(a, b), diff(a, b)
    g.close()


def standalone_reads_etf(lib):
    a, _ = start("archipelago", None, True)
    a.etf[...] = a.et + 1.0e-3 * a.fsm * (1.0 + np.arange(a.et.shape[1])[None, :] / 64.0)
    assert np.count_nonzero(a.etf != a.et) > a.et.size // 4
    b = a.copy()
    OracleTile(a).call("realvertvl")
    g = PomGpu(b, libpath=lib)
    g.call("realvertvl")
    g.download()
    assert not diff(a, b), diff(a, b)
    # ... and it clears a pending wr instead of forming it first: one launch
    g.run(2)
    g.prof_begin()
    g.call("realvertvl")
    prof = g.prof_end()
    assert launches(prof, "k_realvertvl") == 1, prof
    OracleTile(a).run(2)
    OracleTile(a).call("realvertvl")
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def writer_between_step_and_read(lib, what):
    a, b = start("seamount", None, True)
    g = PomGpu(b, libpath=lib)
    g.run(2)
    OracleTile(a).run(2)
    if what == "et":
        new = a.et + 0.01 * a.fsm
        g._chk(g.L.pomgpu_upload_2d(g.h, P2["et"], g._p(new)), "upload_2d")
    elif what == "w":
        new = np.ascontiguousarray(a.w * 1.5 + 1.0e-5)
        g._chk(g.L.pomgpu_upload_3d(g.h, P3["w"], g._p(new)), "upload_3d")
    else:                                                     # the whole state, wr's slot included: the caller's wr wins
        c = a.copy()
        c.w[...] = a.w * 1.5
        c.wr[...] = 7.0
        g.upload(c)
        assert np.all(read_wr(g) == 7.0)
        g.close()
        return
    assert same_bits(read_wr(g), a.wr)
    g.close()


def output_file(lib, tmp_path):
    """The output file (write_output_pnetcdf, io_pnetcdf.F:57-410) has no variable for wr -- its `w` is the sigma velocity; the reference
    writes wr to its auxiliary debug file only (:988, :1642), which the library does not produce.  What the writer owes wr is what
    pomgpu_materialize promises: after it, the mirrors are current.  One launch by the writer, none by the read that follows."""
    from scipy.io import netcdf_file
    a, b = start("island", None, False)
    g = PomGpu(b, libpath=lib)
    g.run(3)
    OracleTile(a).run(3)
    g.prof_begin()
    g.write_file("output", tmp_path / "out.nc", title="island", time_start="2000-01-01 00:00:00 +00:00")
    g.io_wait()
    prof = g.prof_end()
    assert launches(prof, "k_realvertvl") == 1, prof
    with netcdf_file(str(tmp_path / "out.nc"), "r", mmap=False) as f:
        assert "wr" not in f.variables
        assert np.array_equal(f.variables["w"][0], a.w) and np.array_equal(f.variables["rho"][0], a.rho[:a.kb - 1])
    g.prof_begin()
    wr = read_wr(g)
    prof = g.prof_end()
    assert launches(prof, "k_realvertvl") == 0 and same_bits(wr, a.wr)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def address_handed_out(lib, name):
    a, b = start("seamount", None, True)
    g = PomGpu(b, libpath=lib)
    g.run(1)
    assert g.device_ptr(name)
    g.prof_begin()
    g.run(3)
    prof = g.prof_end()
    assert launches(prof, "k_realvertvl") == 3, prof
    g.download()
    OracleTile(a).run(4)
    assert not diff(a, b), diff(a, b)
    g.close()


def switch_flipped_live(lib):
    a, b = start("archipelago", None, True)
    ot = OracleTile(a)
    g = PomGpu(b, libpath=lib)
    g.run(2)                                                  # wr pending
    ot.run(2)
    g.switch("WR_NODEFER", 1)
    g.run(1)                                                  # formed at the end of its own step again
    ot.run(1)
    g.prof_begin()
    assert same_bits(read_wr(g), a.wr)
    assert launches(g.prof_end(), "k_realvertvl") == 0
    g.switch("WR_NODEFER", None)
    g.run(2)                                                  # pending again
    ot.run(2)
    g.switch("WR_NODEFER", 1)                                 # the switch does not stand between a pending wr and its reader
    assert same_bits(read_wr(g), a.wr)
    g.run(1)
    ot.run(1)
    g.switch("WR_NODEFER", None)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def dti2_changed_while_pending(lib):
    a, b = start("seamount", None, True)
    g = PomGpu(b, libpath=lib)
    g.run(2)
    OracleTile(a).run(2)
    g.get_con()
    g.set_con(dti2=float(b.dti2) * 2.0)
    assert same_bits(read_wr(g), a.wr)
    g.close()


def lazy_equals_eager(lib, steps=4):
    """no oracle: a context with POMGPU_WR_NODEFER and one without, every array"""
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=ISPLIT)
    oracle_finish_initial(a)
    b = a.copy()
    ga, gb = PomGpu(a, libpath=lib), PomGpu(b, libpath=lib)
    ga.switch("WR_NODEFER", 1)
    ga.prof_begin()
    gb.prof_begin()
    ga.run(steps)
    gb.run(steps)
    assert launches(ga.prof_end(), "k_realvertvl") == steps and launches(gb.prof_end(), "k_realvertvl") == 0
    ga.download()
    gb.download()
    assert not diff(a, b, skip=()), diff(a, b, skip=())
    assert np.any(a.wr != 0.)
    ga.close()
    gb.close()
