"""TEST HELPER: the round trips through tclim, sclim (k_ts_update) and rmean (k_profq) read only where they change bits, on one tile
(k_advt2_col's RTF words, k_baropg_rs's column plane; pomgpu_ctx::rt_words, rt_cols).

Shared by tests/test_rt_flags_emulated.py (host builds of the kernel sources) and tests/test_gpu_rt_flags.py (the device): every check
takes the library to load.  The bar is bit for bit on 64-bit patterns over every array of BLK2D + BLK3D but the scratch set, against
the CPU oracle, which makes every round trip in place; the same run under POMGPU_RT_LOAD (today's reads) and run(n) against n x run(1)
give the same bits.  Which launches read flags is taken from the event profile's counts ts_rt_flags and profq_rm_flags.

Every run starts one oracle step in (iint = 1 has no 3-D body) and makes four more: level kb of tb differs under its round trip from
the third step (copy_kb leaves values there that the advection never held).

The climatology takes three forms.  "case": as the case makes it -- T, S next to tclim, sclim, sigma-density next to rmean: no word of
T / S has a bit set, the column plane marks the cells holding -0.0 (masked columns).  "all": every cell of tclim, sclim, rmean becomes
y * 1000 + 3, far from the field: the subtraction rounds, nearly every bit is set.  "part": a seeded 30 % of the cells, drawn cell by
cell over the whole array, so that set and clear bits share words, cache lines, rows and column blocks.

A climatology a thousand times the field is a pressure gradient and a diffusion of T the model was never meant to take: at dte = 6 s the
oracle itself meets its velocity check (vamax 5e41) in the third step.  The two perturbed forms therefore step with dte = 0.6 ms (dti =
18 ms; swtch = 1 day keeps the step count of the switch inside an int): after the five steps u stays below 25 m/s, every field is finite
and error_status is 0 in every shape -- inputs_are_what_they_claim checks that.  The round trips do not care about the time step."""
import numpy as np

from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D, P3
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial

SCRATCH = {"tps", "fluxua", "fluxva", "zflux"}
ISPLIT = 30
TS, RM, TSK, PROFQ = "ts_rt_flags", "profq_rm_flags", "k_ts_update", "k_profq"
# 8x8x6, 20x17x6: kbm1 = 5, one column block.  65x49x21: two column blocks (62 + 3 columns) -- a 64-lane wavefront of k_ts_update reads two words --
# and 49 rows = six 8-row workgroups and one row.  The archipelago: -0.0 in rho on interior land, flagged and unflagged columns in one cache
# line.  130x17x6: three column blocks
SHAPES = [("seamount", (8, 8, 6)), ("seamount", (20, 17, 6)), ("seamount", (65, 49, 21)), ("archipelago", (65, 49, 21)), ("seamount", (130, 17, 6))]
SHAPE_IDS = ["8x8x6", "20x17x6", "65x49x21", "archipelago", "130x17x6"]
CLIMS = ["case", "all", "part"]
NSTEPS = 4


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


def diff(a, b, names=None, skip=SCRATCH):
    return [n for n in (names or BLK2D + BLK3D) if n not in skip and not same_bits(a.field(n), b.field(n))]


def perturb(st, clim, seed=7):
    """tclim, sclim, rmean of st in the form `clim`, in place"""
    if clim == "case":
        return
    rng = np.random.default_rng(seed)
    for n in ("tclim", "sclim", "rmean"):
        y = st.field(n)
        pick = np.ones(y.shape, bool) if clim == "all" else rng.random(y.shape) < 0.3
        y[pick] = y[pick] * 1000. + 3.


def round_trip_changes(x, y):
    rt = (x - y) + y
    return rt.view(np.uint64) != x.view(np.uint64)


_STARTS = {}


def start(case="seamount", size=(65, 49, 21), clim="case"):
    """(oracle's state NSTEPS further, the library's copy) one step in, the climatology in its form: the oracle runs once per (case, size,
    clim) and is shared, unchanged, by every check"""
    key = (case, size, clim)
    if key not in _STARTS:
        a = make_case(case, *size, isplit=ISPLIT, **(dict(dte=6.0) if clim == "case" else dict(dte=6.e-4, swtch=1.0)))
        oracle_finish_initial(a)
        OracleTile(a).run(1)
        perturb(a, clim)
        b = a.copy()
        OracleTile(a).run(NSTEPS)
        assert int(a.error_status) == 0
        _STARTS[key] = (a, b)
    a, b = _STARTS[key]
    return a, b.copy()


def gpu(st, lib, rt_load=False):
    g = PomGpu(st, libpath=lib)                               # the perturbed arrays go in by upload, before the first step
    if rt_load:
        g.switch("RT_LOAD", 1)
    return g


def count(prof, name):
    return prof.get(name, (0, 0.0))[0]


def counts(prof):
    return count(prof, TS), count(prof, RM), count(prof, TSK), count(prof, PROFQ)


def read3(g, name):
    out = np.empty_like(g.st.field(name))
    g._chk(g.L.pomgpu_download_3d(g.h, P3[name], g._p(out)), "download_3d")
    return out


def write3(g, name, new):
    g._chk(g.L.pomgpu_upload_3d(g.h, P3[name], g._p(np.ascontiguousarray(new))), "upload_3d")


def lateral_to_internal(g, n, between=None):
    """one internal step routine by routine (advance.f:6-59); `between` runs behind lateral_viscosity"""
    g.set_con(iint=n)
    g.call("get_time")
    g.get_con()
    g.call("lateral_viscosity")
    if between:
        between()
    g.call("mode_interaction")
    for iext in range(1, ISPLIT + 1):
        g.set_con(iext=iext)
        g.call("mode_external")
    g.set_con(iext=ISPLIT + 1)
    g.call("mode_internal")
    g.check_velocity()


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def inputs_are_what_they_claim(case, size, clim):
    """the three forms on the state the runs start from, interior cells of levels 1..kbm1: "case" sets no bit for T, S and only cells
    holding -0.0 for rho; "part" sets 0.2 .. 0.4 of the bits of T and of rho (the pick is 30 %); "all" more than half.  (S of the
    seamount is 35 next to an sclim of 35: whole numbers make every round trip exact, its bits stay clear -- T's set the shared word.)
    The oracle's five steps stay finite with error_status 0"""
    a, b = start(case, size, clim)
    kbm1 = b.kb - 1
    inner = (slice(0, kbm1), slice(1, -1), slice(1, -1))
    for x, y in (("tb", "tclim"), ("sb", "sclim"), ("rho", "rmean")):
        ch = round_trip_changes(b.field(x), b.field(y))[inner]
        if clim == "case" and x != "rho":
            assert not ch.any(), (x, int(ch.sum()))
        elif clim == "case":
            neg0 = b.field(x).view(np.uint64)[inner] == np.uint64(1 << 63)
            assert np.array_equal(ch, neg0), (x, int(ch.sum()), int(neg0.sum()))
        elif x == "sb":
            assert ch.mean() < (0.4 if clim == "part" else 1.01), (x, ch.mean())
        elif clim == "part":
            assert 0.2 < ch.mean() < 0.4, (x, ch.mean())
        else:
            assert ch.mean() > 0.5, (x, ch.mean())
    assert a.iint == b.iint + NSTEPS and int(a.error_status) == 0
    for n in BLK2D + BLK3D:
        assert np.all(np.isfinite(a.field(n))), n


def same_bits_every_way(lib, case, size, clim, oracle=True):
    """run(4) with flags, run(4) under POMGPU_RT_LOAD and 4 x run(1) with flags: byte-identical among themselves and equal to four oracle
    steps; every k_ts_update and k_profq launch of the flag runs read flags, none under the switch"""
    a, b = start(case, size, clim)
    c, d = b.copy(), b.copy()
    gb, gc, gd = gpu(b, lib), gpu(c, lib, rt_load=True), gpu(d, lib)
    gb.prof_begin(); gb.run(NSTEPS); pb = gb.prof_end()
    gc.prof_begin(); gc.run(NSTEPS); pc = gc.prof_end()
    gd.prof_begin()
    for _ in range(NSTEPS):
        gd.run(1)
    pd = gd.prof_end()
    assert counts(pb) == (NSTEPS,) * 4 and counts(pd) == (NSTEPS,) * 4 and counts(pc) == (0, 0, NSTEPS, NSTEPS), (pb, pc, pd)
    for g in (gb, gc, gd):
        g.download()
    assert not diff(b, c) and not diff(b, d), (diff(b, c), diff(b, d))
    if oracle:
        assert a.iint == b.iint and not diff(a, b), diff(a, b)
    for g in (gb, gc, gd):
        g.close()


def switch_on_a_live_context(lib):
    """POMGPU_RT_LOAD is read at launch time: flipped between two run(2), each half counts its own way and the bits are the oracle's"""
    a, b = start("archipelago", (65, 49, 21), "part")
    g = gpu(b, lib)
    g.prof_begin(); g.run(2); p0 = g.prof_end()
    g.switch("RT_LOAD", 1)
    g.prof_begin(); g.run(1); p1 = g.prof_end()
    g.switch("RT_LOAD", None)
    g.prof_begin(); g.run(1); p2 = g.prof_end()
    assert counts(p0) == (2, 2, 2, 2) and counts(p1) == (0, 0, 1, 1) and counts(p2) == (1, 1, 1, 1), (p0, p1, p2)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def decision_address_handed_out(lib):
    """after pomgpu_device_3d on rmean the library no longer sees every writer: no launch reads flags"""
    a, b = start("archipelago", (65, 49, 21), "part")
    g = gpu(b, lib)
    assert g.device_ptr("rmean")
    g.prof_begin(); g.run(NSTEPS); prof = g.prof_end()
    assert counts(prof) == (0, 0, NSTEPS, NSTEPS), prof
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def decision_advt2_single(lib):
    """POMGPU_ADVT2_SINGLE: T and S advected one by one, by kernels that form no words -- k_ts_update reads tclim, sclim whole; rho's plane
    does not depend on it"""
    a, b = start("seamount", (65, 49, 21), "part")
    g = gpu(b, lib)
    g.switch("ADVT2_SINGLE", 1)
    g.prof_begin(); g.run(NSTEPS); prof = g.prof_end()
    assert counts(prof) == (0, NSTEPS, NSTEPS, NSTEPS), prof
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def decision_stand_alone_pair(lib):
    """pomgpu_baropg and pomgpu_profq called directly: baropg makes the round trip in place, profq reads no flag; against the same pair
    under POMGPU_RT_LOAD"""
    _, b = start("archipelago", (65, 49, 21), "part")
    c = b.copy()
    out = []
    for st, rt_load in ((b, False), (c, True)):
        g = gpu(st, lib, rt_load)
        g.prof_begin()
        g.call("baropg_mcc" if int(st.npg) == 2 else "baropg")
        g.call("profq")
        prof = g.prof_end()
        assert counts(prof)[:2] == (0, 0) and count(prof, PROFQ) == 1, prof
        g.download()
        g.close()
    assert not diff(b, c), diff(b, c)


def observer_between_routines(lib, how):
    """an upload or a download between pomgpu_lateral_viscosity and pomgpu_mode_internal stores rho's round trip and drops the column plane:
    that step's k_profq reads no flag (and no rmean), the steps around it do; T / S words live inside mode_internal and are not concerned.
    The upload writes rho's own (round-tripped) values back, so the oracle's four steps remain the reference"""
    a, b = start("archipelago", (65, 49, 21), "part")
    g = gpu(b, lib)

    def look():
        rho = read3(g, "rho")
        if how == "upload":
            write3(g, "rho", rho)

    seen, first = [], int(b.iint) + 1
    for n in range(NSTEPS):
        g.prof_begin()
        lateral_to_internal(g, first + n, look if n == 1 else None)
        seen.append(counts(g.prof_end()))
    assert seen == [(1, 1, 1, 1), (1, 0, 1, 1), (1, 1, 1, 1), (1, 1, 1, 1)], seen
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def upload_changes_rho(lib):
    """another rho uploaded between lateral_viscosity and mode_internal (rho + 0.37: next to rmean no longer, the subtraction rounds):
    its round trip, stored by the upload's materialize for the OLD rho and owed to nobody for the new one, is not applied -- and the plane
    of the old rho, which marks the masked columns alone, must not be used on it.  Against the same sequence under POMGPU_RT_LOAD"""
    _, b = start("archipelago", (65, 49, 21), "case")
    c = b.copy()
    for st, rt_load in ((b, False), (c, True)):
        g = gpu(st, lib, rt_load)

        def swap():
            rho = read3(g, "rho")
            new = rho + 0.37
            ch = round_trip_changes(new, st.field("rmean"))[:-1, 1:-1, 1:-1]
            assert ch.mean() > 0.01, ch.mean()                  # (a stale plane would leave these cells without their round trip)
            write3(g, "rho", new)

        first = int(st.iint) + 1
        g.prof_begin()
        lateral_to_internal(g, first, swap)
        lateral_to_internal(g, first + 1)
        prof = g.prof_end()
        assert count(prof, RM) == (0 if rt_load else 1), prof
        g.download()
        g.close()
    assert not diff(b, c), diff(b, c)
