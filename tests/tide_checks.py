"""TEST HELPER: the checks of the tide (harmonic open-boundary forcing and harmonic analysis), shared by tests/test_tides_emulated.py (host
build of the kernel sources) and tests/test_gpu_tides.py (the device): every check takes the library to load.  The bar of the forcing is the
CPU oracle with base + tide in its boundary lines (tests/tide_expect.py), bit for bit on 64-bit patterns; the bar of the sums is a numpy
restatement, bit for bit; the bar of the solve is numpy.linalg.solve within 64 eps cond(M) max|x|."""
import numpy as np
import pytest

import tide_expect as X
from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D, P2
from extpom_amd.model import PomGpu
from extpom_amd.lib import PomGpuError
from oracle.pyoracle import OracleTile, oracle_finish_initial

SCRATCH = {"tps", "fluxua", "fluxva", "zflux"}
CASES = [("island", (20, 17, 6)), ("archipelago", (8, 8, 6)), ("seamount", (65, 49, 21))]
NCS = [1, 2, 8]
STEPS = 4
ISPLIT = {"island": 6, "archipelago": 6, "seamount": 7}      # odd at the largest: the pair path ends in a substep alone
# the switches the existing external-mode tests reach each path with, and the kernel whose launches show that it ran
PATHS = {
    "default": ((), "k_ext_step_adv"),
    "mode2": ((), "k_ext_step"),                              # mode 2 has no advave in the substep: the kernel without it
    "march": ((("EXT_MARCH", 1), ("EXT_ROWS", 6)), "k_ext_step_adv"),
    "split": ((("EXT_SPLIT", 1),), "k_ext_uvaf"),
    "rim_kernel": ((("ADVAVE_SEPARATE", 1), ("EXT_RIM_KERNEL", 1)), "k_ext_step_rim"),
    "pair": ((("EXT_PAIR", 1), ("EXT_ROWS2", 5)), "k_ext_pair"),
    "loop": ((("EXT_LOOP", 1),), "k_ext_loop"),
}
DEVICE_ONLY = ("pair", "loop")                                 # the host build has neither (neighbour lanes, the grid barrier): shown excluded there


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


def diff(a, b, skip=SCRATCH):
    return [n for n in BLK2D + BLK3D if n not in skip and not same_bits(a.field(n), b.field(n))]


def start(case, size, nml=None, lramp=False, time0=0.0, isplit=None):
    a = make_case(case, *size, dte=6.0, isplit=isplit or ISPLIT[case], **(nml or {}))
    oracle_finish_initial(a)
    if lramp:
        a.lramp = True
    if time0:
        a.time0 = time0
        a.time = time0
    return a, a.copy()


def counts(prof):
    return {k: n for k, (n, _) in prof.items()}


def refused(fn, text):
    with pytest.raises(PomGpuError) as e:
        fn()
    assert text in str(e.value), str(e.value)


# ---- 1: the forcing against the oracle ---------------------------------------------------------------------------------------------------------
def forcing(lib, case, size, nc, with_un, nml=None, lramp=False, time0=0.0, path="default", sides=X.SIDES, steps=STEPS, isplit=None, excluded=False):
    a, b = start(case, size, nml, lramp, time0, isplit)
    im, jm = size[0], size[1]
    omega = X.OMEGA[:nc]
    lines = X.make_lines(nc, im, jm, with_un, sides)
    coef = X.coefficients(lines, nc, im, jm)
    bd0 = b.bdry.copy()
    g = PomGpu(b, libpath=lib)
    switches, kernel = PATHS[path]
    for name, val in switches:
        g.switch(name, val)
    g.set_tides(omega=omega, **lines)
    assert g.tide_count() == nc
    g.prof_begin()
    g.run(steps)
    prof = counts(g.prof_end())
    g.download()
    g.close()
    if excluded:
        assert kernel not in prof, prof                       # the path is not one this build or this shape takes: the dispatch left it out
    else:
        assert prof.get(kernel, 0) > 0, (path, sorted(prof))  # the path under test did run
    assert prof.get("k_tide_table", 0) == steps, prof
    X.oracle_steps(a, omega, coef, steps)
    assert int(a.iint) == int(b.iint) and int(b.error_status) == 0
    assert not diff(a, b), (case, size, nc, with_un, path, diff(a, b))
    assert same_bits(b.bdry, bd0) and same_bits(a.bdry, bd0)  # the stored boundary arrays keep their bits
    return a


def tide_matters(lib):
    """the comparison is not one of a tide that does nothing: with the tide elb, uab, vab differ from the tide-free oracle, and a tide with
    normal velocities differs from the one without"""
    a = forcing(lib, "island", (20, 17, 6), 2, True)
    a0 = forcing(lib, "island", (20, 17, 6), 2, False)
    free, _ = start("island", (20, 17, 6))
    OracleTile(free).run(STEPS)
    for f in ("elb", "uab", "vab", "u", "t"):
        assert not same_bits(a.field(f), free.field(f)), f
    assert not same_bits(a.elb, a0.elb)


def phasors(lib):
    """pomgpu_tide_phasors equals the Python phasors bit for bit: a libm difference shows up here and not everywhere"""
    _, b = start("archipelago", (8, 8, 6), time0=0.75)
    g = PomGpu(b, libpath=lib)
    g.set_tides(omega=X.OMEGA)
    for iint in (1, 2, 7, 1000, 123457):
        for iext in (1, 2, ISPLIT["archipelago"]):
            got = g.tide_phasors(iint, iext)
            want = np.array(X.phasors(X.OMEGA, X.tide_time(b, iint, iext)))
            assert same_bits(got, want), (iint, iext)
    g.close()


def stand_alone(lib):
    """a host that strings the routines together: the tide enters its pomgpu_mode_external calls alike"""
    from wr_on_demand_checks import step_by_routine
    import wr_on_demand_checks as W
    a, b = start("island", (20, 17, 6), isplit=W.ISPLIT)
    nc = 2
    lines = X.make_lines(nc, 20, 17)
    g = PomGpu(b, libpath=lib)
    g.set_tides(omega=X.OMEGA[:nc], **lines)
    for n in (1, 2, 3):
        step_by_routine(g, n)
    g.download()
    g.close()
    X.oracle_steps(a, X.OMEGA[:nc], X.coefficients(lines, nc, 20, 17), 3)
    assert not diff(a, b), diff(a, b)


# ---- 2: tiles ---------------------------------------------------------------------------------------------------------------------------------
TILE_GRID, TILE_KB, TILE_ISPLIT, TILE_STEPS, TILE_NC = (67, 59), 11, 10, 3, 2


def run_tiles(lib, nx, ny, tides):
    """nx x ny tiles of island under the wide-halo external mode, one host thread each; {rank: (tile, state, (rounds, side rounds))}"""
    import threading
    from extpom_amd import decomp
    from extpom_amd.cases import finish_initial
    from forcing_files_checks import Board, device_mover, host_mover
    mover = host_mover if lib is not None else device_mover
    IMg, JMg = TILE_GRID
    world = nx * ny
    iml, jml = decomp.local_size(IMg, JMg, nx, ny)
    tiles = [decomp.make_tile(r, IMg, JMg, iml, jml, n_proc=world) for r in range(world)]
    board, out, errs = Board(world), {}, []
    lines = X.make_lines(TILE_NC, IMg, JMg)

    def rank(r):
        try:
            tile = tiles[r]
            st = make_case("island", IMg, JMg, TILE_KB, tile=tile, dte=6.0, isplit=TILE_ISPLIT)
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
            if tides and r % 2 == 0:
                g.set_tides(omega=X.OMEGA[:TILE_NC], im_global=IMg, jm_global=JMg, **lines)      # before the extended tile exists ...
            assert g.set_wide_external(True, min(t.im for t in tiles), min(t.jm for t in tiles))
            if tides and r % 2 == 1:
                g.set_tides(omega=X.OMEGA[:TILE_NC], im_global=IMg, jm_global=JMg, **lines)      # ... and behind it

            def dens(s, a, b, c):
                g.upload(s); g.call("dens", a, b, c); g.download(s)

            def baropg(s):
                g.upload(s); g.call("baropg_mcc" if int(s.npg) == 2 else "baropg"); g.download(s)

            finish_initial(st, dens, baropg)
            g.upload(st)
            board.barrier.wait()
            r0, s0 = g.exchange_rounds(), g.exchange_rounds_side()
            g.run(TILE_STEPS)
            rounds = (g.exchange_rounds() - r0, g.exchange_rounds_side() - s0)
            g.download()
            assert int(st.error_status) == 0
            g.close()
            out[r] = (tile, st, rounds)
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


def tiles(lib, nx=2, ny=2):
    """2 x 2 tiles with the tide equal the single tile with the tide on the cells they own, bit for bit; the message rounds are those without"""
    IMg, JMg = TILE_GRID
    one = make_case("island", IMg, JMg, TILE_KB, dte=6.0, isplit=TILE_ISPLIT)
    oracle_finish_initial(one)
    free = one.copy()
    g = PomGpu(one, libpath=lib)
    g.set_tides(omega=X.OMEGA[:TILE_NC], **X.make_lines(TILE_NC, IMg, JMg))
    g.run(TILE_STEPS)
    g.download()
    g.close()
    OracleTile(free).run(TILE_STEPS)
    assert not same_bits(one.elb, free.elb)
    on, off = run_tiles(lib, nx, ny, True), run_tiles(lib, nx, ny, False)
    bad = []
    for r, (tile, st, rounds) in on.items():
        io, jo, im, jm = tile.i_off, tile.j_off, tile.im, tile.jm
        sl_j = slice(0 if jo == 0 else 1, jm if jo + jm == JMg else jm - 1)       # the cells the tile owns
        sl_i = slice(0 if io == 0 else 1, im if io + im == IMg else im - 1)
        for f in ("elb", "el", "uab", "vab", "ua", "va", "etf", "utf", "vtf", "u", "v", "t", "s"):
            x, ref = st.field(f), one.field(f)
            if x.ndim == 3:
                x, ref = x[:TILE_KB - 1], ref[:TILE_KB - 1]
            ref = ref[..., jo:jo + jm, io:io + im][..., sl_j, sl_i]
            if not same_bits(ref, x[..., :jm, :im][..., sl_j, sl_i]):
                bad.append((r, f))
        assert rounds == off[r][2], (r, rounds, off[r][2])
    assert not bad, bad


# ---- 3: off means off ----------------------------------------------------------------------------------------------------------------------------
def off_means_off(lib, case="island", size=(20, 17, 6)):
    a, b = start(case, size)
    g0 = PomGpu(a, libpath=lib)                               # never heard of tides
    g0.prof_begin()
    g0.run(5)
    p0 = counts(g0.prof_end())
    g0.download()
    g0.close()
    g = PomGpu(b, libpath=lib)
    g.set_tides(omega=X.OMEGA[:3], **X.make_lines(3, size[0], size[1]))
    g.set_tides()                                             # the table cleared
    assert g.tide_count() == 0
    g.prof_begin()
    g.run(5)
    p1 = counts(g.prof_end())
    g.download()
    assert p1 == p0, {k: (p0.get(k), p1.get(k)) for k in set(p0) | set(p1) if p0.get(k) != p1.get(k)}
    assert not diff(a, b) and same_bits(a.bdry, b.bdry)
    g.close()


def zero_tide_is_no_tide(lib, case="island", size=(20, 17, 6)):
    a, b = start(case, size)
    g0 = PomGpu(a, libpath=lib)
    g0.prof_begin()
    g0.run(5)
    p0 = counts(g0.prof_end())
    g0.download()
    g0.close()
    g = PomGpu(b, libpath=lib)
    g.set_tides(omega=X.OMEGA[:3], **X.make_lines(3, size[0], size[1], scale=0.0))
    g.prof_begin()
    g.run(5)
    p1 = counts(g.prof_end())
    g.download()
    g.close()
    assert not diff(a, b), diff(a, b)
    assert p1.pop("k_tide_table") == 5                        # one launch per internal step is all the tide adds; every other count is as without
    assert p1 == p0, {k: (p0.get(k), p1.get(k)) for k in set(p0) | set(p1) if p0.get(k) != p1.get(k)}


# ---- 4: the analysis ---------------------------------------------------------------------------------------------------------------------------
FIELDS = PomGpu.HARMONIC_FIELDS


def harmonic_sums(lib, steps, every, nc=2, case="island", size=(20, 17, 6)):
    """sums and matrix bit for bit against the numpy restatement: the library steps one step at a time and the fields are downloaded behind each"""
    _, b = start(case, size)
    omega = X.OMEGA[:nc]
    g = PomGpu(b, libpath=lib)
    g.set_tides(omega=omega, **X.make_lines(nc, size[0], size[1]))
    g.set_harmonic_analysis(True, every=every)
    np_ = 1 + 2 * nc
    sums = {f: np.zeros((np_,) + b.field(f).shape) for f in FIELDS}
    M = np.zeros((np_, np_))
    n, t2 = 0, [0.0, 0.0]
    for _ in range(steps):
        g.run(1)
        g.download()
        if int(b.iint) % every:
            continue
        t = X.sample_time(b, int(b.iint))
        bas = X.basis(omega, t)
        for f in FIELDS:
            X.accumulate_field(sums[f], b.field(f), bas)
        X.accumulate_matrix(M, bas)
        t2 = [t if n == 0 else t2[0], t]
        n += 1
    assert g.harmonic_count() == n
    Mg, tg = g.harmonic_matrix()
    assert same_bits(Mg, M) and (n == 0 or list(tg) == t2)
    for f in FIELDS:
        assert same_bits(g.harmonic_sums(f), sums[f]), f
    if n:
        assert np.any(sums["elb"][1] != 0.0)
    g.harmonic_reset()
    assert g.harmonic_count() == 0 and not g.harmonic_sums("elb").any() and not g.harmonic_matrix()[0].any()
    g.close()


def solve_bound(M, x):
    return 64.0 * np.finfo(np.float64).eps * np.linalg.cond(M) * np.abs(x).max()


def harmonic_solve(lib, nc=2, case="island", size=(20, 17, 6)):
    """coefficients against numpy.linalg.solve on the same sums; the window is long enough for cond(M) < 100, which the test asserts"""
    _, b = start(case, size)
    b.dti = 1800.0                                            # the analysis alone: samples half an hour apart, 48 of them (a day)
    omega = (X.OMEGA[0], X.OMEGA[4])[:nc]
    g = PomGpu(b, libpath=lib)
    g.set_tides(omega=omega)                                  # a table with no ON side
    g.set_harmonic_analysis(True)
    rng = np.random.default_rng(5)
    for n in range(1, 49):
        g.set_con(iint=n)
        for q, f in enumerate(FIELDS):
            x = rng.standard_normal(b.field(f).shape) + 0.3 * q
            g._chk(g.L.pomgpu_upload_2d(g.h, P2[f], g._p(x)), "upload_2d")
        g.harmonic_accumulate()
    M, _ = g.harmonic_matrix()
    assert np.linalg.cond(M) < 100.0, np.linalg.cond(M)
    for f in FIELDS:
        s = g.harmonic_sums(f)
        want = np.linalg.solve(M, s.reshape(s.shape[0], -1)).reshape(s.shape)
        got = g.harmonic_solve(f)
        err = np.abs(got - want).max()
        assert err <= solve_bound(M, want), (f, err, solve_bound(M, want))
    g.close()


def closed_form(lib, case="island", size=(20, 17, 6)):
    """elb = Z0 + sum A cos(omega t_n - g) uploaded before each harmonic_accumulate over an integer number of periods: Z0, A, g come back
    within the solve's bound, which pins the sign of the phase"""
    _, b = start(case, size)
    period = 12.0 * 3600.0
    omega = (2.0 * np.pi / period, 2.0 * np.pi / (2.0 * period))          # two periods and one period in a window of a day
    b.dti = 900.0
    nsamp = int(2 * period / b.dti)
    g = PomGpu(b, libpath=lib)
    g.set_tides(omega=omega)
    g.set_harmonic_analysis(True)
    shape = b.elb.shape
    jj, ii = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    Z0 = 0.2 + 0.01 * ii
    A = [0.5 + 0.02 * jj, 0.1 + 0.01 * ii]
    G = [np.mod(10.0 + 7.0 * ii + 3.0 * jj, 360.0), np.mod(200.0 + 11.0 * jj, 360.0)]
    for n in range(1, nsamp + 1):
        g.set_con(iint=n)
        t = X.sample_time(b, n)
        x = Z0 + sum(A[c] * np.cos(omega[c] * t - np.deg2rad(G[c])) for c in range(2))
        g._chk(g.L.pomgpu_upload_2d(g.h, P2["elb"], g._p(np.ascontiguousarray(x))), "upload_2d")
        g.harmonic_accumulate()
    M, (t0, t1) = g.harmonic_matrix()
    assert g.harmonic_count() == nsamp and t0 == X.sample_time(b, 1) and t1 == X.sample_time(b, nsamp)
    assert np.linalg.cond(M) < 100.0
    coef = g.harmonic_solve("elb")
    want = np.stack([Z0] + [f(np.deg2rad(G[c])) * A[c] for c in range(2) for f in (np.cos, np.sin)])
    # the signal is in the basis's span, so the residual is the rounding of the samples and sums (eps max|x| each, times the matrix's condition)
    bound = solve_bound(M, want)
    assert np.abs(coef - want).max() <= bound, (np.abs(coef - want).max(), bound)
    # amplitude and phase from C, S within the bound: |dA| <= |dC| + |dS|, |dg| <= (|dC| + |dS|) / A radians
    mean, amp, pha = g.harmonic_constants("elb")
    dg = np.abs((pha - np.stack(G) + 180.0) % 360.0 - 180.0)
    assert np.abs(mean - Z0).max() <= bound and np.abs(amp - np.stack(A)).max() <= 2.0 * bound, (np.abs(amp - np.stack(A)).max(), bound)
    assert (dg <= np.degrees(2.0 * bound / np.stack(A)) + 360.0 * np.finfo(np.float64).eps).all(), dg.max()
    g.close()


def harmonic_launches(lib, size=(20, 17, 6)):
    """k_harm_accum once per sampled step, nothing lazy formed, every other count as without the analysis, the flow untouched"""
    a, b = start("seamount", size)
    g0 = PomGpu(a, libpath=lib)
    g0.run(2)
    g0.prof_begin()
    g0.run(6)
    off = counts(g0.prof_end())
    g0.download()
    g0.close()
    g = PomGpu(b, libpath=lib)
    g.set_tides(omega=X.OMEGA[:8])
    g.run(2)
    g.set_harmonic_analysis(True, every=3)
    g.prof_begin()
    g.run(6)                                                  # iint 3 .. 8: samples at 3 and 6
    on = counts(g.prof_end())
    g.download()
    assert on.pop("k_harm_accum") == 2 and g.harmonic_count() == 2
    assert "k_tide_table" not in on                           # no side carries a tide: nobody reads phasors, none are sent
    assert on == off, {k: (off.get(k), on.get(k)) for k in set(on) | set(off) if off.get(k) != on.get(k)}
    assert not any(k.startswith(("k_realvertvl", "k_restore_fields")) for k in on), on
    assert not diff(a, b)
    g.set_harmonic_analysis(False)
    assert g.harmonic_count() == -1
    g.close()


# ---- 5: hosts ------------------------------------------------------------------------------------------------------------------------------------
def refusals(lib):
    """every refusal leaves the state and the table as they were"""
    import ctypes
    from extpom_amd import lib as L
    size = (20, 17, 6)
    a, b = start("island", size)
    nc = 2
    lines = X.make_lines(nc, size[0], size[1])
    coef = X.coefficients(lines, nc, size[0], size[1])
    g = PomGpu(b, libpath=lib)
    refused(lambda: g.set_harmonic_analysis(True), "no constituent table")
    g.set_tides(omega=X.OMEGA[:nc], **lines)
    bad = X.make_lines(nc, size[0], size[1], seed=3)
    refused(lambda: g.set_tides(omega=X.OMEGA + (1e-4,), **X.make_lines(9, size[0], size[1])), "0..8")
    refused(lambda: g.set_tides(omega=(1e-4, float("nan")), **bad), "not finite")
    bad["west"]["un_amp"] = bad["west"]["un_amp"].copy()
    bad["west"]["un_amp"][1, 5] = float("inf")
    refused(lambda: g.set_tides(omega=X.OMEGA[:nc], **bad), "not finite")
    refused(lambda: g.set_tides(omega=X.OMEGA[:nc], im_global=size[0] - 1, **X.make_lines(nc, size[0] - 1, size[1], seed=3)), "outside the global line")
    m = L.FileMeta(b"", b"", size[0], size[1], 1, 1, 0, None)
    om = np.array(X.OMEGA[:nc])
    one = np.zeros((nc, max(size)))
    ptrs = (ctypes.c_void_p * 16)(*([None, one.ctypes.data] + [None] * 14))    # east is ON and has no elC
    refused(lambda: g._chk(g.L.pomgpu_set_tides(g.h, nc, g._p(om), 1, ptrs, ctypes.byref(m)), "set_tides"), "no elevation line")
    refused(lambda: g._chk(g.L.pomgpu_set_tides(g.h, -1, g._p(om), 0, ptrs, ctypes.byref(m)), "set_tides"), "0..8")
    refused(lambda: g.set_harmonic_analysis(True, every=0), "every")
    refused(lambda: g.harmonic_accumulate(), "is off")
    refused(lambda: g.tune_placement(), "tide table")
    g.set_harmonic_analysis(True)
    refused(lambda: g.harmonic_solve("elb"), "singular")
    g.set_harmonic_analysis(False)
    assert g.tide_count() == nc
    g.set_con(error_status=0)
    g.run(2)                                                  # the table is the one registered first
    g.download()
    g.close()
    X.oracle_steps(a, X.OMEGA[:nc], coef, 2)
    assert not diff(a, b), diff(a, b)


def fp32_builds_refuse(lib):
    _, b = start("seamount", (9, 8, 5), isplit=6)
    g = PomGpu(b, libpath=lib)
    for fn in (lambda: g.set_tides(omega=X.OMEGA[:1], **X.make_lines(1, 9, 8)), lambda: g.set_harmonic_analysis(True), g.harmonic_accumulate,
               lambda: g.harmonic_solve("elb")):
        refused(fn, "fp32-storage variant")
    assert g.tide_count() == 0
    g.close()


# ---- 6: files ------------------------------------------------------------------------------------------------------------------------------------
HERE = __import__("os").path.dirname(__import__("os").path.abspath(__file__))
KW = dict(title="tide test", time_start="2000-01-01 00:00:00 +00:00")


def check_harmonics_header(path, nc, im, jm):
    """the whole header against tests/golden/harmonics_file_schema.json"""
    import json
    import os
    from scipy.io import netcdf_file
    want = json.load(open(os.path.join(HERE, "golden", "harmonics_file_schema.json")))
    fill = lambda t: t.replace("{title}", KW["title"])
    with netcdf_file(str(path), "r", mmap=False) as f:
        assert f.version_byte == want["version_byte"]
        got_g = [[k, v.decode() if isinstance(v, bytes) else v] for k, v in f._attributes.items()]
        assert got_g == [[k, fill(v)] for k, v in want["global_atts"]], got_g
        assert [[k, v] for k, v in f.dimensions.items()] == [["ncon", nc], ["y", jm], ["x", im]], f.dimensions
        assert list(f.variables) == [v["name"] for v in want["vars"]], list(f.variables)
        for v in want["vars"]:
            q = f.variables[v["name"]]
            assert list(q.dimensions) == v["dims"] and q.typecode() == "d" and q.data.dtype.str == ">f8", v["name"]
            got_a = [[k, a.decode() if isinstance(a, bytes) else a] for k, a in q._attributes.items()]
            assert got_a == v["atts"], (v["name"], got_a)


def harmonics_file(lib, tmp, case="island", size=(20, 17, 6), nc=2):
    """the file against its schema and against harmonic_solve through scipy: omega, count, times and the means bit for bit; amplitude and phase
    are the device's hypot and atan2 of the solved C, S against numpy's of the same C, S -- each function within the OpenCL bounds that the
    device library documents (hypot 4 ulp, atan2 6 ulp; a degree conversion and the fold into [0, 360) one rounding each): 4 eps A and
    8 eps 360 degrees.  Writing resets nothing."""
    import os
    from scipy.io import netcdf_file
    _, b = start(case, size)
    omega = X.OMEGA[:nc]
    g = PomGpu(b, libpath=lib)
    g.set_tides(omega=omega, **X.make_lines(nc, size[0], size[1]))
    g.set_harmonic_analysis(True)
    g.run(2 * nc + 3)
    path = os.path.join(str(tmp), "h.harmonics.nc")
    g.write_file("harmonics", path, **KW)
    g.io_wait()
    check_harmonics_header(path, nc, size[0], size[1])
    M, (t0, t1) = g.harmonic_matrix()
    eps = np.finfo(np.float64).eps
    with netcdf_file(path, "r", mmap=False) as f:
        assert same_bits(np.array(f.variables["omega"].data, dtype=np.float64), np.array(omega))
        assert float(f.variables["count"].data) == g.harmonic_count() == 2 * nc + 3
        assert float(f.variables["t_first"].data) == t0 and float(f.variables["t_last"].data) == t1
        for name in FIELDS:
            c = g.harmonic_solve(name)[:, :size[1], :size[0]]
            C, S = c[1::2], c[2::2]
            assert same_bits(np.array(f.variables[name + "_mean"].data, dtype=np.float64), c[0]), name
            amp = np.array(f.variables[name + "_amp"].data, dtype=np.float64)
            pha = np.array(f.variables[name + "_pha"].data, dtype=np.float64)
            A = np.hypot(C, S)
            assert (np.abs(amp - A) <= 4.0 * eps * A).all(), name
            assert ((pha >= 0.0) & (pha < 360.0)).all(), name
            d = np.abs((pha - np.degrees(np.arctan2(S, C)) + 180.0) % 360.0 - 180.0)
            assert (d <= 8.0 * eps * 360.0).all(), (name, d.max())
        assert np.any(np.array(f.variables["elb_amp"].data) > 0.0)
    assert g.harmonic_count() == 2 * nc + 3                   # writing resets nothing
    g.close()


def write_tide_file(path, omega, lines):
    """a CDF-2 file an outside tool would write, by tests/golden/tide_file_schema.json"""
    from scipy.io import netcdf_file
    with netcdf_file(str(path), "w", version=2) as f:
        f.createDimension("ncon", len(omega))
        v = f.createVariable("omega", "d", ("ncon",))
        v[:] = np.array(omega)
        for side, d in lines.items():
            n = next(iter(d.values())).shape[1]
            dim = "n_" + side
            f.createDimension(dim, n)
            for k, a in d.items():
                v = f.createVariable(k + "." + side, "d", ("ncon", dim))
                v[:] = a
    return path


def tide_file(lib, tmp, case="island", size=(20, 17, 6), nc=3):
    """a tide file read back equals set_tides with the same numbers: the same run, bit for bit; refused files leave the table as it was"""
    import json
    import os
    from scipy.io import netcdf_file
    schema = json.load(open(os.path.join(HERE, "golden", "tide_file_schema.json")))
    a, b = start(case, size)
    omega = X.OMEGA[:nc]
    lines = X.make_lines(nc, size[0], size[1], sides=("east", "south", "north"))
    del lines["south"]["un_amp"], lines["south"]["un_pha"]     # a side with elevation alone
    assert {k + ".{side}" for d in lines.values() for k in d} <= {v["name"] for v in schema["per_side"]["vars"]} and schema["required"][0]["name"] == "omega"
    path = write_tide_file(os.path.join(str(tmp), "t.tide.nc"), omega, lines)
    g1 = PomGpu(a, libpath=lib)
    g1.set_tides(omega=omega, **lines)
    g2 = PomGpu(b, libpath=lib)
    g2.set_tide_file(path)
    assert g2.tide_count() == nc
    bad = os.path.join(str(tmp), "bad.tide.nc")
    broken = {k: dict(v) for k, v in lines.items()}
    del broken["east"]["el_pha"]
    refused(lambda: g2.set_tide_file(write_tide_file(bad, omega, broken)), "without its phase")
    short = X.make_lines(nc, size[0] - 1, size[1], sides=("south",))
    refused(lambda: g2.set_tide_file(write_tide_file(bad, omega, short)), "el_amp.south")
    with netcdf_file(bad, "w", version=2) as f:
        f.createDimension("n", 3)
        f.createVariable("x", "d", ("n",))[:] = np.zeros(3)
    refused(lambda: g2.set_tide_file(bad), "omega is absent")
    refused(lambda: g2.set_tide_file(os.path.join(str(tmp), "none.nc")), "cannot open")
    assert g2.tide_count() == nc
    g2.set_con(error_status=0)
    for g in (g1, g2):
        g.run(3)
        g.download()
        g.close()
    assert not diff(a, b) and int(b.iint) == 3, diff(a, b)
    free, _ = start(case, size)
    OracleTile(free).run(3)
    assert not same_bits(free.elb, b.elb)
