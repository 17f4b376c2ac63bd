"""TEST HELPER: proft of T and S in one lane (k_proft_ts_reg): kh read once, the matrix's coefficients formed once, each tracer its own
right-hand side, level 1, bottom value and back substitution.

Shared by tests/test_proft_shared_emulated.py (host build of the kernel sources, a serial grid) and tests/test_gpu_proft_shared.py (the
device): every check takes the library to load.  The bar is the CPU oracle, bit for bit on 64-bit patterns, over every COMMON array
that is not scratch (the restart list, uf and vf among them), after run(3): the first step skips the 3-D body, two run it.  The
library's event profile says which path ran: the one-lane kernel and the twin share the name k_proft_reg2, the one-lane kernel also
counts `proft_ts_lane`; two single launches show as k_proft_reg (k_proft beyond the register kernels)."""
import threading

import numpy as np

from uv_tail_fused_checks import ISPLIT, diff, launches
from extpom_amd import decomp
from extpom_amd.cases import finish_initial, make_case
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial

CASES = ["archipelago", "seamount"]
PAIRS = [(t, s) for t in (1, 2, 3, 4) for s in (1, 2, 3, 4)]
# which launch serves a pair of surface conditions.  One lane: the same class of condition (flux: 1, 2; value: 3, 4) and no short-wave
# term on either tracer.  Twin: the same instantiation (both with the term, or both without) but not one lane.  Two launches otherwise.
LANE = {(1, 1), (3, 3)}
TWIN = {(1, 3), (3, 1), (2, 2), (2, 4), (4, 2), (4, 4)}
KB_LANE_MAX = 56                                              # three vectors of 64 levels do not fit a wave's registers: kb 57..64 keeps the twin
TWIN2, SINGLE, SCRATCH_KERNEL, COUNTER = "k_proft_reg2", "k_proft_reg", "k_proft", "proft_ts_lane"
# (im, jm, kb): the smallest tile; a partial last wave of odd and even width; kb at and just past every template bound the launcher
# distinguishes (24 | 25, 50 | 51, the one-lane kernel's last 56 | 57, the register kernels' last 64 | 65)
SHAPES = [(8, 8, 6), (65, 49, 21), (66, 50, 21), (65, 49, 24), (65, 49, 25), (65, 49, 50), (65, 49, 51), (65, 49, 56), (65, 49, 57), (65, 49, 64), (65, 49, 65)]


def path_of(nbct, nbcs, kb, twin_switch=False):
    if kb > 64 or kb < 6:
        return "scratch"
    if (nbct, nbcs) in LANE and kb <= KB_LANE_MAX and not twin_switch:
        return "lane"
    return "twin" if (nbct, nbcs) in LANE | TWIN else "single"


def assert_path(prof, path, body):
    got = {k: launches(prof, k) for k in (TWIN2, SINGLE, SCRATCH_KERNEL, COUNTER)}
    want = {"lane": {TWIN2: body, SINGLE: 0, SCRATCH_KERNEL: 0, COUNTER: body}, "twin": {TWIN2: body, SINGLE: 0, SCRATCH_KERNEL: 0, COUNTER: 0},
            "single": {TWIN2: 0, SINGLE: 2 * body, SCRATCH_KERNEL: 0, COUNTER: 0}, "scratch": {TWIN2: 0, SINGLE: 0, SCRATCH_KERNEL: 2 * body, COUNTER: 0}}[path]
    assert got == want, (path, got)


def surface_fields(a):
    """the 2-D surface fields a case leaves at zero, on the water of the whole (single) tile: a heat flux, a salt flux a twentieth of it
    with another pattern, short-wave radiation.  Set before the state is copied: the library's copy goes through its upload."""
    jj, ii = np.meshgrid(np.arange(a.jm, dtype=np.float64), np.arange(a.im, dtype=np.float64), indexing="ij")
    if not np.any(a.wtsurf):
        a.wtsurf[:a.jm, :a.im] = 2.0e-6 * np.sin(0.37 * ii + 0.11 * jj) * a.fsm[:a.jm, :a.im]
    if not np.any(a.wssurf):
        a.wssurf[:a.jm, :a.im] = 1.0e-7 * np.cos(0.23 * ii - 0.31 * jj) * a.fsm[:a.jm, :a.im]
    if not np.any(a.swrad):
        a.swrad[:a.jm, :a.im] = -5.0e-5 * (1.0 + 0.5 * np.sin(0.19 * ii + 0.29 * jj)) * a.fsm[:a.jm, :a.im]


def exercises(a, nbct, nbcs):
    """a kernel that handed S one of T's operands would pass on a state where the two are equal"""
    w = a.fsm != 0.
    assert np.any(a.t != a.s) and np.any(a.tb != a.sb)
    assert np.any(a.wtsurf[w] != 0.) and np.any(a.wssurf[w] != 0.) and np.any(a.wtsurf[w] != a.wssurf[w])
    assert np.any(a.tsurf[w] != a.ssurf[w])
    if nbct in (2, 4) or nbcs in (2, 4):
        assert np.any(a.swrad[w] != 0.)


def start(case, size, nbct=1, nbcs=1):
    a = make_case(case, *size, dte=6.0, isplit=ISPLIT, nbct=nbct, nbcs=nbcs)
    surface_fields(a)
    oracle_finish_initial(a)
    exercises(a, nbct, nbcs)
    return a, a.copy()


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def whole_steps(lib, case, size, nbct=1, nbcs=1, steps=3, switch=False):
    """run(steps) against the oracle, and the path the profile shows"""
    a, b = start(case, size, nbct, nbcs)
    g = PomGpu(b, libpath=lib)
    if switch:
        g.switch("PROFT_TWIN", 1)
    g.prof_begin()
    g.run(steps)
    prof = g.prof_end()
    assert_path(prof, path_of(nbct, nbcs, size[2], switch), steps - 1)
    OracleTile(a).run(steps)
    g.download()
    assert a.iint == b.iint and not diff(a, b), (nbct, nbcs, diff(a, b))
    exercises(a, nbct, nbcs)
    g.close()


def switch_flipped_live(lib, nbc=1):
    """POMGPU_PROFT_TWIN set and unset between the steps of one context: the path follows at once, the bits are the oracle's"""
    a, b = start("archipelago", (65, 49, 21), nbc, nbc)
    ot = OracleTile(a)
    g = PomGpu(b, libpath=lib)
    g.run(1)
    ot.run(1)
    for n, sw in ((2, None), (1, 1), (2, None), (1, 1), (1, None)):
        g.switch("PROFT_TWIN", sw)
        g.prof_begin()
        g.run(n)
        assert_path(g.prof_end(), "twin" if sw else "lane", n)
        ot.run(n)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def lane_equals_twin(lib, steps=4, size=(65, 49, 21)):
    """no oracle (the fp32 study builds have none): a context with POMGPU_PROFT_TWIN and one without, every array, scratch included, for
    both classes of surface condition"""
    for nbc in (1, 3):
        a = make_case("archipelago", *size, dte=6.0, isplit=ISPLIT, nbct=nbc, nbcs=nbc)
        oracle_finish_initial(a)
        exercises(a, nbc, nbc)
        b = a.copy()
        ga, gb = PomGpu(a, libpath=lib), PomGpu(b, libpath=lib)
        ga.switch("PROFT_TWIN", 1)
        ga.prof_begin()
        gb.prof_begin()
        ga.run(steps)
        gb.run(steps)
        assert_path(ga.prof_end(), "twin", steps - 1)
        assert_path(gb.prof_end(), "lane", steps - 1)
        ga.download()
        gb.download()
        assert not diff(a, b, skip=()), (nbc, diff(a, b, skip=()))
        assert np.any(a.t != a.tb)                            # the steps moved T
        ga.close()
        gb.close()


def tiles_2x2(lib, grid=(97, 59), isplit=7, steps=3):
    """2x2 tiles of the fourth case under the library's own exchange, one thread per tile (the movers of tests/test_kernels_emulated_tiles.py):
    every tile takes the one-lane kernel, owned cells equal the single-tile oracle"""
    import test_kernels_emulated_tiles as T
    world, kb = 4, T.KB                                       # (compare_with_single_tile runs the oracle at T.KB = 11 levels)
    iml, jml = decomp.local_size(*grid, 2, 2)
    board, out, errs = T.Board(world), {}, []
    tiles = [decomp.make_tile(r, *grid, iml, jml, n_proc=world) for r in range(world)]

    def rank(r):
        try:
            tile = tiles[r]
            st = make_case("archipelago", *grid, kb, tile=tile, dte=6.0, isplit=isplit)
            g = PomGpu(st, libpath=lib)
            g.set_transport(tile, lambda *a: T.transport(board, tile, *a), agree=lambda mine: board.allmin(r, mine))

            def dens(s, a, b, c):
                g.upload(s); g.call("dens", a, b, c); g.download(s)

            def baropg(s):
                g.upload(s); g.call("baropg"); g.download(s)

            finish_initial(st, dens, baropg)
            g.upload(st)
            g.prof_begin()
            g.run(steps)
            assert_path(g.prof_end(), "lane", steps - 1)
            g.download()
            out[r] = (tile, st, g.exchange_rounds())
        except Exception as e:                                # a dead rank must not leave the others at the barrier
            errs.append(e)
            board.barrier.abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    T.compare_with_single_tile(out, {}, grid=grid, isplit=isplit, case="archipelago", steps=steps, min_rounds=2)
