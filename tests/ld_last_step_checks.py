"""TEST HELPER: l and dtef reach memory only in the last step of a pomgpu_run call on one tile (k_profq's LD flag, launch_profq).

Shared by tests/test_ld_last_step_emulated.py (host builds of the kernel sources) and tests/test_gpu_ld_last_step.py (the device):
every check takes the library to load.  The bar is bit for bit on 64-bit patterns: a context stepped with run(n) against one stepped
with n x run(1) (which stores in every step), and both against the CPU oracle.  The oracle carries BOTH arrays -- l is on the restart
list, dtef is a COMMON array of the reference and of oracle/pom_fields.h that profq rewrites in every call -- so diff() over BLK2D +
BLK3D compares dtef as well.  Which launches stored is read from the event profile's count profq_ld_store.

What no check here can see: that a launch with LD = 0 leaves the two arrays alone (an observer always comes after a launch that
stores).  The write counter of the device shows that (profiles/ld_last_step_pmc.txt)."""
import threading

import numpy as np

from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D, P3, RESTART_2D, RESTART_3D
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial

SCRATCH = {"tps", "fluxua", "fluxva", "zflux"}
ISPLIT = 30
COUNT, PROFQ = "profq_ld_store", "k_profq"
# (case, (im, jm, kb), switch): the smallest shapes at which every phase of the walk down and both workgroup shapes exist.
# kb = 6: kbm2 = 4, levels 1, 2, two in LDS, kbm1, kb and no memory-phase level.  65x49x21: the 2-row shape, KL = 9, memory-phase levels.
# Under POMGPU_PROFQ_ROWS8 (KL = 19): kb = 21 has kA = kbm2 = 19 and no memory phase, kb = 30 has one.  The archipelago: land inside, a curved grid
SHAPES = [("seamount", (8, 8, 6), None), ("seamount", (20, 17, 6), None), ("seamount", (65, 49, 21), None),
          ("seamount", (65, 49, 21), "PROFQ_ROWS8"), ("seamount", (65, 49, 30), "PROFQ_ROWS8"), ("archipelago", (65, 49, 21), None)]
SHAPE_IDS = ["8x8x6", "20x17x6", "65x49x21", "65x49x21-rows8", "65x49x30-rows8", "archipelago"]
# a quiet NaN with a payload no arithmetic delivers (hardware NaNs are 0x7ff8000000000000 or carry an operand's payload)
NAN_BITS = np.uint64(0x7FF8DEAD0BADBEEF)


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


def diff(a, b, names=None, skip=SCRATCH):
    return [n for n in (names or BLK2D + BLK3D) if n not in skip and not same_bits(a.field(n), b.field(n))]


def start(case="seamount", size=(65, 49, 21), warm=1):
    """(oracle's state, the library's copy) `warm` steps in: from there every step runs the 3-D body (iint = 1 skips it, advance.f:362)"""
    a = make_case(case, *size, dte=6.0, isplit=ISPLIT)
    oracle_finish_initial(a)
    if warm:
        OracleTile(a).run(warm)
    return a, a.copy()


def gpu(st, lib, switch=None, eager=False):
    g = PomGpu(st, libpath=lib)
    if switch:
        g.switch(switch, 1)
    if eager:
        g.switch("LD_EAGER", 1)
    return g


def count(prof, name=COUNT):
    return prof.get(name, (0, 0.0))[0]


def read3(g, name):
    out = np.empty_like(g.st.field(name))
    g._chk(g.L.pomgpu_download_3d(g.h, P3[name], g._p(out)), "download_3d")
    return out


def write3(g, name, new):
    g._chk(g.L.pomgpu_upload_3d(g.h, P3[name], g._p(np.ascontiguousarray(new))), "upload_3d")


def step_by_routine(g, n):
    """one internal step as the Fortran host makes it (advance.f:6-59 routine by routine)"""
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


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def same_bits_either_way(lib, case, size, switch=None, eager=False, oracle=True):
    """run(4) against 4 x run(1): every array of the restart list and dtef byte-identical, the profile count 1 against 4 (4 and 4 under
    POMGPU_LD_EAGER); with the oracle: every array that is not scratch -- l and dtef among them -- equals four oracle steps"""
    a, b = start(case, size)
    c = b.copy()
    gb, gc = gpu(b, lib, switch, eager), gpu(c, lib, switch, eager)
    gb.prof_begin()
    gb.run(4)
    pb = gb.prof_end()
    gc.prof_begin()
    for _ in range(4):
        gc.run(1)
    pc = gc.prof_end()
    assert count(pb, PROFQ) == count(pc, PROFQ) == 4, (pb, pc)
    assert count(pb) == (4 if eager else 1) and count(pc) == 4, (pb, pc)
    gb.download()
    gc.download()
    names = RESTART_2D + RESTART_3D + ["dtef"]
    assert not diff(b, c, names), diff(b, c, names)
    assert np.any(b.l != 0.) and np.any(b.dtef != 0.) and np.all(np.isfinite(b.l)) and np.all(np.isfinite(b.dtef))
    if oracle:
        OracleTile(a).run(4)
        assert a.iint == b.iint and not diff(a, b) and not diff(a, c), (diff(a, b), diff(a, c))
    gb.close()
    gc.close()


def last_step_stores_every_cell(lib, case, size, switch=None):
    """l and dtef filled with a NaN pattern no arithmetic delivers, then run(3): the last step's launch has written every cell
    (1:im, 1:jm, 1:kb) -- rim columns, levels 1 and kb included -- with the oracle's bits"""
    a, b = start(case, size)
    g = gpu(b, lib, switch)
    poison = np.full(b.l.shape, NAN_BITS, dtype=np.uint64).view(np.float64)
    for n in ("l", "dtef"):
        write3(g, n, poison)
        assert np.all(read3(g, n).view(np.uint64) == NAN_BITS)
    g.prof_begin()
    g.run(3)
    assert count(g.prof_end()) == 1
    OracleTile(a).run(3)
    for n in ("l", "dtef"):
        got = read3(g, n)
        assert got.shape == (b.kb, b.jm, b.im)                  # one tile: the whole array is (1:im, 1:jm, 1:kb)
        assert not np.any(got.view(np.uint64) == NAN_BITS) and not np.any(np.isnan(got)), n
        assert same_bits(got, a.field(n)), n
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def decision_run(lib, eager=False):
    """run(4): one launch stores (four under POMGPU_LD_EAGER); the switch is read at launch time, so flipping it on a live context counts at once"""
    a, b = start()
    g = gpu(b, lib, eager=eager)
    g.prof_begin()
    g.run(4)
    prof = g.prof_end()
    assert count(prof, PROFQ) == 4 and count(prof) == (4 if eager else 1), prof
    g.switch("LD_EAGER", None if eager else 1)
    g.prof_begin()
    g.run(3)
    prof = g.prof_end()
    assert count(prof, PROFQ) == 3 and count(prof) == (1 if eager else 3), prof
    g.download()
    OracleTile(a).run(7)
    assert not diff(a, b), diff(a, b)
    g.close()


def decision_advance(lib):
    """four pomgpu_advance calls: four launches store"""
    a, b = start()
    g = gpu(b, lib)
    g.prof_begin()
    for n in range(4):
        g.set_con(iint=int(b.iint) + 1)
        g.advance()
    prof = g.prof_end()
    assert count(prof, PROFQ) == 4 and count(prof) == 4, prof
    g.download()
    OracleTile(a).run(4)
    assert not diff(a, b), diff(a, b)
    g.close()


def decision_address_handed_out(lib, name="t"):
    """run(4) after pomgpu_device_3d handed out any address: the library no longer sees every reader, four launches store"""
    a, b = start()
    g = gpu(b, lib)
    assert g.device_ptr(name)
    g.prof_begin()
    g.run(4)
    prof = g.prof_end()
    assert count(prof, PROFQ) == 4 and count(prof) == 4, prof
    g.download()
    OracleTile(a).run(4)
    assert not diff(a, b), diff(a, b)
    g.close()


def decision_direct_calls(lib):
    """pomgpu_mode_internal (the routine-by-routine host's step) and pomgpu_profq called directly: one storing launch each"""
    a, b = start()
    g = gpu(b, lib)
    g.prof_begin()
    step_by_routine(g, int(b.iint) + 1)
    prof = g.prof_end()
    assert count(prof, PROFQ) == 1 and count(prof) == 1, prof
    g.download()
    OracleTile(a).run(1)
    assert not diff(a, b), diff(a, b)
    g.prof_begin()
    g.call("profq")
    prof = g.prof_end()
    assert count(prof, PROFQ) == 1 and count(prof) == 1, prof
    g.close()


def decision_tune_placement(lib):
    """pomgpu_tune_placement (forced on this small grid by POMGPU_TUNE_FORCE) with steps = 3: every trial is one untimed step and a
    pomgpu_run(3) -- two storing launches of four per trial, the same mix for every layout"""
    a, b = start()
    g = gpu(b, lib)
    g.switch("TUNE_FORCE", 1)
    g.prof_begin()
    r = g.tune_placement(3, 3)
    prof = g.prof_end()
    assert r["tried"] >= 1 and count(prof, PROFQ) == 4 * r["tried"] and count(prof) == 2 * r["tried"], (r, prof)
    g.download()
    OracleTile(a).run(4 * r["tried"])
    assert not diff(a, b), diff(a, b)
    g.close()


def decision_record_step(lib):
    """forcing and lateral records (dti = 360 s: lateral_bc asks for a record every 10 steps, the surface forcing every 30): the step in
    front of one that asks for a record stores as well -- a run that ends at a missing record leaves its last completed step whole.
    run(1) (no 3-D body), then run(11) = steps 2..12: step 9 and step 12 store"""
    import forcing_files_checks as fc
    a, _, _ = fc.start("seamount", fc.BASE, 12)
    b = a.copy()
    b.forcing_records, b.lateral_records = a.forcing_records, a.lateral_records
    g = gpu(b, lib)
    g.set_forcing_records(1, 4)
    g.set_lateral_records(1, 4)
    g.run(1)
    g.prof_begin()
    g.run(11)
    prof = g.prof_end()
    assert count(prof, PROFQ) == 11 and count(prof) == 2, prof
    OracleTile(a).run(12)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()


def decision_two_tiles(lib, tiles_module):
    """run(4) on a 2-tile context with the exchange hook (rank threads of tests/test_kernels_emulated_tiles.py): tiles store in every step"""
    from extpom_amd import decomp
    from extpom_amd.cases import finish_initial
    T = tiles_module
    grid, kb, world = (97, 59), 11, 2
    iml, jml = decomp.local_size(*grid, 2, 1)
    board, errs, seen = T.Board(world), [], {}
    tiles = [decomp.make_tile(r, *grid, iml, jml, n_proc=world) for r in range(world)]

    def rank(r):
        try:
            tile = tiles[r]
            st = make_case("island", *grid, kb, tile=tile, dte=6.0, isplit=7)
            g = PomGpu(st, libpath=lib)
            g.set_exchange(lambda ptrs, nzs: T.exchange(board, tile, [T.view(p, nz, tile) for p, nz in zip(ptrs, nzs)]))
            g.set_order_exchange(lambda *a: T.order(board, tile, *a))

            def dens(s, a, b, c):
                g.upload(s); g.call("dens", a, b, c); g.download(s)

            def baropg(s):
                g.upload(s); g.call("baropg_mcc" if int(s.npg) == 2 else "baropg"); g.download(s)
            finish_initial(st, dens, baropg)
            g.upload(st)
            g.run(1)                                            # iint = 1: no 3-D body
            g.prof_begin()
            g.run(4)
            seen[r] = g.prof_end()
            g.close()
        except Exception as e:                                  # a dead rank must not leave the other at the barrier
            errs.append(e)
            board.barrier.abort()
    threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for r in range(world):
        assert count(seen[r], PROFQ) == 4 and count(seen[r]) == 4, seen[r]


def observers_between_calls(lib, tmp_path):
    """after run(3) the restart file's l and a plain download are the oracle's; a run(2) behind them still matches five oracle steps"""
    import restart_expect as rx
    a, b = start("archipelago")
    ot = OracleTile(a)
    g = gpu(b, lib)
    g.run(3)
    ot.run(3)
    g.write_file("restart", tmp_path / "restart.nc", title="archipelago", time_start=rx.START)
    g.io_wait()
    vals, _, _ = rx.file_values(tmp_path / "restart.nc")
    assert same_bits(vals["l"], a.l) and np.any(a.l != 0.)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.prof_begin()
    g.run(2)
    assert count(g.prof_end()) == 1
    ot.run(2)
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()
