"""TEST HELPER: the fresh-water forcing on the device -- pomgpu_water with records from pomgpu_set_water_files / _record, and ssurf from the
surface record (pomgpu_set_surface_sss).

Shared by tests/test_water_emulated.py (host build of the kernel sources) and tests/test_gpu_water.py (the device): every check takes the
library to load (None: the product library on device 0).  The reference's `water_` cannot be called (read_water_pnetcdf_ is a trap in
oracle/ref_traps.c), so the schedule is pinned by restatement alone (tests/water_expect.py): before each of the oracle's run(1) the
restatement writes wssurfb wssurff wssurf (and ssurf) into the oracle's bound state -- `water` writes arrays nothing else in surface_forcing
touches, so placing its writes in front of the step is exact -- and asserts that its own `time` is blkcon's after the step.  The bar is bit
for bit on 64-bit patterns, every array of blk2d and blk3d but the library's four scratch arrays, bdry and blkcon (diff of
tests/forcing_files_checks.py).  dti = 360 s: iwater = 240.  A check that crosses a record change starts at iint = iwater - 3 with
non-zero wssurfb wssurff in the state, as restore_across_a_record_change jumps iint and time."""
import os

import numpy as np

import forcing_expect as fx
import water_expect as wx
from extpom_amd.cases import make_case
from extpom_amd.model import PomGpu
from forcing_files_checks import BASE, SIZE, diff, same_bits, status
from oracle.pyoracle import OracleTile, oracle_finish_initial

IWATER = 240
UNPACK, LD = "k_frc_unpack", "profq_ld_store"


def count(prof, name):
    return prof.get(name, (0, 0.0))[0]


def start(case, size=SIZE, numbers=(0, 1, 2), **nml):
    """(state with st.water_records, raw global fields)"""
    cont_bry = nml.pop("cont_bry", 0)
    a = make_case(case, *size, **dict(BASE, **nml))
    oracle_finish_initial(a)
    a.cont_bry = cont_bry                                     # (read_input zeroes it without a restart file: set as a restart would)
    assert wx.iwater_of(a) == IWATER
    raw = wx.raw_water(a, numbers)
    a.water_records = wx.records(a, raw)
    return a, raw


def jump(a, iint, nb=0, nf=1):
    """the state as step `iint` has left it as far as water goes: record nb in wssurfb, nf in wssurff"""
    a.iint = iint
    a.time = wx.get_time(a, iint)
    a.wssurfb[:a.jm, :a.im] = a.water_records[nb]
    a.wssurff[:a.jm, :a.im] = a.water_records[nf]
    return a


def oracle_steps(ot, a, steps, sss=None):
    """`steps` oracle steps with the restatement's writes in front of each; [(iint, fnew, records read)]"""
    log = []
    for _ in range(steps):
        n = int(a.iint) + 1
        time, fnew, read = wx.water(a, n, a.water_records)
        if sss is not None:
            wx.surface_sss(a, n, sss)
        ot.run(1)
        assert int(a.iint) == n and float(a.time) == time, (n, float(a.time), time)
        log.append((n, fnew, read))
    return log


def setter_steps(g, steps):
    """the host path: before every step the water records its schedule may ask for, then run(1)"""
    first = int(g.st.iint)
    for n in range(first + 1, first + steps + 1):
        g.set_water_records(first=n // IWATER, count=2)
        g.run(1)


def three_ways(lib, tmp, a, raw, steps, expect_reads):
    """file path = setter path (two contexts, scratch arrays included) = oracle; returns (oracle state, file state, the oracle's log)"""
    b, s = a.copy(), a.copy()
    b.water_records = s.water_records = a.water_records
    prefix = str(tmp / "case")
    wx.write_all(prefix, raw)
    g = PomGpu(b, libpath=lib)
    g.set_water_files(prefix)
    g.prof_begin()
    g.run(steps)                                              # ONE call across the record change
    prof = g.prof_end()
    g.download()
    log = oracle_steps(OracleTile(a), a, steps)
    assert sum(len(r) for _, _, r in log) == expect_reads == count(prof, UNPACK), (log, prof.get(UNPACK))
    assert int(a.error_status) == 0 and not diff(a, b), diff(a, b)
    g.close()
    h = PomGpu(s, libpath=lib)
    setter_steps(h, steps)
    h.download()
    assert not diff(b, s, skip=()), diff(b, s, skip=())
    h.close()
    return a, b, log


# ---- 1: the start --------------------------------------------------------------------------------------------------------------------
def start_from_record_zero(lib, tmp, case):
    a, raw = start(case)
    init = a.copy()
    a, b, log = three_ways(lib, tmp, a, raw, 3, 2)
    assert [r for _, _, r in log] == [[0, 1], [], []]         # record 0, not 1: no "+ 1"; both in step 1 and none after it
    A = (slice(0, a.jm), slice(0, a.im))
    assert same_bits(b.wssurfb[A], a.water_records[0]) and same_bits(b.wssurff[A], a.water_records[1])
    # files 0000 and 0001 are consumed in step 1 and none after it: with only those two the run goes through, step by step
    c = init.copy()
    prefix = str(tmp / "two")
    wx.write_all(prefix, {n: raw[n] for n in (0, 1)})
    g = PomGpu(c, libpath=lib)
    g.set_water_files(prefix)
    g.run(1)
    os.remove(wx.name(prefix, 0))
    os.remove(wx.name(prefix, 1))
    g.run(2)
    g.download()
    assert not diff(b, c, skip=()), diff(b, c, skip=())
    # water off: wssurf stays what the host uploaded and s is another
    g.set_water(False)
    d = init.copy()
    g.upload(d)
    g.run(3)
    g.download()
    assert same_bits(d.wssurf, init.wssurf) and same_bits(d.wssurff, init.wssurff) and not same_bits(b.wssurf, init.wssurf)
    assert not same_bits(d.s, b.s) and "s" in diff(d, b)
    g.close()


# ---- 2: a record change --------------------------------------------------------------------------------------------------------------
def across_a_record_change(lib, tmp, case, cont_bry=0):
    a, raw = start(case, cont_bry=cont_bry)
    assert int(a.cont_bry) == cont_bry
    jump(a, IWATER - 3)
    a, b, log = three_ways(lib, tmp, a, raw, 5, 1)
    # the fetch happens at iint = 240 whatever cont_bry says (with it in the schedule: at 233, outside these steps)
    assert [(n, r) for n, _, r in log] == [(238, []), (239, []), (240, [2]), (241, []), (242, [])]
    fnew = [f for _, f, _ in log]
    assert fnew[1] > .99 and fnew[2] == 0. and fnew[3] == wx.get_time(a, 241) - 1. and 0. < fnew[3] < .01
    A = (slice(0, a.jm), slice(0, a.im))
    assert same_bits(b.wssurfb[A], a.water_records[1]) and same_bits(b.wssurff[A], a.water_records[2])


# ---- 3: no iend guard ----------------------------------------------------------------------------------------------------------------
def last_step_reads_one_more(lib, tmp, case):
    a, raw = start(case, days=IWATER * 360. / 86400.)
    assert int(a.iend) == IWATER
    jump(a, IWATER - 3)
    init = a.copy()
    b = init.copy()
    prefix = str(tmp / "case")
    wx.write_all(prefix, raw)
    g = PomGpu(b, libpath=lib)
    g.set_water_files(prefix)
    g.prof_begin()
    g.run(3)
    prof = g.prof_end()
    g.download()
    ot = OracleTile(a)
    oracle_steps(ot, a, 2)
    at239 = a.copy()
    log = oracle_steps(ot, a, 1)
    assert log == [(IWATER, 0., [2])] and int(a.iint) == int(a.iend)
    assert int(b.error_status) == 0 and not diff(a, b), diff(a, b)
    assert same_bits(b.wssurff[:a.jm, :a.im], a.water_records[2]) and count(prof, UNPACK) == 1
    assert count(prof, LD) == 2                               # the step in front of the fetch and the call's last
    g.close()
    # 0002 absent: the run fails in step 240 and leaves what step 239 left, l and dtef included
    os.remove(wx.name(prefix, 2))
    c = init.copy()
    g = PomGpu(c, libpath=lib)
    g.set_water_files(prefix)
    g.prof_begin()
    rc = g.L.pomgpu_run(g.h, 3)
    prof = g.prof_end()
    err, msg = status(g)
    assert rc == -1 and err == 1 and "water.0002.nc" in msg and "cannot open" in msg, (rc, err, msg)
    g.download()
    assert int(c.iint) == IWATER
    assert count(prof, LD) == 1 and count(prof, "k_profq") == 2   # the storing launch is step 239's
    moved = diff(at239, c)
    assert all(m.startswith("blkcon") for m in moved), moved  # get_time and the error alone
    assert np.any(c.l != 0.) and np.any(c.dtef != 0.)
    g.close()


# ---- 4: SSS --------------------------------------------------------------------------------------------------------------------------
def sss_into_ssurf(lib, tmp, case):
    """nbcs = 3; cont_bry = 27 at dti = 360 s: surface reads record 1 at iint = 1 and record 2 at iint = 3"""
    steps = 4
    a = make_case(case, *SIZE, **dict(BASE, nbcs=3))
    oracle_finish_initial(a)
    a.cont_bry = 27
    assert int(a.nbcs) == 3 and int(a.cont_bry) == 27
    raw_s = fx.raw_sfrc(a, 3)
    a.forcing_records = fx.forcing_records(a, raw_s)
    a.water_records = {}
    sss = [r[1] for r in a.forcing_records["surface"]]
    init = a.copy()
    b, s, off = init.copy(), init.copy(), init.copy()
    for x in (b, s, off):
        x.forcing_records = a.forcing_records
    sfrc = fx.write_sfrc(tmp / "case.sfrc.nc", raw_s, types={"SSS": "f"})
    ot = OracleTile(a)
    used = []
    for _ in range(steps):
        n = int(a.iint) + 1
        used.append(wx.surface_sss(a, n, sss))
        ot.run(1)
    assert used == [1, None, 2, None]
    A = (slice(0, a.jm), slice(0, a.im))
    g = PomGpu(b, libpath=lib)                                # by file
    g.set_surface_sss(True)
    g.set_forcing_files(sfrc=sfrc)
    g.run(steps)
    g.download()
    assert int(b.error_status) == 0 and not diff(a, b), diff(a, b)
    assert same_bits(b.ssurf[A], sss[1]) and not same_bits(sss[0], sss[1])
    g.close()
    h = PomGpu(s, libpath=lib)                                # by setters
    h.set_surface_sss(True)
    for n in range(1, steps + 1):
        h.set_forcing_records(first=(n + 27) // 30 + 1, count=2)
        h.run(1)
    h.download()
    assert not diff(b, s, skip=()), diff(b, s, skip=())
    h.close()
    o = PomGpu(off, libpath=lib)                              # switch off: ssurf is the uploaded one, bit for bit
    o.set_forcing_files(sfrc=sfrc)
    o.run(steps)
    o.download()
    assert same_bits(off.ssurf, init.ssurf) and not same_bits(off.ssurf[A], b.ssurf[A])
    assert "s" in diff(off, b)                                # and at nbcs = 3 the salt solve saw the difference
    o.close()


# ---- 5: file forms and refusals ------------------------------------------------------------------------------------------------------
FORMS = {
    "cdf2_double": dict(),
    "cdf1_double": dict(version=1),
    "cdf2_float": dict(dtype="f"),
    "cdf1_float": dict(version=1, dtype="f"),
    "cdf2_double_among_others": dict(odd=True),
    "cdf1_float_among_others": dict(version=1, dtype="f", odd=True),
}
SMALL = (8, 8, 6)
OBLONG = (9, 8, 6)                                            # a transposed `w` has other dimension lengths only where im /= jm


def water_alone(g, iint):
    g.set_con(iint=iint, time=wx.get_time(g.st, iint))
    return g.L.pomgpu_water(g.h)


def file_forms(lib, tmp):
    a, raw = start("seamount", SMALL, numbers=(0, 1))
    want = a.copy()
    want.water_records = a.water_records
    time, _, read = wx.water(want, 1, want.water_records)
    assert read == [0, 1] and np.any(want.wssurf != 0.)
    want.iint, want.time = 1, time
    for form, kw in FORMS.items():
        b = a.copy()
        prefix = str(tmp / form)
        wx.write_all(prefix, raw, **kw)
        g = PomGpu(b, libpath=lib)
        g.set_water_files(prefix)
        assert water_alone(g, 1) == 0, (form, status(g))
        g.download()
        assert not diff(want, b, skip=()), (form, diff(want, b, skip=()))
        g.close()


def refusals(lib, tmp):
    a, raw = start("seamount", OBLONG, numbers=(0, 1))
    b = a.copy()
    g = PomGpu(b, libpath=lib)
    g.run(2)
    g.download()
    before = b.copy()

    def unchanged(cause):
        now = b.copy()
        g._chk(g.L.pomgpu_download(g.h, g._p(now.blk1d), g._p(now.blk2d), g._p(now.blk3d), g._p(now.bdry), g._p(now.con)), "download")
        moved = [m for m in diff(before, now, skip=()) if not m.startswith("blkcon")]   # (iint, time, dti, error_status: the test's own)
        assert not moved, (cause, moved)

    def refused(cause, iint=1, **kw):
        prefix = str(tmp / ("bad%d" % len(os.listdir(tmp))))
        wx.write_all(prefix, raw, **kw)
        g.set_con(error_status=0)
        g.set_water_files(prefix)
        rc = water_alone(g, iint)
        err, msg = status(g)
        assert rc == -1 and err == 1 and cause in msg and ".water." in msg, (cause, rc, err, msg)
        unchanged(cause)
        return prefix

    refused("variable w is absent", drop=True)
    refused("variable w has the dimension lengths", transpose=True)
    refused("variable w has the dimension lengths", extra_col=True)
    good = refused("has no file name", iint=9999 * IWATER)    # record (iint + iwater) / iwater = 10000: the format prints ****
    # the setter after files
    g.set_con(error_status=0)
    x = np.zeros((a.jm, a.im))
    rc = g.L.pomgpu_set_water_record(g.h, 0, g._p(x))
    err, msg = status(g)
    assert rc == -1 and err == 1 and "come from a file" in msg, (rc, err, msg)
    unchanged("setter after files")
    # iwater < 1, in frc_interp's words
    g.set_con(error_status=0, dti=100000.)
    rc = water_alone(g, 1)
    err, msg = status(g)
    assert rc == -1 and err == 1 and "dti is longer than the record interval" in msg, (rc, err, msg)
    unchanged("iwater < 1")
    # and after all that the good files still serve
    g.set_con(error_status=0, dti=360.)
    assert water_alone(g, 1) == 0 and good
    g.download()
    assert same_bits(b.wssurff[:a.jm, :a.im], a.water_records[1])
    g.close()
    # the other setter's refusals are its own: n >= 1 there, n >= 0 here
    h = PomGpu(a.copy(), libpath=lib)
    assert h.L.pomgpu_set_forcing_record(h.h, 0, 0, h._p(x), h._p(x)) == -1
    assert h.L.pomgpu_set_water_record(h.h, -1, h._p(x)) == -1 and h.L.pomgpu_set_water_record(h.h, 0, h._p(x)) == 0
    h.close()


# ---- 7: the fp32-storage build: file path = setter path ------------------------------------------------------------------------------
def file_equals_setters_f32(lib, tmp):
    """no oracle for this build: two contexts of one library across the record change"""
    a, raw = start("archipelago")
    jump(a, IWATER - 2)
    b, s = a.copy(), a.copy()
    b.water_records = s.water_records = a.water_records
    prefix = str(tmp / "case")
    wx.write_all(prefix, raw, dtype="f")
    g = PomGpu(b, libpath=lib)
    g.set_water_files(prefix)
    g.run(3)
    g.download()
    h = PomGpu(s, libpath=lib)
    setter_steps(h, 3)
    h.download()
    assert not diff(b, s, skip=()), diff(b, s, skip=())
    assert same_bits(b.wssurff[:a.jm, :a.im], a.water_records[2]) and np.any(b.wssurf != a.wssurf)
    g.close()
    h.close()


# ---- 6: tiles ------------------------------------------------------------------------------------------------------------------------
TILE_WATER_STEPS = 3                                          # dti = 120 s on the tiles' grid: iwater = 720; step 1 reads records 0 and 1


def run_tiles(lib, mover, prefix):
    """2x2 tiles under the library exchange and the wide-halo external mode, one host thread each, every rank reading its own window
    of the water files (prefix None: water off); ({rank: state}, {rank: (rounds, rounds on the side stream)}, the tiles)"""
    import threading
    from extpom_amd import decomp
    from extpom_amd.cases import finish_initial
    import forcing_files_checks as ffc
    IMg, JMg = ffc.TILE_GRID
    iml, jml = decomp.local_size(IMg, JMg, 2, 2)
    tiles = [decomp.make_tile(r, IMg, JMg, iml, jml, n_proc=4) for r in range(4)]
    board, out, rounds, errs = ffc.Board(4), {}, {}, []

    def rank(r):
        try:
            tile = tiles[r]
            st = make_case("archipelago", IMg, JMg, ffc.TILE_KB, tile=tile, dte=6.0, isplit=ffc.TILE_ISPLIT)
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
            assert g.set_wide_external(True, min(t.im for t in tiles), min(t.jm for t in tiles))

            def dens(s, a, b, c):
                g.upload(s); g.call("dens", a, b, c); g.download(s)

            def baropg(s):
                g.upload(s); g.call("baropg_mcc" if int(s.npg) == 2 else "baropg"); g.download(s)

            finish_initial(st, dens, baropg)
            g.upload(st)
            board.barrier.wait()
            r0, s0 = g.exchange_rounds(), g.exchange_rounds_side()
            if prefix is not None:
                g.set_water_files(prefix, im_global=IMg, jm_global=JMg)
            g.run(TILE_WATER_STEPS)
            g.download()
            rounds[r] = (g.exchange_rounds() - r0, g.exchange_rounds_side() - s0)
            assert int(st.error_status) == 0
            g.close()
            out[r] = st
        except Exception:                                   # a dead rank must not leave the others at the barrier
            import traceback
            errs.append(traceback.format_exc())
            board.barrier.abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs[0]
    return out, rounds, tiles


def tiles_equal_single_tile(lib, tmp):
    """owned cells of the 2x2 run equal the single tile's, bit for bit, with every rank reading its own window; water adds no message
    round: pomgpu_exchange_rounds and _side are those of the same run with water off"""
    import forcing_files_checks as ffc
    mover = ffc.host_mover if lib is not None else ffc.device_mover
    IMg, JMg = ffc.TILE_GRID
    one = make_case("archipelago", IMg, JMg, ffc.TILE_KB, dte=6.0, isplit=ffc.TILE_ISPLIT)
    g = PomGpu(one, libpath=lib)

    def dens(s, a, b, c):
        g.upload(s); g.call("dens", a, b, c); g.download(s)

    def baropg(s):
        g.upload(s); g.call("baropg_mcc" if int(s.npg) == 2 else "baropg"); g.download(s)

    from extpom_amd.cases import finish_initial
    finish_initial(one, dens, baropg)
    g.upload(one)
    raw = wx.raw_water(one, (0, 1))
    prefix = str(tmp / "tiles")
    wx.write_all(prefix, raw, dtype="f")
    g.set_water_files(prefix)
    g.run(TILE_WATER_STEPS)
    g.download()
    g.close()
    assert same_bits(one.wssurfb[:JMg, :IMg], raw[0]) and same_bits(one.wssurff[:JMg, :IMg], raw[1])
    on, rounds_on, tiles = run_tiles(lib, mover, prefix)
    off, rounds_off, _ = run_tiles(lib, mover, None)
    assert rounds_on == rounds_off and all(r[0] > 0 and r[1] > 0 for r in rounds_on.values()), (rounds_on, rounds_off)
    for r, tile in enumerate(tiles):
        st = on[r]
        # the cells this tile owns: its patch without the line it shares with a neighbour to the west / south (decomp: one line of overlap each way)
        lo_i, lo_j = (1 if tile.n_west >= 0 else 0), (1 if tile.n_south >= 0 else 0)
        hi_i, hi_j = (st.im - 1 if tile.n_east >= 0 else st.im), (st.jm - 1 if tile.n_north >= 0 else st.jm)
        L = (slice(lo_j, hi_j), slice(lo_i, hi_i))
        G = (slice(st.j_off + lo_j, st.j_off + hi_j), slice(st.i_off + lo_i, st.i_off + hi_i))
        for n in ("wssurfb", "wssurff", "wssurf"):            # every cell of the patch, ghost lines too: each rank read its own window
            W = (slice(st.j_off, st.j_off + st.jm), slice(st.i_off, st.i_off + st.im))
            assert same_bits(st.field(n)[:st.jm, :st.im], one.field(n)[W]), (r, n)
        bad = [n for n in ("s", "sb", "t", "tb", "u", "v", "rho", "elb", "uab", "vab")
               if not same_bits(st.field(n)[(Ellipsis,) + L], one.field(n)[(Ellipsis,) + G])]
        assert not bad, (r, bad)
        assert not same_bits(st.s, off[r].s)                  # and water did move S on every tile
