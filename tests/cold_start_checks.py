"""The checks of pomgpu_cold_start (PomGpu.cold_start), each taking the library to load (None: the product library on device 0), so that
tests/test_cold_start_emulated.py (the host builds) and tests/test_gpu_cold_start.py (the device) cannot drift apart.  The bar is
tests/cold_start_expect.py's restatement of the reference's readers, read_grid and initial_conditions with the oracle's dens / baropg:
64-bit patterns on every array of blk2d and blk3d but the four scratch arrays, on bdry, blk1d and blkcon."""
import os
import threading

import numpy as np
import pytest

import cold_start_expect as E
from cold_start_expect import diff, same_bits
from extpom_amd import decomp
from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D
from extpom_amd.lib import PomGpuError
from extpom_amd.model import PomGpu, gpu_finish_initial
from oracle.pyoracle import OracleTile, oracle_finish_initial

CASE = "archipelago"
_cache = {}


def one_tile(im, jm):
    return decomp.make_tile(0, im, jm, im, jm)


def inputs(tmp, size, case=CASE, tiles=None, tag="", **kw):
    """(fields, paths) of one generated file set; the fields are asserted to hold what the checks need"""
    im, jm, kb = size
    nml = kw.pop("nml", {})
    f = E.case_fields(case, im, jm, kb, **nml)
    for j, i in kw.pop("land", ()):                         # more land cells (0-based) than the case has
        f["fsm"][j, i], f["h"][j, i] = 0.0, 1.0
        for n in ("T", "S", "Tclim", "Sclim"):
            f[n][..., j, i] = 0.0
    if case == CASE:
        E.assert_case_is_demanding(f, kb, tiles if tiles is not None else [one_tile(im, jm)])
    paths = E.write_files(tmp, f, tag=tag, **kw)
    E.assert_file_types(paths, kw.get("kind", "d"), kw.get("fsm_kind", "b"), kw.get("version", 2))
    return f, paths


def records(f, tile):
    """the two records restore_interior asks for in the first steps (what st.restore_records holds in make_case's states): months 1, 2 of
    the clim file on the tile's cells"""
    w = (slice(None), slice(tile.j_off, tile.j_off + tile.jm), slice(tile.i_off, tile.i_off + tile.im))
    return [(np.ascontiguousarray(f["Tclim"][n][w]), np.ascontiguousarray(f["Sclim"][n][w])) for n in range(2)]


def cold(lib, paths, tile, kb, nml, img=None, jmg=None, chunk_kb=None, f=None, **kw):
    b = E.blank_state(tile, kb, **nml)
    if f is not None:
        b.restore_records = records(f, tile)                # handed over by the constructor's upload: record slots survive the cold start
    g = PomGpu(b, libpath=lib, **kw)
    if chunk_kb:
        g.switch("IO_CHUNK_KB", chunk_kb)
    info = g.cold_start(*paths, im_global=img, jm_global=jmg)
    return g, b, info


def status(g):
    g.L.pomgpu_get_con(g.h, g._p(g.st.con))
    return int(g.st.error_status), g.L.pomgpu_last_error(g.h).decode()


# ---- 1: the state ---------------------------------------------------------------------------------------------------------------------
def state_equals_the_expectation(lib, tmp, size, nml=None, **kw):
    nml = nml or {}
    im, jm, kb = size
    f, paths = inputs(tmp, size, nml=nml, **kw)
    tile = one_tile(im, jm)
    a, cflmin = E.expected_state(paths, tile, kb, **nml)
    g, b, info = cold(lib, paths, tile, kb, nml)
    g.download()
    g.close()
    assert not diff(a, b), diff(a, b)
    assert info == {"cflmin": cflmin, "period": a.period} and int(b.error_status) == 0
    # the file's level kb of T, S did not arrive; the expectation is not the trivial one
    assert not b.tb[kb - 1].any() and not b.sb[kb - 1].any() and b.tb[:kb - 1].any() and (b.tb != b.sb).any()
    assert (b.dum != b.fsm).any() and (b.dvm != b.fsm).any() and (b.tclim[kb - 1] != 0).any()
    if float(b.ramp) == 0.0:
        # ramp as the reference's COMMON holds it until the first get_time (advance.f:69-72): baropg's "ramp*" leaves zeros of either sign,
        # and diff() above has compared the signs
        assert not b.drhox.any() and not b.drx2d.any() and np.signbit(b.drhox).any() and not np.signbit(b.drhox).all()
    else:
        assert b.drhox.any() and b.drx2d.any()
    return a, b


def many_runs_per_variable(lib, tmp, size=(65, 49, 21)):
    """POMGPU_IO_CHUNK_KB at its minimum: a buffer holds one band of rows, so a 21-level variable is 20 or 21 runs and both pinned buffers are
    reused many times"""
    im, jm, kb = size
    f, paths = inputs(tmp, size)
    tile = one_tile(im, jm)
    a, _ = E.expected_state(paths, tile, kb)
    g, b, _ = cold(lib, paths, tile, kb, {}, chunk_kb=1)
    g.download()
    g.close()
    assert not diff(a, b), diff(a, b)


def other_writers_files(lib, tmp, size=(20, 17, 6)):
    """an NC_FLOAT file set, and one with the variables in another order, extra variables, attributes, other dimension names, CDF-1, a
    fixed record dimension in clim and fsm as NC_SHORT / NC_INT"""
    im, jm, kb = size
    tile = one_tile(im, jm)
    for tag, kw in (("f", dict(kind="f")), ("s", dict(shuffle=True, version=1, fixed_clim=True, fsm_kind="h")), ("i", dict(fsm_kind="i", kind="f"))):
        f, paths = inputs(tmp, size, tag=tag, **kw)
        with open(paths[0], "rb") as fh:
            assert fh.read(4) == b"CDF" + bytes([kw.get("version", 2)])
        a, cflmin = E.expected_state(paths, tile, kb)
        g, b, info = cold(lib, paths, tile, kb, {})
        g.download()
        g.close()
        assert not diff(a, b), (tag, diff(a, b))
        assert info["cflmin"] == cflmin
        if kw.get("kind") == "f":                           # the float files hold other numbers than the double ones
            assert not same_bits(b.dx, f["dx"])


# ---- 2: steps after it ----------------------------------------------------------------------------------------------------------------
def steps_after_it(lib, tmp, case, size=(65, 49, 21), steps=4):
    im, jm, kb = size
    f, paths = inputs(tmp, size, case=case)
    tile = one_tile(im, jm)
    a, _ = E.expected_state(paths, tile, kb)
    a.restore_records = records(f, tile)
    u = a.copy()
    g, b, _ = cold(lib, paths, tile, kb, {}, f=f)
    h = PomGpu(u, libpath=lib)                               # a second context that uploaded the expected state
    OracleTile(a).run(steps)
    g.run(steps)
    h.run(steps)
    g.download()
    h.download()
    g.close()
    h.close()
    assert int(a.error_status) == 0 and a.u.any() and a.el.any()
    assert not diff(a, b), diff(a, b)
    assert not diff(u, b), diff(u, b)


# ---- 3: tiles -------------------------------------------------------------------------------------------------------------------------
TILE_GRID, TILE_KB, TILE_ISPLIT, TILE_STEPS = (97, 59), 11, 20, 4


def tiles(lib, tmp):
    """2x2 tiles, the east and north ones trimmed: every rank names the same files with its own i0, j0 and no message round is spent on
    the start; each tile equals the restatement on ITS window (its own period included); four steps under the wide halo equal the single
    tile on the cells a tile owns"""
    from forcing_files_checks import Board, device_mover, host_mover
    mover = host_mover if lib is not None else device_mover
    IMg, JMg = TILE_GRID
    nml = dict(dte=6.0, isplit=TILE_ISPLIT)
    iml, jml = decomp.local_size(IMg, JMg, 2, 2)
    tl = [decomp.make_tile(r, IMg, JMg, iml, jml, n_proc=4) for r in range(4)]
    assert {(t.im, t.jm) for t in tl} == {(50, 31), (49, 31), (50, 30), (49, 30)}
    # land in every tile's window line (the owner's last-but-one line) and on its ghost line, which the archipelago lacks at this size
    si, sj = tl[1].i_off, tl[2].j_off
    land = [(10, si - 1), (12, si), (40, si - 1), (43, si), (sj - 1, 10), (sj, 13), (sj - 1, 70), (sj, 73)]
    f, paths = inputs(tmp, (IMg, JMg, TILE_KB), tiles=tl, nml=nml, land=land)
    board, out, errs = Board(4), {}, []

    def rank(r):
        try:
            tile = tl[r]
            st = E.blank_state(tile, TILE_KB, **nml)
            st.restore_records = records(f, tile)
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
            assert g.set_wide_external(True, min(t.im for t in tl), min(t.jm for t in tl))
            rounds = g.exchange_rounds()
            info = g.cold_start(*paths, im_global=IMg, jm_global=JMg)
            assert g.exchange_rounds() == rounds, "the cold start posted a message round"
            g.download()
            first = st.copy()
            board.barrier.wait()
            g.run(TILE_STEPS)
            g.download()
            assert int(st.error_status) == 0
            g.close()
            out[r] = (first, info, st)
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
    periods = set()
    for r in range(4):
        a, cflmin = E.expected_state(paths, tl[r], TILE_KB, **nml)
        first, info, _ = out[r]
        assert not diff(a, first), (r, diff(a, first))
        assert info == {"cflmin": cflmin, "period": a.period}
        periods.add(a.period)
    assert len(periods) > 1, "every tile has the same period: the per-tile midpoint is not exercised"
    one = one_tile(IMg, JMg)
    g, s, _ = cold(lib, paths, one, TILE_KB, nml, f=f)
    g.run(TILE_STEPS)
    g.download()
    g.close()
    bad = []
    for r in range(4):
        tile, st = tl[r], out[r][2]
        io, jo, im, jm = tile.i_off, tile.j_off, tile.im, tile.jm
        sl_j = slice(0 if jo == 0 else 1, jm if jo + jm == JMg else jm - 1)       # the cells the tile owns
        sl_i = slice(0 if io == 0 else 1, im if io + im == IMg else im - 1)
        for n in BLK2D + BLK3D:
            if n in E.SCRATCH:
                continue
            if not same_bits(s.field(n)[..., jo:jo + jm, io:io + im][..., sl_j, sl_i], st.field(n)[..., :jm, :im][..., sl_j, sl_i]):
                bad.append((r, n))
    assert not bad, bad


# ---- 4: refusals ----------------------------------------------------------------------------------------------------------------------
def refusals(lib, tmp, size=(8, 8, 6)):
    """every refusal leaves mirrors, slots and blkcon as they were (but error_status = 1) and names the file and the cause"""
    im, jm, kb = size
    tile = one_tile(im, jm)
    f, good = inputs(tmp, size, tag="good")
    want, _ = E.expected_state(good, tile, kb)
    # the state every refusal must leave is NOT what the files would produce: another case, stepped, so that a reader which wrote a plane,
    # period or rf* before refusing a later file would show
    b = make_case("seamount", im, jm, kb)
    oracle_finish_initial(b)
    b.rfe = b.rfw = 0.5
    g = PomGpu(b, libpath=lib)
    g.run(2)
    g.download()
    before = b.copy()
    assert all(not same_bits(before.field(n), want.field(n)) for n in ("h", "dx", "cor", "tb", "tclim", "aru", "dum", "cbc", "l", "el"))
    assert before.period != want.period and before.rfe != want.rfe
    count = [0]

    def refused(cause, which, paths, img=None, jmg=None, nml=None):
        count[0] += 1
        if nml:
            g.set_con(**nml)
        with pytest.raises(PomGpuError) as e:
            g.cold_start(*paths, im_global=img, jm_global=jmg)
        es, msg = status(g)
        assert es == 1 and cause in msg and (which is None or os.path.basename(paths[which]) in msg), (cause, msg)
        assert "status -1" in str(e.value)
        g.set_con(error_status=0, **{k: getattr(before, k) for k in (nml or {})})
        g.download()
        assert not diff(before, b), (cause, diff(before, b))

    names = [(0, n) for n in ["z", "zz"] + list(E.GRID_PLANES)] + [(1, n) for n in ("Level", "T", "S")] + [(2, n) for n in ("Tclim", "Sclim")]
    for q, (which, n) in enumerate(names):                  # each required name dropped in turn
        refused(f"variable {n} is absent", which, E.write_files(tmp, f, drop=(n,), tag=f"drop{q}"))
    refused("variable dx has NetCDF type 4", 0, E.write_files(tmp, f, retype={"dx": "i"}, tag="ty0"))
    refused("variable T has NetCDF type 4", 1, E.write_files(tmp, f, retype={"T": "i"}, tag="ty2"))
    refused("variable Sclim has NetCDF type 3", 2, E.write_files(tmp, f, retype={"Sclim": "h"}, tag="ty3"))
    refused("variable h has the dimension lengths (8, 7)", 0, E.write_files(tmp, f, reshape={"h": ("y", "short")}, tag="sh0"))
    refused("variable z has the dimension lengths (8, 8)", 0, E.write_files(tmp, f, reshape={"z": ("y", "x")}, tag="sh1"))
    refused("variable S has the dimension lengths (unlimited, 8, 8, 7)", 1, E.write_files(tmp, f, reshape={"S": ("Time", "Level", "y", "short")}, tag="sh2"))
    refused("variable Tclim has the dimension lengths (unlimited, 6, 8, 7)", 2, E.write_files(tmp, f, reshape={"Tclim": ("month", "zlev", "y", "short")}, tag="sh3"))
    refused("9 records, wanted >= 10", 2, E.write_files(tmp, f, clim_records=9, tag="nine"))
    refused("(>= 10, 6, 8, 8)", 2, E.write_files(tmp, f, clim_records=9, fixed_clim=True, tag="nine_fixed"))
    short = dict(f, T=f["T"][:kb - 2], S=f["S"][:kb - 2], Level=f["Level"][:kb - 2])
    refused("levels, wanted >= 5", 1, E.write_files(tmp, short, tag="levels"))
    for which, keep in ((0, 0.9), (1, 0.6), (2, 0.7)):      # a file shorter than begin + size
        p = E.write_files(tmp, f, tag=f"trunc{which}")
        os.truncate(p[which], int(os.path.getsize(p[which]) * keep))
        refused("beyond the file's", which, p)
    for which in range(3):                                  # CDF-5 and HDF5 magic
        p = E.write_files(tmp, f, tag=f"cdf5{which}")
        with open(p[which], "r+b") as fh:
            fh.seek(3)
            fh.write(b"\x05")
        refused("CDF version 5", which, p)
    p = E.write_files(tmp, f, tag="hdf")
    with open(p[1], "r+b") as fh:
        fh.write(b"\x89HDF")
    refused("HDF5", 1, p)
    refused("does not fit the global grid", 0, good, img=im - 1)
    refused("variable dx has the dimension lengths (8, 8)", 0, good, jmg=jm + 1)     # a larger global grid: the variables are misshapen
    eq = dict(f, lat_rho=f["lat_rho"].copy())
    eq["lat_rho"][jm // 2 - 1, im // 2 - 1] = 0.0
    refused("cor(im/2, jm/2) of this tile is zero", 0, E.write_files(tmp, eq, tag="equator"))
    two = dict(f, fsm=f["fsm"].copy())
    two["fsm"][3, 4] = 2.0
    refused("variable fsm holds 2.000000 at global (5, 4), neither 0 nor 1", 0, E.write_files(tmp, two, tag="fsm2"))
    refused("invalid value for npg", None, good, nml=dict(npg=3))
    refused("cannot open", None, [good[0], str(tmp / "absent.nc"), good[2]])
    assert count[0] == 43
    # the context is as usable as before: the same call with the good files goes through and gives the files' state (time, iint stay)
    g.cold_start(*good)
    g.download()
    g.close()
    assert int(b.iint) == 2 and b.time == before.time
    b.con[...] = want.con
    assert not diff(want, b), diff(want, b)


# ---- 5: a context that has stepped ----------------------------------------------------------------------------------------------------
def on_a_context_that_has_stepped(lib, tmp, size=(20, 17, 6)):
    """lazy wr, uf vf pending, valid depth sums of u, v, forcing-free steps behind it: the cold start leaves the same state as on a fresh
    context, and the steps that follow are the fresh context's"""
    im, jm, kb = size
    tile = one_tile(im, jm)
    f, paths = inputs(tmp, size)
    a, _ = E.expected_state(paths, tile, kb)
    live = make_case("seamount", im, jm, kb)
    oracle_finish_initial(live)
    live.restore_records = records(f, tile)
    live.con[...] = a.con                                   # read_input's constants are the run's; time, iint are set below
    g = PomGpu(live, libpath=lib)
    g.run(3)
    g.cold_start(*paths)
    g.download()
    assert int(live.iint) == 3 and live.time != 0.0          # time and iint stay untouched ...
    live_con = live.con.copy()
    live.con[...] = a.con
    live.period = a.period
    assert not diff(a, live), diff(a, live)                 # ... and everything else is the fresh context's
    live.con[...] = live_con
    g.set_con(iint=0, time=0.0)
    h, b, _ = cold(lib, paths, tile, kb, {}, f=f)
    g.run(2)
    h.run(2)
    g.download()
    h.download()
    g.close()
    h.close()
    assert not diff(b, live), diff(b, live)


# ---- 6: the fp32 builds ---------------------------------------------------------------------------------------------------------------
def f32_equals_gpu_finish_initial(lib, tmp, size=(65, 49, 21)):
    """the fp32-storage builds have no oracle: the bar is model.gpu_finish_initial -- today's way in, an upload and a download around every
    routine -- on the SAME library, fed the files' fields; cbc by math.log, as everywhere"""
    im, jm, kb = size
    tile = one_tile(im, jm)
    f, paths = inputs(tmp, size)
    a, cflmin = E.expected_readers(paths, tile, kb)
    gpu_finish_initial(a, libpath=lib)
    E.bottom_friction(a)
    g, b, info = cold(lib, paths, tile, kb, {})
    g.download()
    g.close()
    assert not diff(a, b), diff(a, b)
    assert info["cflmin"] == cflmin
    assert same_bits(b.tb, b.tb.astype(np.float32)) and not same_bits(a.q2lb, a.l * a.q2b) and b.drx2d.any()


# ---- 7: the whole of program pom ----------------------------------------------------------------------------------------------------
def cold_start_to_restart_and_on(lib, tmp, size=(65, 49, 21), steps=5):
    """cold_start, forcing files, run, write_file("restart"); then a fresh context -- cold start, forcing files, read_restart -- and one
    more step: the bits of the oracle started from the reader's state (tests/restart_expect.py), fed the records tests/forcing_expect.py
    restates.  The forced steps of the first context equal the oracle's too."""
    import forcing_expect as fx
    import forcing_files_checks as ffc
    import restart_expect as rx
    im, jm, kb = size
    nml = dict(ffc.BASE)
    tile = one_tile(im, jm)
    f, paths = inputs(tmp, size, nml=nml)

    def oracle_start():
        a, _ = E.expected_state(paths, tile, kb, **nml)
        a.restore_records = records(f, tile)
        return a

    a = oracle_start()
    ns, nl, _, _ = ffc.schedule(a, steps)
    raw_s, raw_l = fx.raw_sfrc(a, ns), fx.raw_lbry(a, nl)
    sfrc, lbry = ffc.files(tmp, raw_s, raw_l)

    def with_records(st):
        st.forcing_records = fx.forcing_records(st, raw_s)
        st.lateral_records = fx.lateral_records(st, raw_l)
        return st

    with_records(a)
    g, b, _ = cold(lib, paths, tile, kb, nml, f=f)
    g.set_forcing_files(sfrc=sfrc, lbry=lbry)
    g.run(steps)
    rst = tmp / "cold.restart.nc"
    g.write_file("restart", rst, title="cold", time_start=rx.START)
    g.io_wait()
    g.download()
    g.close()
    OracleTile(a).run(steps)
    assert int(a.error_status) == 0 and a.wusurf.any() and a.u.any()
    assert not diff(a, b), diff(a, b)
    h, c, _ = cold(lib, paths, tile, kb, nml, f=f)
    h.set_forcing_files(sfrc=sfrc, lbry=lbry)
    time0, iint = h.read_restart(rst)
    assert iint == steps and time0 == a.time
    h.run(1)
    h.download()
    h.close()
    a2 = with_records(oracle_start())
    rx.assign_from_file(a2, rst)
    OracleTile(a2).run(1)
    assert not diff(a2, c), diff(a2, c)
    assert not same_bits(a2.t, a.t)
