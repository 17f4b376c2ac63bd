"""The checks of pomgpu_set_lateral_sides -- the lbry file feeding any of the four open boundaries --, each taking the library to load (None:
the product library on device 0), shared by tests/test_lateral_sides_emulated.py and tests/test_gpu_lateral_sides.py.  The files and the
expected records are tests/lateral_sides_expect.py's (numpy, without the code under test); the bar is the CPU oracle fed those records and
a second context fed them through set_lateral_records: 64-bit patterns of every array of blk2d and blk3d, bdry and blkcon
(forcing_files_checks.diff), so the tangential lines that only reach vbwf, vabwf, ubnf ... are covered."""
import threading

import numpy as np
import pytest

import forcing_expect as fx
import forcing_files_checks as ffc
import lateral_sides_expect as LS
import ztosig_line_files_checks as zlf
from extpom_amd import decomp
from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D
from extpom_amd.lib import PomGpuError
from extpom_amd.model import PomGpu
from forcing_files_checks import diff, same_bits, status
from oracle.pyoracle import OracleTile, oracle_finish_initial

SIZE = (65, 49, 21)
STEPS = 21                                                    # ibc = 10 at dti = 360 s: lateral_bc reads records 1, 2 at step 1, 3 at step 10, 4 at step 20
ALL = 15
OPEN = {"archipelago": ALL, "island": ALL, "seamount": LS.EAST | LS.WEST}   # the sides a case's water reaches (seamount: closed north and south)


def set_sides(g, mask):
    g.set_lateral_sides(east=bool(mask & 1), south=bool(mask & 2), west=bool(mask & 4), north=bool(mask & 8))


# ---- the conditions on the inputs, on the arrays, before any library is loaded --------------------------------------------------------------
def assert_inputs_are_demanding(st, recs, mask):
    """every ON side's temp / salt line differs from the tclim / sclim line it replaces, its u, v and zeta lines are non-zero, and
    consecutive records differ"""
    assert len(recs) >= 2
    for side in LS.SIDES:
        if not LS.on(mask, side):
            continue
        n = st.jm if LS.along_j(side) else st.im
        for r, rec in enumerate(recs):
            for var, clim in (("temp", st.tclim), ("salt", st.sclim)):
                assert not same_bits(rec[LS.place(side, var)][:, :n], LS.clim_line(st, clim, side)), (side, var, r)
            for var in ("u", "v"):
                assert rec[LS.place(side, var)][:, :n].any(), (side, var, r)
            assert rec[LS.ELEV[side]][:n].any(), (side, "zeta", r)
        for r in range(len(recs) - 1):
            for at in [LS.place(side, v) for v in ("temp", "salt", "u", "v")] + [LS.ELEV[side]]:
                assert not same_bits(recs[r][at], recs[r + 1][at]), (side, at, r)


def assert_the_new_lines_enter_the_step(a_all, a_two, open_sides=ALL):
    """the ORACLE's state after the run with the mask's records differs from its state with the default-mask records in t, uaf / ua and el:
    otherwise the new lines never entered the step and the comparison shows nothing.  open_sides: a case with closed sides (seamount's
    north and south are land) can meet this through its open ones alone, which is what the caller's mask then holds"""
    assert open_sides & (LS.WEST | LS.NORTH)
    assert not same_bits(a_all.t, a_two.t), "t"
    assert not same_bits(a_all.uaf, a_two.uaf) or not same_bits(a_all.ua, a_two.ua), "uaf / ua"
    assert not same_bits(a_all.el, a_two.el), "el"


# ---- 1: file path = setter path = oracle across record changes ------------------------------------------------------------------------------
def file_setters_oracle(lib, tmp, case, mask=ALL, nml=None, dtype="d", chunk_kb=None, setters=True, steps=STEPS, size=SIZE):
    nml = dict(ffc.BASE) if nml is None else nml
    a, raw_s, _ = ffc.start(case, nml, steps, size=size)
    _, nl, _, ibc = ffc.schedule(a, steps)
    assert ibc == 10 and nl >= 4
    two = a.copy()                                            # the default mask's records: forcing_expect's own
    raw_l = LS.raw_lbry(a, nl)
    a.lateral_records = LS.lateral_records(a, raw_l, mask)
    assert mask & OPEN[case] == mask, "the mask names open sides only"
    assert_inputs_are_demanding(a, a.lateral_records, mask)
    assert max(a.jm, a.im) > 64 and a.jm_local + a.im_local > 64, "lines longer than a wavefront, several workgroups"
    b, s = a.copy(), a.copy()
    sfrc = fx.write_sfrc(tmp / "case.sfrc.nc", raw_s)
    lbry = LS.write_lbry(tmp / "case.lbry.nc", raw_l, mask, dtype=dtype)
    OracleTile(a).run(steps)
    OracleTile(two).run(steps)
    assert int(a.error_status) == 0 and int(two.error_status) == 0
    assert_the_new_lines_enter_the_step(a, two, mask)
    g = PomGpu(b, libpath=lib)
    if chunk_kb:
        g.switch("IO_CHUNK_KB", chunk_kb)
    set_sides(g, mask)
    g.set_forcing_files(sfrc=sfrc, lbry=lbry)
    g.run(steps)                                              # ONE call across every record change
    g.download()
    assert not diff(a, b), diff(a, b)
    g.close()
    if setters:
        h = PomGpu(s, libpath=lib)
        ffc.step_with_setters(h, steps)
        h.download()
        assert not diff(b, s, skip=()), diff(b, s, skip=())   # two contexts of one library: the scratch arrays too
        h.close()


# ---- 2: every mask ----------------------------------------------------------------------------------------------------------------------------
def every_mask(lib, tmp, size, case="archipelago"):
    """masks 1..15 with a file that holds ONLY the ON sides' variables: after lateral_bc's first call (records 1 and 2) every b and f line
    and the four elevation lines equal the expectation, and after one whole step the state -- every member of bdry -- is the oracle's"""
    init, raw_s, _ = ffc.start(case, ffc.BASE, 1, size=size)
    assert init.im != init.jm or size == (8, 8, 6)
    raw_l = LS.raw_lbry(init, 2)
    sfrc = fx.write_sfrc(tmp / "case.sfrc.nc", raw_s)
    for mask in range(1, 16):
        a = init.copy()
        a.lateral_records = LS.lateral_records(a, raw_l, mask)
        assert_inputs_are_demanding(a, a.lateral_records, mask)
        want = a.lateral_records
        lbry = LS.write_lbry(tmp / f"m{mask}.lbry.nc", raw_l, mask)
        from scipy.io import netcdf_file
        with netcdf_file(lbry, "r", mmap=False) as nc:
            assert set(nc.variables) == set(LS.names(mask)), "the file holds the ON sides' variables only"
        for whole_step in (False, True):
            b = init.copy()
            g = PomGpu(b, libpath=lib)
            set_sides(g, mask)
            g.set_forcing_files(sfrc=sfrc, lbry=lbry)
            if whole_step:
                o = a.copy()
                OracleTile(o).run(1)
                g.run(1)
                g.download()
                assert not diff(o, b), (mask, diff(o, b))
            else:
                g.set_con(iint=1)
                g.call("lateral_bc")
                g.download()
                for at, name in enumerate(LS.ORDER16):
                    for rec, sfx in ((0, "b"), (1, "f"))[0 if name[0] in "ts" else 1:]:   # the reference refreshes the b copies of t, s alone (bounds_forcing.f:742-753)
                        assert same_bits(b.field(name + sfx), want[rec][at]), (mask, name + sfx)
                for side, at in LS.ELEV.items():
                    assert same_bits(b.field("el" + LS.LETTER[side]), want[1][at]), (mask, side)
            g.close()


# ---- 3: the default is today's ------------------------------------------------------------------------------------------------------------------
def default_is_todays(lib, tmp, size=(20, 17, 6), steps=11):
    """with the default mask a four-sided file gives the state a two-sided file gives (the oracle's, fed forcing_expect's records); naming
    EAST|SOUTH explicitly gives the same state as never calling"""
    a, raw_s, raw_two = ffc.start("archipelago", ffc.BASE, steps, size=size)
    init = a.copy()
    raw_four = LS.raw_lbry(init, raw_two["zeta.east"].shape[0])
    assert all(same_bits(raw_four[n], raw_two[n]) for n in fx.LBRY)
    two = fx.write_lbry(tmp / "two.lbry.nc", raw_two)
    four = LS.write_lbry(tmp / "four.lbry.nc", raw_four, ALL)
    sfrc = fx.write_sfrc(tmp / "case.sfrc.nc", raw_s)
    OracleTile(a).run(steps)
    got = []
    for lbry, explicit in ((two, False), (four, False), (two, True), (four, True)):
        b = init.copy()
        g = PomGpu(b, libpath=lib)
        if explicit:
            g.set_lateral_sides(east=True, south=True)
        g.set_forcing_files(sfrc=sfrc, lbry=lbry)
        g.run(steps)
        g.download()
        g.close()
        assert not diff(a, b), (lbry, explicit, diff(a, b))
        got.append(b)
    for b in got[1:]:
        assert not diff(got[0], b, skip=()), diff(got[0], b, skip=())


# ---- 4: z levels with sides -------------------------------------------------------------------------------------------------------------------
def assert_z_records_are_demanding(st, recs, mask):
    kb = st.kb
    assert len(recs) >= 2
    for name, edge, _, at in LS.zvars(mask):
        n = st.jm if edge in (0, 2) else st.im
        a = [r[at] for r in recs]
        assert all(x[kb - 1].any() and np.isfinite(x).all() for x in a) and not same_bits(a[0], a[1])
        assert same_bits(a[0][:, 0], a[0][:, 1]) and same_bits(a[0][:, n - 1], a[0][:, n - 2]) and a[0][:, 0].any() and a[0][:, n - 1].any()
        clim = st.sclim if name.startswith("salt") else st.tclim
        assert not same_bits(a[0][:, :n], LS.clim_line(st, clim, LS.SIDES[edge]))


def z_file_setters_oracle(lib, tmp, case, size=SIZE, mask=ALL, kind="d", chunk_kb=None, setters=True, steps=STEPS):
    """mask 15 under set_z_inputs(lbry=True): the expectation for edges 2 and 3 comes from ztosig_line_expect.ztosig_line, which the recorded
    digests hold to the reference's ztosig_"""
    a, raw_s, _ = ffc.start(case, ffc.BASE, steps, size=size)
    _, nl, _, ibc = ffc.schedule(a, steps)
    assert ibc == 10 and nl >= 4
    raw_l = LS.raw_lbry_z(a, nl, kind=kind)
    a.lateral_records = LS.lateral_records_z(a, raw_l, mask)
    assert_z_records_are_demanding(a, a.lateral_records, mask)
    b, s = a.copy(), a.copy()
    sfrc = fx.write_sfrc(tmp / "case.sfrc.nc", raw_s)
    lbry = LS.write_lbry_z(tmp / "case.lbry.nc", raw_l, mask, kind=kind)
    g = PomGpu(b, libpath=lib)
    if chunk_kb:
        g.switch("IO_CHUNK_KB", chunk_kb)
    g.set_z_inputs(lbry=True)
    set_sides(g, mask)
    g.set_forcing_files(sfrc=sfrc, lbry=lbry)
    g.run(steps)
    OracleTile(a).run(steps)
    g.download()
    assert int(a.error_status) == 0 and not diff(a, b), diff(a, b)
    g.close()
    if setters:
        h = PomGpu(s, libpath=lib)
        ffc.step_with_setters(h, steps)
        h.download()
        assert not diff(b, s, skip=()), diff(b, s, skip=())
        h.close()


def all_on_z_after_a_cold_start(lib, tmp, case="archipelago", size=SIZE, steps=STEPS, mask=ALL):
    """init, clim and lbry on three different sets of z levels, the lbry file four-sided: the cold start of tests/ztosig_files_checks.py,
    then one run across three lateral records (dti = 180 s, as in ztosig_line_files_checks.all_on_z_after_a_cold_start)"""
    import ztosig_files_checks as zfc
    assert len({zfc.KS_INIT, zfc.KS_CLIM, zlf.KS_LBRY}) == 3
    im, jm, kb = size
    nml = dict(dte=6.0, isplit=30)
    f, paths = zfc.z_inputs(tmp, size, case=case, nml=nml)
    tile = zfc.one_tile(im, jm)
    a, _ = zfc.expected_state_z(paths, tile, kb, True, True, **nml)
    recs = zfc.records(paths, tile, kb, True)
    a.restore_records = recs
    _, nl, _, ibc = ffc.schedule(a, steps)
    assert ibc == 20 and nl == 3
    raw_l = LS.raw_lbry_z(a, nl)
    a.lateral_records = LS.lateral_records_z(a, raw_l, mask)
    assert_z_records_are_demanding(a, a.lateral_records, mask)
    lbry = LS.write_lbry_z(tmp / "case.lbry.nc", raw_l, mask)
    g, b, _ = zfc.cold(lib, paths, tile, kb, True, True, nml, recs=recs)
    g.set_z_inputs(init=True, clim=True, lbry=True)
    set_sides(g, mask)
    g.set_forcing_files(lbry=lbry)
    OracleTile(a).run(steps)
    g.run(steps)
    g.download()
    g.close()
    assert int(a.error_status) == 0 and a.u.any() and a.el.any() and float(np.abs(a.u).max()) < 20.0
    assert not diff(a, b), diff(a, b)


# ---- 5: tiles -------------------------------------------------------------------------------------------------------------------------------
TILE_GRID, TILE_KB, TILE_STEPS = (37, 29), 6, 4


def tiles(lib, tmp, mask=ALL):
    """2x2 tiles of 37x29x6, the east and north ones trimmed, wide halo, the library's exchange, z levels on: every rank names the same
    four-sided file with its own i0, j0.  After the first lateral_bc every tile's b and f lines equal the restatement on its window, ghost
    ends included, with no message round spent; after four steps owned cells equal the single tile's.  Two ranks: NC_FLOAT numbers read in
    1-KiB chunks (the file is NC_FLOAT for all)"""
    from forcing_files_checks import Board, device_mover, host_mover
    mover = host_mover if lib is not None else device_mover
    IMg, JMg = TILE_GRID
    nml = dict(dte=6.0, isplit=8)                            # the wide halo wants tiles of isplit + 7 cells
    one = make_case("archipelago", IMg, JMg, TILE_KB, **nml)
    oracle_finish_initial(one)
    iml, jml = decomp.local_size(IMg, JMg, 2, 2)
    tl = [decomp.make_tile(r, IMg, JMg, iml, jml, n_proc=4) for r in range(4)]
    assert len({(t.im, t.jm) for t in tl}) == 4 and any(t.im < t.im_local for t in tl) and any(t.jm < t.jm_local for t in tl)
    _, nl, _, _ = ffc.schedule(one, TILE_STEPS)
    raw_l = LS.raw_lbry_z(one, nl, kind="f")
    sj, si = tl[2].j_off, tl[1].i_off                         # the seams: a missing value at either ghost end whose fill needs the window point
    for name, edge, _, _ in LS.zvars(mask):
        c = sj if edge in (0, 2) else si
        raw_l[name][:, 0, c - 1:c + 3] = (21.0, 0.0, 0.0, 22.0)
    assert_inputs_are_demanding(one, LS.lateral_records_z(one, raw_l, mask), mask)
    lbry = LS.write_lbry_z(tmp / "tiles.lbry.nc", raw_l, mask, kind="f")
    board, out, errs = Board(4), {}, []

    def rank(r):
        try:
            tile = tl[r]
            st = make_case("archipelago", IMg, JMg, TILE_KB, tile=tile, **nml)
            for n in BLK2D + BLK3D:                           # the finished initial state, cut to the tile
                st.field(n)[..., :tile.jm, :tile.im] = one.field(n)[..., tile.j_off:tile.j_off + tile.jm, tile.i_off:tile.i_off + tile.im]
            for n in ("tbe", "sbe", "tbw", "sbw"):
                st.field(n)[:, :tile.jm] = one.field(n)[:, tile.j_off:tile.j_off + tile.jm]
            for n in ("tbn", "sbn", "tbs", "sbs"):
                st.field(n)[:, :tile.im] = one.field(n)[:, tile.i_off:tile.i_off + tile.im]
            st.con[...] = one.con
            want = LS.lateral_records_z(st, raw_l, mask)
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
            if r % 2:
                g.switch("IO_CHUNK_KB", 1)
            g.set_z_inputs(lbry=True)
            set_sides(g, mask)
            g.set_forcing_files(lbry=lbry, im_global=IMg, jm_global=JMg)
            rounds = g.exchange_rounds()
            g.set_con(iint=1)
            g.call("lateral_bc")                              # records 1 and 2 into the b and f lines
            assert g.exchange_rounds() == rounds, "lateral_bc posted a message round"
            g.download()
            for at, name in enumerate(LS.ORDER16):
                for rec, sfx in ((0, "b"), (1, "f"))[0 if name[0] in "ts" else 1:]:
                    assert same_bits(st.field(name + sfx), want[rec][at]), (r, name + sfx)
            for side, at in LS.ELEV.items():
                assert same_bits(st.field("el" + LS.LETTER[side]), want[1][at]), (r, side)
            g.set_con(iint=0)
            board.barrier.wait()
            g.run(TILE_STEPS)
            g.download()
            assert int(st.error_status) == 0
            g.close()
            out[r] = (st, want)
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
    # the ghost end of the south-west tile's WEST line is not what it would be without the window point
    t0, w0 = tl[0], out[0][1]
    assert t0.n_north != -1 and w0[0][0][:, t0.jm - 1].any() and not same_bits(w0[0][0][:, t0.jm - 1], w0[0][0][:, t0.jm - 2])
    s = one.copy()
    g = PomGpu(s, libpath=lib)
    g.set_z_inputs(lbry=True)
    set_sides(g, mask)
    g.set_forcing_files(lbry=lbry)
    g.run(TILE_STEPS)
    g.download()
    g.close()
    bad = []
    for r in range(4):
        tile, st = tl[r], out[r][0]
        io, jo, im, jm = tile.i_off, tile.j_off, tile.im, tile.jm
        sl_j = slice(0 if jo == 0 else 1, jm if jo + jm == JMg else jm - 1)       # the cells the tile owns
        sl_i = slice(0 if io == 0 else 1, im if io + im == IMg else im - 1)
        for n in BLK2D + BLK3D:
            if n in ffc.SCRATCH:
                continue
            if not same_bits(s.field(n)[..., jo:jo + jm, io:io + im][..., sl_j, sl_i], st.field(n)[..., :jm, :im][..., sl_j, sl_i]):
                bad.append((r, n))
    assert not bad, bad


# ---- 6: refusals on a foreign, stepped state ----------------------------------------------------------------------------------------------------
def refusals(lib, tmp, size=(8, 8, 6)):
    """every refusal names its cause and leaves a foreign state (seamount, stepped) and the registration as they were (but error_status = 1)"""
    im, jm, kb = size
    a, raw_s, _ = ffc.start("seamount", ffc.BASE, 11, size=size)
    raw = LS.raw_lbry(a, 3)
    rawz = LS.raw_lbry_z(a, 3)
    b = a.copy()
    g = PomGpu(b, libpath=lib)
    g.run(2)
    g.download()
    before = b.copy()

    def check(call, *causes):
        with pytest.raises(PomGpuError) as e:
            call()
        es, msg = status(g)
        assert es == 1 and all(c in msg for c in causes), (causes, msg)
        assert "status -1" in str(e.value)
        g.set_con(error_status=0)
        g.download()
        assert not diff(before, b), (causes, diff(before, b))

    for bad in (0, 16, -1):                                   # the mask itself
        rc = g.L.pomgpu_set_lateral_sides(g.h, bad)
        es, msg = status(g)
        assert rc == -1 and es == 1 and "outside 1..15" in msg and str(bad) in msg, (bad, rc, msg)
        g.set_con(error_status=0)
    g.download()
    assert not diff(before, b)
    count = 0
    for mask in (LS.WEST, LS.NORTH | LS.EAST, ALL):           # every variable of an ON side absent, named in the message
        set_sides(g, mask)
        for name in LS.names(mask):
            check(lambda: g.set_forcing_files(lbry=LS.write_lbry(tmp / "absent.lbry.nc", raw, mask, drop=(name,))), f"variable {name} is absent", "absent.lbry.nc")
            count += 1
    assert count == 5 + 10 + 20
    set_sides(g, ALL)
    # a wrong line length: the axes of a side swapped (im != jm would show; here another length altogether), a wrong level count
    short = dict(raw)
    short["zeta.west"] = raw["zeta.west"][:, :jm - 1]
    check(lambda: g.set_forcing_files(lbry=LS.write_lbry(tmp / "len.lbry.nc", short, ALL)), "variable zeta.west has the dimension lengths", f"wanted (records, {jm})")
    short = dict(raw)
    short["temp.north"] = raw["temp.north"][:, :, :im - 1]
    check(lambda: g.set_forcing_files(lbry=LS.write_lbry(tmp / "len3.lbry.nc", short, ALL)), "variable temp.north has the dimension lengths", f"wanted (records, {kb}, {im})")
    short = dict(raw)
    short["v.west"] = np.concatenate([raw["v.west"], raw["v.west"][:, -1:]], axis=1)
    check(lambda: g.set_forcing_files(lbry=LS.write_lbry(tmp / "lev.lbry.nc", short, ALL)), "variable v.west has the dimension lengths", f"wanted (records, {kb}, {jm})")
    g.set_z_inputs(lbry=True)                                 # ... and with z: temp / salt on the levels of z, u / v on sigma levels
    ks = zlf.KS_LBRY
    check(lambda: g.set_forcing_files(lbry=LS.write_lbry_z(tmp / "zlev.lbry.nc", rawz, ALL, levels_of={"salt.west": ks + 1})),
          f"variable salt.west has the dimension lengths (unlimited, {ks + 1}, {jm}), wanted (records, {ks}, {jm})")
    check(lambda: g.set_forcing_files(lbry=LS.write_lbry_z(tmp / "zsig.lbry.nc", rawz, ALL, levels_of={"temp.north": kb})),
          f"variable temp.north has the dimension lengths (unlimited, {kb}, {im}), wanted (records, {ks}, {im})")
    check(lambda: g.set_forcing_files(lbry=LS.write_lbry_z(tmp / "zu.lbry.nc", rawz, ALL, levels_of={"u.north": ks})),
          f"variable u.north has the dimension lengths (unlimited, {ks}, {im}), wanted (records, {kb}, {im})")
    check(lambda: g.set_forcing_files(lbry=LS.write_lbry_z(tmp / "zlen.lbry.nc", rawz, ALL, length_of={"temp.west": jm + 1})), "variable temp.west has the dimension lengths")
    g.set_z_inputs(lbry=False)
    # an OFF side's variables absent or misshapen: NOT refused.  Nothing above was registered: the mask is still free
    set_sides(g, LS.EAST | LS.WEST)
    odd = dict(raw)
    odd["temp.north"] = raw["temp.north"][:, :2, :3]
    names = tuple(n for n in LS.names(ALL) if not n.endswith(".south"))
    good = fx.write_file(str(tmp / "good.lbry.nc"), odd, names)
    g.set_forcing_files(lbry=good)
    g.download()
    assert not diff(before, b), diff(before, b)
    # a registered file pins the mask; the same mask again is fine
    check(lambda: set_sides(g, ALL), "set_lateral_sides", "an lbry file is registered", "mask 5")
    set_sides(g, LS.EAST | LS.WEST)
    # a second registration with a refused file keeps the first one in use
    check(lambda: g.set_forcing_files(lbry=LS.write_lbry(tmp / "late.lbry.nc", raw, LS.EAST | LS.WEST, drop=("u.west",))), "variable u.west is absent")
    # a record beyond the file at the fetch: three records, lateral_bc at step 10 of a fresh context asks for record 4 at step 20
    c = a.copy()
    h = PomGpu(c, libpath=lib)
    set_sides(h, LS.EAST | LS.WEST)
    h.set_forcing_files(lbry=good)
    rc = h.L.pomgpu_run(h.h, 21)
    err, msg = status(h)
    assert rc != 0 and err == 1 and "record 4" in msg and "lateral_bc" in msg and "good.lbry.nc" in msg, (rc, err, msg)
    h.download()
    assert int(c.iint) == 20
    h.close()
    g.close()


# ---- 7: the fp32 builds -----------------------------------------------------------------------------------------------------------------------
def f32_record_equals_fp64(lib64, lib32, tmp, size=(20, 17, 6)):
    """records are doubles in every build and nothing is rounded: after lateral_bc's first call the b and f lines of every ON side hold the
    fp64 library's, which are the expectation's; OFF sides equal the round32 expectation (tclim, sclim are kept in fp32 there)"""
    a, _, _ = ffc.start("archipelago", ffc.BASE, 1, size=size)
    for mask, onz in ((ALL, False), (ALL, True), (LS.SOUTH | LS.WEST, False), (LS.EAST | LS.NORTH, True)):
        raw = LS.raw_lbry_z(a, 2) if onz else LS.raw_lbry(a, 2)
        records = LS.lateral_records_z if onz else LS.lateral_records
        want, want32 = records(a, raw, mask), records(a, raw, mask, round32=True)
        p = (LS.write_lbry_z if onz else LS.write_lbry)(tmp / f"f32_{mask}_{int(onz)}.lbry.nc", raw, mask)
        got = []
        for lib in (lib64, lib32):
            b = a.copy()
            g = PomGpu(b, libpath=lib)
            g.set_z_inputs(lbry=onz)
            set_sides(g, mask)
            g.set_forcing_files(lbry=p)
            g.set_con(iint=1)
            g.call("lateral_bc")
            g.download()
            g.close()
            got.append(b)
        rounded = False
        for side in LS.SIDES:
            for var in ("temp", "salt", "u", "v"):
                at = LS.place(side, var)
                for rec, sfx in ((0, "b"), (1, "f"))[0 if var in ("temp", "salt") else 1:]:
                    name = LS.ORDER16[at] + sfx
                    assert same_bits(got[0].field(name), want[rec][at]), (mask, onz, name)
                    assert same_bits(got[1].field(name), (want if LS.on(mask, side) else want32)[rec][at]), (mask, onz, name)
                if LS.on(mask, side) and var in ("temp", "salt") and onz:   # a mapped line is no float32 number: a rounding would show
                    assert not same_bits(want[0][at], want[0][at].astype(np.float32).astype(np.float64))
                if not LS.on(mask, side) and var in ("temp", "salt"):
                    rounded = rounded or not same_bits(want[0][at], want32[0][at])
        assert rounded or mask == ALL, "an OFF side's line that the fp32 builds round"
