"""TEST HELPER: forcing records read on the device from the files pomgpu_set_forcing_files names (wind, heat, surface, lateral_bc,
restore_interior without PnetCDF).

Shared by tests/test_forcing_files_emulated.py (host build of the kernel sources) and tests/test_gpu_forcing_files.py (the device):
every check takes the library to load (None: the product library on device 0).  The files are written at run time with
scipy.io.netcdf_file from seeded fields (tests/forcing_expect.py), the expected records are that helper's numpy restatement of the
reference's readers, and the bar is the CPU oracle fed those records -- bit for bit on 64-bit patterns, every array of blk2d and
blk3d but the library's four scratch arrays (as in every other suite), bdry and blkcon."""
import ctypes
import os

import numpy as np

import forcing_expect as fx
from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D, P2
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial

SCRATCH = {"tps", "fluxua", "fluxva", "zflux"}
SIZE = (65, 49, 21)
# dti = 360 s: wind / heat / surface change record every 30 steps, lateral_bc every 10
BASE = dict(dte=6.0, isplit=60)
# name -> (keywords of make_case, steps of the ONE run call).  62 steps at dti = 360 s: wind, heat and surface change record at steps 30
# and 60 (cont_bry = 7: at 23 and 53), lateral_bc consumes 8 records (cont_bry: 9).  dte4_isplit24 (tests/off_default.py) has dti = 96 s,
# iwind = 112 and ibc = 37: 226 steps, the surface records change at 112 and 224, lateral_bc consumes 8 records.
VARIANTS = {
    "base": (dict(BASE), 62),
    "cont_bry": (dict(BASE, cont_bry=7), 62),
    "dte4_isplit24": (dict(dte=4.0, isplit=24), 226),
    "rhoref": (dict(BASE, rhoref=1027.0), 62),
}
# THE HOST BUILD IS SLOW (a step of one context a quarter of a second), so tests/test_forcing_files_emulated.py deviates from the device
# run, which does everything on both cases: (a) the second context fed by the setters runs on ONE case per variant (HOST_SETTERS; the
# oracle, the stricter bar, on both); (b) dte4_isplit24 runs its 226 steps on archipelago only -- on seamount 115 steps, ONE change of the
# surface records and 5 lateral records (HOST_STEPS).
HOST_SETTERS = {"base": "archipelago", "cont_bry": "seamount", "dte4_isplit24": "seamount", "rhoref": "archipelago"}
HOST_STEPS = {("seamount", "dte4_isplit24"): 115}


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def diff(a, b, skip=SCRATCH):
    out = [n for n in BLK2D + BLK3D if n not in skip and not same_bits(a.field(n), b.field(n))]
    if not same_bits(a.bdry, b.bdry):
        out.append("bdry")
    if a.con.tobytes() != b.con.tobytes():
        out.append("blkcon: " + ", ".join(n for n in a.con.dtype.names if a.con[n].tobytes() != b.con[n].tobytes()))
    return out


def schedule(st, steps):
    """(surface records, lateral records) the reference's schedule asks for in steps 1..steps (bounds_forcing.f:884-902, :612, :734)"""
    cb, iend = int(st.cont_bry), int(st.iend)
    istep = int(.125 * 86400. / float(st.dti))
    ibc = int(float(np.float32(1.) / np.float32(24.)) * 86400. / float(st.dti))
    top = lambda per: max([(1 + cb) // per + 1] + [(n + cb + per) // per + 1 for n in range(1, steps + 1) if (n == 1 or (n + cb) % per == 0) and n != iend])
    return top(istep), top(ibc), istep, ibc


def start(case, nml, steps, size=SIZE, round32=False, extra_s=0, extra_l=0):
    """(the oracle's state carrying the expected records, raw sfrc fields, raw lbry fields)"""
    a = make_case(case, *size, **nml)
    oracle_finish_initial(a)
    ns, nl, _, _ = schedule(a, steps)
    raw_s, raw_l = fx.raw_sfrc(a, ns + extra_s), fx.raw_lbry(a, nl + extra_l)
    a.forcing_records = fx.forcing_records(a, raw_s)
    a.lateral_records = fx.lateral_records(a, raw_l, round32=round32)
    return a, raw_s, raw_l


def files(tmp, raw_s, raw_l, tag="", **kw):
    return fx.write_sfrc(tmp / f"case{tag}.sfrc.nc", raw_s, **kw), fx.write_lbry(tmp / f"case{tag}.lbry.nc", raw_l, **kw)


def step_with_setters(g, steps):
    """the host path: before every step the records its schedule may ask for (this one and the next), then run(1)"""
    st = g.st
    cb = int(st.cont_bry)
    _, _, istep, ibc = schedule(st, 1)
    first = int(st.iint)
    for n in range(first + 1, first + steps + 1):
        g.set_forcing_records(first=(n + cb) // istep + 1, count=2)
        g.set_lateral_records(first=(n + cb) // ibc + 1, count=2)
        g.run(1)


def status(g):
    """(error_status, last_error) without raising"""
    g.L.pomgpu_get_con(g.h, g._p(g.st.con))
    return int(g.st.error_status), g.L.pomgpu_last_error(g.h).decode()


# ---- 1: file path = setter path = oracle -------------------------------------------------------------------------------------------
def file_setters_oracle(lib, tmp, case, variant):
    nml, steps = VARIANTS[variant]
    with_setters = True
    if lib is not None:                                       # the host build: see HOST_SETTERS, HOST_STEPS
        steps = HOST_STEPS.get((case, variant), steps)
        with_setters = HOST_SETTERS[variant] == case
    a, raw_s, raw_l = start(case, nml, steps)
    assert len(a.lateral_records) > 4 and len(a.forcing_records["wind"]) >= 3
    b, s = a.copy(), a.copy()
    sfrc, lbry = files(tmp, raw_s, raw_l)
    g = PomGpu(b, libpath=lib)
    g.set_forcing_files(sfrc=sfrc, lbry=lbry)
    g.run(steps)                                              # ONE call across every record change
    OracleTile(a).run(steps)
    g.download()
    assert int(a.error_status) == 0 and not diff(a, b), diff(a, b)
    g.close()
    if with_setters:
        h = PomGpu(s, libpath=lib)
        step_with_setters(h, steps)
        h.download()
        assert not diff(b, s, skip=()), diff(b, s, skip=())   # two contexts of one library: the scratch arrays too
        h.close()
    if variant == "rhoref":                                   # the heat conversion did move
        d = make_case(case, *SIZE, **BASE)
        assert not same_bits(fx.heat_record(d, raw_s["shflux"][0], raw_s["swrad"][0])[0], a.forcing_records["heat"][0][0])


# ---- 2: the taper alone ------------------------------------------------------------------------------------------------------------
def taper_alone(lib, tmp, size):
    a = make_case("archipelago", *size, **BASE)
    oracle_finish_initial(a)
    raw_s = fx.raw_sfrc(a, 2)
    want = fx.forcing_records(a, raw_s)["wind"]
    assert np.count_nonzero(a.dum[:a.jm, :a.im] == 0.) > 0 and np.count_nonzero(a.dum[:a.jm, :a.im]) > 0   # land touches the taper
    g = PomGpu(a.copy(), libpath=lib)
    g.set_forcing_files(sfrc=fx.write_sfrc(tmp / "t.sfrc.nc", raw_s))
    g.set_con(iint=1)
    g.call("get_time")
    g.call("wind")                                            # iint = 1: record 1, the shift to wusurfb / wvsurfb, record 2
    A = (slice(0, a.jm), slice(0, a.im))
    for name, rec, f in (("wusurfb", 0, 0), ("wvsurfb", 0, 1), ("wusurff", 1, 0), ("wvsurff", 1, 1)):
        got = np.empty_like(a.field(name))
        g._chk(g.L.pomgpu_download_2d(g.h, P2[name], g._p(got)), "download_2d")
        bad = np.argwhere(got[A].view(np.uint64) != want[rec][f].view(np.uint64))
        assert bad.size == 0, f"{name}: {len(bad)} cells differ, first (j,i) = {bad[:5].tolist()}"
        assert same_bits(got[a.jm:], a.field(name)[a.jm:]) and same_bits(got[:, a.im:], a.field(name)[:, a.im:])   # beyond (im,jm): untouched
    # row jm is not row 1 tapered once: the statement order matters for these fields
    raw1 = -fx.window(a, raw_s["sustr"][0]) / 1025.
    assert not same_bits(want[0][0][a.jm - 1, 1:a.im - 1],
                         raw1[0, 1:a.im - 1] / 3.0 * (a.dum[a.jm - 2, 1:a.im - 1] + a.dum[a.jm - 1, 0:a.im - 2] + a.dum[a.jm - 1, 2:a.im]))
    g.close()


# ---- 3: file layouts ---------------------------------------------------------------------------------------------------------------
LAYOUTS = {
    "cdf2_double_unlimited": dict(),
    "cdf1_float_unlimited": dict(version=1, dtype="f"),
    "cdf2_float_fixed": dict(dtype="f", unlimited=False),
    "cdf1_double_fixed": dict(version=1, unlimited=False),
    "cdf2_double_unlimited_odd": dict(odd=True),
    "cdf1_float_unlimited_odd": dict(version=1, dtype="f", odd=True),
    "cdf2_mixed_types": dict(types={"sustr": "f", "swrad": "f", "SST": "f", "zeta.east": "f", "u.south": "f", "temp.east": "f", "Sclim": "f"}),
}


def layouts(lib, tmp, steps=11):
    """every layout leaves the state the first one leaves, and that is the oracle's; clim registered too (12 and 14 months): step 2
    fetches the restore records 1 and 2 = months 11 and 12"""
    a, raw_s, raw_l = start("seamount", BASE, steps, extra_s=1, extra_l=1)
    raw_c = fx.raw_clim(a, 14)
    raw_c12 = {k: v[:12] for k, v in raw_c.items()}
    a.restore_records = fx.restore_records(a, raw_c, 2)
    init = a.copy()
    OracleTile(a).run(steps)
    for n, (name, kw) in enumerate(LAYOUTS.items()):
        b = init.copy()
        sfrc, lbry = files(tmp, raw_s, raw_l, tag=str(n), **kw)
        clim = fx.write_clim(tmp / f"case{n}.clim.nc", raw_c if n % 2 else raw_c12, **kw)
        g = PomGpu(b, libpath=lib)
        g.set_forcing_files(sfrc=sfrc, lbry=lbry, clim=clim)
        g.run(steps)
        g.download()
        assert not diff(a, b), (name, diff(a, b))
        g.close()


def restore_across_a_record_change(lib, tmp):
    """restore_interior alone under a dti that makes 30 days three steps: iint = 2 loads records 1 and 2 (months 11, 12), iint = 3 shifts
    and loads record 3 (month 1, the wrap of mod(n+9,12)+1), iint = 4, 5 interpolate, iint = 6 loads record 4"""
    a = make_case("archipelago", *SIZE, **BASE)
    oracle_finish_initial(a)
    raw_c = fx.raw_clim(a, 12)
    a.restore_records = fx.restore_records(a, raw_c, 4)
    a.dti = 864000.
    b = a.copy()
    ot = OracleTile(a)
    g = PomGpu(b, libpath=lib)
    g.set_forcing_files(clim=fx.write_clim(tmp / "r.clim.nc", raw_c, dtype="f"))
    for n in range(2, 7):
        a.iint = n
        a.time = float(a.dti) * n / 86400.
        g.set_con(iint=n, time=float(a.time))
        ot.call("restore_interior")
        g.call("restore_interior")
        g.download()
        assert not diff(a, b), (n, diff(a, b))
    assert not same_bits(a.trstrb, a.trstrf)
    g.close()


# ---- 4: iint == iend ---------------------------------------------------------------------------------------------------------------
def exact_records_to_iend(lib, tmp):
    iend = 30
    nml = dict(BASE, days=iend * 360. / 86400.)
    a, raw_s, raw_l = start("seamount", nml, iend)
    assert int(a.iend) == iend and len(a.forcing_records["wind"]) == 2 and len(a.lateral_records) == 4   # step 30 shifts and reads nothing
    init = a.copy()
    b = init.copy()
    sfrc, lbry = files(tmp, raw_s, raw_l)
    g = PomGpu(b, libpath=lib)
    g.set_forcing_files(sfrc=sfrc, lbry=lbry)
    g.run(iend)
    ot = OracleTile(a)
    ot.run(19)
    at19 = a.copy()
    ot.run(iend - 19)
    g.download()
    assert int(b.error_status) == 0 and not diff(a, b), diff(a, b)
    g.close()
    # one record fewer: step 20 asks lateral_bc for record 4
    c = init.copy()
    g = PomGpu(c, libpath=lib)
    g.set_forcing_files(sfrc=sfrc, lbry=fx.write_lbry(tmp / "short.lbry.nc", raw_l, nrec=3))
    rc = g.L.pomgpu_run(g.h, iend)
    err, msg = status(g)
    assert rc != 0 and err == 1 and "record 4" in msg and "lateral_bc" in msg, (rc, err, msg)
    g.download()
    assert int(c.iint) == 20
    # what step 19 left is intact but for what step 20 wrote before lateral_bc asked: get_time (blkcon), the surface fields' interpolation
    # and the shift of the lateral "b" copies (bdry)
    moved = set(diff(at19, c))
    assert all(m in ("wusurf", "wvsurf", "wtsurf", "swrad", "bdry") or m.startswith("blkcon") for m in moved), moved
    g.close()


# ---- 5: refusals at registration ---------------------------------------------------------------------------------------------------
def refusals(lib, tmp):
    a, raw_s, raw_l = start("seamount", BASE, 11)
    raw_c = fx.raw_clim(a, 12)
    b = a.copy()
    g = PomGpu(b, libpath=lib)
    g.run(2)
    g.download()
    before = b.copy()
    good_s, good_l = files(tmp, raw_s, raw_l, tag="good")

    def refused(cause, im_global=None, **paths):
        m = __import__("extpom_amd.lib", fromlist=["FileMeta"]).FileMeta(b"", b"", im_global or b.im, b.jm, 1, 1, 0, None)
        enc = lambda p: None if p is None else str(p).encode()
        g.set_con(error_status=0)
        rc = g.L.pomgpu_set_forcing_files(g.h, enc(paths.get("sfrc")), enc(paths.get("lbry")), enc(paths.get("clim")), ctypes.byref(m))
        err, msg = status(g)
        assert rc == -1 and err == 1 and cause in msg, (cause, rc, err, msg)
        now = b.copy()
        g.download(now)
        now.error_status = 0
        before.error_status = 0
        assert not diff(before, now, skip=()), (cause, diff(before, now, skip=()))

    for names, kind, raw, write in ((fx.SFRC, "sfrc", raw_s, fx.write_sfrc), (fx.LBRY, "lbry", raw_l, fx.write_lbry), (fx.CLIM, "clim", raw_c, fx.write_clim)):
        for name in names:                                    # every name the reference's readers look up is looked up here, by that name
            refused(f"variable {name} is absent", **{kind: write(tmp / "a.nc", raw, drop=(name,))})
    refused("variable swrad has NetCDF type 3", sfrc=fx.write_sfrc(tmp / "b.nc", {k: np.round(v) for k, v in raw_s.items()}, types={"swrad": "h"}))
    refused("variable SST has the dimension lengths", sfrc=fx.write_sfrc(tmp / "c.nc", raw_s, transpose=("SST",)))
    refused("variable u.east has the dimension lengths", lbry=fx.write_lbry(tmp / "d.nc", raw_l, kb_off=1))
    refused("variable Tclim has the dimension lengths", clim=fx.write_clim(tmp / "d2.nc", {k: v[:11] for k, v in raw_c.items()}, unlimited=False))
    raw = bytearray(open(good_s, "rb").read())
    raw[3] = 5
    open(tmp / "e.nc", "wb").write(raw)
    refused("CDF version 5", sfrc=tmp / "e.nc")
    raw = open(good_l, "rb").read()
    open(tmp / "f.nc", "wb").write(raw[:len(raw) * 3 // 5])
    refused("truncated", lbry=tmp / "f.nc")
    open(tmp / "g.nc", "wb").write(raw[:40])
    refused("ends inside its header", lbry=tmp / "g.nc")
    refused("does not fit the global grid", im_global=b.im - 1, sfrc=good_s)
    refused("cannot open", sfrc=tmp / "nowhere.nc")
    # nothing was registered by any of them: the step still runs on constant forcing, and the setters still work
    g.set_con(error_status=0)
    g.set_forcing_records(first=1, count=1)
    # a setter on a source that has a file
    h = PomGpu(a.copy(), libpath=lib)
    h.set_forcing_files(sfrc=good_s, lbry=good_l, clim=fx.write_clim(tmp / "good.clim.nc", raw_c))
    x = np.zeros((a.jm, a.im))
    x3 = np.zeros((a.kb, a.jm, a.im))
    ptrs = (ctypes.c_void_p * 20)(*[r.ctypes.data for r in a.lateral_records[0]])
    for setter in (lambda: h.L.pomgpu_set_forcing_record(h.h, 0, 1, h._p(x), h._p(x)), lambda: h.L.pomgpu_set_lateral_record(h.h, 1, ptrs),
                   lambda: h.L.pomgpu_set_restore_record(h.h, 1, h._p(x3), h._p(x3))):
        rc = setter()
        err, msg = status(h)
        assert rc == -1 and err == 1 and "come from a file" in msg, (rc, err, msg)
        h.set_con(error_status=0)
    g.close()
    h.close()


# ---- 7: the fp32 study builds: file path = setter path -----------------------------------------------------------------------------
def file_equals_setters_f32(lib, tmp, steps=11):
    """no oracle for these builds: two contexts of one library.  The west / north lines come from the tclim, sclim mirrors, which these
    builds keep in fp32 (round32); the restore records are doubles on both paths and rounded by the same load kernel."""
    a, raw_s, raw_l = start("archipelago", BASE, steps, round32=True)
    raw_c = fx.raw_clim(a, 12)
    a.restore_records = fx.restore_records(a, raw_c, 2)
    b, s = a.copy(), a.copy()
    sfrc, lbry = files(tmp, raw_s, raw_l, dtype="f")
    g = PomGpu(b, libpath=lib)
    g.set_forcing_files(sfrc=sfrc, lbry=lbry, clim=fx.write_clim(tmp / "case.clim.nc", raw_c))
    g.run(steps)
    g.download()
    h = PomGpu(s, libpath=lib)
    step_with_setters(h, steps)
    h.download()
    assert not diff(b, s, skip=()), diff(b, s, skip=())
    assert np.any(b.tbw != a.tbw) and np.any(b.wusurf != a.wusurf) and np.any(b.trstr != a.trstr)
    g.close()
    h.close()


# ---- 6: tiles ----------------------------------------------------------------------------------------------------------------------
TILE_GRID, TILE_KB, TILE_ISPLIT, TILE_STEPS = (97, 59), 11, 20, 32     # 2x2 tiles of 50x31, the east / north ones trimmed to 49 / 30; dti = 120 s:
                                                                       # lateral_bc changes record at step 30; w = 24 <= 30 - 3


class Board:
    """what the ranks of one run share: a mailbox per (sender, receiver, direction) and a barrier"""

    def __init__(self, world):
        import threading
        self.box = {}
        self.barrier = threading.Barrier(world)

    def allmin(self, me, value):
        self.box[("min", me)] = int(value)
        self.barrier.wait()
        m = min(v for k, v in self.box.items() if k[0] == "min")
        self.barrier.wait()
        return m


OPP8 = (1, 0, 3, 2, 7, 6, 5, 4)


def host_mover(board, tile, g):
    """host build: the staging buffers are host memory; the library has completed the round's stream before the call"""
    nb = PomGpu.neighbours8(tile)
    buf = lambda p, n: np.ctypeslib.as_array((ctypes.c_double * n).from_address(p))

    def move(send, scount, recv, rcount):
        for d in range(8):
            if nb[d] >= 0 and scount[d]:
                board.box[(tile.rank, nb[d], d)] = buf(send[d], scount[d]).copy()
        board.barrier.wait()
        for d in range(8):
            if nb[d] >= 0 and rcount[d]:
                buf(recv[d], rcount[d])[:] = board.box[(nb[d], tile.rank, OPP8[d])]
        board.barrier.wait()
    return move, False


def device_mover(board, tile, g):
    """the device: the asynchronous, event-ordered mover of tests/gpu_tiles_threads.py -- copies enqueued on the stream of the round"""
    import torch
    from extpom_amd.halo import _DevPtr
    dev = torch.device("cuda", 0)
    nb, r = PomGpu.neighbours8(tile), tile.rank
    w = lambda p, n: torch.as_tensor(_DevPtr(p, (n,)), device=dev)

    def move(send, scount, recv, rcount):
        cs = torch.cuda.ExternalStream(g.current_stream())
        packed = torch.cuda.Event()
        packed.record(cs)
        for d in range(8):
            if nb[d] >= 0 and scount[d]:
                board.box[(r, nb[d], d)] = (send[d], scount[d], packed)
        board.barrier.wait()
        with torch.cuda.stream(cs):
            for d in range(8):
                if nb[d] >= 0 and rcount[d]:
                    p, n, ev = board.box[(nb[d], r, OPP8[d])]
                    assert n == rcount[d]
                    cs.wait_event(ev)
                    w(recv[d], n).copy_(w(p, n), non_blocking=True)
        taken = torch.cuda.Event()
        taken.record(cs)
        board.box[("taken", r)] = taken
        board.barrier.wait()
        for d in range(8):
            if nb[d] >= 0 and scount[d]:
                cs.wait_event(board.box[("taken", nb[d])])
        board.barrier.wait()
    return move, True


def run_tiles(lib, tmp, mover, use_files, raw_s, raw_l):
    """2x2 tiles under the library exchange and the wide-halo external mode, one host thread each; {rank: state}"""
    import threading
    from extpom_amd import decomp
    from extpom_amd.cases import finish_initial
    IMg, JMg = TILE_GRID
    iml, jml = decomp.local_size(IMg, JMg, 2, 2)
    tiles = [decomp.make_tile(r, IMg, JMg, iml, jml, n_proc=4) for r in range(4)]
    assert {(t.im, t.jm) for t in tiles} == {(50, 31), (49, 31), (50, 30), (49, 30)}
    board, out, errs = Board(4), {}, []
    if use_files:
        sfrc, lbry = files(tmp, raw_s, raw_l, tag="tiles", dtype="f")

    def rank(r):
        try:
            tile = tiles[r]
            st = make_case("archipelago", IMg, JMg, TILE_KB, tile=tile, dte=6.0, isplit=TILE_ISPLIT)
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
            st.forcing_records = fx.forcing_records(st, raw_s)          # per tile: its own window, im, jm, dum, dvm
            st.lateral_records = fx.lateral_records(st, raw_l)
            g.upload(st)
            board.barrier.wait()
            if use_files:
                g.set_forcing_files(sfrc=sfrc, lbry=lbry, im_global=IMg, jm_global=JMg)
                g.run(TILE_STEPS)
            else:
                step_with_setters(g, TILE_STEPS)
            g.download()
            assert int(st.error_status) == 0 and g.exchange_rounds_side() > 0
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
    return out


def tiles_file_equals_setters(lib, tmp):
    mover = host_mover if lib is not None else device_mover
    g = make_case("archipelago", *TILE_GRID, TILE_KB, dte=6.0, isplit=TILE_ISPLIT)
    oracle_finish_initial(g)
    ns, nl, _, _ = schedule(g, TILE_STEPS)
    raw_s, raw_l = fx.raw_sfrc(g, ns), fx.raw_lbry(g, nl)
    by_file = run_tiles(lib, tmp, mover, True, raw_s, raw_l)
    by_setter = run_tiles(lib, tmp, mover, False, raw_s, raw_l)
    for r in range(4):
        assert not diff(by_file[r], by_setter[r], skip=()), (r, diff(by_file[r], by_setter[r], skip=()))
    assert np.any(by_file[1].wusurf != 0.) and np.any(by_file[0].tbw != 0.)
    # every tile tapered at ITS edge lines: the seam columns of the two western tiles' wind differ from the single tile's taper there
    one = fx.forcing_records(g, raw_s)["wind"][0][0]
    t0 = by_file[0]
    assert not same_bits(fx.forcing_records(t0, raw_s)["wind"][0][0][:, t0.im - 1], one[:t0.jm, t0.im - 1])
