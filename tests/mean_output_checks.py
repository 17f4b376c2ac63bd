"""TEST HELPER: the time-mean output (pomgpu_set_mean_output ... pomgpu_write_output_mean; no counterpart in the reference).

Shared by tests/test_mean_output_emulated.py (host build of the kernel sources) and tests/test_gpu_mean_output.py (the device): every
check takes the library to load (None: the product library on device 0).  The expectation is a numpy RESTATEMENT kept here, not the
library's: a twin context of the same library runs the same case one step at a time and is downloaded after every step, `acc = acc + x`
is kept in step order from +0.0, and the mean is `acc / n` -- odd n (7, then 3), so that the division is inexact.  The state itself is
held to the oracle by the other suites; this one pins the accumulation and the point of the step at which it happens.  Every comparison
is on 64-bit patterns."""
import ctypes
import os
import threading

import numpy as np

from extpom_amd import decomp
from extpom_amd.cases import finish_initial, make_case
from extpom_amd.layout import BLK2D, BLK3D, P2, P3
from extpom_amd.model import PomGpu
from extpom_amd.lib import PomGpuError
from oracle.pyoracle import oracle_finish_initial

FIELDS = PomGpu.MEAN_FIELDS
ISPLIT = 9                                                    # odd: the external mode's result ends in the other generation of its arrays
SIZES = [(65, 49, 21), (20, 17, 6), (9, 8, 5)]                # 65x49x21: n3 = 66885 is odd -- every other array 8-byte aligned only, an odd tail
# both cases at every size; run(7) as one call and seven pomgpu_advance calls, each on both cases and at every size
MATRIX = [(case, size, ("run", "advance")[(c + s) % 2]) for c, case in enumerate(("archipelago", "seamount")) for s, size in enumerate(SIZES)]


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def diff(a, b):
    """every array of blk2d and blk3d and bdry, the library's scratch arrays included: two contexts of one library making the same calls"""
    out = [n for n in BLK2D + BLK3D if not same_bits(a.field(n), b.field(n))]
    if not same_bits(a.bdry, b.bdry):
        out.append("bdry")
    return out


def start(case, size, **nml):
    a = make_case(case, *size, **dict(dict(dte=6.0, isplit=ISPLIT), **nml))
    oracle_finish_initial(a)
    return a


class Restatement:
    """acc = acc + x per step from +0.0, x downloaded from a twin context that runs one step at a time; mean() = acc / n"""

    def __init__(self, st, lib, prepare=None):
        self.st = st
        self.g = PomGpu(st, libpath=lib)
        if prepare:
            prepare(self.g)
        self.reset()

    def reset(self):
        self.acc = {n: np.zeros_like(self.st.field(n)) for n in FIELDS}
        self.n = 0

    def add(self):
        for n in FIELDS:
            self.acc[n] = self.acc[n] + self.st.field(n)
        self.n += 1

    def step(self, count=1, accumulate=True):
        for _ in range(count):
            self.g.run(1)
            self.g.download()
            if accumulate:
                self.add()

    def mean(self, name):
        return self.acc[name] / float(self.n)


def owned(st, x):
    return x[..., :st.jm, :st.im]


def wrong_fields(g, want):
    """names whose mean differs from the restatement somewhere on (im, jm)"""
    return [n for n in FIELDS if not same_bits(owned(g.st, g.mean(n)), owned(g.st, want.mean(n)))]


def advance_steps(g, count):
    """`count` calls of pomgpu_advance, the host keeping iint as pom.f:17-19 does"""
    for _ in range(count):
        g.get_con()
        g.set_con(iint=int(g.st.iint) + 1)
        g.advance()


# ---- 1: every field equals the restatement, and the state is the state of the run with the mean off --------------------------------
def every_field(lib, case, size, how, tmp=None, forcing=False):
    prepare = None
    if forcing:                                               # the file forcing of tests/forcing_files_checks.py: steps 1 and 10 fetch records
        import forcing_files_checks as ff
        a, raw_s, raw_l = ff.start(case, ff.BASE, 10, size=size)
        sfrc, lbry = ff.files(tmp, raw_s, raw_l)
        prepare = lambda g: g.set_forcing_files(sfrc=sfrc, lbry=lbry)
    else:
        a = start(case, size)
    b, o = a.copy(), a.copy()
    want = Restatement(a, lib, prepare)
    g, h = PomGpu(b, libpath=lib), PomGpu(o, libpath=lib)     # the mean on / the same calls with the mean off
    if prepare:
        prepare(g), prepare(h)
    g.set_mean_output(True)
    assert g.mean_count() == 0 and h.mean_count() == -1
    for n in (7, 3):                                          # the second interval through the switch: it zeroes sums and count
        for c in (g, h):
            c.run(n) if how == "run" else advance_steps(c, n)
        want.step(n)
        assert g.mean_count() == n
        bad = wrong_fields(g, want)
        assert not bad, (case, size, how, n, bad)
        assert g.mean_count() == n                            # reading a mean resets nothing
        g.set_mean_output(True)
        want.reset()
    assert any(np.any(want.st.field(n) != 0.) for n in ("u", "w", "elb"))
    g.download(), h.download()
    assert not diff(b, o), diff(b, o)
    for c in (g, h, want.g):
        c.close()


# ---- 2: the mean file ----------------------------------------------------------------------------------------------------------------
def file_parts(path):
    """(header bytes, {variable: values}) of an output file: its variables lie back to back behind the header, all doubles"""
    from scipy.io import netcdf_file
    with netcdf_file(str(path), "r", mmap=False) as f:
        var = {k: np.array(v.data, dtype=np.float64) for k, v in f.variables.items()}
    raw = open(path, "rb").read()
    return raw[:len(raw) - 8 * sum(v.size for v in var.values())], var


def mean_file(lib, tmp, chained, case="archipelago", size=(20, 17, 6)):
    a = start(case, size)
    b = a.copy()
    want = Restatement(a, lib)
    g = PomGpu(b, libpath=lib)
    g.set_mean_output(True)
    kw = dict(title=case, time_start="2000-01-01 00:00:00 +00:00")
    g.run(7)
    want.step(7)
    for n, tag in ((7, "a"), (3, "b")):
        means = {k: g.mean(k) for k in FIELDS}
        assert not wrong_fields(g, want)
        snap, mean = tmp / f"snap_{tag}.nc", tmp / f"mean_{tag}.nc"
        g.write_file("output", snap, **kw)
        assert g.mean_count() == n                            # the snapshot file leaves the sums alone
        g.write_file("output_mean", mean, **kw)
        assert g.mean_count() == 0
        if tag == "a":
            if not chained:
                g.io_wait()
            g.run(3)                                          # chained: enqueued while the writer's thread still copies the snapshot
            want.reset()
            want.step(3)
        g.io_wait()
        hs, vs = file_parts(snap)
        hm, vm = file_parts(mean)
        assert hs == hm and len(hs) > 1000
        assert list(vs) == list(vm)
        for k in vs:
            if k in FIELDS:
                nlev = vm[k].shape[1] if vm[k].ndim == 4 else None     # (time, levels, y, x): kbm1 levels of u v t s rho, kb of w
                m = means[k] if nlev is None else means[k][:nlev]
                assert same_bits(vm[k].reshape(owned(b, m).shape), owned(b, m)), (tag, k)
            else:
                assert same_bits(vs[k], vm[k]), (tag, k)
        assert not same_bits(vs["u"], vm["u"]) and not same_bits(vs["elb"], vm["elb"])
    assert g.mean_count() == 0
    g.close()
    want.g.close()


# ---- 3: laziness is kept -------------------------------------------------------------------------------------------------------------
def launch_counts(lib, size=(65, 49, 21)):
    b = start("seamount", size)
    g = PomGpu(b, libpath=lib)
    g.run(2)
    g.prof_begin()
    g.run(5)
    off = {k: n for k, (n, _) in g.prof_end().items()}
    g.set_mean_output(True)
    g.prof_begin()
    g.run(5)
    on = {k: n for k, (n, _) in g.prof_end().items()}
    assert "k_mean_accum" not in off and on.pop("k_mean_accum") == 5, (off, on)
    assert on == off, {k: (off.get(k), on.get(k)) for k in set(on) | set(off) if off.get(k) != on.get(k)}
    assert off["k_profq"] == 5 and not any(k.startswith(("k_realvertvl", "k_restore_fields")) for k in off), off   # five full steps, nothing lazy formed
    g.close()


# ---- 4: the switch on a live context ---------------------------------------------------------------------------------------------------
def switching(lib, size=(20, 17, 6)):
    a = start("archipelago", size)
    b = a.copy()
    want = Restatement(a, lib)
    g = PomGpu(b, libpath=lib)
    g.run(2)
    want.step(2, accumulate=False)                            # steps before the switch do not count
    g.set_mean_output(True)
    assert g.mean_count() == 0
    g.run(3)
    want.step(3)
    assert g.mean_count() == 3 and not wrong_fields(g, want)
    g.set_mean_output(True)                                   # again: sums and count from zero
    want.reset()
    assert g.mean_count() == 0
    g.run(1)
    want.step(1)
    assert g.mean_count() == 1 and not wrong_fields(g, want)
    g.set_mean_output(False)
    assert g.mean_count() == -1
    try:
        g.mean("u")
        raise AssertionError("mean() with the mean off was served")
    except PomGpuError:
        pass
    g.run(1)                                                  # and the step goes on without it
    want.step(1, accumulate=False)
    g.download()
    assert not [n for n in FIELDS if not same_bits(b.field(n), a.field(n))]
    g.close()
    want.g.close()


# ---- 5: refusals leave state and count as they were ------------------------------------------------------------------------------------
def refusals(lib, tmp, size=(9, 8, 5)):
    a = start("seamount", size)
    g = PomGpu(a, libpath=lib)
    g.run(2)
    before = g.download().copy()

    def unchanged(count):
        assert g.mean_count() == count
        now = a.copy()
        g.download(now)
        assert not diff(before, now), diff(before, now)

    m = ctypes.c_void_p()
    assert g.L.pomgpu_mean_accumulate(g.h) == -1 and b"off" in g.L.pomgpu_last_error(g.h)      # the mean off
    unchanged(-1)
    g.set_mean_output(True)
    try:                                                      # a write at count 0: no file is touched
        g.write_file("output_mean", tmp / "none.nc")
        raise AssertionError("a mean file of no steps was written")
    except PomGpuError as e:
        assert "no step" in str(e)
    assert not os.path.exists(tmp / "none.nc")
    unchanged(0)
    g.run(1)
    before = g.download().copy()
    means = {k: g.mean(k) for k in FIELDS}
    for name in ("wr", "ub", "el"):                           # names outside the nine fields
        try:
            g.mean(name)
            raise AssertionError(name)
        except PomGpuError:
            pass
    buf = np.empty_like(a.field("wr"))
    assert g.L.pomgpu_mean_download(g.h, 1, P3["wr"], g._p(buf)) == -1
    assert g.L.pomgpu_mean_download(g.h, 0, P2["el"], g._p(buf)) == -1
    assert g.L.pomgpu_mean_download(g.h, 0, P3["u"], g._p(buf)) == -1      # u's slot number read as a blk2d slot
    unchanged(1)
    try:                                                      # its trial steps are real steps
        g.tune_placement(steps=1, max_try=1)
        raise AssertionError("tune_placement with the mean on")
    except PomGpuError as e:
        assert "tune first" in str(e)
    unchanged(1)
    assert not [k for k in FIELDS if not same_bits(means[k], g.mean(k))]
    g.close()


def refused_in_fp32_storage(lib_f32, size=(9, 8, 5)):
    a = make_case("seamount", *size, dte=6.0, isplit=ISPLIT)
    g = PomGpu(a, libpath=lib_f32)
    try:
        g.set_mean_output(True)
        raise AssertionError("the fp32-storage build took the switch")
    except PomGpuError as e:
        assert "not in the fp32-storage variant (download and write from the host)" in str(e)
    assert g.mean_count() == -1
    g.run(2)
    g.close()


# ---- the entry point, for hosts that string the routines together --------------------------------------------------------------------
def step_by_routine(g, n, after_external=None, accumulate=True):
    g.set_con(iint=n)
    g.call("get_time")
    g.get_con()
    g.call("lateral_viscosity")
    g.call("mode_interaction")
    for iext in range(1, ISPLIT + 1):
        g.set_con(iext=iext)
        g.call("mode_external")
    if after_external:
        after_external()
    g.set_con(iext=ISPLIT + 1)
    g.call("mode_internal")
    if accumulate:
        g.mean_accumulate()
    g.check_velocity()


def entry_point(lib, size=(20, 17, 6)):
    """the Fortran host's sequence with pomgpu_mean_accumulate behind mode_internal; and once in the MIDDLE of a step, behind the last
    external substep, where the 2-D result still lives in the other generation of the external mode's arrays: x is what a download
    shows at that moment"""
    a = start("archipelago", size)
    b = a.copy()
    g, t = PomGpu(b, libpath=lib), PomGpu(a, libpath=lib)
    g.set_mean_output(True)
    acc = {n: np.zeros_like(a.field(n)) for n in FIELDS}

    def add():
        t.download()
        for n in FIELDS:
            acc[n] = acc[n] + a.field(n)

    for n in (1, 2, 3):
        step_by_routine(g, n)
        step_by_routine(t, n, accumulate=False)
        add()
    step_by_routine(g, 4, after_external=g.mean_accumulate)
    step_by_routine(t, 4, after_external=add, accumulate=False)
    add()
    assert g.mean_count() == 5
    bad = [n for n in FIELDS if not same_bits(owned(b, g.mean(n)), owned(b, acc[n] / 5.))]
    assert not bad, bad
    g.close()
    t.close()


def every_element(lib, size):
    """the kernel alone: three accumulations of uploaded random fields through the entry point, no step in between -- EVERY element of
    every accumulator, the first and the last one of each array included (cells a model state keeps at zero: corners, level kb)"""
    a = start("seamount", size)
    g = PomGpu(a, libpath=lib)
    g.set_mean_output(True)
    rng = np.random.default_rng(int(np.prod(size)))
    acc = {n: np.zeros_like(a.field(n)) for n in FIELDS}
    for _ in range(3):
        for n in FIELDS:
            x = rng.standard_normal(a.field(n).shape) * 10.0 ** rng.integers(-3, 4)
            up, slot = (g.L.pomgpu_upload_3d, P3[n]) if n in P3 else (g.L.pomgpu_upload_2d, P2[n])
            g._chk(up(g.h, slot, g._p(x)), "upload")
            acc[n] = acc[n] + x
        g.mean_accumulate()
    assert g.mean_count() == 3
    bad = [n for n in FIELDS if not same_bits(g.mean(n), acc[n] / 3.)]
    assert not bad, bad
    g.close()


# ---- 6: tiles ------------------------------------------------------------------------------------------------------------------------
TILE_GRID, TILE_KB, TILE_ISPLIT, TILE_STEPS = (67, 59), 11, 7, 3


def run_tiles(lib, case, mean):
    """2x2 tiles under the library's exchange and the wide-halo external mode, one host thread each; {rank: (tile, means, state, rounds)}"""
    from forcing_files_checks import Board, device_mover, host_mover
    mover = host_mover if lib is not None else device_mover
    IMg, JMg = TILE_GRID
    iml, jml = decomp.local_size(IMg, JMg, 2, 2)
    tiles = [decomp.make_tile(r, IMg, JMg, iml, jml, n_proc=4) for r in range(4)]
    board, out, errs = Board(4), {}, []

    def rank(r):
        try:
            tile = tiles[r]
            st = make_case(case, IMg, JMg, TILE_KB, tile=tile, dte=6.0, isplit=TILE_ISPLIT)
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
            if mean:
                g.set_mean_output(True)
            g.run(TILE_STEPS)
            rounds = (g.exchange_rounds() - r0, g.exchange_rounds_side() - s0)
            means = {k: g.mean(k) for k in FIELDS} if mean else None
            assert not mean or g.mean_count() == TILE_STEPS
            g.download()
            assert int(st.error_status) == 0 and rounds[1] > 0
            g.close()
            out[r] = (tile, means, st, rounds)
        except Exception:                                     # a dead rank must not leave the others at the barrier
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


def tiles(lib, case="archipelago"):
    IMg, JMg = TILE_GRID
    one = make_case(case, IMg, JMg, TILE_KB, dte=6.0, isplit=TILE_ISPLIT)
    oracle_finish_initial(one)
    g = PomGpu(one, libpath=lib)
    g.set_mean_output(True)
    g.run(TILE_STEPS)
    single = {k: g.mean(k) for k in FIELDS}
    g.close()
    on, off = run_tiles(lib, case, True), run_tiles(lib, case, False)
    bad = []
    for r, (tile, means, st, rounds) in on.items():
        io, jo, im, jm = tile.i_off, tile.j_off, tile.im, tile.jm
        sl_j = slice(0 if jo == 0 else 1, jm if jo + jm == JMg else jm - 1)       # the cells the tile owns
        sl_i = slice(0 if io == 0 else 1, im if io + im == IMg else im - 1)
        for k in FIELDS:
            ref = single[k][..., jo:jo + jm, io:io + im][..., sl_j, sl_i]
            if not same_bits(ref, means[k][..., :jm, :im][..., sl_j, sl_i]):
                bad.append((r, k))
        assert rounds == off[r][3], (r, rounds, off[r][3])    # the accumulation adds no message round on either stream
        assert not diff(st, off[r][2]), (r, diff(st, off[r][2]))
    assert not bad, bad
    assert np.any(single["w"] != 0.) and np.any(single["uab"] != 0.)
