"""The checks of pomgpu_ztosig_line (PomGpu.ztosig_line), each taking the library to load (None: the product library on device 0), so that
tests/test_ztosig_line_emulated.py (the host builds) and tests/test_gpu_ztosig_line.py (the device) cannot drift apart.  The bar is
tests/ztosig_line_expect.py's restatement, which tests/test_ztosig_line_vs_reference.py holds to the reference's compiled ztosig_ called as
the commented blocks of bounds_forcing.f:636-716 call it, and the digests of that routine's own output in tests/golden/ztosig_line.json:
64-bit patterns on every point."""
import json
import os

import numpy as np
import pytest

import ztosig_line_expect as ZL
from cold_start_expect import diff
from extpom_amd import decomp
from extpom_amd.cases import make_case
from extpom_amd.lib import PomGpuError
from extpom_amd.model import PomGpu
from oracle.pyoracle import oracle_finish_initial
from ztosig_checks import one_tile, state_of, status
from ztosig_line_expect import same_bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ztosig_line.json")
_golden = {}


def golden(im, jm, ks, kb, edge, salt):
    if not _golden:
        with open(GOLDEN) as fh:
            _golden.update(json.load(fh))
    return _golden[f"{im}x{jm}x{ks}x{kb}{ZL.EDGES[edge]}{'S' if salt else 'T'}"]


def padded_line(srcw, n_local):
    """(ks, n + 2) -> (ks, n_local + 2): the line and its window points where the call wants them, junk behind"""
    out = np.full((srcw.shape[0], n_local + 2), 31.0)
    out[:, :srcw.shape[1]] = srcw
    return out


def first_difference(got, want):
    bad = np.argwhere(np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))
    return (len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]) if len(bad) else None


# ---- 1: the stand-alone routine on one tile, all four edges -----------------------------------------------------------------------------
def standalone_equals_the_expectation(lib, shape, salt=False):
    """every edge of one shape on ONE context; the state does not change.  The lines are doubles in every build: the fp32 builds give the
    fp64 result"""
    im, jm, ks, kb = shape
    g = b = before = None
    for edge in range(4):
        zs, line, zz, h = ZL.make_inputs(im, jm, ks, kb, edge, salt=salt)
        hl = ZL.depth_line(h, edge)
        ZL.assert_inputs_are_demanding(zs, line, zz, hl, edge)
        want = ZL.ztosig_line(zs, ZL.with_window(line), zz, hl, edge)
        ZL.assert_result_is_demanding(want)
        gold = golden(im, jm, ks, kb, edge, salt)
        assert {n: ZL.digest(a) for n, a in (("zs", zs), ("line", line), ("zz", zz), ("h", h))} == gold["inputs"], "the generator has drifted from the golden file's"
        assert ZL.digest(want) == gold["reference"], "the restatement differs from the reference's recorded output"
        b = state_of(one_tile(im, jm), kb, zz, h)             # the depth differs per edge: a context each
        before = b.copy()
        g = PomGpu(b, libpath=lib)
        got = g.ztosig_line(edge, zs, ZL.with_window(line))
        assert ZL.digest(got) == gold["reference"], (ZL.EDGES[edge], first_difference(got, want))
        assert not first_difference(got, want) and (got[kb - 1] != 0).any()
        g.download()
        g.close()
        assert int(b.error_status) == 0 and not diff(before, b), diff(before, b)


def trimmed_tile_keeps_its_padding(lib, shape=(20, 17, 5, 6)):
    """a tile whose arrays are larger than (im, jm): the window point sits behind point n, what lies behind it is not read, and the points
    beyond n come out zero"""
    im, jm, ks, kb = shape
    for edge in range(4):
        zs, line, zz, h = ZL.make_inputs(im, jm, ks, kb, edge)
        want = ZL.ztosig_line(zs, ZL.with_window(line), zz, ZL.depth_line(h, edge), edge)
        tile = decomp.make_tile(0, im, jm, im + 3, jm + 2)
        assert (tile.im, tile.jm, tile.im_local, tile.jm_local) == (im, jm, im + 3, jm + 2)
        b = state_of(tile, kb, zz, h)
        b.h[:, im:], b.h[jm:, :] = 500.0, 500.0
        n, nl = (jm, jm + 2) if ZL.along_j(edge) else (im, im + 3)
        g = PomGpu(b, libpath=lib)
        got = g.ztosig_line(edge, zs, padded_line(ZL.with_window(line), nl))
        g.close()
        assert got.shape == (kb, nl) and same_bits(got[:, :n], want), (edge, first_difference(got[:, :n], want))
        assert not got[:, n:].any() and not np.signbit(got[:, n:]).any()


# ---- 2: tiles ---------------------------------------------------------------------------------------------------------------------------
TILE_GRID, TILE_KB, TILE_KS = (37, 29), 6, 5


def tiles(lib):
    """2x2 tiles, the east and north ones trimmed: every rank maps every line with ITS h -- east with its own h(imm1,j), whether or not the
    tile lies on that edge --, a ghost end from the window point beyond it.  Each tile's line is the single tile's on that tile's piece,
    ghost ends included: the line of the whole edge under the depth of the tile's column / row.  No message round is posted."""
    IMg, JMg = TILE_GRID
    iml, jml = decomp.local_size(IMg, JMg, 2, 2)
    tl = [decomp.make_tile(r, IMg, JMg, iml, jml, n_proc=4) for r in range(4)]
    assert len({(t.im, t.jm) for t in tl}) == 4 and any(t.im < iml for t in tl) and any(t.jm < jml for t in tl), "trimmed east / north tiles"
    seen = set()
    for edge in range(4):
        zs, line, zz, h = ZL.make_inputs(IMg, JMg, TILE_KS, TILE_KB, edge, salt=edge % 2 == 1)
        h = 20.0 + np.abs(h) + 7.0 * np.arange(IMg)[None, :] + 3.0 * np.arange(JMg)[:, None]   # every column / row another depth line
        h[5, :], h[:, 6] = 0.75, 1.0
        for r, t in enumerate(tl):
            aj = ZL.along_j(edge)
            off, n, nl = (t.j_off, t.jm, t.jm_local) if aj else (t.i_off, t.im, t.im_local)
            lo_phys, hi_phys = ((t.n_south, t.n_north) if aj else (t.n_west, t.n_east))
            lo_phys, hi_phys = lo_phys == -1, hi_phys == -1
            gl = line.copy()
            # a missing value at a ghost end whose fill-in needs the window point beyond it: the neighbour inside the tile is missing too
            k = 0
            if not hi_phys:
                gl[k, off + n - 1], gl[k, off + n - 2], gl[k, off + n] = 0.0, 0.0, 19.0 + r
            if not lo_phys:
                gl[k, off], gl[k, off + 1], gl[k, off - 1] = 0.0, 0.0, 23.0 + r
            hw = h[t.j_off:t.j_off + t.jm, t.i_off:t.i_off + t.im]
            hl = ZL.depth_line(hw, edge)
            srcw = ZL.window_of(gl, off, n)
            want = ZL.ztosig_line(zs, srcw, zz, hl, edge, lo_phys, hi_phys)
            # ... which is the whole line's value there (the single tile of the global grid under this tile's depth line)
            hg = (h[:, t.i_off + (t.im - 2 if edge == 0 else 1)] if aj else h[t.j_off + (1 if edge == 1 else t.jm - 2), :])
            whole = ZL.ztosig_line(zs, ZL.with_window(gl), zz, hg, edge)
            a0, a1 = (0 if lo_phys else off), (len(hg) if hi_phys else off + n)
            assert same_bits(want[:, a0 - off:a1 - off], whole[:, a0:a1])
            if not hi_phys:
                assert hl[n - 1] > 1.0 and want[0, n - 1] != want[0, n - 2]
                no_window = srcw.copy()
                no_window[:, -1] = 0.0
                assert not same_bits(ZL.ztosig_line(zs, no_window, zz, hl, edge, lo_phys, hi_phys)[:, n - 1], want[:, n - 1]), "the window point shows"
                seen.add("hi")
            if not lo_phys:
                no_window = srcw.copy()
                no_window[:, 0] = 0.0
                assert not same_bits(ZL.ztosig_line(zs, no_window, zz, hl, edge, lo_phys, hi_phys)[:, 0], want[:, 0]), "the window point shows"
                seen.add("lo")
            st = state_of(t, TILE_KB, zz, h)
            g = PomGpu(st, libpath=lib)
            rounds = g.exchange_rounds()
            got = g.ztosig_line(edge, zs, padded_line(srcw, nl))
            assert g.exchange_rounds() == rounds, "a message round was posted"
            g.close()
            assert same_bits(got[:, :n], want), (edge, r, first_difference(got[:, :n], want))
            assert not got[:, n:].any()
    assert seen == {"lo", "hi"}


# ---- 3: refusals, on a foreign, stepped state -------------------------------------------------------------------------------------------
def refusals_and_a_stepped_context(lib, size=(20, 17, 6), ks=5):
    """a context that has stepped keeps arrays lazily: the call completes them first, refuses bad arguments before anything is written,
    maps onto the state's own h and zz and leaves every mirror as it was"""
    im, jm, kb = size
    zs, line, _, _ = ZL.make_inputs(im, jm, ks, kb, 0)
    srcw = ZL.with_window(line)
    b = make_case("archipelago", im, jm, kb)
    oracle_finish_initial(b)
    g = PomGpu(b, libpath=lib)
    g.run(2)
    g.download()
    before = b.copy()
    assert before.wr.any() and before.tclim.any()
    out = np.full((kb, jm), 4.5)

    def refused(cause, zs_, edge=0, ks_=None, src_=srcw, out_=out):
        z = np.ascontiguousarray(zs_, dtype=np.float64)
        rc = g.L.pomgpu_ztosig_line(g.h, edge, g._p(z), len(z) if ks_ is None else ks_, None if src_ is None else g._p(src_), None if out_ is None else g._p(out_))
        es, msg = status(g)
        assert rc == -1 and es == 1 and cause in msg and msg.startswith("ztosig_line"), (rc, es, msg)
        g.set_con(error_status=0)
        g.download()
        assert not diff(before, b), (cause, diff(before, b))
        assert (out == 4.5).all()

    refused("outside 2..300", zs[:1])
    refused("outside 2..300", np.arange(1.0, 302.0), ks_=301)
    refused("outside 2..300", zs, ks_=0)
    refused("increase strictly", [5.0, 9.0, 9.0, 20.0, 30.0])
    refused("increase strictly", [5.0, 9.0, 8.0, 20.0, 30.0])
    refused("not finite", [5.0, 9.0, np.nan, 20.0, 30.0])
    refused("not finite", [5.0, 9.0, 12.0, 20.0, np.inf])
    refused("none of 0 east", zs, edge=4)
    refused("none of 0 east", zs, edge=-1)
    refused("must be given", zs, src_=None)
    refused("must be given", zs, out_=None)
    with pytest.raises(ValueError):
        g.ztosig_line(0, zs, srcw[:, :-1])
    with pytest.raises(ValueError):
        g.ztosig_line(1, zs, srcw)                            # im + 2 wanted
    with pytest.raises(PomGpuError):
        g.ztosig_line(0, zs[::-1], srcw)
    g.set_con(error_status=0)
    for edge in range(4):
        ln = ZL.make_inputs(im, jm, ks, kb, edge)[1]
        hl = ZL.depth_line(before.h, edge)
        want = ZL.ztosig_line(zs, ZL.with_window(ln), b.zz, hl, edge)
        got = g.ztosig_line(edge, zs, ZL.with_window(ln))
        assert same_bits(got, want) and want.any(), (edge, first_difference(got, want))
    g.download()
    assert int(b.error_status) == 0 and not diff(before, b), diff(before, b)
    g.run(1)                                                  # ... and the context steps on
    g.download()
    g.close()
    assert int(b.error_status) == 0 and not same_bits(b.t, before.t)
