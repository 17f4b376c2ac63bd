"""The checks of pomgpu_ztosig (PomGpu.ztosig), each taking the library to load (None: the product library on device 0), so that
tests/test_ztosig_emulated.py (the host builds) and tests/test_gpu_ztosig.py (the device) cannot drift apart.  The bar is
tests/ztosig_expect.py's restatement, which tests/test_ztosig_vs_reference.py holds to the reference's compiled routine, and the digests
of that routine's own output in tests/golden/ztosig.json: 64-bit patterns on every cell."""
import json
import os
import threading

import numpy as np
import pytest

import ztosig_expect as Z
from cold_start_expect import blank_state, diff
from extpom_amd import decomp
from extpom_amd.cases import make_case
from extpom_amd.lib import PomGpuError
from extpom_amd.model import PomGpu
from oracle.pyoracle import oracle_finish_initial
from ztosig_expect import same_bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ztosig.json")
_golden = {}


def golden(im, jm, ks, kb, salt):
    if not _golden:
        with open(GOLDEN) as fh:
            _golden.update(json.load(fh))
    return _golden[f"{im}x{jm}x{ks}x{kb}{'S' if salt else 'T'}"]


def one_tile(im, jm):
    return decomp.make_tile(0, im, jm, im, jm)


def state_of(tile, kb, zz, h, fill=9.25):
    """a blank state with the tile's window of h, the sigma levels and a target array that is not zero"""
    st = blank_state(tile, kb)
    st.zz = zz
    st.h[:tile.jm, :tile.im] = h[tile.j_off:tile.j_off + tile.jm, tile.i_off:tile.i_off + tile.im]
    st.tclim = fill
    st.sclim = fill
    return st


def padded(tile, a, value=0.0):
    """the tile's window of a global (..., jm, im) array inside (..., jm_local, im_local)"""
    out = np.full(a.shape[:-2] + (tile.jm_local, tile.im_local), value)
    out[..., :tile.jm, :tile.im] = a[..., tile.j_off:tile.j_off + tile.jm, tile.i_off:tile.i_off + tile.im]
    return out


def status(g):
    g.L.pomgpu_get_con(g.h, g._p(g.st.con))
    return int(g.st.error_status), g.L.pomgpu_last_error(g.h).decode()


# ---- 1: the stand-alone routine on one tile ---------------------------------------------------------------------------------------------
def standalone_equals_the_expectation(lib, shape, salt=False, f32=False):
    im, jm, ks, kb = shape
    zs, src, zz, h = Z.make_inputs(im, jm, ks, kb, salt=salt)
    Z.assert_inputs_are_demanding(zs, src, zz, h)
    want = Z.ztosig(zs, src, zz, h)
    Z.assert_result_is_demanding(want)
    gold = golden(im, jm, ks, kb, salt)
    assert {n: Z.digest(a) for n, a in (("zs", zs), ("src", src), ("zz", zz), ("h", h))} == gold["inputs"], "the generator has drifted from the golden file's"
    assert Z.digest(want) == gold["reference"], "the restatement differs from the reference's recorded output"
    tile = one_tile(im, jm)
    b = state_of(tile, kb, zz, h)
    before = b.copy()
    g = PomGpu(b, libpath=lib)
    g.ztosig(zs, src, "sclim" if salt else "tclim")
    g.download()
    g.close()
    got, other = (b.sclim, "tclim") if salt else (b.tclim, "sclim")
    if f32:                                                  # computed in fp64, rounded once at the store; the edge copies carry the rounded value
        want = want.astype(np.float32).astype(np.float64)
        assert not same_bits(want, Z.ztosig(zs, src, zz, h))
    else:
        assert Z.digest(got) == gold["reference"]
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert not len(bad), (len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    assert int(b.error_status) == 0 and (got[kb - 1] != 0).any()
    before.field("sclim" if salt else "tclim")[...] = got    # nothing else has changed
    assert same_bits(b.field(other), before.field(other)) and not diff(before, b), diff(before, b)


def trimmed_tile_keeps_its_padding(lib, shape=(20, 17, 5, 6)):
    """a tile whose arrays are larger than (im, jm): the source's padding is not read into the result and t's padding keeps what it held"""
    im, jm, ks, kb = shape
    zs, src, zz, h = Z.make_inputs(im, jm, ks, kb)
    want = Z.ztosig(zs, src, zz, h)
    tile = decomp.make_tile(0, im, jm, im + 3, jm + 2)
    assert (tile.im, tile.jm, tile.im_local, tile.jm_local) == (im, jm, im + 3, jm + 2) and tile.n_east == -1 and tile.n_north == -1
    b = state_of(tile, kb, zz, h)
    b.h[:, im:], b.h[jm:, :] = 500.0, 500.0
    g = PomGpu(b, libpath=lib)
    g.ztosig(zs, padded(tile, src, 30.0), "tb")
    g.download()
    g.close()
    assert same_bits(b.tb[:, :jm, :im], want)
    assert not b.tb[:, jm:, :].any() and not b.tb[:, :, im:].any()


# ---- 2: tiles ---------------------------------------------------------------------------------------------------------------------------
TILE_GRID, TILE_KB, TILE_KS = (97, 59), 11, 7


def tiles(lib):
    """2x2 tiles, the east and north ones trimmed, under the library's exchange: each tile is handed ITS window of the source, ghost cells
    included, as the reference's ztosig is; the ghost lines of t arrive through one message round; every cell of a tile, ghost lines and
    corners included, is the single tile's result on that window"""
    from forcing_files_checks import Board, device_mover, host_mover
    mover = host_mover if lib is not None else device_mover
    IMg, JMg = TILE_GRID
    zs, src, zz, h = Z.make_inputs(IMg, JMg, TILE_KS, TILE_KB)
    want = Z.ztosig(zs, src, zz, h)
    iml, jml = decomp.local_size(IMg, JMg, 2, 2)
    tl = [decomp.make_tile(r, IMg, JMg, iml, jml, n_proc=4) for r in range(4)]
    assert {(t.im, t.jm) for t in tl} == {(50, 31), (49, 31), (50, 30), (49, 30)}
    board, out, errs = Board(4), {}, []

    def rank(r):
        try:
            tile = tl[r]
            st = state_of(tile, TILE_KB, zz, h)
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
            rounds = g.exchange_rounds()
            board.barrier.wait()
            g.ztosig(zs, padded(tile, src), "tclim")
            assert g.exchange_rounds() == rounds + 1
            g.download()
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
    for r in range(4):
        t = tl[r]
        w = want[:, t.j_off:t.j_off + t.jm, t.i_off:t.i_off + t.im]
        got = out[r].tclim[:, :t.jm, :t.im]
        bad = np.argwhere(got.view(np.uint64) != np.ascontiguousarray(w).view(np.uint64))
        assert not len(bad), (r, len(bad), bad[:4].tolist())
    # the seam is not trivial: the ghost lines hold values, and they are not the edge copies a single tile would make
    t0 = tl[0]
    ghost = out[0].tclim[:, :t0.jm, t0.im - 1]
    assert ghost.any() and not same_bits(ghost, out[0].tclim[:, :t0.jm, t0.im - 2])


# ---- 3: refusals, on a foreign, stepped state -------------------------------------------------------------------------------------------
def refusals_and_a_stepped_context(lib, size=(20, 17, 6), ks=5):
    """a context that has stepped keeps arrays lazily: the call completes them first, refuses bad arguments before anything changes, and
    then maps onto the state's own h and zz"""
    im, jm, kb = size
    zs, src, _, _ = Z.make_inputs(im, jm, ks, kb)
    b = make_case("archipelago", im, jm, kb)
    oracle_finish_initial(b)
    g = PomGpu(b, libpath=lib)
    g.run(2)
    g.download()
    before = b.copy()
    assert before.wr.any() and before.tclim.any()

    def refused(cause, zs_, src_=src, t="tclim", ks_=None):
        z = np.ascontiguousarray(zs_, dtype=np.float64)
        rc = g.L.pomgpu_ztosig(g.h, g._p(z), len(z) if ks_ is None else ks_, g._p(src_), g._a(t) if isinstance(t, str) else t)
        es, msg = status(g)
        assert rc == -1 and es == 1 and cause in msg and msg.startswith("ztosig"), (rc, es, msg)
        g.set_con(error_status=0)
        g.download()
        assert not diff(before, b), (cause, diff(before, b))

    refused("outside 2..300", zs[:1])
    refused("outside 2..300", np.arange(1.0, 302.0), ks_=301)
    refused("outside 2..300", zs, ks_=0)
    refused("increase strictly", [5.0, 9.0, 9.0, 20.0, 30.0])
    refused("increase strictly", [5.0, 9.0, 8.0, 20.0, 30.0])
    refused("not finite", [5.0, 9.0, np.nan, 20.0, 30.0])
    refused("not finite", [5.0, 9.0, 12.0, 20.0, np.inf])
    bogus = np.zeros(4)
    refused("blk3d array", zs, t=g._p(bogus))
    refused("blk3d array", zs, t=g._p(b.h))                  # a 2-D COMMON array
    with pytest.raises(ValueError):
        g.ztosig(zs, src[:, :-1], "tclim")
    with pytest.raises(PomGpuError):
        g.ztosig(zs[::-1], src, "tclim")
    g.set_con(error_status=0)
    want = Z.ztosig(zs, src, b.zz, before.h)
    assert (before.h[1:-1, 1:-1] <= 1.0).any() and want.any()
    g.ztosig(zs, src, "tclim")
    g.download()
    assert same_bits(b.tclim, want) and int(b.error_status) == 0
    before.tclim = want
    assert not diff(before, b), diff(before, b)
    g.run(1)                                                  # ... and the context steps on
    g.download()
    g.close()
    assert int(b.error_status) == 0 and not same_bits(b.t, before.t)
