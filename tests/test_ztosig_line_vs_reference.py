"""tests/ztosig_line_expect.py's restatement of the line mapping against the reference's OWN compiled ztosig_, called as the commented
blocks of bounds_forcing.f:636-716 call it: the line spread across the tile (ts1(i,j,k) = t_e(j,k) for every i; south, north: along j),
hs = h(imm1,j) / h(i,2) / h(2,j) / h(i,jmm1) spread likewise, and the column im/2 (the row jm/2) of the result kept.  Bit for bit on
every point: the four edges, T-like and S-like, every combination of physical ends (an end towards a neighbour tile is the whole line's
value there: what the owner computes and the exchange brings), and a second sampled column and row."""
import numpy as np
import pytest

import ztosig_line_expect as ZL
from oracle.refharness import have_ref
from test_ztosig_vs_reference import reference_ztosig

pytestmark = pytest.mark.skipif(not have_ref(65, 49, 21), reason="reference build not present")


def block(zs, line, zz, h, edge, sample=None):
    """the commented block: (kb, n) = ts2(im/2, :, :) or ts2(:, jm/2, :) of the reference's ztosig_ (sample: another column / row, 1-based)"""
    jm, im = h.shape
    ks = len(zs)
    hl = ZL.depth_line(h, edge)
    if ZL.along_j(edge):
        ts1 = np.broadcast_to(line[:, :, None], (ks, jm, im))
        hs = np.broadcast_to(hl[:, None], (jm, im))
        return reference_ztosig(zs, ts1, zz, hs)[:, :, (sample or im // 2) - 1]
    ts1 = np.broadcast_to(line[:, None, :], (ks, jm, im))
    hs = np.broadcast_to(hl[None, :], (jm, im))
    return reference_ztosig(zs, ts1, zz, hs)[:, (sample or jm // 2) - 1, :]


@pytest.mark.parametrize("salt", [False, True], ids=["T", "S"])
@pytest.mark.parametrize("edge", range(4), ids=ZL.EDGES)
@pytest.mark.parametrize("shape", ZL.SHAPES, ids=str)
def test_restatement_equals_the_references_block(shape, edge, salt):
    im, jm, ks, kb = shape
    zs, line, zz, h = ZL.make_inputs(im, jm, ks, kb, edge, salt=salt)
    hl = ZL.depth_line(h, edge)
    ZL.assert_inputs_are_demanding(zs, line, zz, hl, edge)
    want = block(zs, line, zz, h, edge)
    got = ZL.ztosig_line(zs, ZL.with_window(line), zz, hl, edge)
    ZL.assert_result_is_demanding(got)
    bad = np.argwhere(np.ascontiguousarray(want).view(np.uint64) != got.view(np.uint64))
    assert not len(bad), (len(bad), bad[:5], want[tuple(bad[0])], got[tuple(bad[0])])


@pytest.mark.parametrize("edge", range(4), ids=ZL.EDGES)
def test_the_sampled_column_and_row_do_not_matter(edge):
    im, jm, ks, kb = 20, 17, 5, 6
    zs, line, zz, h = ZL.make_inputs(im, jm, ks, kb, edge)
    want = block(zs, line, zz, h, edge)
    for sample in (2, 3, (im if ZL.along_j(edge) else jm) - 1):
        assert ZL.same_bits(block(zs, line, zz, h, edge, sample), want)


@pytest.mark.parametrize("ends", [(True, True), (True, False), (False, True), (False, False)], ids=str)
@pytest.mark.parametrize("edge", range(4), ids=ZL.EDGES)
def test_every_combination_of_physical_ends(edge, ends):
    """a tile's piece of the line: a physical end copies, an end towards a neighbour equals the whole line's value there"""
    im, jm, ks, kb = 65, 49, 33, 21
    zs, line, zz, h = ZL.make_inputs(im, jm, ks, kb, edge, salt=edge % 2 == 1)
    hl = ZL.depth_line(h, edge)
    n = len(hl)
    want = block(zs, line, zz, h, edge)
    first, last = (0 if ends[0] else 9), (n if ends[1] else n - 11)
    got = ZL.ztosig_line(zs, ZL.window_of(line, first, last - first), zz, hl[first:last], edge, *ends)
    if ends[0] and ends[1]:
        assert ZL.same_bits(got, want)
        return
    lo, hi = (0 if ends[0] else first), (n if ends[1] else last)
    assert ZL.same_bits(got[:, lo - first:hi - first], want[:, lo:hi])
    # a copied end is only right on a tile that has that end: the piece's inner ends are NOT copies
    if not ends[0]:
        assert not ZL.same_bits(got[:, 0], got[:, 1])
    if not ends[1]:
        assert not ZL.same_bits(got[:, -1], got[:, -2])


def test_without_the_single_precision_maximum_the_line_differs():
    im, jm, ks, kb = 20, 17, 5, 6
    zs, line, zz, h = ZL.make_inputs(im, jm, ks, kb, 0)
    keep = ZL.neighbour_max
    try:
        ZL.neighbour_max = lambda own, prev, nxt, edge: np.maximum(own, np.maximum(prev, nxt))
        wide = ZL.ztosig_line(zs, ZL.with_window(line), zz, ZL.depth_line(h, 0), 0)
    finally:
        ZL.neighbour_max = keep
    assert not ZL.same_bits(wide, block(zs, line, zz, h, 0))
