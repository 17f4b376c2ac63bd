"""tests/ztosig_expect.py's restatement of ztosig / splinc / splint against the reference's OWN compiled code: `ztosig_` of the reference
build (oracle/build_ref.sh compiles initialize.f unmodified).  Every array extent of the routine is an argument, so the one library serves
every shape; its exchange3d_mpi is a no-op with blkpar's four neighbours at -1.  Bit for bit on every cell, for each combination of
physical edges the routine can be told."""
import ctypes

import numpy as np
import pytest

import ztosig_expect as Z
from oracle.refharness import RefLib, have_ref

pytestmark = pytest.mark.skipif(not have_ref(65, 49, 21), reason="reference build not present")


def reference_ztosig(zs, src, zz, h, nbr=(-1, -1, -1, -1)):
    ref = RefLib(65, 49, 21)
    ref.par[-4:] = -1
    ks, jm, im = src.shape
    kb = len(zz)
    zs, src, zz, h = (np.ascontiguousarray(a, dtype=np.float64) for a in (zs, src, zz, h))
    t = np.full((kb, jm, im), 7.5)
    I = lambda v: ctypes.byref(ctypes.c_int(v))
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    ref.call("ztosig", P(zs), P(src), P(zz), P(h), P(t), I(im), I(jm), I(ks), I(kb), I(im), I(jm), *[I(n) for n in nbr])
    return t


@pytest.mark.parametrize("shape", Z.SHAPES, ids=str)
@pytest.mark.parametrize("salt", [False, True], ids=["T", "S"])
def test_restatement_equals_the_references_ztosig(shape, salt):
    im, jm, ks, kb = shape
    zs, src, zz, h = Z.make_inputs(im, jm, ks, kb, salt=salt)
    Z.assert_inputs_are_demanding(zs, src, zz, h)
    want = reference_ztosig(zs, src, zz, h)
    got = Z.ztosig(zs, src, zz, h)
    Z.assert_result_is_demanding(got)
    bad = np.argwhere(want.view(np.uint64) != got.view(np.uint64))
    assert not len(bad), (len(bad), bad[:5], want[tuple(bad[0])], got[tuple(bad[0])])


@pytest.mark.parametrize("nbr", [(3, -1, -1, -1), (-1, 3, 3, -1), (3, 3, 3, 3), (-1, -1, -1, 3)], ids=str)
def test_edge_copies_follow_the_neighbour_arguments(nbr):
    im, jm, ks, kb = 20, 17, 5, 6
    zs, src, zz, h = Z.make_inputs(im, jm, ks, kb)
    want = reference_ztosig(zs, src, zz, h, nbr)
    got = Z.ztosig(zs, src, zz, h, *[n == -1 for n in nbr])
    assert Z.same_bits(want, got)


def test_without_the_single_precision_maximum_most_cells_differ():
    """the finding the restatement rests on: amax1 is the REAL(4) intrinsic"""
    im, jm, ks, kb = 20, 17, 5, 6
    zs, src, zz, h = Z.make_inputs(im, jm, ks, kb)
    keep = Z.neighbour_max
    try:
        Z.neighbour_max = lambda s: np.maximum(np.maximum(s[:, 1:-1, :-2], s[:, 1:-1, 2:]), np.maximum(s[:, :-2, 1:-1], s[:, 2:, 1:-1]))
        wide = Z.ztosig(zs, src, zz, h)
    finally:
        Z.neighbour_max = keep
    want = reference_ztosig(zs, src, zz, h)
    assert (wide.view(np.uint64) != want.view(np.uint64)).mean() > 0.3
