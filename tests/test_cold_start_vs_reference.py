"""The cold start's expectation against the reference's OWN code, at 65x49x21 (the size the suite builds the reference for): the restated
reader output is placed in the reference's COMMON blocks (oracle/refharness.py), the reference's dens runs twice, then its update_initial
(which calls its baropg / baropg_mcc) and its bottom_friction -- and the result equals tests/cold_start_expect.py's expectation, the
oracle's dens / baropg and math.log included, on every array, for npg = 1 and npg = 2.

read_grid and initial_conditions themselves end in oracle/ref_traps.c's aborts (their readers call PnetCDF) and cannot be called: their
lines -- dz dzz cor period art aru arv d dt, the masks, tsurf ssurf, the boundary lines and rf* -- are pinned by the restatement alone."""
import pytest

import cold_start_checks as C
import cold_start_expect as E
from oracle.refharness import RefLib, have_ref

SIZE = (65, 49, 21)
pytestmark = pytest.mark.skipif(not have_ref(*SIZE), reason="reference build not present")


@pytest.mark.parametrize("npg,ramp", [(1, 1.0), (2, 1.0), (1, 0.0), (2, 0.0)])
def test_expectation_equals_the_references_own_tail(tmp_path, npg, ramp):
    """ramp = 0 is what the reference's COMMON holds when initialize runs (get_time assigns it first, advance.f:69-72): drhox, drhoy,
    drx2d, dry2d are then zeros whose signs are compared too"""
    im, jm, kb = SIZE
    nml = dict(npg=npg, ramp=ramp)
    f, paths = C.inputs(tmp_path, SIZE, nml=nml)
    tile = C.one_tile(im, jm)
    want, _ = E.expected_state(paths, tile, kb, **nml)
    st, _ = E.expected_readers(paths, tile, kb, **nml)
    ref = RefLib(im, jm, kb)
    ref.put(st)
    ref.call("dens", ref.f3("sclim"), ref.f3("tclim"), ref.f3("rmean"))      # initialize.f:416
    ref.call("dens", ref.f3("sb"), ref.f3("tb"), ref.f3("rho"))              # :425
    ref.get(st)
    st.tsurf, st.ssurf = st.tb[0], st.sb[0]                                  # :437-460, restated
    st.rfe = st.rfw = st.rfn = st.rfs = 1.0
    for b, src in (("tb", st.tb), ("sb", st.sb)):
        st.field(b + "e")[:kb - 1] = src[:kb - 1, :, im - 1]
        st.field(b + "w")[:kb - 1] = src[:kb - 1, :, 0]
        st.field(b + "n")[:kb - 1] = src[:kb - 1, jm - 1, :]
        st.field(b + "s")[:kb - 1] = src[:kb - 1, 0, :]
    ref.put(st)
    ref.call("update_initial")                                               # :466-521, with the reference's baropg / baropg_mcc
    ref.call("bottom_friction")                                              # :524-544
    ref.get(st)
    assert int(st.error_status) == 0 and bool(st.drhox.any()) == (ramp != 0.0) and st.cbc.any()
    assert not E.diff(want, st), E.diff(want, st)
