"""The CPU oracle against the reference itself.  ALL COMMON-block arrays -- not only the restart list -- and bdry and blkcon
must be bit-identical after every step, and so must each hot-path routine called on its own.  The reference's side is stored
in tests/golden/oracle_vs_reference_65x49x21.json: per array a digest of the state of the reference build (oracle/_ref, the
unmodified sources, oracle/build_ref.sh) on the same inputs, written by `tests/golden/make_golden.py refcheck`.
oracle_vs_reference_archipelago_65x49x21.json (`make_golden.py archipelago`) holds the same for the fourth case, the only one on
which the oracle's curvature terms, its cross-direction metric neighbours, cor(i-1,j) and its interior masks are not trivial."""
import ctypes
import json
import os

import numpy as np
import pytest

from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D
from oracle.pyoracle import OracleTile, oracle_finish_initial
from oracle.refharness import state_digests

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_reference_65x49x21.json")
GOLDEN_ARCHIPELAGO = os.path.join(os.path.dirname(GOLDEN), "oracle_vs_reference_archipelago_65x49x21.json")


@pytest.fixture(scope="module")
def ref_archipelago():
    with open(GOLDEN_ARCHIPELAGO) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ref():
    with open(GOLDEN) as f:
        return json.load(f)


def _diff(st, want):
    """what of st differs from the reference's bits; a NaN counts as a difference wherever it is (it equals nothing)"""
    got = state_digests(st)
    bad = [n for n in want if got[n] != want[n]]
    floats = [(n, st.field(n)) for n in BLK2D + BLK3D] + [("bdry", st.bdry)]
    floats += [("con." + n, st.con[n]) for n in st.con.dtype.names if st.con.dtype[n].kind == "f"]
    return bad + [n for n, a in floats if n not in bad and np.isnan(a).any()]


def _steps(rec):
    """(step, whole expected state) in order: a stored record after the first holds only the arrays that changed"""
    cur = dict(rec["init"])
    for n in sorted(rec["steps"], key=int):
        cur.update(rec["steps"][n])
        yield int(n), dict(cur)


@pytest.mark.parametrize("case,nml", [("seamount", dict(dte=6.0, isplit=30)),
                                      ("island", dict(dte=6.0, isplit=30, nadv=1)),
                                      ("basin", dict(dte=6.0, isplit=10, nitera=2)),
                                      ("island", dict(dte=6.0, isplit=30, npg=2))])
def test_full_state_bit_identical(ref, case, nml):
    _full_state(ref, case, nml)


@pytest.mark.parametrize("nml", [dict(), dict(nadv=1), dict(nitera=2), dict(npg=2), dict(mode=2)], ids=str)
def test_full_state_bit_identical_archipelago(ref_archipelago, nml):
    """12 steps of the fourth case: curved grid, interior land, both signs on the open edges, every forcing field live"""
    _full_state(ref_archipelago, "archipelago", dict(dte=6.0, isplit=30, **nml))


def _full_state(ref, case, nml):
    rec = ref["full_state"][json.dumps([case, nml], sort_keys=True)]
    b = make_case(case, 65, 49, 21, **nml)
    oracle_finish_initial(b)
    assert not _diff(b, rec["init"]), f"initial state: {_diff(b, rec['init'])}"
    ot = OracleTile(b)
    want = list(_steps(rec))
    assert [n for n, _ in want] == list(range(1, 13))
    for n, w in want:
        ot.run(1)
        assert not _diff(b, w), f"step {n}: {_diff(b, w)}"


def test_each_routine_bit_identical(ref):
    """call the routines one by one on a warm state (step 3: all branches live)"""
    _each_routine(ref, "seamount")


def test_each_routine_bit_identical_archipelago(ref_archipelago):
    """the same on the warm state of the fourth case (proft with nbc 1-4 on a non-zero swrad and wssurf)"""
    _each_routine(ref_archipelago, "archipelago")


def _each_routine(ref, case):
    a = make_case(case, 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    OracleTile(a).run(3)
    a.iint = 4
    a.iext = 7
    warm, calls = ref["each_routine"]["warm"], ref["each_routine"]["calls"]
    assert not _diff(a, warm), f"warm state: {_diff(a, warm)}"
    done = []

    def both(label, name, or_args=()):
        y = a.copy()
        ot = OracleTile(y)
        ot.call(name, *or_args(ot) if callable(or_args) else or_args)
        want = dict(warm, **calls[label])
        assert not _diff(y, want), f"{label}: {_diff(y, want)}"
        done.append(label)

    for name in ("advave", "advct", "advu", "advv", "baropg", "baropg_mcc", "profq", "profu", "profv", "vertvl", "realvertvl",
                 "lateral_viscosity", "mode_interaction", "mode_external", "mode_internal", "check_velocity"):
        both(name, name)
    both("advq", "advq", lambda o: (o.a3("q2b"), o.a3("q2"), o.a3("uf")))
    for r in ("advt1", "advt2"):
        both(r, r, lambda o: (o.a3("tb"), o.a3("t"), o.a3("tclim"), o.a3("uf")))
    both("dens", "dens", lambda o: (o.a3("s"), o.a3("t"), o.a3("rho")))
    for nbc in (1, 2, 3, 4):
        both(f"proft/{nbc}", "proft", lambda o: (o.a3("uf"), o.a2("wtsurf"), o.a2("tsurf"), ctypes.c_int(nbc)))
    for idx in (1, 2, 4, 5, 6):
        both(f"bcond/{idx}", "bcond", (ctypes.c_int(idx),))
    for idx in (3, 5):
        both(f"bcondorl/{idx}", "bcondorl", (ctypes.c_int(idx),))
    assert sorted(done) == sorted(calls)


def test_domain_stats_matches_reference_to_rounding(ref):
    """advance.f:644-756 uses the SUM intrinsic (order of additions is the compiler's): 1e-13 relative"""
    a = make_case("island", 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    OracleTile(a).run(5)
    rec = ref["domain_stats"]
    assert not _diff(a, rec["state"]), f"step 5: {_diff(a, rec['state'])}"
    out = (ctypes.c_double * 8)()
    OracleTile(a).call("domain_stats", out, ctypes.c_int(0))
    np.testing.assert_allclose(np.array(list(out)), np.array([float.fromhex(v) for v in rec["values"]]), rtol=1e-13, atol=0)


def test_forcing_bit_identical_across_record_changes(ref):
    """surface_forcing (wind, heat, surface: bounds_forcing.f:871-983) and lateral_bc (:593-868) inside advance
    (advance.f:14-18), fed with the same records through the readers' entry points.  62 steps: the surface records
    shift at step 60 (0.125 d / 180 s), the lateral ones every 20 steps (1/24 d).  The whole bdry block is compared
    (incl. the members the reference never refreshes, :742-753)."""
    from extpom_amd.cases import make_forcing_records, make_lateral_records
    b = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30, days=0.4)
    oracle_finish_initial(b)
    make_forcing_records(b, 4)
    make_lateral_records(b, 5)
    rec = ref["forcing"]
    assert not _diff(b, rec["init"]), f"initial state: {_diff(b, rec['init'])}"
    want = dict(_steps(rec))
    assert sorted(want) == [1, 2, 19, 20, 21, 40, 41, 59, 60, 61, 62]
    ot = OracleTile(b)
    for n in range(1, 63):
        ot.run(1)
        if n in want:
            assert not _diff(b, want[n]), f"step {n}: {_diff(b, want[n])}"
    assert float(np.abs(b.tsurf).max()) > 0 and not np.array_equal(b.wusurfb, b.wusurff)


def test_ramped_forcing_bit_identical(ref):
    """lramp = .true.: ramp = time/period grows every step (advance.f:66-72) and scales the open-boundary
    velocities and the pressure gradient"""
    b = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30)
    b.lramp = True
    oracle_finish_initial(b)
    rec = ref["ramped"]
    assert not _diff(b, rec["init"]), f"initial state: {_diff(b, rec['init'])}"
    ot = OracleTile(b)
    for _ in range(6):
        ot.run(1)
    (n, want), = _steps(rec)
    assert n == 6 and 0.0 < b.ramp < 1.0 and not _diff(b, want), _diff(b, want)
