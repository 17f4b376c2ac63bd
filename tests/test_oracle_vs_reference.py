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


# ---- the run constants off their defaults (tests/off_default.py; tests/golden/off_default_constants_65x49x21.json holds the reference's
# side, `make_golden.py constants`): at the defaults horcon = tprni = smoth, the four rf* are 1 and the biases 0, so an oracle that
# reads one for another would agree with the reference in every test above
@pytest.fixture(scope="module")
def ref_constants():
    import off_default
    return off_default.golden_records()


def _off_default_runs():
    import off_default as od
    return ([("all/" + case, case, {}) for case in od.GOLDEN_STEPS] + [("all/archipelago/" + b, "archipelago", nml) for b, nml in od.BRANCHES.items()])


@pytest.mark.parametrize("run,case,nml", _off_default_runs(), ids=[r[0] for r in _off_default_runs()])
def test_off_default_constants_bit_identical(ref_constants, run, case, nml):
    """every constant moved at once: archipelago after 1, 2, 3, 6, 12 steps, seamount after 1, 3, 6, four namelist branches after 4 --
    all arrays, bdry and every blkcon member"""
    import off_default as od
    want = ref_constants[run]
    assert sorted(want) == list(od.GOLDEN_STEPS[case] if not nml else (4,))
    b = od.off_default_case(case, 65, 49, 21, oracle_finish_initial, **nml)
    ot = OracleTile(b)
    done = 0
    for n in sorted(want):
        ot.run(n - done)
        done = n
        assert not _diff(b, want[n]), f"{run}: step {n}: {_diff(b, want[n])}"
    assert b.rfe == 0.9 and b.tbias == 2.0 and b.ntp == 4 and 0.0 < b.ramp < 1.0


_BASELINES = {}


def _baseline(consts):
    """the oracle after 4 steps of archipelago at the default constants (for an ntp entry: at that entry's nbct), computed once"""
    import off_default as od
    nml = od.baseline_of(consts)
    key = json.dumps(nml, sort_keys=True)
    if key not in _BASELINES:
        a = od.constants_case("archipelago", 65, 49, 21, oracle_finish_initial, nml)
        OracleTile(a).run(4)
        _BASELINES[key] = a
    return _BASELINES[key]


def _single_names():
    import off_default as od
    return list(od.SINGLES)


@pytest.mark.parametrize("name", _single_names())
def test_single_constant_bit_identical_and_live(ref_constants, name):
    """one constant moved alone, 4 steps of archipelago: the reference's bits -- and NOT the bits of the default-constant run in at
    least one prognostic field, without which the entry would test nothing (vmaxl: see below)"""
    import off_default as od
    from extpom_amd.layout import PROGNOSTIC
    consts = od.SINGLES[name]
    (n, want), = ref_constants["single/" + name].items()
    b = od.constants_case("archipelago", 65, 49, 21, oracle_finish_initial, consts)
    OracleTile(b).run(4)
    assert n == 4 and not _diff(b, want), f"{name}: {_diff(b, want)}"
    base = _baseline(consts)
    moved = [f for f in PROGNOSTIC if b.field(f).tobytes() != base.field(f).tobytes()]
    if name == "vmaxl":
        # check_velocity (advance.f:611-641) compares and reports; no array depends on vmaxl.  What it moves is error_status.
        assert not moved and b.error_status == 1 and base.error_status == 0
    else:
        assert moved, f"{name}: the constant leaves every prognostic field as the defaults do"
