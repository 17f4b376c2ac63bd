"""The HIP path with every run constant OFF the value initialize.f:80-168 hard-codes (tests/off_default.py).

All other GPU tests run at horcon = tprni = smoth = 0.1, rfe = rfw = rfn = rfs = 1, tbias = sbias = 0, ntp = 2, ispadv = 1, lramp = .false.:
a kernel that reads one constant where it means another, the wrong Jerlov column, an edge factor of the wrong side, or that drops a bias, is
bit-identical to the reference in all of them.  The CPU chain under these constants is pinned elsewhere (oracle = reference:
tests/test_oracle_vs_reference.py; emulated kernels = oracle: tests/test_kernels_emulated.py); what exists on the device only -- the lane
shifts and LDS slabs, the device reciprocals, the marching and the paired external substep -- is pinned here.  fp64, so every comparison
is bit for bit (DESIGN.md "Parity"); the shapes are the smallest at which each distinct copy of the constant-bearing code runs."""
import ctypes

import numpy as np
import pytest

import off_default as od
from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D
from oracle.refharness import state_digests

pytestmark = pytest.mark.gpu
SCRATCH = {"tps", "fluxua", "fluxva", "zflux"}


def _gpu(st):
    from extpom_amd.model import PomGpu
    return PomGpu(st, device=0)


def _oracle():
    from oracle.pyoracle import OracleTile, oracle_finish_initial
    return OracleTile, oracle_finish_initial


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


def diff(a, b):
    return [n for n in BLK2D + BLK3D if n not in SCRATCH and not same_bits(a.field(n), b.field(n))] + ([] if same_bits(a.bdry, b.bdry) else ["bdry"])


@pytest.fixture(scope="module")
def gold():
    return od.golden_records()


def _reproduces(gold, run, case, consts, **extra):
    """every non-scratch COMMON array and bdry after every stored step hash to what the REFERENCE left there"""
    _, oracle_finish_initial = _oracle()
    st = od.constants_case(case, 65, 49, 21, oracle_finish_initial, consts, **extra)
    g = _gpu(st)
    done = 0
    for step in sorted(gold[run]):
        g.run(step - done)
        done = step
        g.download()
        got, want = state_digests(st), gold[run][step]
        bad = [n for n in BLK2D + BLK3D + ["bdry"] if n not in SCRATCH and got[n] != want[n]]
        assert not bad, f"{run}: step {step}: {bad} differ from the reference"
    g.get_con()
    status = int(st.error_status)
    g.close()
    return st, status


RUNS = [("all/" + case, case, {}) for case in od.GOLDEN_STEPS] + [("all/archipelago/" + b, "archipelago", nml) for b, nml in od.BRANCHES.items()]


@pytest.mark.parametrize("run,case,nml", RUNS, ids=[r[0] for r in RUNS])
def test_gpu_reproduces_reference_digests_off_default(gold, run, case, nml):
    """every constant moved at once: archipelago after 1, 2, 3, 6, 12 steps, seamount after 1, 3, 6, four namelist branches after 4"""
    assert sorted(gold[run]) == list(od.GOLDEN_STEPS[case] if not nml else (4,))
    st, status = _reproduces(gold, run, case, od.FULL, **nml)
    assert status == 0 and 0.0 < st.ramp < 1.0


@pytest.mark.parametrize("name", list(od.SINGLES))
def test_gpu_reproduces_reference_digests_single_constant(gold, name):
    """one constant moved alone, 4 steps of archipelago: a difference names the constant.  ispadv = 2, 4: the host's iext % ispadv logic and
    the non-fused substep as the product path; vmaxl: check_velocity raises error_status at step 1, as the reference does, and stepping goes on"""
    run = "single/" + name
    st, status = _reproduces(gold, run, "archipelago", od.SINGLES[name])
    assert state_digests(st)["con.error_status"] == gold[run][4]["con.error_status"]
    assert status == (1 if name == "vmaxl" else 0)


def _against_oracle(a, steps=3, prof=False):
    OracleTile, _ = _oracle()
    b = a.copy()
    OracleTile(a).run(steps)
    g = _gpu(b)
    if prof:
        g.prof_begin()
    g.run(steps)
    p = g.prof_end() if prof else None
    g.download()
    g.close()
    assert not diff(a, b), diff(a, b)
    return p


@pytest.mark.parametrize("im,jm,kb", [(66, 50, 21), (128, 12, 21), (64, 48, 50), (64, 48, 70)])
def test_off_default_constants_match_oracle(im, jm, kb):
    """66x50, 128x12: the two-columns-per-lane kernels; kb = 50: the <50> register instantiations; kb = 70: the work-vector column
    kernels, which carry the second copy of the Jerlov table"""
    _, oracle_finish_initial = _oracle()
    _against_oracle(od.off_default_case("archipelago", im, jm, kb, oracle_finish_initial))


def _switch_sets():
    from test_gpu_parity import SWITCH_SETS
    return SWITCH_SETS


@pytest.mark.parametrize("switches", _switch_sets())
def test_off_default_constants_general_kernels(monkeypatch, switches):
    """the general kernels behind the fast paths (the six switch sets of tests/test_gpu_parity.py) at 65x49x21"""
    _, oracle_finish_initial = _oracle()
    for v in switches:
        monkeypatch.setenv(v, "1")
    _against_oracle(od.off_default_case("archipelago", 65, 49, 21, oracle_finish_initial))


def test_off_default_constants_marching_external_substep(monkeypatch):
    """k_ext_march forced onto a small grid with a ragged last segment: its own statement of the filter, alpha and the boundary radiation"""
    _, oracle_finish_initial = _oracle()
    monkeypatch.setenv("POMGPU_EXT_MARCH", "1")
    monkeypatch.setenv("POMGPU_EXT_ROWS", "6")
    _against_oracle(od.off_default_case("archipelago", 200, 93, 11, oracle_finish_initial, isplit=10))


@pytest.mark.parametrize("im,jm,kb,isplit,rows2", [(200, 93, 11, 10, "6"), (130, 97, 9, 7, "5")])
def test_off_default_constants_two_external_substeps_per_pass(monkeypatch, im, jm, kb, isplit, rows2):
    """k_ext_march2 (two substeps per pass), even and odd isplit.  The path is refused when ispadv != 1: the off-default set keeps ispadv = 1"""
    _, oracle_finish_initial = _oracle()
    monkeypatch.setenv("POMGPU_EXT_PAIR", "1")
    monkeypatch.setenv("POMGPU_EXT_ROWS2", rows2)
    prof = _against_oracle(od.off_default_case("archipelago", im, jm, kb, oracle_finish_initial, isplit=isplit), prof=True)
    assert prof.get("k_ext_pair", (0, 0))[0] == 3 * (isplit // 2), prof.keys()     # the path under test did run


LIVE_CON = dict(grav=9.81, kappa=0.41, rhoref=1027.0, horcon=0.2, tprni=0.25, umol=2e-5, smoth=0.08, alpha=0.225, nbct=4, nbcs=3, ntp=5,
                ispadv=3, tbias=2.0, sbias=1.0, rfe=0.9, rfw=0.8, rfn=0.7, rfs=0.6)


def test_constants_changed_on_a_live_context():
    """pomgpu_set_con moves the constants after two steps at the defaults (nbct = 2): the kernels' copy and the host's decisions (nbct, nbcs,
    ispadv) follow at once; three more steps, bit for bit throughout"""
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("archipelago", 65, 49, 21, dte=6.0, isplit=30, nbct=2)
    oracle_finish_initial(a)
    b = a.copy()
    ot, g = OracleTile(a), _gpu(b)
    for n in range(1, 6):
        if n == 3:
            g.set_con(**LIVE_CON)
            for k, v in LIVE_CON.items():
                setattr(a, k, v)
        ot.run(1)
        g.run(1)
        g.download()
        assert not diff(a, b), f"step {n}: {diff(a, b)}"
    g.close()
    assert b.ntp == 5 and b.ispadv == 3 and b.rfn == 0.7


_WARM = []


def _warm():
    """the off-default state of archipelago after three steps of the oracle, computed once"""
    if not _WARM:
        OracleTile, oracle_finish_initial = _oracle()
        a = od.off_default_case("archipelago", 65, 49, 21, oracle_finish_initial)
        OracleTile(a).run(3)
        a.iint, a.iext = 4, 7
        _WARM.append(a)
    return _WARM[0].copy()


def _routines():
    from test_gpu_parity import ROUTINES_ARCHIPELAGO, _rid
    return ROUTINES_ARCHIPELAGO, [_rid(r) for r in ROUTINES_ARCHIPELAGO]


@pytest.mark.parametrize("name,fields,ints", _routines()[0], ids=_routines()[1])
def test_each_routine_bit_identical_to_oracle_off_default(name, fields, ints):
    """each routine alone on the warm off-default state: where a run above differs, this names the routine"""
    OracleTile, _ = _oracle()
    a = _warm()
    b = a.copy()
    ot = OracleTile(a)
    ot.call(name, *[ot.a3(f) for f in fields], *[ctypes.c_int(i) for i in ints])
    g = _gpu(b)
    g.call(name, *fields, *ints)
    g.download()
    g.close()
    assert not diff(a, b), f"{name}: {diff(a, b)}"
