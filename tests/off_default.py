"""The run constants OFF the values initialize.f:80-168 hard-codes: one place for the values that
tests/golden/make_golden.py `constants`, tests/test_oracle_vs_reference.py, tests/test_kernels_emulated.py,
tests/test_kernels_emulated_tiles.py, tests/test_gpu_off_default_constants.py and tests/gpu_tiles_worker.py share.

Every kernel reads its physics from the scalars of blkcon.  At the defaults horcon = tprni = smoth = 0.1, rfe = rfw = rfn = rfs = 1
and tbias = sbias = 0: a kernel that reads one where it means another, or drops a bias, cannot be told from a right one.  Here every
value differs from its default AND from every other value of the set, so that a swap of any two shows.

A plain module (not a conftest): nothing here changes how the suite is collected or run.
"""
from extpom_amd.cases import make_case

# members of blkcon that make_case takes as keywords (run_constants).  ispadv stays 1: with any other value the host leaves the
# fused / marching / paired external substeps, and those are the ones that must run under these constants.
ALL = dict(tbias=2.0, sbias=1.0, grav=9.81, kappa=0.41, rhoref=1027.0, horcon=0.2, tprni=0.25, umol=2e-5,
           smoth=0.08, alpha=0.225, aam_init=50.0, nbct=2, nbcs=3, ntp=4)
# set AFTER finish_initial, which resets the four rf* to 1 (initialize.f:442-445); lramp is the host's logical beside blkcon
POST = dict(rfe=0.9, rfw=0.8, rfn=0.7, rfs=0.6, lramp=True)
# st.small, set BEFORE finish_initial (q2b = small there); run_constants overwrites a keyword of this name
SMALL = 2.0e-9
FULL = dict(ALL, small=SMALL, **POST)

DEFAULT_NML = dict(dte=6.0, isplit=30)

# One constant (or the smallest group that has an effect) moved alone.  ntp is read by proft under nbc = 2 and 4 only
# (solver.f:1604-1611): its entries carry that nbct, and their default-constant baseline is the run with the same nbct.
SINGLES = {k: {k: v} for k, v in ALL.items() if k != "ntp"}
SINGLES["ntp"] = dict(nbct=2, ntp=4)
SINGLES.update({k: {k: v} for k, v in POST.items()})
SINGLES["small"] = dict(small=SMALL)
SINGLES.update({
    "ispadv2": dict(ispadv=2),
    "ispadv4": dict(ispadv=4),                      # 30 % 4 != 0: the last substeps of a step go without advave
    "nbct1_nbcs2": dict(nbct=1, nbcs=2),
    "nbct3_nbcs4": dict(nbct=3, nbcs=4),
    "nbct2_ntp1": dict(nbct=2, ntp=1),
    "nbct2_ntp3": dict(nbct=2, ntp=3),
    "nbct2_ntp5": dict(nbct=2, ntp=5),
    "nbct4_ntp5": dict(nbct=4, ntp=5),
    "vmaxl": dict(vmaxl=0.05),                      # error_status becomes 1 at step 1 on every side; stepping goes on
    "dte4_isplit24": dict(dte=4.0, isplit=24),
})

# the namelist branches ALL is crossed with
BRANCHES = {"mode2": dict(mode=2), "mode4": dict(mode=4), "npg2_nadv1": dict(npg=2, nadv=1), "nitera2_sw08": dict(nitera=2, sw=0.8)}


def baseline_of(consts):
    """the default-constant run a SINGLES entry must differ from: nothing moved -- but for the ntp entries the same nbct"""
    return dict(nbct=consts["nbct"]) if "ntp" in consts else {}


def _check_distinct():
    from extpom_amd.namelist import DEFAULTS
    for typ in (float, int):                        # a real cannot stand in for an integer member, nor the other way round
        vals = [v for v in FULL.values() if type(v) is typ]
        assert len(set(vals)) == len(vals), "two constants of the off-default set share a value"
    for k, v in FULL.items():
        d = dict(DEFAULTS, small=1.0e-9, rfe=1.0, rfw=1.0, rfn=1.0, rfs=1.0)[k]
        assert v != d, k


_check_distinct()


GOLDEN = "off_default_constants_65x49x21"       # tests/golden/<this>.json, written by `tests/golden/make_golden.py constants`
GOLDEN_STEPS = {"archipelago": (1, 2, 3, 6, 12), "seamount": (1, 3, 6)}


def golden_records():
    """{run: {step: the reference's whole state as oracle.refharness.state_digests}} of the stored file.  Runs: "all/archipelago",
    "all/seamount", "all/archipelago/<branch>" and "single/<entry>".  The file keeps "base" -- the reference after 4 steps of
    archipelago at the DEFAULT constants -- in full; the first record of a run holds what differs from it, a later one what differs
    from the record before."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN + ".json")) as f:
        return expand_records(json.load(f))


def expand_records(doc):
    out = {}
    for name, run in doc["runs"].items():
        cur, out[name] = dict(doc["base"]), {}
        for n in sorted(run, key=int):
            cur.update(run[n])
            out[name][int(n)] = dict(cur)
    return out


def split(consts):
    """(keywords of make_case, small or None, what is set after finish_initial) of a flat dict of constants"""
    nml = {k: v for k, v in consts.items() if k not in POST and k != "small"}
    post = {k: v for k, v in consts.items() if k in POST}
    return nml, consts.get("small"), post


def apply_post(st, post=POST):
    for k, v in post.items():
        setattr(st, k, v)
    return st


def constants_case(case, im, jm, kb, finish, consts, tile=None, **extra):
    """the finished state of `case` with the constants `consts` (a flat dict: members of ALL, POST, `small`, dte, isplit ...);
    finish(st) is the caller's finish_initial (oracle_finish_initial, ref_finish_initial, ...)"""
    nml, small, post = split(consts)
    st = make_case(case, im, jm, kb, tile=tile, **dict(DEFAULT_NML, **dict(nml, **extra)))
    if small is not None:
        st.small = small
    finish(st)
    return apply_post(st, post)


def off_default_case(case, im, jm, kb, finish, tile=None, **extra):
    """the finished state with ALL, SMALL and POST applied; extra: further keywords of make_case (a namelist branch, isplit, ...)"""
    return constants_case(case, im, jm, kb, finish, FULL, tile=tile, **extra)
