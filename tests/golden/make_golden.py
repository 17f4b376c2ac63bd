"""Generates tests/golden/seamount_65x49x21.json (+ .npz planes) and tests/golden/kb50_256x192x50.json by running the REFERENCE itself
(oracle/_ref/libpomref_65x49x21.so, built from the unmodified sources by oracle/build_ref.sh) on
the inputs of extpom_amd.cases.  Run from the repo root in a container that has /root/reference:

    oracle/build_ref.sh 65 49 21 && oracle/build_ref.sh 256 192 50 && python tests/golden/make_golden.py [kb50 | kb50long NAME | forced | refcheck | archipelago | constants]

The fixture holds, per configuration and checkpoint step, the SHA-256 of every restart-list field
(the prognostic state, reference io_pnetcdf.F:1724-1886) exactly as the reference left it in its
COMMON blocks, and float64 planes of a few fields for tolerance-based (GPU) comparisons.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from extpom_amd.cases import make_case  # noqa: E402
from extpom_amd.layout import RESTART_2D, RESTART_3D  # noqa: E402
from oracle.refharness import RefLib, ref_finish_initial  # noqa: E402

IM, JM, KB = 65, 49, 21
CONFIGS = {
    # name: (case, namelist overrides, checkpoints)
    "seamount_default": ("seamount", dict(dte=6.0, isplit=30), [1, 2, 3, 10, 100]),
    "seamount_nadv1": ("seamount", dict(dte=6.0, isplit=30, nadv=1), [3, 20]),
    "seamount_nitera2": ("seamount", dict(dte=6.0, isplit=30, nitera=2), [3, 20]),
    "seamount_mode2": ("seamount", dict(dte=6.0, isplit=30, mode=2), [3, 20]),
    "seamount_mode4": ("seamount", dict(dte=6.0, isplit=30, mode=4), [3, 20]),
    "seamount_nbct2": ("seamount", dict(dte=6.0, isplit=30, nbct=2), [3, 10]),
    "seamount_nbc3": ("seamount", dict(dte=6.0, isplit=30, nbct=3, nbcs=3), [3, 20]),
    "island_default": ("island", dict(dte=6.0, isplit=30), [3, 40]),
    "basin_default": ("basin", dict(dte=6.0, isplit=30), [3, 40]),
    "basin_alpha": ("basin", dict(dte=6.0, isplit=10, alpha=0.225), [3, 20]),
    "seamount_npg2": ("seamount", dict(dte=6.0, isplit=30, npg=2), [3, 20]),      # baropg_mcc
    "island_npg2": ("island", dict(dte=6.0, isplit=30, npg=2), [3, 20]),
}
PLANES = {"seamount_default": [10, 100], "island_default": [40], "basin_default": [40]}
PLANE_FIELDS = ["el", "et", "ua", "va", "u", "v", "t", "s", "q2", "km", "rho", "w"]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


# kb = 50: the level count of the benchmarked grid (2048x1536x50), i.e. the <50> instantiations of the register-resident
# column kernels; reference build oracle/_ref/libpomref_256x192x50.so (oracle/build_ref.sh 256 192 50)
CONFIGS_KB50 = {
    "basin50_default": ("basin", dict(dte=6.0, isplit=30), [1, 3]),
    "basin50_nadv1": ("basin", dict(dte=6.0, isplit=30, nadv=1), [3]),
    "basin50_npg2": ("basin", dict(dte=6.0, isplit=30, npg=2), [3]),
    "seamount50_default": ("seamount", dict(dte=6.0, isplit=30), [3]),
}


# north_star's bar -- 1000 internal steps -- at the benchmark's level count: checkpoints 100 / 500 / 1000 of the reference
# itself at 256x192x50 (about ten minutes of one core per configuration; `kb50long NAME` writes kb50_1000steps_NAME.json)
CONFIGS_KB50_LONG = {
    "basin50_default": ("basin", dict(dte=6.0, isplit=30), [100, 500, 1000]),
    "seamount50_default": ("seamount", dict(dte=6.0, isplit=30), [100, 500, 1000]),
}


# One configuration stepped by the reference's OWN `advance` (advance.f:6-59) instead of the harness's restatement of its
# sequence: surface_forcing and lateral_bc run as the reference calls them (their PnetCDF readers are the input hooks of
# oracle/ref_traps.c, fed the records of extpom_amd.cases), print_section / write_output / write_restart stay silent
# because iprint and irestart lie beyond the run (prtd1 = 0.5 d -> iprint = 120 steps at dti = 360 s).
FORCED = ("seamount", dict(dte=6.0, isplit=60, days=1.0, prtd1=0.5), [1, 2, 10, 11, 30, 31])


def generate_forced():
    from extpom_amd.cases import make_forcing_records, make_lateral_records
    case, nml, checkpoints = FORCED
    st = make_case(case, 65, 49, 21, **nml)
    ref_finish_initial(st)
    make_forcing_records(st, 4)
    make_lateral_records(st, 8)
    lib = RefLib(65, 49, 21)
    lib.mpi_init()
    lib.put(st)
    assert int(lib.con["iprint"][0]) > max(checkpoints) and int(lib.con["irestart"][0]) > max(checkpoints)
    cfg = {"case": case, "nml": nml, "forcing_records": 4, "lateral_records": 8, "steps": {}}
    for n in range(1, max(checkpoints) + 1):
        lib.con["iint"][0] = n
        lib.call("advance")                      # the reference's own subroutine
        if n in checkpoints:
            lib.get(st)
            cfg["steps"][str(n)] = {f: digest(st.field(f)) for f in RESTART_2D + RESTART_3D}
            cfg["steps"][str(n)]["bdry"] = digest(st.bdry)
    assert int(lib.con["error_status"][0]) == 0
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "forced_advance_65x49x21.json"), "w") as f:
        json.dump({"grid": [65, 49, 21], "fields": RESTART_2D + RESTART_3D, "config": cfg}, f, indent=1, sort_keys=True)
    print("forced_advance done", flush=True)


# tests/test_oracle_vs_reference.py: the reference's WHOLE state (every COMMON array, bdry, blkcon; oracle.refharness.state_digests)
# after every step and after each hot-path routine on its own, so that the oracle is held to it where oracle/_ref cannot be built.
# A record after the first of a sequence holds only the arrays whose digest changed (tests/test_oracle_vs_reference.py rebuilds it).
REFCHECK_FULL_STATE = [("seamount", dict(dte=6.0, isplit=30)), ("island", dict(dte=6.0, isplit=30, nadv=1)),
                       ("basin", dict(dte=6.0, isplit=10, nitera=2)), ("island", dict(dte=6.0, isplit=30, npg=2))]
REFCHECK_FORCING_STEPS = (1, 2, 19, 20, 21, 40, 41, 59, 60, 61, 62)


def refcheck_key(case, nml):
    return json.dumps([case, nml], sort_keys=True)


def _delta(prev, cur):
    return {k: v for k, v in cur.items() if prev.get(k) != v}


def _refcheck_full_state(case, nml):
    """every COMMON array, bdry and blkcon of the reference after each of 12 steps"""
    from oracle.refharness import state_digests
    a = make_case(case, 65, 49, 21, **nml)
    ref_finish_initial(a)
    prev = state_digests(a)
    rec = {"init": prev, "steps": {}}
    lib = RefLib(65, 49, 21)
    lib.put(a)
    for n in range(1, 13):
        lib.con["iint"][0] = n
        lib.advance()
        lib.get(a)
        cur = state_digests(a)
        rec["steps"][str(n)] = _delta(prev, cur)
        prev = cur
    return rec


def _refcheck_each_routine(case):
    """each routine on its own, from the state after three steps (all branches live)"""
    import ctypes
    from oracle.refharness import state_digests
    a = make_case(case, 65, 49, 21, dte=6.0, isplit=30)
    ref_finish_initial(a)
    lib = RefLib(65, 49, 21)
    lib.put(a)
    for n in range(1, 4):
        lib.con["iint"][0] = n
        lib.advance()
    lib.get(a)
    a.iint = 4
    a.iext = 7
    warm = state_digests(a)
    calls = {}

    def ref_call(label, name, args=()):
        x = a.copy()
        lib.put(x)
        lib.call(name, *args(lib) if callable(args) else args)
        lib.get(x)
        calls[label] = _delta(warm, state_digests(x))

    i = lambda v: ctypes.byref(ctypes.c_int(v))
    for name in ("advave", "advct", "advu", "advv", "baropg", "baropg_mcc", "profq", "profu", "profv", "vertvl", "realvertvl",
                 "lateral_viscosity", "mode_interaction", "mode_external", "mode_internal", "check_velocity"):
        ref_call(name, name)
    ref_call("advq", "advq", lambda l: (l.f3("q2b"), l.f3("q2"), l.f3("uf")))
    for r in ("advt1", "advt2"):
        ref_call(r, r, lambda l: (l.f3("tb"), l.f3("t"), l.f3("tclim"), l.f3("uf")))
    ref_call("dens", "dens", lambda l: (l.f3("s"), l.f3("t"), l.f3("rho")))
    for nbc in (1, 2, 3, 4):
        ref_call(f"proft/{nbc}", "proft", lambda l: (l.f3("uf"), l.f2("wtsurf"), l.f2("tsurf"), i(nbc)))
    for idx in (1, 2, 4, 5, 6):
        ref_call(f"bcond/{idx}", "bcond", (i(idx),))
    for idx in (3, 5):
        ref_call(f"bcondorl/{idx}", "bcondorl", (i(idx),))
    return {"warm": warm, "calls": calls}


# The fourth case (extpom_amd.cases: archipelago -- curved grid, interior land, both signs on the open edges, every forcing field
# live), in files of its own: `make_golden.py archipelago` writes oracle_vs_reference_archipelago_65x49x21.json (refcheck style),
# archipelago_65x49x21.json and archipelago_256x192x50.json (restart-list digests).  The files above are not touched by it.
ARCH = dict(dte=6.0, isplit=30)
REFCHECK_ARCHIPELAGO = [dict(ARCH), dict(ARCH, nadv=1), dict(ARCH, nitera=2), dict(ARCH, npg=2), dict(ARCH, mode=2)]
CONFIGS_ARCHIPELAGO = {
    "archipelago_default": ("archipelago", dict(ARCH), [1, 2, 3, 10, 100]),
    "archipelago_nadv1": ("archipelago", dict(ARCH, nadv=1), [3, 20]),
    "archipelago_nitera2": ("archipelago", dict(ARCH, nitera=2), [3, 20]),
    "archipelago_npg2": ("archipelago", dict(ARCH, npg=2), [3, 20]),
    "archipelago_mode2": ("archipelago", dict(ARCH, mode=2), [3, 20]),
    "archipelago_mode4": ("archipelago", dict(ARCH, mode=4), [3, 20]),
    "archipelago_nbct2": ("archipelago", dict(ARCH, nbct=2), [3, 20]),
    "archipelago_nbc3": ("archipelago", dict(ARCH, nbct=3, nbcs=3), [3, 20]),
}
CONFIGS_ARCHIPELAGO_KB50 = {
    "archipelago50_default": ("archipelago", dict(ARCH), [1, 3]),
    "archipelago50_npg2": ("archipelago", dict(ARCH, npg=2), [1, 3]),
}


def generate_archipelago():
    out = {"grid": [65, 49, 21], "full_state": {}}
    for nml in REFCHECK_ARCHIPELAGO:
        out["full_state"][refcheck_key("archipelago", nml)] = _refcheck_full_state("archipelago", nml)
    out["each_routine"] = _refcheck_each_routine("archipelago")
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "oracle_vs_reference_archipelago_65x49x21.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("archipelago refcheck done", flush=True)
    generate(65, 49, 21, CONFIGS_ARCHIPELAGO, {}, "archipelago_65x49x21")
    generate(256, 192, 50, CONFIGS_ARCHIPELAGO_KB50, {}, "archipelago_256x192x50")


# The run constants off their defaults (tests/off_default.py): `make_golden.py constants` writes off_default_constants_65x49x21.json,
# state_digests of the reference's WHOLE state (every COMMON array, bdry, blkcon) under the full off-default set -- archipelago after
# steps 1, 2, 3, 6, 12, seamount after 1, 3, 6, the set crossed with four namelist branches after 4 -- and, after 4 steps of
# archipelago, under every entry of SINGLES.  "base" is the reference's state after 4 steps at the DEFAULT constants; the first record
# of every run holds what differs from it and a later record what differs from the one before (off_default.expand_records rebuilds them).
def generate_constants():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import off_default as od
    from oracle.refharness import state_digests

    def run(case, consts, steps, **extra):
        a = od.constants_case(case, 65, 49, 21, ref_finish_initial, consts, **extra)
        lib = RefLib(65, 49, 21)
        lib.put(a)
        rec = {}
        for n in range(1, max(steps) + 1):
            lib.con["iint"][0] = n
            lib.advance()
            if n in steps:
                lib.get(a)
                rec[n] = state_digests(a)
        return rec

    base = run("archipelago", {}, (4,))[4]
    runs = {}
    for case, steps in od.GOLDEN_STEPS.items():
        runs["all/" + case] = run(case, od.FULL, steps)
    for name, nml in od.BRANCHES.items():
        runs["all/archipelago/" + name] = run("archipelago", od.FULL, (4,), **nml)
    for name, consts in od.SINGLES.items():
        runs["single/" + name] = run("archipelago", consts, (4,))
        print(name, "done", flush=True)
    out = {"grid": [65, 49, 21], "base": base, "runs": {}}
    for name, rec in runs.items():
        prev, out["runs"][name] = base, {}
        for n in sorted(rec):
            out["runs"][name][str(n)] = _delta(prev, rec[n])
            prev = rec[n]
    assert od.expand_records(out) == runs
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, od.GOLDEN + ".json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True, separators=(",", ":"))
    print("constants done", flush=True)


def generate_refcheck():
    import ctypes
    from extpom_amd.cases import make_forcing_records, make_lateral_records
    from oracle.refharness import state_digests
    out = {"grid": [65, 49, 21], "full_state": {}}
    for case, nml in REFCHECK_FULL_STATE:
        out["full_state"][refcheck_key(case, nml)] = _refcheck_full_state(case, nml)
    out["each_routine"] = _refcheck_each_routine("seamount")

    # domain_stats (the SUM intrinsic) after five steps of the island case
    a = make_case("island", 65, 49, 21, dte=6.0, isplit=30)
    ref_finish_initial(a)
    lib = RefLib(65, 49, 21)
    lib.put(a)
    for n in range(1, 6):
        lib.con["iint"][0] = n
        lib.advance()
    lib.get(a)
    lib.mpi_init()
    vals = [ctypes.c_double() for _ in range(8)]
    lib.call("domain_stats", *[ctypes.byref(v) for v in vals])
    out["domain_stats"] = {"state": state_digests(a), "values": [v.value.hex() for v in vals]}

    # forcing records changing inside the run
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30, days=0.4)
    ref_finish_initial(a)
    make_forcing_records(a, 4)
    make_lateral_records(a, 5)
    prev = state_digests(a)
    rec = {"init": prev, "steps": {}}
    lib = RefLib(65, 49, 21)
    lib.put(a)
    for n in range(1, max(REFCHECK_FORCING_STEPS) + 1):
        lib.con["iint"][0] = n
        lib.advance()
        if n in REFCHECK_FORCING_STEPS:
            lib.get(a)
            cur = state_digests(a)
            rec["steps"][str(n)] = _delta(prev, cur)
            prev = cur
    out["forcing"] = rec

    # lramp = .true.
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30)
    a.lramp = True
    ref_finish_initial(a)
    init = state_digests(a)
    lib = RefLib(65, 49, 21)
    lib.put(a)
    for n in range(1, 7):
        lib.con["iint"][0] = n
        lib.advance()
    lib.get(a)
    out["ramped"] = {"init": init, "steps": {"6": _delta(init, state_digests(a))}}

    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "oracle_vs_reference_65x49x21.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("refcheck done", flush=True)


def main():
    if "constants" in sys.argv[1:]:
        return generate_constants()
    if "archipelago" in sys.argv[1:]:
        return generate_archipelago()
    if "refcheck" in sys.argv[1:]:
        return generate_refcheck()
    if "forced" in sys.argv[1:]:
        return generate_forced()
    if "kb50long" in sys.argv[1:]:
        name = sys.argv[sys.argv.index("kb50long") + 1]
        return generate(256, 192, 50, {name: CONFIGS_KB50_LONG[name]}, {}, "kb50_1000steps_" + name)
    if "kb50" not in sys.argv[1:]:
        generate(65, 49, 21, CONFIGS, PLANES, "seamount_65x49x21")
    generate(256, 192, 50, CONFIGS_KB50, {}, "kb50_256x192x50")


def generate(IM, JM, KB, CONFIGS, PLANES, stem):
    out = {"grid": [IM, JM, KB], "fields": RESTART_2D + RESTART_3D, "configs": {}}
    planes = {}
    for name, (case, nml, checkpoints) in CONFIGS.items():
        st = make_case(case, IM, JM, KB, **nml)
        ref_finish_initial(st)
        cfg = {"case": case, "nml": nml, "init": {f: digest(st.field(f)) for f in RESTART_2D + RESTART_3D},
               "steps": {}}
        lib = RefLib(IM, JM, KB)
        lib.put(st)
        for n in range(1, max(checkpoints) + 1):
            lib.con["iint"][0] = n
            lib.advance()
            if n in checkpoints:
                lib.get(st)
                cfg["steps"][str(n)] = {f: digest(st.field(f)) for f in RESTART_2D + RESTART_3D}
                if n in PLANES.get(name, []):
                    for f in PLANE_FIELDS:
                        a = st.field(f)
                        planes[f"{name}/{n}/{f}"] = (a if a.ndim == 2 else a[[0, KB // 2, KB - 2]]).copy()
        out["configs"][name] = cfg
        print(name, "done", flush=True)
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, stem + ".json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    if planes:
        np.savez_compressed(os.path.join(here, stem + "_planes.npz"), **planes)


if __name__ == "__main__":
    import threading
    threading.stack_size(1 << 30)       # the reference's automatic (im,jm,kb) arrays live on the caller's stack
    t = threading.Thread(target=main)
    t.start()
    t.join()
