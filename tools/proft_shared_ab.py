#!/usr/bin/env python3
"""Developer measurement (not the bench contract): the step on ONE tile with proft of T and S in one lane (the default: k_proft_ts_reg,
kh read once and the matrix's coefficients formed once) and with POMGPU_PROFT_TWIN (the twin: the tracer on blockIdx.z, each half
reading kh and forming the coefficients for itself), the two taking turns on one live context -- placement moves a kernel more than
this change does, so the comparison stays inside one process.  The timed blocks carry events around the steps only; one more block per
side with every kernel bracketed gives the kernels' own durations: k_proft_reg2 under either shape, and its neighbours, which must not move.

    python tools/proft_shared_ab.py [--workload basin2048] [--steps 10] [--rounds 8] [--tune]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROFT = "k_proft_reg2"
NEIGHBOURS = ("k_advt2x2_col", "k_advt2_col", "k_bcond4_edges", "k_ts_update")
KERNELS = (PROFT, "proft_ts_lane") + NEIGHBOURS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="basin2048")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--tune", action="store_true", help="pomgpu_tune_placement before the measurement")
    a = ap.parse_args()
    import bench
    from extpom_amd import dist as pdist
    case, im, jm, kb, desc = bench.WORKLOADS[a.workload]
    st = bench.build_state(a.workload, pdist.tile_for_rank(0, 1, im, jm))
    g = bench.gpu_initialise(st, 0, None)
    g.run(2)
    tuned = g.tune_placement(3, 10) if a.tune else None
    g.run(3)
    g.sync()
    acc = {"default": [], "PROFT_TWIN": []}
    dev = {"default": [], "PROFT_TWIN": []}
    for _ in range(a.rounds):
        for tag in acc:
            g.switch("PROFT_TWIN", 1 if tag != "default" else None)
            g.run(1)
            g.sync()
            g.prof_begin(only="phase_step")                   # the steps as a whole carry events, no kernel does
            t0 = time.perf_counter()
            g.run(a.steps)
            g.sync()
            acc[tag].append((time.perf_counter() - t0) / a.steps * 1e3)
            prof = g.prof_end()
            dev[tag].append(prof["phase_step"][1] / prof["phase_step"][0])
    kern = {}
    for tag in acc:                                           # every kernel bracketed: their own durations, not the step's
        g.switch("PROFT_TWIN", 1 if tag != "default" else None)
        g.run(1)
        g.sync()
        g.prof_begin()
        g.run(a.steps)
        g.sync()
        prof = g.prof_end()
        kern[tag] = {k: {"launches": prof[k][0], "mean_ms": round(prof[k][1] / prof[k][0], 4)} for k in KERNELS if k in prof and prof[k][0]}
    g.switch("PROFT_TWIN", None)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"workload": desc, "library_build_id": g.L.pomgpu_build_id().decode(), "steps_per_block": a.steps, "rounds": a.rounds, "placement": tuned,
           "wall_ms_per_step": {t: {"min": round(min(v), 3), "median": round(med(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]} for t, v in acc.items()},
           "device_ms_per_step": {t: {"min": round(min(v), 3), "median": round(med(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]} for t, v in dev.items()},
           "kernels_in_a_fully_profiled_block": kern}
    out["median_saving_ms"] = {"wall": round(med(acc["PROFT_TWIN"]) - med(acc["default"]), 3), "device": round(med(dev["PROFT_TWIN"]) - med(dev["default"]), 3)}
    out["every_one_lane_block_below_every_twin_block"] = {"wall": max(acc["default"]) < min(acc["PROFT_TWIN"]), "device": max(dev["default"]) < min(dev["PROFT_TWIN"])}
    tw, on = kern.get("PROFT_TWIN", {}), kern.get("default", {})
    if PROFT in tw and PROFT in on:
        out["k_proft_reg2_ms"] = {"twin": tw[PROFT]["mean_ms"], "one_lane": on[PROFT]["mean_ms"], "saving": round(tw[PROFT]["mean_ms"] - on[PROFT]["mean_ms"], 4)}
        out["neighbours_moved_ms"] = {k: round(on[k]["mean_ms"] - tw[k]["mean_ms"], 4) for k in NEIGHBOURS if k in on and k in tw}
    print(json.dumps(out))
    g.close()


if __name__ == "__main__":
    main()
