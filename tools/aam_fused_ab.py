#!/usr/bin/env python3
"""Developer measurement (not the bench contract): the step on ONE tile with aam and aam2d formed inside advct's march (the default:
k_advct_col<8, true>, no k_aam_pair and no k_vint) and with POMGPU_AAM_NOFUSE (k_advct_col + k_aam_pair + k_vint), the two taking turns
on one live context -- placement moves a kernel more than this change does, so the comparison stays inside one process.  The timed
blocks carry events around the steps only; one more block per side with every kernel bracketed gives the kernels' own durations
(k_advq2_col and k_advt2x2_col read aam next, from the spare array every other step: they must not move).

    python tools/aam_fused_ab.py [--workload basin2048] [--steps 10] [--rounds 8] [--tune]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_advct_col", "k_aam_pair", "k_aam", "k_vint", "k_aam_copy", "k_advq2_col", "k_advt2x2_col", "advct_aam_fused")
SW = "AAM_NOFUSE"


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
    acc = {"default": [], SW: []}
    dev = {"default": [], SW: []}
    for _ in range(a.rounds):
        for tag in acc:
            g.switch(SW, 1 if tag != "default" else None)
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
        g.switch(SW, 1 if tag != "default" else None)
        g.run(1)
        g.sync()
        g.prof_begin()
        g.run(a.steps)
        g.sync()
        prof = g.prof_end()
        kern[tag] = {k: {"launches": prof[k][0], "mean_ms": round(prof[k][1] / prof[k][0], 4)} for k in KERNELS if k in prof and prof[k][0]}
    g.switch(SW, None)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"workload": desc, "library_build_id": g.L.pomgpu_build_id().decode(), "steps_per_block": a.steps, "rounds": a.rounds, "placement": tuned,
           "wall_ms_per_step": {t: {"min": round(min(v), 3), "median": round(med(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]} for t, v in acc.items()},
           "device_ms_per_step": {t: {"min": round(min(v), 3), "median": round(med(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]} for t, v in dev.items()},
           "kernels_in_a_fully_profiled_block": kern}
    out["median_saving_ms"] = {"wall": round(med(acc[SW]) - med(acc["default"]), 3), "device": round(med(dev[SW]) - med(dev["default"]), 3)}
    out["every_fused_block_below_every_unfused_block"] = {"wall": max(acc["default"]) < min(acc[SW]), "device": max(dev["default"]) < min(dev[SW])}
    pair, fused = kern.get(SW, {}), kern.get("default", {})
    if "k_advct_col" in pair and "k_advct_col" in fused:
        removed = sum(pair[k]["mean_ms"] for k in ("k_aam_pair", "k_aam", "k_vint") if k in pair)
        out["removed_kernels_ms"] = round(removed, 4)
        out["k_advct_col_growth_ms"] = round(fused["k_advct_col"]["mean_ms"] - pair["k_advct_col"]["mean_ms"], 4)
    print(json.dumps(out))
    g.close()


if __name__ == "__main__":
    main()
