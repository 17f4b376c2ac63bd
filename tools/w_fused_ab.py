#!/usr/bin/env python3
"""Developer measurement (not the bench contract): the step on ONE tile with w formed inside the q2 / q2l advection march (the default:
k_advq_col<2, true> under the profile name k_advq2_col, no k_vertvl in mode_internal) and with POMGPU_W_NOFUSE (the pair k_vertvl +
k_advq2_col), the two taking turns on one live context -- placement moves a kernel more than this change does, so the comparison
stays inside one process.  The timed blocks carry events around the steps only; one more block per side with every kernel bracketed
gives the kernels' own durations (k_advt2x2_col and k_advuv_col read w next: they must not move).

    python tools/w_fused_ab.py [--workload basin2048] [--steps 10] [--rounds 8] [--tune]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_vertvl", "k_advq2_col", "k_advt2x2_col", "k_advuv_col")


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
    acc = {"default": [], "W_NOFUSE": []}
    dev = {"default": [], "W_NOFUSE": []}
    for _ in range(a.rounds):
        for tag in acc:
            g.switch("W_NOFUSE", 1 if tag != "default" else None)
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
        g.switch("W_NOFUSE", 1 if tag != "default" else None)
        g.run(1)
        g.sync()
        g.prof_begin()
        g.run(a.steps)
        g.sync()
        prof = g.prof_end()
        kern[tag] = {k: {"launches": prof[k][0], "mean_ms": round(prof[k][1] / prof[k][0], 4)} for k in KERNELS if k in prof and prof[k][0]}
    g.switch("W_NOFUSE", None)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"workload": desc, "library_build_id": g.L.pomgpu_build_id().decode(), "steps_per_block": a.steps, "rounds": a.rounds, "placement": tuned,
           "wall_ms_per_step": {t: {"min": round(min(v), 3), "median": round(med(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]} for t, v in acc.items()},
           "device_ms_per_step": {t: {"min": round(min(v), 3), "median": round(med(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]} for t, v in dev.items()},
           "kernels_in_a_fully_profiled_block": kern}
    out["median_saving_ms"] = {"wall": round(med(acc["W_NOFUSE"]) - med(acc["default"]), 3), "device": round(med(dev["W_NOFUSE"]) - med(dev["default"]), 3)}
    out["every_fused_block_below_every_unfused_block"] = {"wall": max(acc["default"]) < min(acc["W_NOFUSE"]), "device": max(dev["default"]) < min(dev["W_NOFUSE"])}
    pair, fused = kern.get("W_NOFUSE", {}), kern.get("default", {})
    if "k_vertvl" in pair and "k_advq2_col" in pair and "k_advq2_col" in fused:
        grow = fused["k_advq2_col"]["mean_ms"] - pair["k_advq2_col"]["mean_ms"]
        out["k_vertvl_ms"] = pair["k_vertvl"]["mean_ms"]
        out["k_advq2_col_growth_ms"] = round(grow, 4)
        out["median_device_saving_as_fraction_of_k_vertvl"] = round(out["median_saving_ms"]["device"] / pair["k_vertvl"]["mean_ms"], 3)
    print(json.dumps(out))
    g.close()


if __name__ == "__main__":
    main()
