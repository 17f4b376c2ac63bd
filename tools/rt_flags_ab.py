#!/usr/bin/env python3
"""Developer measurement (not the bench contract): the step on ONE tile with the round trips through tclim, sclim (k_ts_update) and rmean
(k_profq) read only where they change bits (the default: k_advt2_col's words, k_baropg_rs's column plane) and with POMGPU_RT_LOAD (both
consumers read their climatology whole, as before), the two taking turns on one live context -- placement moves a kernel more than this
change does, so the comparison stays inside one process.  The timed blocks carry events around the steps only; one more block per side
with every kernel bracketed gives the kernels' own durations: the two consumers, the two producers (which form the flags under either
setting of the switch: it is read where the consumers are launched), and from the RT_LOAD side's rates the saving the bytes predict.

    python tools/rt_flags_ab.py [--workload basin2048] [--steps 10] [--rounds 8] [--tune]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SW = "RT_LOAD"
CONSUMERS = {"k_ts_update": 17, "k_profq": 21}                # array passes of a launch under RT_LOAD (k_profq: an unobserved step's, l and dtef not stored)
PRODUCERS = ("k_advt2x2_col", "k_baropg")
KERNELS = tuple(CONSUMERS) + PRODUCERS + ("ts_rt_flags", "profq_rm_flags")


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
    out["every_flag_block_below_every_RT_LOAD_block"] = {"wall": max(acc["default"]) < min(acc[SW]), "device": max(dev["default"]) < min(dev[SW])}
    # the prediction from bytes, at the rates the RT_LOAD side's kernels ran at in this job: a launch that moves P passes in t ms and is
    # spared p of them saves t * p / P.  k_ts_update: tclim, sclim at levels 1..kbm1 of kb; k_profq: rmean, one pass
    on, off = kern.get("default", {}), kern.get(SW, {})
    spared = {"k_ts_update": 2. * (kb - 1) / kb, "k_profq": 1.}
    if all(k in off for k in CONSUMERS):
        pred = {k: round(off[k]["mean_ms"] * spared[k] / CONSUMERS[k], 4) for k in CONSUMERS}
        out["predicted_saving_ms"] = dict(pred, total=round(sum(pred.values()), 4))
        out["kernel_saving_ms"] = {k: round(off[k]["mean_ms"] - on[k]["mean_ms"], 4) for k in CONSUMERS if k in on}
        out["producers_moved_ms"] = {k: round(on[k]["mean_ms"] - off[k]["mean_ms"], 4) for k in PRODUCERS if k in on and k in off}
        out["median_saving_at_least_half_of_predicted"] = {"device": out["median_saving_ms"]["device"] >= .5 * sum(pred.values()),
                                                            "wall": out["median_saving_ms"]["wall"] >= .5 * sum(pred.values())}
    print(json.dumps(out))
    g.close()


if __name__ == "__main__":
    main()
