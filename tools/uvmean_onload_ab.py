#!/usr/bin/env python3
"""Developer measurement (not the bench contract): the step on ONE tile with the depth-mean correction of u, v applied by the kernels
that load them (the default: no k_int_uvmean in mode_internal) and with POMGPU_UVMEAN_PASS (the pass k_int_uvmean_reg2 in front of
the unchanged kernels), the two taking turns on one live context -- placement moves a kernel more than this change does, so the
comparison stays inside one process.  The timed blocks carry events around the steps only; one more block per side with every kernel
bracketed gives the kernels' own durations: the pass that goes, and what each kernel that now corrects on load grew by.

    python tools/uvmean_onload_ab.py [--workload basin2048] [--steps 10] [--rounds 8] [--tune]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PASS = "k_int_uvmean_reg2"
READERS = ("k_advct_col", "k_coef_eta", "k_advq2_col", "k_profq", "k_bcond6_edges", "k_advt2x2_col", "k_bcond4_edges", "k_advuv_col", "k_profuv_filter_reg2",
           "k_bcondorl3", "k_uv_filter_rim")
KERNELS = (PASS,) + READERS


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
    acc = {"default": [], "UVMEAN_PASS": []}
    dev = {"default": [], "UVMEAN_PASS": []}
    for _ in range(a.rounds):
        for tag in acc:
            g.switch("UVMEAN_PASS", 1 if tag != "default" else None)
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
        g.switch("UVMEAN_PASS", 1 if tag != "default" else None)
        g.run(1)
        g.sync()
        g.prof_begin()
        g.run(a.steps)
        g.sync()
        prof = g.prof_end()
        kern[tag] = {k: {"launches": prof[k][0], "mean_ms": round(prof[k][1] / prof[k][0], 4)} for k in KERNELS if k in prof and prof[k][0]}
    g.switch("UVMEAN_PASS", None)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"workload": desc, "library_build_id": g.L.pomgpu_build_id().decode(), "steps_per_block": a.steps, "rounds": a.rounds, "placement": tuned,
           "wall_ms_per_step": {t: {"min": round(min(v), 3), "median": round(med(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]} for t, v in acc.items()},
           "device_ms_per_step": {t: {"min": round(min(v), 3), "median": round(med(v), 3), "max": round(max(v), 3), "all": [round(x, 3) for x in v]} for t, v in dev.items()},
           "kernels_in_a_fully_profiled_block": kern}
    out["median_saving_ms"] = {"wall": round(med(acc["UVMEAN_PASS"]) - med(acc["default"]), 3), "device": round(med(dev["UVMEAN_PASS"]) - med(dev["default"]), 3)}
    out["every_on_load_block_below_every_pass_block"] = {"wall": max(acc["default"]) < min(acc["UVMEAN_PASS"]), "device": max(dev["default"]) < min(dev["UVMEAN_PASS"])}
    ps, on = kern.get("UVMEAN_PASS", {}), kern.get("default", {})
    if PASS in ps:
        out["k_int_uvmean_ms"] = ps[PASS]["mean_ms"]
        out["growth_ms"] = {k: round(on[k]["mean_ms"] * on[k]["launches"] / a.steps - ps[k]["mean_ms"] * ps[k]["launches"] / a.steps, 4) for k in READERS if k in on and k in ps}
        out["median_device_saving_as_fraction_of_k_int_uvmean"] = round(out["median_saving_ms"]["device"] / ps[PASS]["mean_ms"], 3)
    print(json.dumps(out))
    g.close()


if __name__ == "__main__":
    main()
