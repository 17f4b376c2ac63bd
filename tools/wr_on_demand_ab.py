#!/usr/bin/env python3
"""Developer measurement (not the bench contract): the step on ONE tile with wr left to whoever reads it (the default) and with
POMGPU_WR_NODEFER (realvertvl at the end of every step), the two taking turns on one live context -- placement moves a kernel
more than this change does, so the comparison stays inside one process (tools/tile_probe.py --ab goes through a transport, where
wr is never left pending).

    python tools/wr_on_demand_ab.py [--workload basin2048] [--steps 10] [--rounds 8] [--tune]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    acc = {"default": [], "WR_NODEFER": []}
    dev = {"default": [], "WR_NODEFER": []}
    wr = {}
    for _ in range(a.rounds):
        for tag in acc:
            g.switch("WR_NODEFER", 1 if tag != "default" else None)
            g.run(1)
            g.sync()
            g.prof_begin(only="k_realvertvl_col")              # the steps as a whole (phase_step) and this one kernel carry events
            t0 = time.perf_counter()
            g.run(a.steps)
            g.sync()
            acc[tag].append((time.perf_counter() - t0) / a.steps * 1e3)
            prof = g.prof_end()
            dev[tag].append(prof["phase_step"][1] / prof["phase_step"][0])
            wr[tag] = prof.get("k_realvertvl_col", (0, 0.0))
    g.switch("WR_NODEFER", None)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"workload": desc, "library_build_id": g.L.pomgpu_build_id().decode(), "steps_per_block": a.steps, "rounds": a.rounds, "placement": tuned,
           "wall_ms_per_step": {t: {"min": round(min(v), 3), "median": round(med(v), 3), "all": [round(x, 3) for x in v]} for t, v in acc.items()},
           "device_ms_per_step": {t: {"min": round(min(v), 3), "median": round(med(v), 3), "all": [round(x, 3) for x in v]} for t, v in dev.items()},
           "k_realvertvl_col_last_block": {t: {"launches": n, "mean_ms": round(ms / n, 4) if n else None} for t, (n, ms) in wr.items()}}
    out["median_saving_ms"] = {"wall": round(med(acc["WR_NODEFER"]) - med(acc["default"]), 3), "device": round(med(dev["WR_NODEFER"]) - med(dev["default"]), 3)}
    print(json.dumps(out))
    g.close()


if __name__ == "__main__":
    main()
