#!/usr/bin/env python3
"""Developer measurement (not the bench contract): what the tide costs at the benchmark size on one GPU.

1. The parent's library (--parent PATH, a libpomgpu.so built from the commit before the tide) and this tree's library with the tide OFF,
   one context each in ONE process, taking turns in blocks of --steps steps: placement and the box move a step more than this change
   may, so the two are compared pair by pair.  The tide-off step must lie within the spread of the parent's own blocks.
2. This tree's library with a tide of eight constituents on all four sides: the step, and k_tide_table's launch.
3. The harmonic analysis at eight constituents beside the time-mean output on the same run: k_harm_accum's and k_mean_accum's time and the
   bytes per second each moves (k_harm_accum: 3 planes read, 51 read and written; k_mean_accum: 9 fields read, 9 accumulators read and written).

    python tools/tide_probe.py --parent /path/to/parent/libpomgpu.so [--workload basin2048] [--steps 10] [--rounds 6]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load_parent(path):
    """the parent's library has none of the tide's entry points, which extpom_amd.lib.load insists on: bind what it exports"""
    import ctypes
    from extpom_amd import lib as L
    lib = ctypes.CDLL(path)
    for name, (res, args) in L._SIGS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    L._cache[path] = lib


def block(g, steps):
    g.prof_begin(only="phase_step")
    g.run(steps)
    g.sync()
    p = g.prof_end()["phase_step"]
    return p[1] / p[0]


def stats(v):
    s = sorted(v)
    return {"min": round(s[0], 3), "median": round(s[len(s) // 2], 3), "max": round(s[-1], 3), "all": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--workload", default="basin2048")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--parent-first", action="store_true", help="make the parent's context before this tree's")
    a = ap.parse_args()
    import bench
    import tide_expect as X
    from extpom_amd import dist as pdist
    case, im, jm, kb, desc = bench.WORKLOADS[a.workload]
    out = {"workload": desc, "steps_per_block": a.steps, "rounds": a.rounds}
    tile = pdist.tile_for_rank(0, 1, im, jm)
    gp = None
    if a.parent:
        load_parent(a.parent)
    if a.parent and a.parent_first:                           # which context is made first decides where its arrays lie: try both orders
        gp = bench.gpu_initialise(bench.build_state(a.workload, tile), 0, None, libpath=a.parent)
    g = bench.gpu_initialise(bench.build_state(a.workload, tile), 0, None)
    out["library_build_id"] = g.L.pomgpu_build_id().decode()
    out["parent_context_made_first"] = bool(a.parent_first)
    g.run(3)
    g.sync()
    if a.parent:
        if gp is None:
            gp = bench.gpu_initialise(bench.build_state(a.workload, tile), 0, None, libpath=a.parent)
        out["parent_build_id"] = gp.L.pomgpu_build_id().decode()
        gp.run(3)
        gp.sync()
        ms = {"parent": [], "tide_off": []}
        for _ in range(a.rounds):
            ms["parent"].append(block(gp, a.steps))
            ms["tide_off"].append(block(g, a.steps))
        gp.close()
        out["device_ms_per_step"] = {k: stats(v) for k, v in ms.items()}
        out["tide_off_median_within_parent_spread"] = min(ms["parent"]) <= stats(ms["tide_off"])["median"] <= max(ms["parent"])
        out["tide_off_minus_parent_median_ms"] = round(stats(ms["tide_off"])["median"] - stats(ms["parent"])["median"], 3)
    off = [block(g, a.steps) for _ in range(2)]
    g.set_tides(omega=X.OMEGA, **X.make_lines(8, im, jm))
    g.run(1)
    on = [block(g, a.steps) for _ in range(a.rounds)]
    out["four_sided_tide_nc8_device_ms_per_step"] = {"off_just_before": stats(off), "on": stats(on)}
    g.set_mean_output(True)
    g.set_harmonic_analysis(True)
    g.run(1)
    g.sync()
    g.prof_begin()
    g.run(a.steps)
    g.sync()
    prof = g.prof_end()
    n2, n3 = g.st.im_local * g.st.jm_local, g.st.im_local * g.st.jm_local * kb
    byt = {"k_harm_accum": (3 + 2 * 51) * n2 * 8, "k_mean_accum": (3 * 3 * n2 + 3 * 6 * n3) * 8, "k_tide_table": int(g.st.isplit) * 8 * 2 * 8}   # isplit substeps x 8 constituents x cos, sin
    out["kernels"] = {k: {"launches": prof[k][0], "mean_ms": round(prof[k][1] / prof[k][0], 4), "bytes": byt[k],
                          "GB_per_s": round(byt[k] / (prof[k][1] / prof[k][0] * 1e-3) / 1e9, 1)} for k in byt if k in prof and prof[k][0]}
    out["analysis_and_mean_on_device_ms_per_step"] = round(prof["phase_step"][1] / prof["phase_step"][0], 3)
    print(json.dumps(out))
    g.close()


if __name__ == "__main__":
    main()
