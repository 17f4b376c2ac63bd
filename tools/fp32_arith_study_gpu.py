"""BASELINE configs[4] with fp32 ARITHMETIC: three builds of the same sources side by side on the GPU --
libpomgpu.so (fp64, the product), libpomgpu_f32.so (-DPOMGPU_STORE_F32: 3-D arrays stored as fp32, every operation fp64) and
libpomgpu_f32a.so (-DPOMGPU_STORE_F32 -DPOMGPU_COMPUTE_F32: the same storage, the stencil kernels of the internal mode computing
in fp32 as well; pomgpu_internal.hpp).  Sibling of tools/fp32_study_gpu.py, which compares the first two.
  part A (tolerance): seamount 65x49x21, basin 256x192x50 and seamount 256x192x50 stepped by the three builds from one state;
                      after n internal steps the largest difference of every prognostic field to the fp64 run, relative to the
                      field's largest magnitude there
  part B (speed):     2048x1536x50, one context per build, interleaved in one process (R rounds of one profiled step each):
                      min ms per kernel, internal mode, fraction of the HBM peak on 4-byte values
  part C (tolerance on the config's own grid): 2048x1536x50, the three builds in one process (60 + 30 + 30 GB of the 288), after
                      1, 10, 100 internal steps
usage: python tools/fp32_arith_study_gpu.py [--skip-small] [--skip-speed] [--skip-full] [--rounds R] [--out DIR]
   writes DIR/fp32_arith_drift_small.json, fp32_arith_kernel_ms_basin2048.json, fp32_arith_drift_basin2048.json (default DIR: profiles/)"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
from extpom_amd import dist as pdist, lib as L
from extpom_amd.cases import make_case
from extpom_amd.layout import P2, P3, PROGNOSTIC
from extpom_amd.model import PomGpu, gpu_finish_initial

BUILDS = (("fp64", None), ("fp32-storage", L.LIBPATH_F32), ("fp32-arith", L.LIBPATH_F32A))
HBM_PEAK_GBPS = bench.HBM_PEAK_GBS   # bench.py's roofline: the HBM peak and the algorithmic 3-D passes of one internal step
PASSES = bench.P_STEP


def rel(x, y):
    return float(np.abs(x - y).max() / max(np.abs(x).max(), 1e-300))


def drift_small(case, dims, steps):
    """the three builds from one state; returns {build: {step: {field: rel}}} for the two fp32 builds"""
    a = make_case(case, *dims, dte=6.0, isplit=30)
    gpu_finish_initial(a, device=0)
    sts = [a] + [a.copy() for _ in BUILDS[1:]]
    gs = [PomGpu(st, device=0, libpath=lp) for st, (_, lp) in zip(sts, BUILDS)]
    out, done = {t: {} for t, _ in BUILDS[1:]}, 0
    for n in steps:
        for g in gs:
            g.run(n - done)
        done = n
        for g in gs:
            g.download()
        for (t, _), st in zip(BUILDS[1:], sts[1:]):
            row = {f: rel(a.field(f), st.field(f)) for f in PROGNOSTIC}
            row["error_status"] = int(st.error_status)
            row["finite"] = bool(all(np.isfinite(st.field(f)).all() for f in PROGNOSTIC))
            out[t][str(n)] = row
            print(f"{case} {dims} {t:13s} step {n:4d}: " + "  ".join(f"{f}={row[f]:.2e}" for f in PROGNOSTIC), flush=True)
    for g in gs:
        g.close()
    return out


def full_size_drift(steps_list, workload="basin2048", builds=BUILDS):
    """the builds (fp64 first) from one initial state of the bench grid; the two fp32 builds share one host state for the compared
    fields (fetched and compared one after the other), so the host holds two copies of the grid, not three"""
    cs, im, jm, kb, desc = bench.WORKLOADS[workload]
    a = bench.build_state(workload, pdist.tile_for_rank(0, 1, im, jm))
    g0 = bench.gpu_initialise(a, 0, None); g0.close()
    b = a.copy()
    g64 = PomGpu(a, device=0)
    g32 = [(t, PomGpu(b, device=0, libpath=lp)) for t, lp in builds[1:]]

    def fetch(g, st):
        for f in PROGNOSTIC:
            dst = ctypes.c_void_p(st.field(f).ctypes.data)
            g._chk((g.L.pomgpu_download_3d if f in P3 else g.L.pomgpu_download_2d)(g.h, (P3 if f in P3 else P2)[f], dst), "download " + f)
        g.get_con()
        return int(st.error_status)
    rows, done = {t: {} for t, _ in builds[1:]}, 0
    for n in steps_list:
        g64.run(n - done)
        for _, g in g32:
            g.run(n - done)
        done = n
        e64 = fetch(g64, a)
        for t, g in g32:
            e = fetch(g, b)
            rows[t][str(n)] = {f: rel(a.field(f), b.field(f)) for f in PROGNOSTIC}
            rows[t][str(n)]["error_status"] = [e64, e]
            print(f"{workload} {t:13s} step {n:4d}: " + "  ".join(f"{f}={rows[t][str(n)][f]:.2e}" for f in PROGNOSTIC), flush=True)
    out = {"workload": desc, "builds": {"fp64": g64.L.pomgpu_version().decode(), **{t: g.L.pomgpu_version().decode() for t, g in g32}},
           "what": "largest |variant - fp64| of a field after n internal steps from identical initial states, relative to the field's largest magnitude (fp64 run)",
           "steps": rows}
    for g in [g64] + [g for _, g in g32]:
        g.close()
    return out


def speed(rounds):
    wl = "basin2048"
    cs, im, jm, kb, desc = bench.WORKLOADS[wl]
    st0 = bench.build_state(wl, pdist.tile_for_rank(0, 1, im, jm))
    g0 = bench.gpu_initialise(st0, 0, None); g0.close()
    ctx = [(t, PomGpu(st0, device=0, libpath=lp)) for t, lp in BUILDS]
    for _, g in ctx:
        g.run(2); g.sync()
    ext = ("k_ext_", "k_advave_", "k_modeint_tail", "k_int_tail", "k_check_velocity", "k_copy2", "k_bcond1")
    acc = {t: {} for t, _ in ctx}
    for r in range(rounds):
        for t, g in ctx:
            g.prof_begin(); g.run(1); prof = g.prof_end()
            prof = {k: v for k, v in prof.items() if not k.startswith("phase_")}   # the phase entries span kernels already counted
            acc[t].setdefault("step", []).append(sum(v[1] for v in prof.values()))
            acc[t].setdefault("internal", []).append(sum(v[1] for k, v in prof.items() if not k.startswith(ext)))
            acc[t].setdefault("external", []).append(sum(v[1] for k, v in prof.items() if k.startswith(ext)))
            for k, v in prof.items():
                acc[t].setdefault(k, []).append(v[1])
    cells = im * jm * kb
    mins = {t: {k: min(v) for k, v in acc[t].items()} for t, _ in ctx}
    names = sorted((k for k in mins["fp64"] if k not in ("step", "internal", "external")), key=lambda k: -mins["fp64"][k])
    print(f"{'min ms':26s}" + "".join(f"{t:>16s}" for t, _ in ctx))
    for n in ["step", "internal", "external"] + names[:20]:
        print(f"{n:26s}" + "".join(f"{mins[t].get(n, 0):16.3f}" for t, _ in ctx))
    frac = {t: PASSES * (8 if t == "fp64" else 4) * cells / (mins[t]["internal"] * 1e-3) / 1e9 / HBM_PEAK_GBPS for t, _ in ctx}
    res = {"workload": desc + ", one MI355X, one context per build, interleaved rounds of one profiled step",
           "rounds": rounds, "builds": {t: g.L.pomgpu_version().decode() for t, g in ctx},
           "step_ms": {t: mins[t]["step"] for t, _ in ctx}, "internal_ms": {t: mins[t]["internal"] for t, _ in ctx},
           "external_ms": {t: mins[t]["external"] for t, _ in ctx},
           "internal_fraction_of_peak": {t: frac[t] for t, _ in ctx},
           "what_fraction": f"{PASSES} algorithmic passes x bytes per stored 3-D value (8 fp64, 4 both fp32 builds) / internal ms / {HBM_PEAK_GBPS:.0f} GB/s",
           "kernel_ms_min": {n: {t: mins[t].get(n, 0.0) for t, _ in ctx} for n in names}}
    for _, g in ctx:
        g.close()
    return res


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles")
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 6
    os.makedirs(out, exist_ok=True)
    if "--skip-small" not in sys.argv:
        res = {"what": "largest |variant - fp64| of a field after n internal steps from one state, relative to the field's largest magnitude (fp64 run)"}
        for case, dims, steps in (("seamount", (65, 49, 21), (1, 10, 100)), ("basin", (256, 192, 50), (1, 10, 100)),
                                  ("seamount", (256, 192, 50), (2, 10, 100))):
            res[f"{case}_{dims[0]}x{dims[1]}x{dims[2]}"] = drift_small(case, dims, steps)
        json.dump(res, open(os.path.join(out, "fp32_arith_drift_small.json"), "w"), indent=1)
    if "--skip-speed" not in sys.argv:
        json.dump(speed(rounds), open(os.path.join(out, "fp32_arith_kernel_ms_basin2048.json"), "w"), indent=1)
    if "--skip-full" not in sys.argv:
        json.dump(full_size_drift([1, 10, 100]), open(os.path.join(out, "fp32_arith_drift_basin2048.json"), "w"), indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
