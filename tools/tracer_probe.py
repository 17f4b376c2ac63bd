#!/usr/bin/env python
"""What does a passive tracer cost per step, and does the pair path pay?

ONE context of the given grid (where its arrays lie moves kernels by up to 12 %, DESIGN.md section 2: every variant shares one placement)
alternates blocks of --steps internal steps with ntr = 0, 1, 2, 4 tracers, --rounds times, the host clock around each block with a device
synchronise on either side; then ntr = 2 with the pair path against two single passes (POMGPU_TR_NOPAIR, read at launch time), alternated
the same way.  Then, per variant, the mean launch time of every kernel of the tracer stage from pomgpu_prof_* and that time as GB/s on
the kernel's algorithmic bytes (arrays read + written once, 8 B x kb x im_local x jm_local each):
  k_tr_update 6, k_tr_update2 12 (trf tr trb trclim read, trb tr written, per field); k_advt2_col 7 (trb trclim aam v u w read, trf
  written), k_advt2x2_col 10; k_proft_reg 3 (trf read and written, kh read), k_proft_reg2 5; k_tr_source 4; k_tr_edges: the edge cells alone.
Every block of steps runs under a time limit of its own (--limit seconds: the process ends there).  Prints one JSON line and, with
--out, writes it to a file.

    python tools/tracer_probe.py --grid 2048x1536x50 [--out profiles/tracer_probe.json]
"""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PASSES = {"k_tr_update": 6, "k_tr_update2": 12, "k_advt2_col": 7, "k_advt2x2_col": 10, "k_proft_reg": 3, "k_proft_reg2": 5, "k_tr_source": 4}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", default="2048x1536x50")
    ap.add_argument("--case", default="basin")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=60, help="seconds one block of steps may take")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    im, jm, kb = (int(v) for v in args.grid.lower().split("x"))

    import numpy as np
    import bench
    from extpom_amd.cases import make_case
    st = make_case(args.case, im, jm, kb, **bench.NML)
    g = bench.gpu_initialise(st, 0, None)                     # the initialisation tail with the HIP kernels
    g.run(3)                                                  # past the model's first step, which skips its 3-D part
    g.sync()
    n3 = kb * st.im_local * st.jm_local
    out = dict(tool="tracer_probe", grid=f"{im}x{jm}x{kb}", case=args.case, rounds=args.rounds, steps=args.steps,
               build_id=g.L.pomgpu_build_id().decode(), array_bytes=8 * n3)
    rng = np.random.default_rng(1)
    field = 1.0 + 0.5 * rng.random((kb, st.jm_local, st.im_local))

    def register(ntr, source=False):
        g.set_tracers(ntr)
        for n in range(1, ntr + 1):
            g.tracer_upload(n, "trb", field)
            g.tracer_upload(n, "tr", field)
            if source:
                g.set_tracer(n, nbc=1, decay=1.0e-6)

    def block():
        signal.alarm(args.limit)                              # a block that hangs ends the process: nothing more is started on the card
        g.sync()
        t = time.perf_counter()
        g.run(args.steps)
        g.sync()
        signal.alarm(0)
        return round((time.perf_counter() - t) * 1e3 / args.steps, 4)

    counts = (0, 1, 2, 4)
    ms = {str(n): [] for n in counts}
    for _ in range(args.rounds):
        for n in counts:
            register(n)
            block()                                           # one untimed block behind the uploads
            ms[str(n)].append(block())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out["ms_per_step"] = ms
    out["ms_per_step_median"] = med
    out["ms_per_step_spread"] = {k: round(max(v) - min(v), 4) for k, v in ms.items()}
    out["per_tracer_ms"] = {"1 unpaired": round(med["1"] - med["0"], 4), "2 (one pair)": round((med["2"] - med["0"]) / 2, 4),
                            "4 (two pairs)": round((med["4"] - med["0"]) / 4, 4)}
    # the pair path against two single passes, on the same two tracers
    register(2)
    ab = {"pair": [], "two singles": []}
    for _ in range(args.rounds):
        for name, sw in (("pair", None), ("two singles", 1)):
            g.switch("TR_NOPAIR", sw)
            block()
            ab[name].append(block())
    out["pair_path_ms_per_step"] = ab
    out["pair_gain_ms_per_step"] = round(float(np.median(ab["two singles"]) - np.median(ab["pair"])), 4)
    # per-kernel times: a pair, two singles, one single with decay
    kern = {}
    for name, ntr, sw, source in (("pair", 2, None, False), ("two singles", 2, 1, False), ("one with decay", 1, None, True)):
        register(ntr, source)
        g.switch("TR_NOPAIR", sw)
        block()
        signal.alarm(args.limit)
        g.prof_begin()
        g.run(args.steps)
        prof = g.prof_end()
        signal.alarm(0)
        t_names = ("k_tr_update", "k_tr_update2", "k_tr_edges", "k_tr_edges2", "k_tr_source", "k_advt2_col", "k_advt2x2_col", "k_proft_reg", "k_proft_reg2", "k_copy_kb")
        kern[name] = {}
        for k in t_names:
            if k in prof:
                cnt, total = prof[k]
                e = dict(launches_per_step=cnt / args.steps, ms_per_launch=round(total / cnt, 4))
                if k in PASSES:
                    e["GBps"] = round(PASSES[k] * 8 * n3 / (total / cnt * 1e-3) / 1e9, 1)
                kern[name][k] = e
    g.switch("TR_NOPAIR", None)
    out["kernels"] = kern
    out["note"] = "k_advt2x2_col, k_proft_reg2 and k_copy_kb also run once per step for T and S; their launches beyond that are the tracers'"
    g.set_tracers(0)
    out["error_status"] = int(g.get_con()["error_status"][0])
    g.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
