#!/usr/bin/env python
"""What do Lagrangian floats cost per step, and does their order in memory matter?

ONE context of the given grid (where its arrays lie moves kernels by several per cent, DESIGN.md section 2: every variant shares one
placement).  For n = 1e5, 1e6, 1e7 floats, seeded at random in the wet cells and registered once in cell order (set_floats(sort=True)) and
once shuffled, blocks of --steps internal steps with the floats on and off alternate --rounds times, the host clock around each block with
a device synchronise on either side.  Then k_float_step's own time per launch from pomgpu_prof_*, and that time per float.  The kernel is a
gather: 88 scattered 8-byte loads a float and step next to 36 bytes of float state read and written coalesced.
Every block of steps runs under a time limit of its own (--limit seconds: the process ends there).  Prints one JSON line and, with
--out, writes it to a file.

    python tools/float_probe.py --grid 2048x1536x50 [--out profiles/float_probe.json]
"""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", default="2048x1536x50")
    ap.add_argument("--case", default="basin")
    ap.add_argument("--counts", default="100000,1000000,10000000")
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
    out = dict(tool="float_probe", grid=f"{im}x{jm}x{kb}", case=args.case, rounds=args.rounds, steps=args.steps,
               build_id=g.L.pomgpu_build_id().decode(), gathers_per_float_and_step=88, state_bytes_per_float=36)
    rng = np.random.default_rng(1)
    wet = np.argwhere(st.fsm[1:jm - 1, 1:im - 1] != 0.0) + 2   # (j, i), 1-based, inside 2..jm-1 x 2..im-1

    def block(prof=False):
        signal.alarm(args.limit)                              # a block that hangs ends the process: nothing more is started on the card
        g.sync()
        if prof:
            g.prof_begin("k_float_step")
        t = time.perf_counter()
        g.run(args.steps)
        g.sync()
        ms = round((time.perf_counter() - t) * 1e3 / args.steps, 4)
        p = g.prof_end() if prof else None
        signal.alarm(0)
        return p if prof else ms

    res = {}
    for n in (int(v) for v in args.counts.split(",")):
        c = wet[rng.integers(0, len(wet), n)]
        x = c[:, 1] + 0.98 * (rng.random(n) - 0.5)
        y = c[:, 0] + 0.98 * (rng.random(n) - 0.5)
        s = -rng.random(n)
        kind = (rng.random(n) < 0.25).astype(np.int32)
        perm = rng.permutation(n)
        for order in ("cell order", "shuffled"):
            put = (lambda: g.set_floats(x, y, s, kind, sort=True)) if order == "cell order" else (lambda: g.set_floats(x[perm], y[perm], s[perm], kind[perm]))
            ms = {"on": [], "off": []}
            for _ in range(args.rounds):
                for name in ("on", "off"):
                    if name == "on":
                        put()
                    else:
                        g.set_floats([], [], [])
                    block()                                   # one untimed block behind the upload
                    ms[name].append(block())
            put()
            block()
            cnt, total = block(prof=True)["k_float_step"]
            F = g.floats()
            e = dict(ms_per_step=ms, ms_per_step_median={k: float(np.median(v)) for k, v in ms.items()},
                     ms_per_step_spread={k: round(max(v) - min(v), 4) for k, v in ms.items()},
                     floats_cost_ms_per_step=round(float(np.median(ms["on"]) - np.median(ms["off"])), 4),
                     k_float_step_launches_per_step=cnt / args.steps, k_float_step_ms_per_launch=round(total / cnt, 4),
                     k_float_step_ns_per_float=round(total / cnt * 1e6 / n, 3), active_at_the_end=int((F["status"] == 0).sum()))
            res.setdefault(str(n), {})[order] = e
            g.set_floats([], [], [])
    out["floats"] = res
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
