#!/usr/bin/env python
"""What does the time-mean output cost per step, and how far is its kernel from a plain stream?

ONE context of the given grid (where its arrays lie moves kernels by up to 12 %, DESIGN.md section 2: the two ways share one placement)
alternates blocks of --steps internal steps with the mean off and on, --rounds times, the host clock around each block with a device
synchronise on either side.  Then, with the mean on:
  k_mean_accum     mean launch time from pomgpu_prof_*, and that time as a fraction of 8 TB/s on the kernel's algorithmic bytes,
                   3 x 8 B x (6 kb + 3) x im_local x jm_local: x read, acc read, acc written;
  k_mean_snapshot  the one launch of pomgpu_write_output_mean (--no-file leaves the file and this figure out: at 2048x1536x50 the
                   file has 8 GB), with the host's time inside the call and until the writer's thread has joined.
Prints one JSON line and, with --out, writes it to a file.

    python tools/mean_output_probe.py --grid 2048x1536x50 [--dir /scratch] [--out profiles/mean_output_2048x1536x50.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", default="2048x1536x50")
    ap.add_argument("--case", default="basin")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-file", action="store_true", help="leave the mean file, and with it k_mean_snapshot, out")
    ap.add_argument("--dir", default=None, help="where the mean file goes (default: the temporary directory)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    im, jm, kb = (int(v) for v in args.grid.lower().split("x"))

    import numpy as np
    import bench
    from extpom_amd.cases import make_case
    st = make_case(args.case, im, jm, kb, **bench.NML)
    g = bench.gpu_initialise(st, 0, None)                     # the initialisation tail with the HIP kernels, single arrays downloaded
    g.run(3)                                                  # past the model's first step, which skips its 3-D part
    g.sync()
    nbytes = 3 * 8 * (6 * kb + 3) * st.im_local * st.jm_local
    out = dict(tool="mean_output_probe", grid=f"{im}x{jm}x{kb}", case=args.case, rounds=args.rounds, steps=args.steps,
               build_id=g.L.pomgpu_build_id().decode(), accum_algorithmic_bytes=nbytes)

    def block():
        g.sync()
        t = time.perf_counter()
        g.run(args.steps)
        g.sync()
        return round((time.perf_counter() - t) * 1e3 / args.steps, 4)

    ms = {"off": [], "on": []}
    for _ in range(args.rounds):
        g.set_mean_output(False)
        ms["off"].append(block())
        g.set_mean_output(True)
        ms["on"].append(block())
    out["ms_per_step"] = ms
    out["ms_per_step_median"] = {k: float(np.median(v)) for k, v in ms.items()}
    out["ms_per_step_spread"] = {k: round(max(v) - min(v), 4) for k, v in ms.items()}
    out["on_minus_off_ms"] = round(out["ms_per_step_median"]["on"] - out["ms_per_step_median"]["off"], 4)
    g.prof_begin(only="k_mean_accum")
    g.run(args.steps)
    n, total = g.prof_end()["k_mean_accum"]
    assert n == args.steps
    out["k_mean_accum_ms"] = round(total / n, 4)
    out["k_mean_accum_fraction_of_8TBps"] = round(nbytes / (total / n * 1e-3) / HBM_BYTES_PER_S, 4)
    if not args.no_file:
        d = tempfile.mkdtemp(prefix="mean_output_probe_", dir=args.dir or tempfile.gettempdir())
        try:
            g.sync()
            g.prof_begin(only="k_mean_snapshot")
            t = time.perf_counter()
            g.write_file("output_mean", os.path.join(d, "mean.nc"), title="probe", time_start="2000-01-01 00:00:00 +00:00")
            out["write_call_s"] = round(time.perf_counter() - t, 4)
            g.io_wait()
            out["write_joined_s"] = round(time.perf_counter() - t, 4)
            n, total = g.prof_end()["k_mean_snapshot"]
            assert n == 1 and g.mean_count() == 0
            out["k_mean_snapshot_ms"] = round(total, 4)
            out["file_bytes"] = os.path.getsize(os.path.join(d, "mean.nc"))
        finally:
            shutil.rmtree(d, ignore_errors=True)
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
