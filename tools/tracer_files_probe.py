#!/usr/bin/env python
"""What do the tracers' time mean, inventory and files cost?

ONE context of the given grid (where its arrays lie moves kernels by up to 12 %, DESIGN.md section 2: everything compared shares one
placement).  For ntr in --tracers (2 and 8): blocks of --steps internal steps with the mean off and on, alternated --rounds times as
tools/mean_output_probe.py does, the host clock around each block with a device synchronise on either side.  Then
  k_mean_accum     per launch with the tracers' table: the kernel's total over a profiled block with tracers registered minus its total
                   over a block with none, per step; its algorithmic bytes are 3 x 8 B x n3 per tracer (tr read, acc read, acc written);
  k_tracer_stats   the two launches of pomgpu_tracer_stats;
  k_tr_unpack      the reader's kernel, summed over one pomgpu_read_tracers;
  wall time        of one restart-kind pomgpu_write_tracers (inside the call / until the writer's thread has joined) and of one
                   pomgpu_read_tracers, with --io-tracers tracers, against tracer_download / tracer_upload of the same trb and tr
                   (the file also carries trf, which has no download: 3 arrays per tracer against 2).
Records, not thresholds.  Prints one JSON line and, with --out, writes it to a file.

    python tools/tracer_files_probe.py --grid 2048x1536x50 [--dir /scratch] [--out profiles/tracer_files_probe.json]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", default="2048x1536x50")
    ap.add_argument("--case", default="basin")
    ap.add_argument("--tracers", default="2,8")
    ap.add_argument("--io-tracers", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-file", action="store_true", help="leave the file write and read out")
    ap.add_argument("--dir", default=None, help="where the file goes (default: the temporary directory)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    im, jm, kb = (int(v) for v in args.grid.lower().split("x"))

    import numpy as np
    import bench
    from extpom_amd.cases import make_case
    st = make_case(args.case, im, jm, kb, **bench.NML)
    g = bench.gpu_initialise(st, 0, None)
    g.run(3)                                                  # past the model's first step, which skips its 3-D part
    g.sync()
    n3 = kb * st.im_local * st.jm_local
    out = dict(tool="tracer_files_probe", grid=f"{im}x{jm}x{kb}", case=args.case, rounds=args.rounds, steps=args.steps,
               build_id=g.L.pomgpu_build_id().decode(), accum_algorithmic_bytes_per_tracer=3 * 8 * n3,
               accum_expected_ms_per_tracer_at_5p4TBps=round(3 * 8 * n3 / 5.4e12 * 1e3, 4))

    def block():
        g.sync()
        t = time.perf_counter()
        g.run(args.steps)
        g.sync()
        return round((time.perf_counter() - t) * 1e3 / args.steps, 4)

    def accum_total():
        g.prof_begin(only="k_mean_accum")
        g.run(args.steps)
        n, total = g.prof_end()["k_mean_accum"]
        return n, total

    g.set_mean_output(True)
    n0, nine_total = accum_total()                            # the nine fields alone
    assert n0 == args.steps
    g.set_mean_output(False)
    out["k_mean_accum_nine_fields_ms"] = round(nine_total / n0, 4)
    ones = np.ones(g.tracer_shape("tr"))
    per = {}
    for ntr in (int(v) for v in args.tracers.split(",")):
        g.set_tracers(ntr)
        for n in range(1, ntr + 1):
            g.tracer_upload(n, "tr", ones)
            g.tracer_upload(n, "trb", ones)
        ms = {"off": [], "on": []}
        for _ in range(args.rounds):
            g.set_mean_output(False)
            ms["off"].append(block())
            g.set_mean_output(True)
            ms["on"].append(block())
        rec = dict(ms_per_step=ms, ms_per_step_median={k: float(np.median(v)) for k, v in ms.items()},
                   ms_per_step_spread={k: round(max(v) - min(v), 4) for k, v in ms.items()})
        rec["on_minus_off_ms"] = round(rec["ms_per_step_median"]["on"] - rec["ms_per_step_median"]["off"], 4)
        n, total = accum_total()
        assert n == 2 * args.steps and g.tracer_mean_count() > 0
        rec["k_mean_accum_tracers_launch_ms"] = round((total - nine_total) / args.steps, 4)
        rec["k_mean_accum_ms_per_tracer"] = round((total - nine_total) / args.steps / ntr, 4)
        rec["k_mean_accum_tracers_TBps"] = round(3 * 8 * n3 * ntr / ((total - nine_total) / args.steps * 1e-3) / 1e12, 3)
        g.sync()
        g.prof_begin()
        g.tracer_stats()
        p = g.prof_end()
        rec["k_tracer_stats_ms"] = round(p["k_tracer_stats"][1], 4)
        rec["k_tracer_stats_fin_ms"] = round(p["k_tracer_stats_fin"][1], 4)
        g.set_mean_output(False)
        per[str(ntr)] = rec
    out["tracers"] = per
    del ones
    if not args.no_file:
        ntr = args.io_tracers
        g.set_tracers(ntr)
        rng = np.random.default_rng(1)
        x = rng.random(g.tracer_shape("tr"))
        d = tempfile.mkdtemp(prefix="tracer_files_probe_", dir=args.dir or tempfile.gettempdir())
        io = dict(tracers=ntr)
        try:
            g.sync()
            t = time.perf_counter()
            for n in range(1, ntr + 1):
                g.tracer_upload(n, "tr", x)
                g.tracer_upload(n, "trb", x)
            io["tracer_upload_tr_trb_s"] = round(time.perf_counter() - t, 4)
            g.run(1)
            g.sync()
            t = time.perf_counter()
            for n in range(1, ntr + 1):
                g.tracer_download(n, "tr")
                g.tracer_download(n, "trb")
            io["tracer_download_tr_trb_s"] = round(time.perf_counter() - t, 4)
            path = os.path.join(d, "probe.tracer.rst.nc")
            t = time.perf_counter()
            g.write_file("tracer_restart", path, title="probe", time_start="2000-01-01 00:00:00 +00:00")
            io["write_call_s"] = round(time.perf_counter() - t, 4)
            g.io_wait()
            io["write_joined_s"] = round(time.perf_counter() - t, 4)
            io["file_bytes"] = os.path.getsize(path)
            g.prof_begin(only="k_tr_unpack")
            t = time.perf_counter()
            g.read_tracers(path)
            io["read_s"] = round(time.perf_counter() - t, 4)
            n, total = g.prof_end()["k_tr_unpack"]
            io["k_tr_unpack_launches"] = n
            io["k_tr_unpack_total_ms"] = round(total, 4)
        finally:
            shutil.rmtree(d, ignore_errors=True)
        out["io"] = io
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
