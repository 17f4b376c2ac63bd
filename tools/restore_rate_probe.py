#!/usr/bin/env python
"""What does a restore rate field cost, at the load and in every step?

Writes a steady rate file (NC_FLOAT, one record of `tau` on --ks z levels) for the given grid and measures in ONE process:
  load        restore_interior's load step (iint = 2: records 1 and 2) with the file registered afresh, the host clock around the call and
              a device synchronise -- the first load reads and maps, the second finds the record in taurstrf -- beside the same call in a
              context without a rate source, and beside pread_floor_s, a plain sequential pread of the file's tau bytes into a pinned buffer;
  k_ts_update per launch, from pomgpu_prof_*: <1> (no rate source: two known scalars), <2> (the steady file: taurstrf alone) and <0> (the
              steady file under the POMGPU_TAU_ARRAYS switch: both arrays), the three interleaved --rounds times, --steps steps each.
<2> and <0> run in the one context that holds the file (the switch is flipped between them); a registered file cannot be taken away
again, so <1> runs in a sibling context of the same process on the same state, in the same interleaving.  Prints one JSON line and, with
--out, writes it to a file.  The file has just been written by this process, so it is normally still in the page cache.

    python tools/restore_rate_probe.py --grid 1024x1024x40 [--dir /scratch] [--out profiles/restore_rate_1024x1024x40.json]
"""
import argparse
import json
import os
import pathlib
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CHUNK = 64 << 20


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", default="1024x1024x40")
    ap.add_argument("--case", default="archipelago")
    ap.add_argument("--ks", type=int, default=33)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the file goes (default: the temporary directory)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    im, jm, kb = (int(v) for v in args.grid.lower().split("x"))
    where = args.dir or tempfile.gettempdir()

    import numpy as np
    import torch
    import restore_rate_checks as C
    import restore_rate_expect as R
    from extpom_amd.cases import make_case
    from extpom_amd.model import PomGpu, gpu_finish_initial
    out = dict(tool="restore_rate_probe", grid=f"{im}x{jm}x{kb}", case=args.case, ks=args.ks, rounds=args.rounds, steps=args.steps)
    d = pathlib.Path(tempfile.mkdtemp(prefix="restore_rate_probe_", dir=where))
    try:
        st = make_case(args.case, im, jm, kb, dte=6.0, isplit=30)
        gpu_finish_initial(st, device=0)
        st.restore_records = [(st.tclim[:, :jm, :im] * (1.0 + 0.01 * r), st.sclim[:, :jm, :im] * (1.0 + 0.001 * r)) for r in range(2)]
        zs = R.levels(args.ks, 1.0625 * float(st.h.max()))
        path = C.write_rate(d / "steady.nc", zs, [R.sponge(im, jm, zs)], kind="f", layout="none")
        tau_bytes = 4 * args.ks * jm * im
        out["file_bytes"], out["tau_bytes"] = os.path.getsize(path), tau_bytes
        plain, rated = PomGpu(st, device=0), PomGpu(st, device=0)
        time2 = float(st.dti) * 2.0 / 86400.0

        def load(g, register):
            if register:
                g.set_restore_rate_file(path)
            g.set_con(iint=2, time=time2)
            g.sync()
            t = time.perf_counter()
            g.call("restore_interior")
            g.sync()
            return round(time.perf_counter() - t, 5)

        out["load_plain_s"] = [load(plain, False) for _ in range(3)]
        out["load_read_and_map_s"] = [load(rated, True) for _ in range(3)]     # registered afresh: taurstrf does not hold the record
        out["load_record_kept_s"] = [load(rated, False) for _ in range(3)]      # the steady record is there already: no read, no map
        pin = torch.empty(CHUNK, dtype=torch.uint8).pin_memory().numpy()
        fd = os.open(path, os.O_RDONLY)
        floors = []
        for _ in range(3):
            t = time.perf_counter()
            off = 0
            while off < tau_bytes:
                n = os.preadv(fd, [memoryview(pin)[:min(CHUNK, tau_bytes - off)]], off)
                if n <= 0:
                    raise OSError("pread failed")
                off += n
            floors.append(round(time.perf_counter() - t, 5))
        os.close(fd)
        out["pread_floor_s"] = floors
        # ---- the step's kernel, the three forms interleaved ----
        for g in (plain, rated):
            g.set_con(iint=0, time=0.0)
            g.run(2)                                            # iint = 2 loads inside the step
            g.sync()
        forms = (("<1>", plain, None, "k_ts_update"), ("<2>", rated, None, "k_ts_update_same"), ("<0>", rated, 1, "k_ts_update"))
        ms = {f[0]: [] for f in forms}
        for _ in range(args.rounds):
            for name, g, sw, kernel in forms:
                g.switch("TAU_ARRAYS", sw)
                g.prof_begin(only=kernel)
                g.run(args.steps)
                prof = g.prof_end()
                n, total = prof[kernel]
                assert n == args.steps and set(prof) & {"k_ts_update", "k_ts_update_same"} == {kernel}, (name, sorted(prof))
                ms[name].append(round(total / n, 4))
        rated.switch("TAU_ARRAYS", None)
        out["k_ts_update_ms"] = ms
        out["k_ts_update_ms_median"] = {k: float(np.median(v)) for k, v in ms.items()}
        out["k_ts_update_ms_spread"] = {k: round(max(v) - min(v), 4) for k, v in ms.items()}
        out["error_status"] = [int(plain.get_con()["error_status"][0]), int(rated.get_con()["error_status"][0])]
        out["page_cache"] = "the file was written by this process just before: the rates are memory-to-memory, not the disk's"
        plain.close()
        rated.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
