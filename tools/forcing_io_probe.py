#!/usr/bin/env python
"""What does a step pay for fetching its forcing records -- from the files on the device (PomGpu.set_forcing_files) and by the host path
(scipy read, numpy post-processing, the setters)?

Writes an sfrc and an lbry file of the given grid with scipy, then in ONE process runs two contexts of the same state, one fed by file
and one by the setters.  A turn is two steps of each: step 60t-1, which fetches nothing, and step 60t, which fetches one wind, one heat,
one surface and one lateral record (dti = 180 s: the surface records change every 60 steps, the lateral ones every 20; blkcon.iint is set
to 60t-2 before the turn, so three turns are six steps, not 180).  Every step is timed with a host clock around run(1) + sync; the host
path's clock also covers its reads, its arithmetic and its setter calls.  Also timed per turn: the bare pread of the same pieces of the files (the
offsets the library reads, found through scipy's mapping) into one bytearray, right after the two steps that have just read them.  The files have just been written by this process, so they are normally still in the page cache: the output says what
fraction of their pages was resident (mincore) before the first and after the last turn -- the read times are then memory-to-memory.

    python tools/forcing_io_probe.py [--grid 1024x1024x40] [--dir /scratch] [--turns 3] [--out profiles/forcing_read_1024x1024x40.json]
    python tools/forcing_io_probe.py --lbry-z [--ks 33] [--out profiles/forcing_read_lbry_z_1024x1024x40.json]
    python tools/forcing_io_probe.py --sides 15 [--lbry-z] [--out profiles/forcing_read_lbry_sides_1024x1024x40.json]
    python tools/forcing_io_probe.py --water --grid 2048x1536x50 [--out profiles/water_forcing_probe.json]
    python tools/forcing_io_probe.py --check      (no GPU: arguments, paths and free space only; reports no time)

--water: a job of its own (water_probe below): one water fetch beside a wind fetch of the same build, and the step with water on and off
in one context.

--lbry-z: a third context of the same job takes its lateral records from an lbry file whose temp / salt lines are on ks z levels
(PomGpu.set_z_inputs(lbry=True)): its fetch steps stand beside the sigma file's, with the bare pread of the bytes it reads, and one more
fetch step with every kernel bracketed gives k_lat_unpack and k_ztosig_line their own durations.
--sides <n>: one more context of the same job feeds the sides of the mask n (PomGpu.set_lateral_sides: east 1, south 2, west 4, north 8)
from an lbry file that holds those sides' variables (with --lbry-z: temp / salt of each on the ks z levels): its fetch steps stand beside
the two-sided file's, and one more fetch step with every kernel bracketed gives the two lateral kernels' own durations.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))                  # forcing_expect: the raw fields, the writers, the readers' arithmetic in numpy
sys.path.insert(0, os.path.join(ROOT, "tools"))
PERIOD, LPERIOD = 60, 20                                         # steps between surface / lateral record changes at dti = 180 s


def water_probe(args, im, jm, kb, where):
    """--water: one context with an sfrc file and the water files registered.  (1) at iint = 1 wind and water each fetch two records
    (wind: two planes a record, water: one): `wind` and `water` alone, host clock around call + sync, against the same calls at iint = 2,
    which fetch nothing.  (2) the step with water on and off, alternating in ONE context (the --ab idea of tools/tile_probe.py): `ab_turns`
    turns of `ab_steps` steps each way, none of which fetches.  (3) a few steps with every kernel bracketed: k_frc_interp1's own time."""
    import numpy as np
    import forcing_expect as fx
    import water_expect as wx
    from extpom_amd.cases import make_case
    from extpom_amd.model import PomGpu
    out = dict(tool="forcing_io_probe --water", grid=f"{im}x{jm}x{kb}", case=args.case)
    st = make_case(args.case, im, jm, kb, dte=6.0, isplit=30)     # dti = 180 s: iwater = 480, the surface records change every 60 steps
    tmp = tempfile.mkdtemp(prefix="water_probe_", dir=where)
    try:
        sfrc = fx.write_sfrc(os.path.join(tmp, "probe.sfrc.nc"), fx.raw_sfrc(st, 2))
        prefix = os.path.join(tmp, "probe")
        wx.write_all(prefix, wx.raw_water(st, (0, 1)))
        g = PomGpu(st, device=0)
        g.set_forcing_files(sfrc=sfrc)
        g.set_water_files(prefix)

        def timed(fn):
            g.sync()
            t = time.perf_counter()
            fn()
            g.sync()
            return round((time.perf_counter() - t) * 1e3, 3)

        def at(iint):
            g.set_con(iint=iint)
            g.call("get_time")

        at(1)
        out["wind_two_fetches_ms"] = timed(lambda: g.call("wind"))
        out["water_two_fetches_ms"] = timed(lambda: g.water())
        at(2)
        out["wind_no_fetch_ms"] = timed(lambda: g.call("wind"))
        out["water_no_fetch_ms"] = timed(lambda: g.water())
        out["fetch_bytes"] = {"wind": 2 * 2 * 8 * im * jm, "water": 2 * 8 * im * jm}
        at(1)                                                     # heat and surface too: every field's "b" and "f" generation is in place
        g.call("heat")
        g.call("surface")
        g.set_con(iint=1)
        g.run(2)                                                  # warm: steps 2, 3
        on, off = [], []
        for _ in range(args.ab_turns):
            g.set_water(True)
            on.append(round(timed(lambda: g.run(args.ab_steps)) / args.ab_steps, 4))
            g.set_water(False)
            off.append(round(timed(lambda: g.run(args.ab_steps)) / args.ab_steps, 4))
        out["step_ms_water_on"], out["step_ms_water_off"] = on, off
        out["step_ms_on_minus_off_median"] = round(float(np.median(on) - np.median(off)), 4)
        out["step_ms_off_spread"] = round(max(off) - min(off), 4)
        g.set_water(True)
        g.prof_begin()
        g.run(3)
        prof = g.prof_end()
        out["kernels_ms"] = {k: [prof[k][0], round(prof[k][1] / max(prof[k][0], 1), 5)] for k in ("k_frc_interp1", "k_frc_interp", "phase_step") if k in prof}
        out["interp1_bytes"] = 3 * 8 * im * jm
        g.download()
        out["error_status"], out["iint"] = int(st.error_status), int(st.iint)
        out["wssurf_nonzero"] = bool(st.wssurf.any())
        g.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--water", action="store_true", help="the water fetch beside a wind fetch, and the step with water on and off")
    ap.add_argument("--ab-turns", type=int, default=4)
    ap.add_argument("--ab-steps", type=int, default=5)
    ap.add_argument("--grid", default="1024x1024x40")
    ap.add_argument("--case", default="basin")
    ap.add_argument("--dir", default=None, help="where the files go (default: the temporary directory)")
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--lbry-z", action="store_true", help="also fetch from an lbry file with temp / salt on z levels")
    ap.add_argument("--ks", type=int, default=33, help="--lbry-z: the z levels of that file")
    ap.add_argument("--sides", type=int, default=0, help="also fetch from an lbry file that feeds the sides of this mask (1..15)")
    ap.add_argument("--check", action="store_true", help="arguments, paths and free space only; no GPU, no time")
    args = ap.parse_args()
    im, jm, kb = (int(v) for v in args.grid.lower().split("x"))
    where = args.dir or tempfile.gettempdir()
    more = args.lbry_z or args.sides
    nrec, nlat = args.turns + 2 + (1 if more else 0), 3 * args.turns + 2 + (3 if more else 0)   # --lbry-z, --sides: one more turn, the bracketed one
    nbytes = 8 * (6 * nrec * im * jm + nlat * (im + jm) * (1 + 4 * kb))
    free = shutil.disk_usage(where).free
    out = dict(tool="forcing_io_probe", grid=f"{im}x{jm}x{kb}", case=args.case, dir=where, file_bytes_about=nbytes, free_bytes=free)
    if not os.path.isdir(where) or not os.access(where, os.W_OK):
        out["error"] = "the directory is not writable"
        print(json.dumps(out))
        return 2
    if free < nbytes + (1 << 30):
        out["skipped"] = "not enough room for the files"
        print(json.dumps(out))
        return 0
    if args.check:
        out["checked"] = "arguments and paths only: no time is reported without a GPU"
        print(json.dumps(out))
        return 0
    if args.water:
        return water_probe(args, im, jm, kb, where)

    import numpy as np
    from scipy.io import netcdf_file
    import forcing_expect as fx
    from restart_io_probe import resident_fraction
    from extpom_amd.cases import make_case
    from extpom_amd.model import PomGpu
    st = make_case(args.case, im, jm, kb, dte=6.0, isplit=30)
    raw_s, raw_l = fx.raw_sfrc(st, nrec), fx.raw_lbry(st, nlat)
    tmp = tempfile.mkdtemp(prefix="forcing_io_probe_", dir=where)
    try:
        sfrc = fx.write_sfrc(os.path.join(tmp, "probe.sfrc.nc"), raw_s)
        lbry = fx.write_lbry(os.path.join(tmp, "probe.lbry.nc"), raw_l)
        if args.lbry_z:
            import ztosig_line_files_checks as zl               # the z-level lines for the state's own depths, the file's writer
            lbry_z = zl.write_lbry_z(os.path.join(tmp, "probe_z.lbry.nc"), zl.raw_lbry_z(st, nlat, ks=args.ks))
        if args.sides:
            import lateral_sides_expect as ls                   # the four-sided fields and the writers of a file of the ON sides
            if args.lbry_z:
                lbry_s = ls.write_lbry_z(os.path.join(tmp, "probe_s.lbry.nc"), ls.raw_lbry_z(st, nlat, ks=args.ks), args.sides)
            else:
                lbry_s = ls.write_lbry(os.path.join(tmp, "probe_s.lbry.nc"), ls.raw_lbry(st, nlat), args.sides)
        del raw_s, raw_l
        out["file_bytes"] = [os.path.getsize(sfrc), os.path.getsize(lbry)]
        out["resident_before"] = [resident_fraction(sfrc), resident_fraction(lbry)]
        a, b = st, st.copy()
        gf, gh = PomGpu(a, device=0), PomGpu(b, device=0)
        gf.set_forcing_files(sfrc=sfrc, lbry=lbry)
        # the host path needs its first records in place before lateral_bc / wind look for them at the first fetch step
        fs, fl = netcdf_file(sfrc, "r", mmap=True), netcdf_file(lbry, "r", mmap=True)
        rec_bytes = 8 * (5 * im * jm + (im + jm) * (1 + 4 * kb))          # SSS is not read by the file path; the host path reads it as the reference does
        fd_s, fd_l = os.open(sfrc, os.O_RDONLY), os.open(lbry, os.O_RDONLY)
        if args.lbry_z:
            c = st.copy()
            gz = PomGpu(c, device=0)
            gz.set_z_inputs(lbry=True)
            gz.set_forcing_files(sfrc=sfrc, lbry=lbry_z)
            fz, fd_z = netcdf_file(lbry_z, "r", mmap=True), os.open(lbry_z, os.O_RDONLY)
            z_bytes = 8 * (5 * im * jm + (im + jm) * (1 + 2 * kb + 2 * args.ks))
            out["z_file_bytes"], out["ks"] = os.path.getsize(lbry_z), args.ks

        if args.sides:
            d = st.copy()
            gs = PomGpu(d, device=0)
            if args.lbry_z:
                gs.set_z_inputs(lbry=True)
            gs.set_lateral_sides(east=bool(args.sides & 1), south=bool(args.sides & 2), west=bool(args.sides & 4), north=bool(args.sides & 8))
            gs.set_forcing_files(sfrc=sfrc, lbry=lbry_s)
            nside = bin(args.sides).count("1")                   # every side: one elevation line and four arrays, two of them on ks levels under --lbry-z
            out["sides"], out["sides_file_bytes"] = args.sides, os.path.getsize(lbry_s)
            out["sides_fetch_bytes"] = 8 * (5 * im * jm + nside * ((im + jm) // 2) * (1 + (2 * kb + 2 * args.ks if args.lbry_z else 4 * kb)))

        def timed(fn):
            t = time.perf_counter()
            fn()
            return round((time.perf_counter() - t) * 1e3, 3)

        def step(g):
            g.run(1)
            g.sync()

        def host_fetch_and_step(n):
            r, rl = n // PERIOD + 2, n // LPERIOD + 2                     # the records the schedule asks for at step n (bounds_forcing.f:897, :755)
            v = fs.variables
            wu, wv = fx.wind_record(b, v["sustr"][r - 1], v["svstr"][r - 1])
            shf, swr = fx.heat_record(b, v["shflux"][r - 1], v["swrad"][r - 1])
            sst, sss = np.array(v["SST"][r - 2], dtype=np.float64), np.array(v["SSS"][r - 2], dtype=np.float64)   # surface asks for record n/60+1 (:977)
            for kind, (x, y) in enumerate(((wu, wv), (shf, swr), (sst, sss))):
                x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
                gh._chk(gh.L.pomgpu_set_forcing_record(gh.h, kind, r - 1 if kind == 2 else r, gh._p(x), gh._p(y)), "set_forcing_record")
            one = {k: np.array(fl.variables[k][rl - 1:rl], dtype=np.float64) for k in fx.LBRY}
            b.lateral_records = [None] * (rl - 1) + fx.lateral_records(b, one, 1)
            gh.set_lateral_records(first=rl, count=1)
            step(gh)

        def where_in_file(f, var, r):
            """(offset, bytes) of record r (1-based) of a variable: scipy's view of the record lies inside its mapping of the file"""
            rec = f.variables[var][r - 1]
            return rec.__array_interface__["data"][0] - f._mm_buf.__array_interface__["data"][0], rec.nbytes

        dest = bytearray(rec_bytes)

        def pread_plan_z(n):
            # the same for the z-level context: the sfrc pieces and record rl of the ten variables of ITS lbry file
            r, rl, at = n // PERIOD + 2, n // LPERIOD + 2, 0
            pieces = [(fd_s, "sustr", r), (fd_s, "svstr", r), (fd_s, "shflux", r), (fd_s, "swrad", r), (fd_s, "SST", r - 1)] + [(fd_z, k, rl) for k in fx.LBRY]
            plan = []
            for fd, var, rec in pieces:
                off, nb = where_in_file(fs if fd == fd_s else fz, var, rec)
                plan.append((fd, off, at, nb))
                at += nb
            assert at == z_bytes
            return plan

        def pread_plan(n):
            # the very reads the file path makes for step n: records r / r-1 of the five sfrc variables it reads and record rl of the ten
            # lbry variables (one tile: each a contiguous piece), every piece into its own place of one buffer
            r, rl, at = n // PERIOD + 2, n // LPERIOD + 2, 0
            pieces = [(fd_s, "sustr", r), (fd_s, "svstr", r), (fd_s, "shflux", r), (fd_s, "swrad", r), (fd_s, "SST", r - 1)] + [(fd_l, k, rl) for k in fx.LBRY]
            plan = []
            for fd, var, rec in pieces:
                off, nb = where_in_file(fs if fd == fd_s else fl, var, rec)
                plan.append((fd, off, at, nb))
                at += nb
            assert at == rec_bytes
            return plan

        def bare_pread(plan):
            for fd, off, at, nb in plan:
                if os.preadv(fd, [memoryview(dest)[at:at + nb]], off) != nb:
                    raise OSError("pread failed")

        res = dict(file_step_ms=[], file_step_nofetch_ms=[], host_step_ms=[], host_step_nofetch_ms=[], bare_pread_ms=[])
        if args.lbry_z:
            res.update(z_file_step_ms=[], z_file_step_nofetch_ms=[], z_bare_pread_ms=[])
            gz.set_con(iint=2)
            step(gz)
        if args.sides:
            res.update(sides_file_step_ms=[], sides_file_step_nofetch_ms=[])
            gs.set_con(iint=2)
            step(gs)
        # warm both contexts (first launches, allocations) on a step of their own, and give the host path the "b" generation of records
        for g in (gf, gh):
            g.set_con(iint=2)
        step(gf)
        host_fetch_and_step(3)
        for t in range(1, args.turns + 1):
            n = PERIOD * t
            for g in (gf, gh):
                g.get_con()
                g.set_con(iint=n - 2)
            res["file_step_nofetch_ms"].append(timed(lambda: step(gf)))
            res["host_step_nofetch_ms"].append(timed(lambda: step(gh)))
            res["file_step_ms"].append(timed(lambda: step(gf)))
            res["host_step_ms"].append(timed(lambda: host_fetch_and_step(n)))
            plan = pread_plan(n)
            res["bare_pread_ms"].append(timed(lambda: bare_pread(plan)))
            if args.lbry_z:
                gz.get_con()
                gz.set_con(iint=n - 2)
                res["z_file_step_nofetch_ms"].append(timed(lambda: step(gz)))
                res["z_file_step_ms"].append(timed(lambda: step(gz)))
                plan = pread_plan_z(n)
                dest_z = bytearray(z_bytes)
                keep, dest = dest, dest_z
                res["z_bare_pread_ms"].append(timed(lambda: bare_pread(plan)))
                dest = keep
            if args.sides:
                gs.get_con()
                gs.set_con(iint=n - 2)
                res["sides_file_step_nofetch_ms"].append(timed(lambda: step(gs)))
                res["sides_file_step_ms"].append(timed(lambda: step(gs)))
        if args.sides:                                            # one more fetch step, every kernel bracketed
            gs.get_con()
            gs.set_con(iint=PERIOD * (args.turns + 1) - 1)
            gs.prof_begin()
            step(gs)
            prof = gs.prof_end()
            out["sides_kernels_ms"] = {k: [prof[k][0], round(prof[k][1], 4)] for k in ("k_lat_unpack", "k_ztosig_line") if k in prof}
            gs.download()
            out["sides_error_status"] = int(d.error_status)
            out["sides_tbwf_nonzero"] = bool(d.tbwf.any())
            gs.close()
        if args.lbry_z:                                           # one more fetch step, every kernel bracketed: the two lateral kernels' own time
            gz.get_con()
            gz.set_con(iint=PERIOD * (args.turns + 1) - 1)
            gz.prof_begin()
            step(gz)
            prof = gz.prof_end()
            out["z_kernels_ms"] = {k: [prof[k][0], round(prof[k][1], 4)] for k in ("k_lat_unpack", "k_ztosig_line") if k in prof}
            gz.download()
            out["z_error_status"] = int(c.error_status)
            out["z_tbef_level_kb_nonzero"] = bool(c.tbef[kb - 1].any())
            out["z_fetch_bytes"] = z_bytes
            os.close(fd_z)
            fz.close()
            gz.close()
        os.close(fd_s)
        os.close(fd_l)
        gf.download()
        gh.download()
        out["same_state"] = bool(np.array_equal(a.blk2d.view(np.uint64), b.blk2d.view(np.uint64)) and np.array_equal(a.blk3d.view(np.uint64), b.blk3d.view(np.uint64))
                                 and np.array_equal(a.bdry.view(np.uint64), b.bdry.view(np.uint64)))   # the two paths computed the same bits
        out["error_status"] = [int(a.error_status), int(b.error_status)]
        out["resident_after"] = [resident_fraction(sfrc), resident_fraction(lbry)]
        out["fetch_bytes"] = rec_bytes
        out.update(res)
        out["file_fetch_ms"] = [round(x - y, 3) for x, y in zip(res["file_step_ms"], res["file_step_nofetch_ms"])]
        if args.sides:
            out["sides_file_fetch_ms"] = [round(x - y, 3) for x, y in zip(res["sides_file_step_ms"], res["sides_file_step_nofetch_ms"])]
        if args.lbry_z:
            out["z_file_fetch_ms"] = [round(x - y, 3) for x, y in zip(res["z_file_step_ms"], res["z_file_step_nofetch_ms"])]
        out["host_fetch_ms"] = [round(x - y, 3) for x, y in zip(res["host_step_ms"], res["host_step_nofetch_ms"])]
        out["page_cache"] = "the files were written by this process just before: resident_* is the fraction of their pages in the page cache"
        fs.close()
        fl.close()
        gf.close()
        gh.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for k in ("dir", "free_bytes", "file_bytes_about"):
        out.pop(k, None)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
