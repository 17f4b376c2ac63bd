#!/usr/bin/env python
"""How long does a cold start from z-level files take beside the sigma-file start of the same job?

Writes two file sets of the given grid in ONE process -- the sigma set of tools/cold_start_io_probe.py (NC_FLOAT, 10 clim records) and a
z-level init / clim pair (NC_FLOAT, --ks levels, `Level` / `z`; tests/ztosig_expect.py's generator on the case's own h and zz) beside the
same grid file -- and times, with a host clock around calls that end in a device synchronise:
  sigma_start_s   PomGpu.cold_start from the sigma set;
  z_start_s       PomGpu.set_z_inputs(init=True, clim=True) + cold_start from the z set, which reads ks instead of kb-1 / kb levels per
                  variable and runs ztosig four times;
  kernels_ms      pomgpu_prof times of k_ztosig (4 launches), k_cold_zts (2) and the k_rst_unpack launches of a second z start.
There is no pass mark: the comparison is the sigma start of the same job, and the line is a record.  Prints one JSON line and, with --out,
writes it to a file.  The files have just been written by this process, so they are normally still in the page cache.

    python tools/cold_start_z_probe.py --grid 1024x1024x40 --ks 33 [--dir /scratch] [--out profiles/cold_start_z_1024x1024x40.json]
    python tools/cold_start_z_probe.py --grid 64x48x10 --ks 7 --lib tests/_emu/libpomgpu_emu.so      (a host build: the tool's own plumbing)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", default="1024x1024x40")
    ap.add_argument("--ks", type=int, default=33)
    ap.add_argument("--case", default="archipelago")
    ap.add_argument("--dir", default=None, help="where the files go (default: the temporary directory)")
    ap.add_argument("--lib", default=None, help="the library to load (default: the product library on device 0)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    im, jm, kb = (int(v) for v in args.grid.lower().split("x"))
    ks = args.ks
    where = args.dir or tempfile.gettempdir()
    out = dict(tool="cold_start_z_probe", grid=f"{im}x{jm}x{kb}", ks=ks, case=args.case, file_type="NC_FLOAT")
    need = 4 * im * jm * (13 + 2 * (kb + 2) + 2 * 10 * kb + 2 * ks + 2 * 10 * ks)
    if shutil.disk_usage(where).free < need + (1 << 30):
        out["skipped"] = "not enough room for the files"
        print(json.dumps(out))
        return 0

    import numpy as np
    from scipy.io import netcdf_file
    import cold_start_expect as E
    import ztosig_expect as Z
    from extpom_amd import decomp
    from extpom_amd.model import PomGpu
    d = pathlib.Path(tempfile.mkdtemp(prefix="cold_start_z_probe_", dir=where))
    try:
        E.NREC_CLIM = 10
        f = E.case_fields(args.case, im, jm, kb, dte=6.0, isplit=30)
        sigma = E.write_files(d, f, kind="f", clim_records=10, stem="sigma")
        grid = (f["zz"][:kb], f["h"])
        zmax = 0.8 * float(f["h"].max())
        zs, t, _, _ = Z.make_inputs(im, jm, ks, kb, grid=grid, zmax=zmax)
        s = Z.make_inputs(im, jm, ks, kb, grid=grid, zmax=zmax, salt=True)[1]
        del f
        zinit, zclim = str(d / "z.init.nc"), str(d / "z.clim.nc")
        with netcdf_file(zinit, "w", version=2) as nc:
            nc.createDimension("Time", None)
            nc.createDimension("Level", ks)
            nc.createDimension("y", jm)
            nc.createDimension("x", im)
            nc.createVariable("Level", "f", ("Level",))[:] = zs
            for n, a in (("T", t), ("S", s)):
                nc.createVariable(n, "f", ("Time", "Level", "y", "x"))[0] = a
        with netcdf_file(zclim, "w", version=2) as nc:
            nc.createDimension("month", None)
            nc.createDimension("z", ks)
            nc.createDimension("y", jm)
            nc.createDimension("x", im)
            nc.createVariable("z", "f", ("z",))[:] = zs
            vt = nc.createVariable("Tclim", "f", ("month", "z", "y", "x"))
            vs = nc.createVariable("Sclim", "f", ("month", "z", "y", "x"))
            for r in range(10):
                vt[r] = t * (1.0 + 0.002 * (r + 1))
                vs[r] = s * (1.0 + 0.0005 * (r + 1))
        del t, s
        zset = [sigma[0], zinit, zclim]
        out["sigma_read_bytes"] = 4 * im * jm * (13 + 2 * (kb - 1) + 2 * kb)
        out["z_read_bytes"] = 4 * im * jm * (13 + 4 * ks)
        tile = decomp.make_tile(0, im, jm, im, jm)
        nml = dict(dte=6.0, isplit=30)

        def start(paths, on_z, prof=False):
            b = E.blank_state(tile, kb, **nml)
            g = PomGpu(b, device=0, libpath=args.lib)
            g.set_z_inputs(init=on_z, clim=on_z)
            g.sync()
            if prof:
                g.prof_begin()
            t0 = time.perf_counter()
            g.cold_start(*paths)
            g.sync()
            dt = time.perf_counter() - t0
            p = g.prof_end() if prof else {}
            g.download()
            g.close()
            return dt, p, b

        start(sigma, False)                                      # untimed: the first start of a process pays for the library's first use
        out["sigma_start_s"] = round(start(sigma, False)[0], 4)
        dt, _, b = start(zset, True)
        out["z_start_s"] = round(dt, 4)
        out["level_kb_of_tb_nonzero"] = bool(b.tb[kb - 1].any())
        _, p, _ = start(zset, True, prof=True)
        out["kernels_ms"] = {n: [int(p[n][0]), round(float(p[n][1]), 3)] for n in ("k_ztosig", "k_cold_zts", "k_rst_unpack") if n in p}
        out["page_cache"] = "the files were written by this process just before: the rates are memory-to-memory, not the disk's"
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
