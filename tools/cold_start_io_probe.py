#!/usr/bin/env python
"""How long does PomGpu.cold_start take beside today's only other way from the reference's input files into the library?

Writes a grid / init / clim file set of the given grid (NC_FLOAT, 10 clim records; tests/cold_start_expect.py's writers), then times in
ONE process, with a host clock around calls that end in a device synchronise:
  cold_start   PomGpu.cold_start on a context that holds read_input's constants;
  host_path    a scipy read of the three files and the readers' assignments into a PomState (the numpy restatement, vectorised),
               model.gpu_finish_initial (an upload and a download of every block around dens, dens and baropg), then PomGpu.upload;
  pread_floor  a plain sequential pread of as many bytes as cold_start reads into one pinned buffer.
same_state says whether the two ways leave the same bits on every array of blk2d / blk3d but the four scratch arrays, on bdry, blk1d and
blkcon -- cor, cbc and period apart: the host path forms them with numpy's vector sin / log, cold_start with libm, and
cor_cbc_max_ulp says how far the two are apart.  Prints one JSON line and, with --out,
writes it to a file.  The files have just been written by this process, so they are normally still in the page cache.

    python tools/cold_start_io_probe.py --grid 1024x1024x40 [--dir /scratch] [--out profiles/cold_start_1024x1024x40.json]
    python tools/cold_start_io_probe.py --check      (no GPU: arguments, paths and free space only; reports no time)
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
    ap.add_argument("--dir", default=None, help="where the files go (default: the temporary directory)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--check", action="store_true", help="arguments, paths and free space only; no GPU, no time")
    args = ap.parse_args()
    im, jm, kb = (int(v) for v in args.grid.lower().split("x"))
    where = args.dir or tempfile.gettempdir()
    read_bytes = 4 * im * jm * (13 + 2 * (kb - 1) + 2 * kb)          # what cold_start reads of an NC_FLOAT set (fsm is NC_BYTE: a little less)
    file_bytes = 4 * im * jm * (13 + 2 * (kb + 2) + 2 * 10 * kb)
    free = shutil.disk_usage(where).free
    out = dict(tool="cold_start_io_probe", grid=f"{im}x{jm}x{kb}", case=args.case, dir=where, file_bytes_about=file_bytes, free_bytes=free)
    if not os.path.isdir(where) or not os.access(where, os.W_OK):
        out["error"] = "the directory is not writable"
        print(json.dumps(out))
        return 2
    if free < file_bytes + (1 << 30):
        out["skipped"] = "not enough room for the files"
        print(json.dumps(out))
        return 0
    if args.check:
        out["checked"] = "arguments and paths only: no time is reported without a GPU"
        print(json.dumps(out))
        return 0

    import numpy as np
    import torch
    import cold_start_expect as E
    from extpom_amd import decomp
    from extpom_amd.model import PomGpu, gpu_finish_initial
    d = pathlib.Path(tempfile.mkdtemp(prefix="cold_start_io_probe_", dir=where))
    try:
        E.NREC_CLIM = 10
        f = E.case_fields(args.case, im, jm, kb, dte=6.0, isplit=30)
        paths = E.write_files(d, f, kind="f", clim_records=10)
        del f
        out["file_bytes"] = sum(os.path.getsize(p) for p in paths)
        out["read_bytes"] = read_bytes
        tile = decomp.make_tile(0, im, jm, im, jm)
        nml = dict(dte=6.0, isplit=30)
        # ---- cold_start ----
        b = E.blank_state(tile, kb, **nml)
        g = PomGpu(b, device=0)
        torch.cuda.synchronize()
        t = time.perf_counter()
        info = g.cold_start(*paths)
        g.sync()
        out["cold_start_s"] = round(time.perf_counter() - t, 4)
        out["cflmin"], out["period"] = info["cflmin"], info["period"]
        g.download()
        g.close()
        # ---- today's other way: scipy, the readers' assignments on the host, gpu_finish_initial, upload ----
        t = time.perf_counter()
        v = E.read_files(paths)
        a = E.blank_state(tile, kb, **nml)
        a.z, a.zz = v["z"][:kb], v["zz"][:kb]
        a.dz[:kb - 1], a.dzz[:kb - 1] = a.z[:kb - 1] - a.z[1:], a.zz[:kb - 1] - a.zz[1:]
        for n, m in E.GRID_PLANES.items():
            a.field(m)[...] = v[n]
        fs = a.fsm
        a.dum, a.dvm = fs, fs
        a.dum[:, 1:][(fs[:, :-1] == 0) & (fs[:, 1:] != 0)] = 0.0
        a.dvm[1:, :][(fs[:-1, :] == 0) & (fs[1:, :] != 0)] = 0.0
        a.cor = 2.0 * 7.29e-5 * np.sin(a.north_e * (a.pi / 180.0))
        a.period = (2.0 * a.pi) / abs(a.cor[jm // 2 - 1, im // 2 - 1]) / 86400.0
        a.art = a.dx * a.dy
        a.aru[1:, 1:] = 0.25 * (a.dx[1:, 1:] + a.dx[1:, :-1]) * (a.dy[1:, 1:] + a.dy[1:, :-1])
        a.arv[1:, 1:] = 0.25 * (a.dx[1:, 1:] + a.dx[:-1, 1:]) * (a.dy[1:, 1:] + a.dy[:-1, 1:])
        a.aru[:, 0], a.arv[:, 0] = a.aru[:, 1], a.arv[:, 1]
        a.aru[0, :], a.arv[0, :] = a.aru[1, :], a.arv[1, :]
        a.d, a.dt = a.h + a.el, a.h + a.et
        a.tb[:kb - 1], a.sb[:kb - 1] = v["T"][0][:kb - 1], v["S"][0][:kb - 1]
        a.tclim, a.sclim = v["Tclim"][9], v["Sclim"][9]
        del v
        out["host_read_s"] = round(time.perf_counter() - t, 4)
        t = time.perf_counter()
        gpu_finish_initial(a, device=0)
        out["gpu_finish_initial_s"] = round(time.perf_counter() - t, 4)
        t = time.perf_counter()
        h = PomGpu(a, device=0)                                  # its constructor is the upload
        h.sync()
        out["upload_s"] = round(time.perf_counter() - t, 4)
        h.close()
        out["host_path_s"] = round(out["host_read_s"] + out["gpu_finish_initial_s"] + out["upload_s"], 4)
        # ---- the same state? ----
        ulp = lambda x, y: int(np.abs(x.view(np.int64) - y.view(np.int64)).max())
        differ = [n for n in E.diff(a, b) if n not in ("cor", "cbc", "con.period")]
        out["same_state"] = not differ
        out["cor_cbc_max_ulp"] = [ulp(a.cor, b.cor), ulp(a.cbc, b.cbc)]
        if differ:
            out["differ"] = differ[:12]
        del a, b
        # ---- the floor: the same number of bytes, sequentially, into one pinned buffer ----
        pin = torch.empty(CHUNK, dtype=torch.uint8).pin_memory().numpy()
        fd = os.open(paths[2], os.O_RDONLY)
        t = time.perf_counter()
        off = 0
        while off < read_bytes:
            n = os.preadv(fd, [memoryview(pin)[:min(CHUNK, read_bytes - off)]], off)
            if n <= 0:
                raise OSError("pread failed")
            off += n
        out["pread_floor_s"] = round(time.perf_counter() - t, 4)
        os.close(fd)
        out["cold_start_gb_s"] = round(read_bytes / out["cold_start_s"] / 1e9, 2)
        out["page_cache"] = "the files were written by this process just before: the rates are memory-to-memory, not the disk's"
    finally:
        shutil.rmtree(d, ignore_errors=True)
    for k in ("dir", "free_bytes", "file_bytes_about"):
        out.pop(k, None)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
