#!/usr/bin/env python
"""How long does PomGpu.read_restart take beside the floor -- a plain sequential pread of the same file into one pinned buffer?

Writes a restart file of the given grid with the library, waits for it, then times the two in turn, `--repeats` times each in ONE
process, with a host clock around calls that end in a device synchronise.  Also timed: copying the same number of bytes from the
pinned buffer to the device, chunk by chunk (no file).  A reader that takes more than floor + that copy is not overlapping its
pread with its copies.  Prints one JSON line.  The file has just been written by this process, so it is normally still in the
page cache: the line says what fraction of its pages was resident (mincore) before the first and after the last read -- the
figures are then memory-to-memory rates, not the disk's.

    python tools/restart_io_probe.py --grid 1024x1024x40 [--dir /scratch] [--repeats 3] [--chunk-kb N]
    python tools/restart_io_probe.py --check      (no GPU: arguments, paths and free space only; reports no time)
"""
import argparse
import ctypes
import json
import mmap
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHUNK = 64 << 20


def resident_fraction(path):
    """fraction of the file's pages in the page cache (mincore on a mapping of it); None if it cannot be told"""
    import numpy as np
    size = os.path.getsize(path)
    if size == 0:
        return 0.0
    libc = ctypes.CDLL(None, use_errno=True)
    npages = (size + mmap.PAGESIZE - 1) // mmap.PAGESIZE
    vec = (ctypes.c_ubyte * npages)()
    with open(path, "rb") as f:
        m = mmap.mmap(f.fileno(), size, prot=mmap.PROT_READ)
        a = np.frombuffer(m, dtype=np.uint8)                    # ctypes' from_buffer wants a writable mapping: numpy gives the address
        rc = libc.mincore(ctypes.c_void_p(a.__array_interface__["data"][0]), ctypes.c_size_t(size), vec)
        del a
        m.close()
    if rc != 0:
        return None
    return round(float(np.frombuffer(vec, dtype=np.uint8).__and__(1).sum()) / npages, 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", default="1024x1024x40")
    ap.add_argument("--case", default="basin")
    ap.add_argument("--dir", default=None, help="where the file goes (default: the temporary directory)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk-kb", type=int, default=0, help="POMGPU_IO_CHUNK_KB for the reader (0: its default)")
    ap.add_argument("--check", action="store_true", help="arguments, paths and free space only; no GPU, no time")
    args = ap.parse_args()
    im, jm, kb = (int(v) for v in args.grid.lower().split("x"))
    where = args.dir or tempfile.gettempdir()
    nbytes = 8 * im * jm * (18 + 19 * kb)
    free = shutil.disk_usage(where).free
    out = dict(tool="restart_io_probe", grid=f"{im}x{jm}x{kb}", case=args.case, dir=where, file_bytes_about=nbytes, free_bytes=free)
    if not os.path.isdir(where) or not os.access(where, os.W_OK):
        out["error"] = "the directory is not writable"
        print(json.dumps(out))
        return 2
    if free < nbytes + (1 << 30):
        out["skipped"] = "not enough room for the file"
        print(json.dumps(out))
        return 0
    if args.check:
        out["checked"] = "arguments and paths only: no time is reported without a GPU"
        print(json.dumps(out))
        return 0

    import numpy as np
    import torch
    from extpom_amd.cases import make_case
    from extpom_amd.model import PomGpu
    st = make_case(args.case, im, jm, kb, dte=6.0, isplit=30)
    g = PomGpu(st, device=0)
    g.run(1)
    path = os.path.join(tempfile.mkdtemp(prefix="restart_io_probe_", dir=where), "restart.nc")
    try:
        t = time.perf_counter()
        g.write_file("restart", path, title="probe", time_start="2000-01-01 00:00:00 +00:00")
        g.io_wait()
        out["write_s"] = round(time.perf_counter() - t, 3)
        size = os.path.getsize(path)
        out["file_bytes"] = size
        out["resident_before"] = resident_fraction(path)
        if args.chunk_kb:
            g.switch("IO_CHUNK_KB", args.chunk_kb)
        pin = torch.empty(CHUNK, dtype=torch.uint8).pin_memory()
        pin_np = pin.numpy()
        dev = torch.empty(CHUNK, dtype=torch.uint8, device="cuda:0")
        fd = os.open(path, os.O_RDONLY)
        read_s, pread_s, h2d_s = [], [], []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            g.read_restart(path)
            g.sync()
            read_s.append(round(time.perf_counter() - t, 4))
            t = time.perf_counter()
            off = 0
            while off < size:
                n = os.preadv(fd, [memoryview(pin_np)[:min(CHUNK, size - off)]], off)
                if n <= 0:
                    raise OSError("pread failed")
                off += n
            torch.cuda.synchronize()
            pread_s.append(round(time.perf_counter() - t, 4))
            t = time.perf_counter()
            off = 0
            while off < size:
                n = min(CHUNK, size - off)
                dev[:n].copy_(pin[:n], non_blocking=True)
                off += n
            torch.cuda.synchronize()
            h2d_s.append(round(time.perf_counter() - t, 4))
        os.close(fd)
        out["resident_after"] = resident_fraction(path)
        out.update(read_restart_s=read_s, pread_floor_s=pread_s, h2d_same_bytes_s=h2d_s,
                   read_restart_gb_s=round(size / min(read_s) / 1e9, 2), pread_floor_gb_s=round(size / min(pread_s) / 1e9, 2),
                   page_cache="the file was written by this process just before: resident_* is the fraction of its pages in the page cache")
    finally:
        g.close()
        shutil.rmtree(os.path.dirname(path), ignore_errors=True)
    for k in ("dir", "free_bytes", "file_bytes_about"):
        out.pop(k, None)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
