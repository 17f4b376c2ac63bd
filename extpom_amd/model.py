"""Host-side mirror of the reference's program flow for the hot path, over the C ABI.

``PomGpu`` owns one tile's device context.  Method names are the reference's subroutine names
(advance, lateral_viscosity, mode_interaction, mode_external, mode_internal, check_velocity, advct,
advq, ... : reference pom/advance.f, pom/solver.f); array arguments are given by field NAME and
resolved to the host address of that COMMON array -- what a Fortran caller passes by reference.
State crosses the boundary only through ``upload`` / ``download`` (whole COMMON blocks).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import lib as _lib
from .layout import P2, P3, PomState
from .lib import Dims, PomGpuError


class PomGpu:
    def __init__(self, st: PomState, device: int = 0, stream: int | None = None, libpath: str | None = None):
        self.L = _lib.load(libpath)
        self.st = st
        d = Dims(st.im, st.jm, st.kb, st.im_local, st.jm_local, st.n_west, st.n_east, st.n_south, st.n_north)
        h = ctypes.c_void_p()
        rc = self.L.pomgpu_create(ctypes.byref(h), ctypes.byref(d), device, ctypes.c_void_p(stream or 0))
        if rc != 0:
            raise PomGpuError(f"pomgpu_create failed with status {rc} (no CPU fallback exists for the hot path)")
        self.h = h
        self._exch_cb = None
        self.upload()

    # ---- plumbing ------------------------------------------------------------------------
    def _chk(self, rc, what):
        if rc != 0:
            raise PomGpuError(f"{what}: status {rc}: {self.L.pomgpu_last_error(self.h).decode()}")

    @staticmethod
    def _p(a):
        return ctypes.c_void_p(a.ctypes.data)

    def tune_placement(self, steps: int = 3, max_try: int = 6):
        """pomgpu_tune_placement: try a few start offsets of the 3-D arrays inside one allocation, keep the fastest (the model
        advances by tried x (steps + 1) internal steps).  Returns {"tried": n, "front_mib": [...], "ms_per_step": [...], "kept": k}."""
        ms = (ctypes.c_double * max_try)()
        fr = (ctypes.c_long * max_try)()
        pd = (ctypes.c_long * max_try)()
        n, k = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(self.L.pomgpu_tune_placement(self.h, steps, max_try, ms, fr, pd, ctypes.byref(n), ctypes.byref(k)), "tune_placement")
        return {"tried": n.value, "front_mib": [int(fr[q]) for q in range(n.value)], "pad_mib": [int(pd[q]) for q in range(n.value)],
                "ms_per_step": [round(float(ms[q]), 3) for q in range(n.value)], "kept": k.value}

    def close(self):
        if getattr(self, "h", None):
            self.L.pomgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, st: PomState | None = None):
        st = st or self.st
        self.st = st
        self._chk(self.L.pomgpu_upload(self.h, self._p(st.blk1d), self._p(st.blk2d), self._p(st.blk3d), self._p(st.bdry),
                                       self._p(st.con), 1 if getattr(st, "lramp", False) else 0), "upload")
        self._chk(self.L.pomgpu_bind_host(self.h, self._p(st.blk2d), self._p(st.blk3d)), "bind_host")
        for n, (tr, sr) in enumerate(getattr(st, "restore_records", []), start=1):
            tr = np.ascontiguousarray(tr, dtype=np.float64)
            sr = np.ascontiguousarray(sr, dtype=np.float64)
            self._chk(self.L.pomgpu_set_restore_record(self.h, n, self._p(tr), self._p(sr)), "set_restore_record")
        if getattr(st, "restore_rate_records", None):
            self.set_restore_rate_records(st.restore_rate_records)

    def set_restore_rate_records(self, records):
        """pomgpu_set_restore_rate_record: records[n-1], (kb, jm, im) in 1/day on the sigma levels, is the restore rate that goes with
        T/S record n (a sponge); None leaves that record's rate at the reference's 1/trst"""
        for n, tau in enumerate(records, start=1):
            if tau is None:
                continue
            tau = np.ascontiguousarray(tau, dtype=np.float64)
            if tau.shape != (self.st.kb, self.st.jm, self.st.im):
                raise ValueError(f"set_restore_rate_records: record {n} is {tau.shape}, not (kb, jm, im) = {(self.st.kb, self.st.jm, self.st.im)}")
            self._chk(self.L.pomgpu_set_restore_rate_record(self.h, n, self._p(tau)), "set_restore_rate_record")

    def set_restore_rate_file(self, path, im_global=None, jm_global=None):
        """pomgpu_set_restore_rate_file: restore_interior takes the rate that goes with T/S record n from record n of this classic NetCDF
        file (`z`, and `tau` on its levels; one record serves every n) and maps it onto the sigma levels with ztosig, on the device.  This
        tile's patch starts at (i_off+1, j_off+1) of the global grid, as in set_forcing_files."""
        st = self.st
        m = _lib.FileMeta(b"", b"", im_global or st.im, jm_global or st.jm, st.i_off + 1, st.j_off + 1, 0, None)
        self._chk(self.L.pomgpu_set_restore_rate_file(self.h, None if path is None else str(path).encode(), ctypes.byref(m)), "set_restore_rate_file")

    def set_forcing_records(self, first: int = 1, count: int = 4):
        """hand records first..first+count-1 of st.forcing_records (wind / heat / surface) to the library: what the
        host's read_wind_pnetcdf etc. would deliver; the library keeps the last four per kind"""
        for kind, name in enumerate(("wind", "heat", "surface")):
            recs = getattr(self.st, "forcing_records", {}).get(name, [])
            for n in range(first, min(first + count, len(recs) + 1)):
                a = np.ascontiguousarray(recs[n - 1][0], dtype=np.float64)
                b = np.ascontiguousarray(recs[n - 1][1], dtype=np.float64)
                self._chk(self.L.pomgpu_set_forcing_record(self.h, kind, n, self._p(a), self._p(b)), "set_forcing_record")

    def set_water_records(self, first: int = 0, count: int = 4):
        """pomgpu_set_water_record: hand records first..first+count-1 of st.water_records (a dict n -> (jm, im) array, n >= 0: what
        read_water_pnetcdf(n, ...) would deliver) to the library, which keeps the last four; the first one switches water on"""
        recs = getattr(self.st, "water_records", {})
        for n in range(first, first + count):
            if n in recs:
                w = np.ascontiguousarray(recs[n], dtype=np.float64)
                if w.shape != (self.st.jm, self.st.im):
                    raise ValueError(f"set_water_records: record {n} is {w.shape}, not (jm, im) = {(self.st.jm, self.st.im)}")
                self._chk(self.L.pomgpu_set_water_record(self.h, n, self._p(w)), "set_water_record")

    def set_water_files(self, prefix, im_global=None, jm_global=None):
        """pomgpu_set_water_files: from now on water takes record n from <prefix>.water.NNNN.nc (one record per file, `w`), on the
        device; switches water on.  This tile's patch starts at (i_off+1, j_off+1) of the global grid, as in set_forcing_files."""
        st = self.st
        m = _lib.FileMeta(b"", b"", im_global or st.im, jm_global or st.jm, st.i_off + 1, st.j_off + 1, 0, None)
        self._chk(self.L.pomgpu_set_water_files(self.h, None if prefix is None else str(prefix).encode(), ctypes.byref(m)), "set_water_files")

    def set_water(self, on: bool = True):
        """pomgpu_set_water: advance / run / surface_forcing call water (on) or leave wssurf alone (off)"""
        self._chk(self.L.pomgpu_set_water(self.h, 1 if on else 0), "set_water")

    def water(self):
        """pomgpu_water (bounds_forcing.f:986-1020) for the current iint and time"""
        self.call("water")

    def set_surface_sss(self, on: bool = True):
        """pomgpu_set_surface_sss: surface also sets ssurf from the record's SSS (bounds_forcing.f:979 uncommented)"""
        self._chk(self.L.pomgpu_set_surface_sss(self.h, 1 if on else 0), "set_surface_sss")

    def set_lateral_records(self, first: int = 1, count: int = 4):
        """hand records first..first+count-1 of st.lateral_records (20 arrays each, see pomgpu.h) to the library"""
        recs = getattr(self.st, "lateral_records", [])
        for n in range(first, min(first + count, len(recs) + 1)):
            arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in recs[n - 1]]
            ptrs = (ctypes.c_void_p * 20)(*[a.ctypes.data for a in arrs])
            self._chk(self.L.pomgpu_set_lateral_record(self.h, n, ptrs), "set_lateral_record")

    def download(self, st: PomState | None = None) -> PomState:
        st = st or self.st
        self._chk(self.L.pomgpu_download(self.h, self._p(st.blk1d), self._p(st.blk2d), self._p(st.blk3d), self._p(st.bdry),
                                         self._p(st.con)), "download")
        return st

    def set_con(self, **kw):
        """update blkcon scalars (iint, iext, ...) on the library side"""
        for k, v in kw.items():
            self.st.con[k][0] = v
        self._chk(self.L.pomgpu_set_con(self.h, self._p(self.st.con), 1 if getattr(self.st, "lramp", False) else 0),
                  "set_con")

    def get_con(self):
        self._chk(self.L.pomgpu_get_con(self.h, self._p(self.st.con)), "get_con")
        return self.st.con

    def sync(self):
        self._chk(self.L.pomgpu_sync(self.h), "sync")

    def current_stream(self) -> int:
        """the hipStream_t the library is enqueueing on right now: inside a transport callback, the stream of the round being served"""
        return int(self.L.pomgpu_current_stream(self.h) or 0)

    def device_ptr(self, name: str) -> int:
        if name in P3:
            return self.L.pomgpu_device_3d(self.h, P3[name])
        return self.L.pomgpu_device_2d(self.h, P2[name])

    def set_exchange(self, fn):
        """fn(list_of_device_addresses, list_of_levels) -- see extpom_amd.halo"""
        def cb(user, ptrs, nz, count):
            fn([ptrs[n] for n in range(count)], [nz[n] for n in range(count)])
        self._exch_cb = _lib.EXCHANGE_FN(cb)
        self._chk(self.L.pomgpu_set_exchange(self.h, self._exch_cb, None), "set_exchange")

    # ---- the library's own exchange (pomgpu.h "transport") ------------------------------------
    @staticmethod
    def neighbours8(tile):
        """ranks in the C ABI's direction order W E S N SW SE NW NE"""
        return [tile.n_west, tile.n_east, tile.n_south, tile.n_north, tile.n_sw, tile.n_se, tile.n_nw, tile.n_ne]

    def set_transport(self, tile, fn, agree=None, stream_ordered=False):
        """callback mover (tests): fn(send, scount, recv, rcount), each a list of eight (device address, doubles).
        stream_ordered: fn enqueues its copies on self.current_stream() (pomgpu_transport_stream_ordered): rounds of the library's second
        stream reach it without that stream having been completed first.
        agree: the host's reduction over ALL ranks -- agree(mine: int) -> min over the ranks -- through which the ranks
        settle whether message rounds may run on the library's second stream (all of them or none, pomgpu.h); without
        it every round stays on the main stream."""
        def cb(user, send, scount, recv, rcount):
            fn([send[d] for d in range(8)], [scount[d] for d in range(8)], [recv[d] for d in range(8)], [rcount[d] for d in range(8)])
        self._tp_cb = _lib.TRANSPORT_FN(cb)
        nb = (ctypes.c_int * 8)(*self.neighbours8(tile))
        self._chk(self.L.pomgpu_set_transport(self.h, nb, self._tp_cb, None), "set_transport")
        if stream_ordered:
            self._chk(self.L.pomgpu_transport_stream_ordered(self.h, 1), "transport_stream_ordered")
        if agree is not None:
            self.side_agree(agree)

    def side_capable(self) -> int:
        """this rank's own answer: could it serve message rounds on a second stream?"""
        return int(self.L.pomgpu_transport_side_capable(self.h))

    def side_agree(self, agree):
        """collective: agree(mine) must return the minimum of `mine` over all ranks of the decomposition.  The ranks first
        compare the digest of the switches that choose which message rounds exist (pomgpu.h): ranks started with different
        POMGPU_* sets are all refused here instead of hanging in a later round."""
        d = int(self.L.pomgpu_switch_digest(self.h))
        lo, hi = int(agree(d)), -int(agree(-d))
        if lo != hi:
            raise PomGpuError("the ranks were created under different POMGPU_* switch sets (those that choose the message rounds): "
                              "give every rank the same environment")
        self._chk(self.L.pomgpu_transport_side_agree(self.h, int(agree(self.side_capable()))), "transport_side_agree")

    def switch(self, name: str, value=None):
        """one developer switch of this live context (pomgpu_debug_switch): value None unsets it.  The library reads its
        switches from the environment once, when the context is created."""
        v = None if value is None else str(value).encode()
        self._chk(self.L.pomgpu_debug_switch(self.h, name.encode(), v), "debug_switch")

    def rccl_nranks(self) -> int:
        """what ncclCommCount says about the transport's communicator (0: no RCCL transport)"""
        return int(self.L.pomgpu_rccl_nranks(self.h))

    def rccl_init(self, tile, id128: bytes, rank: int, nranks: int, librccl: str | None = None):
        """production mover: grouped ncclSend / ncclRecv on the library's stream"""
        nb = (ctypes.c_int * 8)(*self.neighbours8(tile))
        buf = ctypes.create_string_buffer(bytes(id128), 128)
        self._chk(self.L.pomgpu_rccl_init(self.h, buf, rank, nranks, nb, librccl.encode() if librccl else None), "rccl_init")

    def clear_transport(self):
        """back to a single tile's behaviour (or to the hooks installed afterwards)"""
        self._chk(self.L.pomgpu_set_transport(self.h, None, _lib.TRANSPORT_FN(), None), "clear_transport")

    def rccl_unique_id(self, librccl: str | None = None) -> bytes:
        buf = ctypes.create_string_buffer(128)
        rc = self.L.pomgpu_rccl_unique_id(buf, librccl.encode() if librccl else None)
        if rc != 0:
            raise PomGpuError(f"pomgpu_rccl_unique_id failed with status {rc}")
        return buf.raw

    def exchange_rounds(self) -> int:
        return int(self.L.pomgpu_exchange_rounds(self.h))

    def exchange_rounds_side(self) -> int:
        """message rounds the library served on its second stream (beside kernels of the main stream)"""
        return int(self.L.pomgpu_exchange_rounds_side(self.h))

    def set_wide_external(self, on: bool, min_im: int, min_jm: int) -> bool:
        """collective; False when the tiles are too narrow (the per-point exchanges stay in use)"""
        rc = self.L.pomgpu_set_wide_external(self.h, 1 if on else 0, int(min_im), int(min_jm))
        if rc == -1 and on and self.L.pomgpu_last_error(self.h).decode().startswith("wide external mode: tiles"):
            return False
        self._chk(rc, "set_wide_external")
        return bool(on)

    def domain_stats(self, sums_only=False):
        """(vtot, atot, mtot, stot, tavg, savg, eavg, ekin) of advance.f:644-756, reduced on the device"""
        out = (ctypes.c_double * 8)()
        self._chk(self.L.pomgpu_domain_stats(self.h, out, 1 if sums_only else 0), "domain_stats")
        return tuple(out)

    TRACER_FILE_KINDS = {"tracer_restart": 0, "tracer_output": 1, "tracer_output_mean": 2}

    def write_file(self, kind, path, title="", time_start="", im_global=None, jm_global=None, create=True, stats=None, trstats=None):
        """kind = "output" | "restart": the reference's NetCDF (CDF-2) files without PnetCDF (io_pnetcdf.F:57-410,
        :1661-2083); this tile's patch at (i_off+1, j_off+1) of the global grid.  kind = "output_mean": the output file with the
        time means of uab vab elb u v t s rho w since set_mean_output or the last such file in place of their values now.
        kind = "tracer_restart" | "tracer_output" | "tracer_output_mean": the tracers' own files (pomgpu_write_tracers); trstats: the
        rank-reduced (ntr, 4) statistics of the two output kinds, None = this tile's own.  kind = "floats": the float file
        (pomgpu_write_floats), output and checkpoint of the Lagrangian floats in one.  kind = "harmonics": mean, amplitude and phase maps of elb uab
        vab per constituent from the harmonic analysis (pomgpu_write_harmonics); writing resets nothing"""
        st = self.st
        m = _lib.FileMeta(title.encode(), time_start.encode(), im_global or st.im, jm_global or st.jm, st.i_off + 1, st.j_off + 1,
                          1 if create else 0, (ctypes.c_double * 8)(*stats) if stats is not None else None)
        if kind == "harmonics":
            self._chk(self.L.pomgpu_write_harmonics(self.h, str(path).encode(), ctypes.byref(m)), "write_harmonics")
            return
        if kind == "floats":
            self._chk(self.L.pomgpu_write_floats(self.h, str(path).encode(), ctypes.byref(m)), "write_floats")
            return
        if kind in self.TRACER_FILE_KINDS:
            ts = None
            if trstats is not None:
                flat = [float(x) for x in np.asarray(trstats, dtype=np.float64).ravel()]
                if len(flat) != 4 * self.tracer_count():
                    raise ValueError(f"write_file: trstats holds {len(flat)} values, not 4 x {self.tracer_count()}")
                ts = (ctypes.c_double * len(flat))(*flat)
            self._chk(self.L.pomgpu_write_tracers(self.h, str(path).encode(), ctypes.byref(m), self.TRACER_FILE_KINDS[kind], ts), "write_" + kind)
            return
        fn = {"output": self.L.pomgpu_write_output, "output_mean": self.L.pomgpu_write_output_mean, "restart": self.L.pomgpu_write_restart}[kind]
        self._chk(fn(self.h, str(path).encode(), ctypes.byref(m)), "write_" + kind)

    MEAN_FIELDS = ("uab", "vab", "elb", "u", "v", "t", "s", "rho", "w")

    def set_mean_output(self, on: bool = True):
        """pomgpu_set_mean_output: from now on every internal step adds uab vab elb u v t s rho w, as they stand after mode_internal,
        to fp64 accumulators on the device; calling it again zeroes them, on=False frees them.  Tune the placement first."""
        self._chk(self.L.pomgpu_set_mean_output(self.h, 1 if on else 0), "set_mean_output")

    def mean_count(self) -> int:
        """internal steps accumulated since set_mean_output or the last mean file; -1 while the mean is off"""
        return int(self.L.pomgpu_mean_count(self.h))

    def mean_accumulate(self):
        """pomgpu_mean_accumulate, for a host that strings the routines together: after mode_internal (advance and run do it themselves)"""
        self._chk(self.L.pomgpu_mean_accumulate(self.h), "mean_accumulate")

    def mean(self, name: str):
        """pomgpu_mean_download: accumulator / count of one of MEAN_FIELDS, shaped like self.st.field(name); resets nothing"""
        if name not in self.MEAN_FIELDS:
            raise PomGpuError(f"mean: {name!r} is not accumulated (one of {' '.join(self.MEAN_FIELDS)})")
        out = np.empty_like(self.st.field(name))
        is3d = name in P3
        self._chk(self.L.pomgpu_mean_download(self.h, 1 if is3d else 0, P3[name] if is3d else P2[name], self._p(out)), "mean_download")
        return out

    # ---- passive tracers (pomgpu.h "passive tracers") ------------------------------------------
    TRACER_ARRAYS = {"trb": 0, "tr": 1, "clim": 2, "source": 3, "wsurf": 4, "surf": 5, "be": 6, "bw": 7, "bn": 8, "bs": 9}

    def tracer_shape(self, name: str):
        """shape of a tracer array on the host: trb tr clim source as tb, wsurf surf as wtsurf, be bw as tbe, bn bs as tbn"""
        st = self.st
        if name in ("trb", "tr", "clim", "source"):
            return (st.kb, st.jm_local, st.im_local)
        if name in ("wsurf", "surf"):
            return (st.jm_local, st.im_local)
        if name in ("be", "bw"):
            return (st.kb, st.jm_local)
        if name in ("bn", "bs"):
            return (st.kb, st.im_local)
        raise PomGpuError(f"tracer array {name!r}: one of {' '.join(self.TRACER_ARRAYS)}")

    def set_tracers(self, n: int):
        """pomgpu_set_tracers: n passive tracers (0..8), every array of theirs +0.0, nbc 1, no decay, no source; 0 frees them"""
        self._chk(self.L.pomgpu_set_tracers(self.h, int(n)), "set_tracers")

    def tracer_count(self) -> int:
        return int(self.L.pomgpu_tracer_count(self.h))

    def tracer_upload(self, n: int, name: str, a):
        """array `name` (TRACER_ARRAYS) of tracer n (1-based); a=None returns clim / source to the default"""
        if a is None:
            self._chk(self.L.pomgpu_tracer_upload(self.h, int(n), self.TRACER_ARRAYS[name], None), "tracer_upload")
            return
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != self.tracer_shape(name):
            raise ValueError(f"tracer_upload: {name} is {a.shape}, not {self.tracer_shape(name)}")
        self._chk(self.L.pomgpu_tracer_upload(self.h, int(n), self.TRACER_ARRAYS[name], self._p(a)), "tracer_upload")

    def tracer_download(self, n: int, name: str):
        out = np.empty(self.tracer_shape(name))
        self._chk(self.L.pomgpu_tracer_download(self.h, int(n), self.TRACER_ARRAYS[name], self._p(out)), "tracer_download")
        return out

    def set_tracer(self, n: int, nbc: int = 1, decay: float = 0.0):
        """pomgpu_tracer_set: surface condition 1 (the flux wsurf) or 3 (the value surf), and the decay rate in 1/s"""
        self._chk(self.L.pomgpu_tracer_set(self.h, int(n), int(nbc), float(decay)), "tracer_set")

    def tracer_get(self, n: int):
        """pomgpu_tracer_get: (nbc, decay) of tracer n as set_tracer or a tracer file left them"""
        nbc, lam = ctypes.c_int(), ctypes.c_double()
        self._chk(self.L.pomgpu_tracer_get(self.h, int(n), ctypes.byref(nbc), ctypes.byref(lam)), "tracer_get")
        return nbc.value, lam.value

    def tracer_stats(self):
        """pomgpu_tracer_stats: (ntr, 4) -- tot avg min max per tracer, reduced on the device; tot is this tile's share of the inventory"""
        out = np.empty((self.tracer_count(), 4))
        self._chk(self.L.pomgpu_tracer_stats(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "tracer_stats")
        return out

    def tracer_mean_count(self) -> int:
        """steps accumulated into the tracers' means; -1 unless the mean is on and tracers are registered"""
        return int(self.L.pomgpu_tracer_mean_count(self.h))

    def tracer_mean(self, n: int):
        """pomgpu_tracer_mean_download: accumulator / count of tracer n, shaped like tr; resets nothing"""
        out = np.empty(self.tracer_shape("tr"))
        self._chk(self.L.pomgpu_tracer_mean_download(self.h, int(n), self._p(out)), "tracer_mean_download")
        return out

    def read_tracers(self, path, im_global=None, jm_global=None):
        """pomgpu_read_tracers: this tile's patch of trNN (and trbNN, trfNN, nbcNN, lamNN where the file has them) of every registered
        tracer from a classic NetCDF file straight into the device arrays.  Returns (time, iint) of the file, applied to nothing."""
        st = self.st
        m = _lib.FileMeta(b"", b"", im_global or st.im, jm_global or st.jm, st.i_off + 1, st.j_off + 1, 0, None)
        t, ii = ctypes.c_double(), ctypes.c_double()
        self._chk(self.L.pomgpu_read_tracers(self.h, str(path).encode(), ctypes.byref(m), ctypes.byref(t), ctypes.byref(ii)), "read_tracers")
        return t.value, ii.value

    # ---- Lagrangian floats (pomgpu.h "Lagrangian floats") ---------------------------------------
    FLOAT_ACTIVE, FLOAT_EXITED, FLOAT_LOST = 0, 1, 2
    FLOAT_SAMPLES = ("lon", "lat", "depth", "t", "s")

    def set_floats(self, x, y, sig, kind=None, ids=None, sort=False):
        """pomgpu_float_upload: floats at the index coordinates x, y (cell centre (i, j) at x = i, y = j) and sigma sig; kind 0 follows w,
        1 keeps its sigma (None: all 0); ids: the caller's numbers (None: 0..n-1).  Empty arrays free the floats.  sort=True orders them
        by containing cell (jc * im + ic, stable) so that neighbours in memory gather from neighbouring cells; ids keep the caller's
        numbering.  Floats drift a few hundredths of a cell a step: a host re-sorts at output times if it wants to."""
        x, y, sig = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (x, y, sig))
        n = x.size
        if y.size != n or sig.size != n:
            raise ValueError(f"set_floats: x, y, sig hold {x.size}, {y.size}, {sig.size} values")
        kind = np.zeros(n, dtype=np.int32) if kind is None else np.ascontiguousarray(kind, dtype=np.int32).ravel()
        ids = np.arange(n, dtype=np.int32) if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ravel()
        if kind.size != n or ids.size != n:
            raise ValueError(f"set_floats: kind, ids hold {kind.size}, {ids.size} values, not {n}")
        if sort and n:
            with np.errstate(invalid="ignore"):
                ic = np.clip(np.floor(np.nan_to_num(x, nan=0.0) + 0.5), 1, self.st.im)
                jc = np.clip(np.floor(np.nan_to_num(y, nan=0.0) + 0.5), 1, self.st.jm)
            order = np.argsort(jc * self.st.im + ic, kind="stable")
            x, y, sig, kind, ids = (np.ascontiguousarray(a[order]) for a in (x, y, sig, kind, ids))
        self._chk(self.L.pomgpu_float_upload(self.h, n, self._p(x), self._p(y), self._p(sig), self._p(kind), self._p(ids)), "float_upload")

    def float_count(self) -> int:
        return int(self.L.pomgpu_float_count(self.h))

    def floats(self) -> dict:
        """pomgpu_float_download: {"x", "y", "sig" (float64), "status", "kind", "id" (int32)}"""
        n = self.float_count()
        out = {k: np.empty(n) for k in ("x", "y", "sig")}
        out.update({k: np.empty(n, dtype=np.int32) for k in ("status", "kind", "id")})
        self._chk(self.L.pomgpu_float_download(self.h, *[self._p(out[k]) for k in ("x", "y", "sig", "status", "kind", "id")]), "float_download")
        return out

    def float_step(self):
        """pomgpu_float_step: the floats' stage alone, for a host that strings the routines together (advance and run do it themselves)"""
        self._chk(self.L.pomgpu_float_step(self.h), "float_step")

    def float_sample(self) -> dict:
        """pomgpu_float_sample: {"lon", "lat", "depth", "t", "s"} of every float, whatever its status"""
        out = np.empty((5, max(self.float_count(), 1)))
        self._chk(self.L.pomgpu_float_sample(self.h, self._p(out)), "float_sample")
        return {k: out[q].copy() for q, k in enumerate(self.FLOAT_SAMPLES)}

    def read_floats(self, path):
        """pomgpu_read_floats: registers the floats of a float file (x y sig required; status kind id where the file has them) as
        set_floats would.  Returns (time, iint) of the file, applied to nothing."""
        m = _lib.FileMeta(b"", b"", self.st.im, self.st.jm, 1, 1, 0, None)
        t, ii = ctypes.c_double(), ctypes.c_double()
        self._chk(self.L.pomgpu_read_floats(self.h, str(path).encode(), ctypes.byref(m), ctypes.byref(t), ctypes.byref(ii)), "read_floats")
        return t.value, ii.value

    # ---- tides (pomgpu.h "tides") -------------------------------------------------------------
    TIDE_SIDES = ("east", "south", "west", "north")             # the order of the POMGPU_SIDE_* bits and of pomgpu_set_tides' lines
    HARMONIC_FIELDS = ("elb", "uab", "vab")

    @staticmethod
    def tide_coefficients(amp, pha):
        """amplitude A and Greenwich-style phase g in degrees, A cos(omega t - g), as the C interface's C = A cos g, S = A sin g"""
        import math
        amp = np.asarray(amp, dtype=np.float64)
        g = np.asarray(pha, dtype=np.float64) * (math.pi / 180.0)
        cos, sin = np.frompyfunc(math.cos, 1, 1), np.frompyfunc(math.sin, 1, 1)      # the C library's, as pomgpu_set_tide_file converts
        return amp * cos(g).astype(np.float64), amp * sin(g).astype(np.float64)

    def set_tides(self, omega=(), im_global=None, jm_global=None, **sides):
        """pomgpu_set_tides: omega in rad/s, one per constituent (none: the table is cleared); per open side that carries a tide
        east= / south= / west= / north= dict(el_amp, el_pha[, un_amp, un_pha]), each (ncon, jm_global | im_global): the elevation in metres and
        the depth-mean NORMAL velocity in m/s in the model's +i / +j sense, as amplitude and phase in degrees, A cos(omega t - g).  The
        GLOBAL lines, the same on every rank: the library cuts this tile's stretch at (i_off+1, j_off+1) and the extended tile's."""
        st = self.st
        omega = np.ascontiguousarray(omega, dtype=np.float64).ravel()
        nc = omega.size
        ig, jg = im_global or st.im, jm_global or st.jm
        unknown = set(sides) - set(self.TIDE_SIDES)
        if unknown:
            raise ValueError(f"set_tides: {sorted(unknown)} is not one of {' '.join(self.TIDE_SIDES)}")
        keep, ptrs, bits = [], [None] * 16, 0
        for s, name in enumerate(self.TIDE_SIDES):
            d = sides.get(name)
            if d is None:
                continue
            bits |= 1 << s
            n = jg if name in ("east", "west") else ig
            for q0, (ka, kp) in enumerate((("el_amp", "el_pha"), ("un_amp", "un_pha"))):
                if d.get(ka) is None and d.get(kp) is None:
                    continue
                if d.get(ka) is None or d.get(kp) is None:
                    raise ValueError(f"set_tides: {name} needs both {ka} and {kp}")
                C, S = self.tide_coefficients(d[ka], d[kp])
                for q, a in ((2 * q0, C), (2 * q0 + 1, S)):
                    a = np.ascontiguousarray(a, dtype=np.float64)
                    if a.shape != (nc, n):
                        raise ValueError(f"set_tides: {name} {ka} is {a.shape}, not (ncon, n_global) = {(nc, n)}")
                    keep.append(a)
                    ptrs[4 * s + q] = a.ctypes.data
        m = _lib.FileMeta(b"", b"", ig, jg, st.i_off + 1, st.j_off + 1, 0, None)
        arr = (ctypes.c_void_p * 16)(*ptrs)
        self._chk(self.L.pomgpu_set_tides(self.h, nc, self._p(omega) if nc else None, bits, arr, ctypes.byref(m)), "set_tides")

    def set_tide_file(self, path, im_global=None, jm_global=None):
        """pomgpu_set_tide_file: the table from a classic NetCDF file -- omega(ncon) and per side el_amp.<side> el_pha.<side> [un_amp.<side>
        un_pha.<side>], (ncon, jm_global | im_global) -- as set_tides would register it"""
        st = self.st
        m = _lib.FileMeta(b"", b"", im_global or st.im, jm_global or st.jm, st.i_off + 1, st.j_off + 1, 0, None)
        self._chk(self.L.pomgpu_set_tide_file(self.h, str(path).encode(), ctypes.byref(m)), "set_tide_file")

    def tide_count(self) -> int:
        return int(self.L.pomgpu_tide_count(self.h))

    def tide_phasors(self, iint: int, iext: int):
        """pomgpu_tide_phasors: (ncon, 2) -- cos and sin of omega t at substep iext of internal step iint, as the host evaluates them"""
        out = np.empty((max(self.tide_count(), 1), 2))
        self._chk(self.L.pomgpu_tide_phasors(self.h, int(iint), int(iext), self._p(out)), "tide_phasors")
        return out[:self.tide_count()]

    def set_harmonic_analysis(self, on: bool = True, every: int = 1):
        """pomgpu_set_harmonic_analysis: from now on every internal step with iint % every == 0 adds elb uab vab, times 1 and times cos / sin
        of every constituent of the tide table, to fp64 sums on the device; calling it again zeroes them, on=False frees them"""
        self._chk(self.L.pomgpu_set_harmonic_analysis(self.h, 1 if on else 0, int(every)), "set_harmonic_analysis")

    def harmonic_accumulate(self):
        """pomgpu_harmonic_accumulate, for a host that strings the routines together (advance and run do it themselves)"""
        self._chk(self.L.pomgpu_harmonic_accumulate(self.h), "harmonic_accumulate")

    def harmonic_count(self) -> int:
        return int(self.L.pomgpu_harmonic_count(self.h))

    def harmonic_reset(self):
        self._chk(self.L.pomgpu_harmonic_reset(self.h), "harmonic_reset")

    def _harm_planes(self):
        return np.empty((1 + 2 * self.tide_count(), self.st.jm_local, self.st.im_local))

    def harmonic_sums(self, name: str):
        """pomgpu_harmonic_sums: (2 ncon + 1, jm_local, im_local) -- the sums of f, f cos, f sin, ... of one of HARMONIC_FIELDS"""
        out = self._harm_planes()
        self._chk(self.L.pomgpu_harmonic_sums(self.h, self.HARMONIC_FIELDS.index(name), self._p(out)), "harmonic_sums")
        return out

    def harmonic_matrix(self):
        """pomgpu_harmonic_matrix: the (2 ncon + 1)^2 normal matrix and (t_first, t_last) of the samples in seconds"""
        n = 1 + 2 * self.tide_count()
        out, t2 = np.empty((n, n)), np.empty(2)
        self._chk(self.L.pomgpu_harmonic_matrix(self.h, self._p(out), self._p(t2)), "harmonic_matrix")
        return out, (float(t2[0]), float(t2[1]))

    def harmonic_solve(self, name: str):
        """pomgpu_harmonic_solve: (2 ncon + 1, jm_local, im_local) -- the mean, then C and S of every constituent"""
        out = self._harm_planes()
        self._chk(self.L.pomgpu_harmonic_solve(self.h, self.HARMONIC_FIELDS.index(name), self._p(out)), "harmonic_solve")
        return out

    def harmonic_constants(self, name: str):
        """(mean, amp, pha) of harmonic_solve: amp (ncon, jm_local, im_local), pha in degrees in [0, 360): g of A cos(omega t - g)"""
        c = self.harmonic_solve(name)
        C, S = c[1::2], c[2::2]
        return c[0], np.hypot(C, S), np.mod(np.degrees(np.arctan2(S, C)), 360.0)

    def read_restart(self, path, im_global=None, jm_global=None):
        """read_restart_pnetcdf (io_pnetcdf.F:2420-2768) without PnetCDF: this tile's patch of the 37 restart fields from a classic
        NetCDF file straight into the device mirrors, d and dt formed from them, time0 = time = the file's time (and cont_bry, if it
        was non-zero, the file's iint).  Returns (time0, iint_in_file); self.st.con is refreshed, the arrays are NOT downloaded."""
        st = self.st
        m = _lib.FileMeta(b"", b"", im_global or st.im, jm_global or st.jm, st.i_off + 1, st.j_off + 1, 0, None)
        t0, ii = ctypes.c_double(), ctypes.c_double()
        self._chk(self.L.pomgpu_read_restart(self.h, str(path).encode(), ctypes.byref(m), ctypes.byref(t0), ctypes.byref(ii)), "read_restart")
        self.get_con()
        return t0.value, ii.value

    def cold_start(self, grid, init, clim, im_global=None, jm_global=None) -> dict:
        """pomgpu_cold_start: initialize.f:24-36 after read_input (initialize_arrays, read_grid, initial_conditions, update_initial,
        bottom_friction) from the reference's <...>.grid.nc, .init.nc and .clim.nc, on the device and without PnetCDF.  blkcon must
        hold read_input's constants (this context's st.con does).  This tile's patch starts at (i_off+1, j_off+1) of the global grid,
        as in read_restart.  Returns {"cflmin": the tile's minimum of cfl over cfl > 0, "period": from the tile's cor(im/2, jm/2)};
        self.st.con is refreshed, NO array is downloaded (download() brings the state over)."""
        st = self.st
        m = _lib.FileMeta(b"", b"", im_global or st.im, jm_global or st.jm, st.i_off + 1, st.j_off + 1, 0, None)
        info = _lib.ColdInfo()
        self._chk(self.L.pomgpu_cold_start(self.h, str(grid).encode(), str(init).encode(), str(clim).encode(), ctypes.byref(m), ctypes.byref(info)),
                  "cold_start")
        self.get_con()
        return {"cflmin": info.cflmin, "period": info.period}

    def set_z_inputs(self, init: bool = False, clim: bool = False, lbry: bool | None = None):
        """pomgpu_set_z_inputs: cold_start takes T, S of the init file (levels in `Level`) and / or Tclim, Sclim of the clim file (levels in
        `z`) as z-level data and maps them onto the sigma levels with ztosig (initialize.f:410-422).  lbry (given: pomgpu_set_z_lateral):
        temp, salt of the lbry file are on the levels of its `z` and every fetched record's lines are mapped (bounds_forcing.f:636-716)"""
        self._chk(self.L.pomgpu_set_z_inputs(self.h, 1 if init else 0, 1 if clim else 0), "set_z_inputs")
        if lbry is not None:
            self._chk(self.L.pomgpu_set_z_lateral(self.h, 1 if lbry else 0), "set_z_lateral")

    def set_lateral_sides(self, east: bool = True, south: bool = True, west: bool = False, north: bool = False):
        """pomgpu_set_lateral_sides: the open boundaries the lbry file feeds (the default is the reference's reader, io_pnetcdf.F:3393-3621).
        A side that is on takes zeta u v temp salt .<side> from the file; one that is off has t s from the line of tclim sclim next to it,
        u v zero and its elevation line as the state holds it, and its variables are not looked up.  Before set_forcing_files(lbry=...)."""
        sides = (1 if east else 0) | (2 if south else 0) | (4 if west else 0) | (8 if north else 0)
        self._chk(self.L.pomgpu_set_lateral_sides(self.h, sides), "set_lateral_sides")

    def set_forcing_files(self, sfrc=None, lbry=None, clim=None, im_global=None, jm_global=None):
        """pomgpu_set_forcing_files: from now on wind / heat / surface (sfrc), lateral_bc (lbry) and restore_interior (clim) take the
        records their schedule asks for from these classic NetCDF files, on the device; None leaves a source as it is.  This tile's
        patch starts at (i_off+1, j_off+1) of the global grid, as in read_restart."""
        st = self.st
        m = _lib.FileMeta(b"", b"", im_global or st.im, jm_global or st.jm, st.i_off + 1, st.j_off + 1, 0, None)
        enc = lambda p: None if p is None else str(p).encode()
        self._chk(self.L.pomgpu_set_forcing_files(self.h, enc(sfrc), enc(lbry), enc(clim), ctypes.byref(m)), "set_forcing_files")

    def io_wait(self):
        """join the host thread that is writing the last output / restart file (sync, the next write and close do it too)"""
        self._chk(self.L.pomgpu_io_wait(self.h), "io_wait")

    def set_order_exchange(self, fn):
        """fn(send_east, n_east, send_north, n_north, recv_west, recv_south): device addresses (baropg_mcc's
        order2d_mpi / order3d_mpi, packed by the library) -- see extpom_amd.halo.Halo.device_order_hook"""
        def cb(user, se, ne, sn, nn, rw, rs):
            fn(se, ne, sn, nn, rw, rs)
        self._order_cb = _lib.ORDER_FN(cb)
        self._chk(self.L.pomgpu_set_order_exchange(self.h, self._order_cb, None), "set_order_exchange")

    # ---- hot path, reference names -------------------------------------------------------
    def _a(self, name):
        return self._p(self.st.field(name))

    def call(self, name, *fields_or_ints):
        fn = getattr(self.L, "pomgpu_" + name)
        args = [self._a(a) if isinstance(a, str) else a for a in fields_or_ints]
        self._chk(fn(self.h, *args), name)

    def ztosig(self, zs, src, t: str):
        """pomgpu_ztosig (initialize.f:547-595): the z-level array src (ks, jm_local, im_local) on the levels zs (metres, positive down)
        splined onto the sigma levels of the COMMON array named t, with the h and zz of the mirrors; nothing is downloaded"""
        zs = np.ascontiguousarray(zs, dtype=np.float64)
        src = np.ascontiguousarray(src, dtype=np.float64)
        if zs.ndim != 1 or src.shape != (zs.size, self.st.jm_local, self.st.im_local):
            raise ValueError(f"ztosig: src {src.shape} is not (ks, jm_local, im_local) = {(zs.size, self.st.jm_local, self.st.im_local)}")
        self._chk(self.L.pomgpu_ztosig(self.h, self._p(zs), int(zs.size), self._p(src), self._a(t)), "ztosig")

    def ztosig_line(self, edge: int, zs, src):
        """pomgpu_ztosig_line (bounds_forcing.f:636-716): one lateral line, edge 0 east, 1 south, 2 west, 3 north, of z-level values
        src (ks, n_local + 2) -- line point a at [:, a], the window points beyond the ends at [:, 0] and [:, n + 1] -- onto the sigma levels
        with that edge's depth line; returns (kb, n_local), n_local = jm_local (east, west) or im_local (south, north)"""
        zs = np.ascontiguousarray(zs, dtype=np.float64)
        src = np.ascontiguousarray(src, dtype=np.float64)
        nl = self.st.jm_local if edge in (0, 2) else self.st.im_local
        if zs.ndim != 1 or src.shape != (zs.size, nl + 2):
            raise ValueError(f"ztosig_line: src {src.shape} is not (ks, n_local + 2) = {(zs.size, nl + 2)}")
        out = np.empty((self.st.kb, nl))
        self._chk(self.L.pomgpu_ztosig_line(self.h, int(edge), self._p(zs), int(zs.size), self._p(src), self._p(out)), "ztosig_line")
        return out

    PROBE_OPS = {"DIVI": (0, 2), "DIVI_F32": (1, 2), "GPOW15": (2, 1), "RAD_Q": (3, 5)}

    def math_probe(self, op, *arrays):
        """pomgpu_math_probe: the device's divi (op "DIVI": a, b; "DIVI_F32": the float overload on a, b narrowed), gpow15 ("GPOW15": x)
        or proft_rad_q ("RAD_Q": swrad, r, omr, x1, x2) on 1-D float64 arrays of one length, one element per lane; returns the results"""
        code = self.PROBE_OPS[op][0] if isinstance(op, str) else int(op)
        arrs = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in arrays]
        n = arrs[0].size if arrs else 0
        if any(a.size != n for a in arrs):
            raise ValueError(f"math_probe: arrays of different lengths {[a.size for a in arrs]}")
        out = np.empty(max(n, 1))
        ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        self._chk(self.L.pomgpu_math_probe(self.h, code, n, ptrs, len(arrs), self._p(out)), "math_probe")
        return out[:n]

    def advance(self):
        self.call("advance")

    def run(self, nsteps: int):
        self._chk(self.L.pomgpu_run(self.h, int(nsteps)), "run")

    def check_velocity(self):
        v = ctypes.c_double()
        i = ctypes.c_int()
        j = ctypes.c_int()
        self._chk(self.L.pomgpu_check_velocity(self.h, ctypes.byref(v), ctypes.byref(i), ctypes.byref(j)), "check_velocity")
        return v.value, i.value, j.value

    # ---- measurement ---------------------------------------------------------------------
    def prof_begin(self, only: str | None = None):
        self._chk(self.L.pomgpu_prof_filter(self.h, (only or "").encode()), "prof_filter")
        self._chk(self.L.pomgpu_prof_begin(self.h), "prof_begin")

    def prof_end(self) -> dict:
        self._chk(self.L.pomgpu_prof_end(self.h), "prof_end")
        out = {}
        for k in range(self.L.pomgpu_prof_count(self.h)):
            name = ctypes.c_char_p()
            n = ctypes.c_long()
            ms = ctypes.c_double()
            self.L.pomgpu_prof_get(self.h, k, ctypes.byref(name), ctypes.byref(n), ctypes.byref(ms))
            out[name.value.decode()] = (n.value, ms.value)
        return out


def gpu_finish_initial(st: PomState, **kw) -> PomState:
    """finish_initial() with the HIP dens / baropg (what the reference's initialize does with its own)."""
    from .cases import finish_initial
    g = PomGpu(st, **kw)

    def dens(s, si, ti, rho):
        g.upload(s)
        g.call("dens", si, ti, rho)
        g.download(s)

    def baropg(s):
        g.upload(s)
        g.call("baropg_mcc" if int(s.npg) == 2 else "baropg")
        g.download(s)

    finish_initial(st, dens, baropg)
    g.close()
    return st
