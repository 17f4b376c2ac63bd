"""pomgpu_read_restart on the device: the pinned two-buffer pipeline and k_cdf_unpack as the GPU runs them (the host build of
tests/test_restart_read_emulated.py replaces the pipeline by a plain loop).  Same bar as there: the oracle started from the state
the reference's reader would leave, built from the file as scipy reads it (tests/restart_expect.py); 64-bit patterns throughout."""
import numpy as np
import pytest

from extpom_amd.cases import cut_tile
from extpom_amd.layout import BLK2D, BLK3D, RESTART_2D, RESTART_3D
import restart_expect
from restart_expect import M, RESTART, UNTOUCHED, check_read_state, diff, expected_state, file_values, fresh, same_bits, written, write_foreign_restart
from restart_expect import make_gpu as _gpu

pytestmark = pytest.mark.gpu
N = 7


def _oracle():
    from oracle.pyoracle import OracleTile, oracle_finish_initial
    return OracleTile, oracle_finish_initial


@pytest.mark.parametrize("case,nml,steps,chunk_kb", [("seamount", {}, N, None), ("island", {}, N, 64), ("archipelago", {}, N, None),
                                                     ("seamount", dict(isplit=7), 3, 26)], ids=str)
def test_round_trip(tmp_path, case, nml, steps, chunk_kb):
    """chunk_kb: POMGPU_IO_CHUNK_KB gives the two pinned buffers that size (never less than one level's band of rows, 25 KB here),
    so a 3-D variable takes 11 (64 KB: two levels per run) or 21 (26 KB: one) runs and both buffers are reused many times"""
    path, a = written(tmp_path, case, nml, steps)
    init = fresh(case, nml)
    b = init.copy()
    g = _gpu(b)
    if chunk_kb:
        g.switch("IO_CHUNK_KB", chunk_kb)
    time0, iint = g.read_restart(path)
    assert iint == steps and time0 == a.time and b.time0 == a.time
    g.download()
    for n in RESTART:
        assert same_bits(b.field(n), a.field(n)), n
    check_read_state(b, init, path)
    assert b.iint == 0 and b.error_status == 0
    g.close()


@pytest.mark.parametrize("case,nml", [("seamount", {}), ("archipelago", {}), ("archipelago", dict(npg=2)), ("seamount", dict(mode=2))], ids=str)
def test_continuation_equals_the_oracle_started_from_the_readers_state(tmp_path, case, nml):
    OracleTile, _ = _oracle()
    path, _w = written(tmp_path, case, nml, N)
    a = expected_state(case, 65, 49, 21, nml, path)
    b = fresh(case, nml)
    ot = OracleTile(a)
    g = _gpu(b)
    g.read_restart(path)
    for n in range(1, M + 1):
        ot.run(1)
        g.run(1)
        g.download()
        assert not diff(a, b) and same_bits(a.bdry, b.bdry), f"step {n}: {diff(a, b)}"
        assert a.iint == b.iint == n and a.time == b.time and a.time0 == b.time0
    g.close()
    u = fresh(case, nml)
    OracleTile(u).run(N + M)
    differs = [n for n in RESTART if not same_bits(u.field(n), b.field(n))]
    if nml.get("mode") == 2:
        assert not differs, differs                             # mode 2 continues seamlessly (measured with the oracle alone)
    elif not nml:
        assert differs                                          # the two default cases do not: the reference's list is not the whole state


def test_rows_longer_than_a_wavefront_256x192x50(tmp_path):
    """archipelago 256x192x50: im is four wavefronts, the 3-D variables are 19.7 MB each, and with 4 MiB buffers each takes five
    runs; round trip and three steps of the continuation"""
    OracleTile, _ = _oracle()
    grid, nml = (256, 192, 50), dict(dte=6.0, isplit=30)
    path, a = written(tmp_path, "archipelago", nml, 2, grid=grid)
    init = fresh("archipelago", nml, grid)
    b = init.copy()
    g = _gpu(b)
    g.switch("IO_CHUNK_KB", 4096)
    g.read_restart(path)
    g.download()
    for n in RESTART:
        assert same_bits(b.field(n), a.field(n)), n
    check_read_state(b, init, path)
    want = expected_state("archipelago", *grid, nml, path)
    ot = OracleTile(want)
    for n in range(1, 4):
        ot.run(1)
        g.run(1)
        g.download()
        assert not diff(want, b) and same_bits(want.bdry, b.bdry), f"step {n}: {diff(want, b)}"
    g.close()


def test_row_length_not_a_multiple_of_64_and_a_2x1_split_on_one_gpu(tmp_path):
    """130x49x21 written as one tile; two contexts on the one GPU read the two halves (66 columns each, two of them shared): each
    holds its window of the file, ghost columns included, and nothing else moved"""
    from extpom_amd import decomp
    grid = (130, 49, 21)
    path, a = written(tmp_path, "island", {}, 3, grid=grid)
    init = fresh("island", {}, grid)
    iml, jml = decomp.local_size(130, 49, 2, 1)
    tiles = [decomp.make_tile(r, 130, 49, iml, jml, n_proc=2) for r in range(2)]
    start = [cut_tile(init, t) for t in tiles]
    state = [t0.copy() for t0 in start]
    ctx = [_gpu(st) for st in state]                            # both contexts alive on the one GPU, each with its own copy stream and buffers
    for g in ctx:
        g.switch("IO_CHUNK_KB", 100)
    for g in ctx:
        g.read_restart(path, im_global=130, jm_global=49)
    for g in reversed(ctx):
        g.download()
    for r, (tile, t0, st) in enumerate(zip(tiles, start, state)):
        io, im, jm = tile.i_off, tile.im, tile.jm
        for n in RESTART:
            assert same_bits(st.field(n)[..., :jm, :im], a.field(n)[..., :jm, io:io + im]), (r, n)
            assert same_bits(st.field(n)[..., jm:, :], t0.field(n)[..., jm:, :]) and same_bits(st.field(n)[..., :, im:], t0.field(n)[..., :, im:]), (r, n)
        assert same_bits(st.d[:jm, :im], (init.h + a.el)[:jm, io:io + im]) and same_bits(st.dt[:jm, :im], (init.h + a.et)[:jm, io:io + im])
        assert not diff(st, t0, UNTOUCHED) and same_bits(st.bdry, t0.bdry)
    for g in ctx:
        g.close()
    # and as one tile: rows of 130 values, two wavefronts and a remainder
    b = init.copy()
    g = _gpu(b)
    g.read_restart(path)
    g.download()
    check_read_state(b, init, path)
    g.close()


@pytest.mark.parametrize("writing", [False, True], ids=["held odd substep", "held odd substep and a file being written"])
def test_reading_into_a_live_context(tmp_path, writing):
    """a held odd external substep (isplit = 7), and a restart file of the same context still being written by its host thread"""
    restart_expect.reading_into_a_live_context(tmp_path, writing)


def test_refusals_leave_the_state_untouched(tmp_path):
    restart_expect.refusals_leave_the_state_untouched(tmp_path)


def test_a_file_of_another_writer_cdf1(tmp_path):
    """scipy's CDF-1 layout (reversed order, extra variables, other dimension names, another alignment) through the device pipeline"""
    path, a = written(tmp_path, "island", {}, 2)
    vals, time, iint = file_values(path)
    write_foreign_restart(tmp_path / "foreign.nc", vals, time, iint, 21, 49, 65, version=1)
    init = fresh("island", {})
    b = init.copy()
    g = _gpu(b)
    g.switch("IO_CHUNK_KB", 64)
    assert g.read_restart(tmp_path / "foreign.nc") == (time, iint)
    g.download()
    check_read_state(b, init, tmp_path / "foreign.nc")
    g.close()


@pytest.mark.parametrize("variant", ["LIBPATH_F32", "LIBPATH_F32A"])
def test_fp32_builds_round_the_3d_fields_as_an_upload_does(tmp_path, variant):
    from extpom_amd import lib
    path, a = written(tmp_path, "archipelago", {}, 2)            # written by the fp64 build
    b = fresh("archipelago", {})
    g = _gpu(b, libpath=getattr(lib, variant))
    g.switch("IO_CHUNK_KB", 64)
    g.read_restart(path)
    g.download()
    for n in RESTART_3D:
        assert same_bits(b.field(n), a.field(n).astype(np.float32).astype(np.float64)), n
    for n in RESTART_2D:
        assert same_bits(b.field(n), a.field(n)), n
    assert same_bits(b.d, b.h + a.el) and same_bits(b.dt, b.h + a.et) and b.time0 == a.time
    g.close()


@pytest.mark.skipif(not __import__("os").path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="AMD flang not installed")
def test_fortran_driver_restarts_from_the_file(tmp_path):
    """pom_gpu_main with nread_rst = 1: read_restart_pnetcdf of pom_gpu_io.f90 builds <wrk_pth>in/<read_rst_file>, the library reads
    it, blkcon and the COMMON blocks come back, and the steps that follow equal the oracle started from the reader's state"""
    import os
    import subprocess
    import __graft_entry__ as ge
    OracleTile, _ = _oracle()
    fdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "extpom_amd", "fortran")
    ge.build_hip()
    subprocess.check_call(["make", "-C", fdir, "IM=65", "JM=49", "KB=21"], stdout=subprocess.DEVNULL)
    nsteps, nml = 4, dict(dte=6.0, isplit=30)
    os.mkdir(tmp_path / "in")
    path, _w = written(tmp_path / "in", "island", nml, N, name="restart.0007.nc")
    a = fresh("island", nml)
    with open(tmp_path / "state.in", "wb") as f:
        np.array([a.im, a.jm, -1, -1, -1, -1, nsteps, len(a.restore_records), a.bdry.size], dtype="<i4").tofile(f)
        for blk in (a.blk1d, a.blk2d, a.blk3d, a.bdry):
            blk.tofile(f)
        f.write(a.con.tobytes())
        for tr, sr in a.restore_records:
            np.ascontiguousarray(tr).tofile(f)
            np.ascontiguousarray(sr).tofile(f)
    (tmp_path / "pom.nml").write_text("&pom_nml\n title = 'island'\n wrk_pth = './'\n netcdf_file = 'nonetcdf'\n mode = 3\n nadv = 2\n nitera = 1\n sw = 0.5\n"
                                      " npg = 1\n dte = 6.\n isplit = 30\n nread_rst = 1\n read_rst_file = 'restart.0007.nc'\n cont_bry = 0\n days = 1\n/\n")
    r = subprocess.run([os.path.join(fdir, "pom_gpu_main"), "state.in", "state.out"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "error_status   0" in r.stdout and "reading file ./in/restart.0007.nc" in r.stdout, r.stdout + r.stderr
    want = expected_state("island", 65, 49, 21, nml, path)
    OracleTile(want).run(nsteps)
    raw = np.fromfile(tmp_path / "state.out", dtype="<f8")
    n2, n3 = a.blk2d.size, a.blk3d.size
    b2, b3 = raw[:n2].reshape(a.blk2d.shape), raw[n2:n2 + n3].reshape(a.blk3d.shape)
    bad = [n for i, n in enumerate(BLK2D) if n not in ("tps", "fluxua", "fluxva", "zflux") and not same_bits(want.blk2d[i], b2[i])]
    bad += [n for i, n in enumerate(BLK3D) if n not in ("tps", "fluxua", "fluxva", "zflux") and not same_bits(want.blk3d[i], b3[i])]
    assert not bad, bad
    con = np.frombuffer(raw[n2 + n3:n2 + n3 + 47].tobytes(), dtype=want.con.dtype)
    assert con["time0"][0] == want.time0 and con["time"][0] == want.time and con["iint"][0] == nsteps
    # a mistyped read_rst_file: the library's message, which names the file and the cause, comes out with the status
    nml_text = (tmp_path / "pom.nml").read_text().replace("restart.0007.nc", "restart.0008.nc")
    (tmp_path / "pom.nml").write_text(nml_text)
    r = subprocess.run([os.path.join(fdir, "pom_gpu_main"), "state.in", "state.out"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert "Error: read_restart_pnetcdf: read_restart: cannot open ./in/restart.0008.nc" in r.stdout and "error_status   1" in r.stdout, r.stdout + r.stderr
