"""pomgpu_read_restart -- read_restart_pnetcdf (io_pnetcdf.F:2420-2768) without PnetCDF -- through the host build of the unmodified
sources (tests/emu): the header parser, the refusals, the life cycle and the kernel's index arithmetic, bit for bit.

The bar is the ORACLE STARTED FROM THE STATE THE REFERENCE'S READER WOULD LEAVE (tests/restart_expect.py builds it from the file
as scipy reads it), not the uninterrupted run: the reference's restart list is not seamless in mode 3."""
import os
import subprocess
import threading

import numpy as np
import pytest

from extpom_amd import decomp
from extpom_amd.cases import finish_initial, make_case
from extpom_amd.layout import BLK2D, BLK3D, RESTART_2D, RESTART_3D
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial
import restart_expect
from restart_expect import M, RESTART, SCRATCH, assign_from_file, check_read_state, diff, expected_state, file_values, fresh, same_bits, write_foreign_restart

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
N = 7


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


def written(tmp_path, case, nml, steps, **kw):
    return restart_expect.written(tmp_path, case, nml, steps, libpath=EMU, **kw)


# ---- 1: round trip --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,nml,steps", [("seamount", {}, N), ("island", {}, N), ("archipelago", {}, N), ("seamount", dict(isplit=7), 3)], ids=str)
def test_round_trip(tmp_path, case, nml, steps):
    """N steps, write_file("restart"), a NEW context on a fresh initial state, read_restart: the 37 fields are the written state,
    d, dt, time0, time follow, and nothing else moved.  isplit = 7, N = 3: an odd substep count -- the current generation of ua, va,
    el ... lives in the second buffer set when the file is written."""
    path, a = written(tmp_path, case, nml, steps)
    init = fresh(case, nml)
    b = init.copy()
    g = PomGpu(b, libpath=EMU)
    time0, iint = g.read_restart(path)
    assert iint == steps and time0 == a.time and b.time0 == a.time      # st.con is refreshed by the call itself
    g.download()
    for n in RESTART:
        assert same_bits(b.field(n), a.field(n)), n
    check_read_state(b, init, path)
    assert b.iint == 0 and b.error_status == 0
    g.close()


@pytest.mark.parametrize("chunk_kb", [26, 64, 200])
def test_round_trip_in_many_runs(tmp_path, chunk_kb):
    """POMGPU_IO_CHUNK_KB: buffers of one, two and seven levels of a 21-level variable (a band of rows is 25 KB) -- runs that end
    on the last level, one level short of it, and exactly"""
    path, a = written(tmp_path, "archipelago", {}, 2)
    init = fresh("archipelago", {})
    b = init.copy()
    g = PomGpu(b, libpath=EMU)
    g.switch("IO_CHUNK_KB", chunk_kb)
    g.read_restart(path)
    g.download()
    for n in RESTART:
        assert same_bits(b.field(n), a.field(n)), n
    check_read_state(b, init, path)
    g.close()


# ---- 2: continuation against the oracle -----------------------------------------------------------------------------------------
CONTINUE = [("seamount", {}), ("archipelago", {}), ("archipelago", dict(npg=2)), ("island", dict(nitera=2)), ("seamount", dict(nadv=1)),
            ("seamount", dict(mode=2)), ("seamount", dict(mode=4)), ("basin", dict(isplit=10, alpha=0.225))]
# measured with the oracle alone at 65x49x21, N = 7, M = 6: mode = 2 continues seamlessly; the two default (mode = 3) cases do not
SEAMLESS = [("seamount", dict(mode=2))]
NOT_SEAMLESS = [("seamount", {}), ("archipelago", {})]


@pytest.mark.parametrize("case,nml", CONTINUE, ids=str)
def test_continuation_equals_the_oracle_started_from_the_readers_state(tmp_path, case, nml):
    path, _ = written(tmp_path, case, nml, N)
    a = expected_state(case, 65, 49, 21, nml, path)
    b = fresh(case, nml)
    ot = OracleTile(a)
    g = PomGpu(b, libpath=EMU)
    g.read_restart(path)
    for n in range(1, M + 1):
        ot.run(1)
        g.run(1)
        g.download()
        assert not diff(a, b) and same_bits(a.bdry, b.bdry), f"step {n}: {diff(a, b)}"
        assert a.iint == b.iint == n and a.time == b.time and a.time0 == b.time0
    g.close()
    if (case, nml) in SEAMLESS or (case, nml) in NOT_SEAMLESS:
        u = fresh(case, nml)
        OracleTile(u).run(N + M)
        differs = [n for n in RESTART if not same_bits(u.field(n), b.field(n))]
        if (case, nml) in SEAMLESS:
            assert not differs, differs
        else:
            assert differs, "the continuation equals the uninterrupted run: DESIGN.md section 8 says it does not"


@pytest.mark.parametrize("case,nml", [("archipelago", dict(mode=2)), ("basin", dict(mode=2))], ids=str)
def test_mode2_continuation_equals_the_uninterrupted_run(tmp_path, case, nml):
    """the three mode = 2 runs measured (seamount is in the list above): 0 of the 37 fields differ from 13 uninterrupted steps"""
    path, _ = written(tmp_path, case, nml, N)
    b = fresh(case, nml)
    g = PomGpu(b, libpath=EMU)
    g.read_restart(path)
    g.run(M)
    g.download()
    g.close()
    a = expected_state(case, 65, 49, 21, nml, path)
    OracleTile(a).run(M)
    assert not diff(a, b), diff(a, b)
    u = fresh(case, nml)
    OracleTile(u).run(N + M)
    differs = [n for n in RESTART if not same_bits(u.field(n), b.field(n))]
    assert not differs, differs


# ---- 3: variables are found by name ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [2, 1])
def test_variables_are_found_by_name_in_a_file_of_another_writer(tmp_path, version):
    """scipy's writer: the 39 variables in reversed order, two extra variables, extra attributes, other dimension names, another
    alignment of the data section; CDF-2 and its CDF-1 twin"""
    path, a = written(tmp_path, "island", {}, 2)
    vals, time, iint = file_values(path)
    other = tmp_path / f"foreign{version}.nc"
    write_foreign_restart(other, vals, time, iint, 21, 49, 65, version=version)
    assert open(other, "rb").read(4) == b"CDF" + bytes([version])
    init = fresh("island", {})
    b = init.copy()
    g = PomGpu(b, libpath=EMU)
    assert g.read_restart(other) == (time, iint)
    g.download()
    for n in RESTART:
        assert same_bits(b.field(n), a.field(n)), n
    check_read_state(b, init, other)
    g.close()


# ---- 4: reading into a live context ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("writing", [False, True], ids=["held odd substep", "held odd substep and a file being written"])
def test_reading_into_a_live_context(tmp_path, writing):
    restart_expect.reading_into_a_live_context(tmp_path, writing, libpath=EMU)


# ---- 5: cont_bry ----------------------------------------------------------------------------------------------------------------
def test_cont_bry_takes_the_files_step_number_only_when_it_was_set(tmp_path):
    path, _ = written(tmp_path, "seamount", {}, N)
    for before, after in ((1, N), (0, 0)):
        b = fresh("seamount", {})
        b.cont_bry = before
        g = PomGpu(b, libpath=EMU)
        g.read_restart(path)
        assert b.cont_bry == after
        g.download()
        assert b.cont_bry == after
        g.close()


def test_cont_bry_shifts_the_forcing_records_of_the_continued_run(tmp_path):
    """dti = 360 s: lateral records change every 10 steps, wind / heat every 30.  With cont_bry = 7 from the file the continued
    run asks for record (iint + 7) / 10 + 1: the change falls on its step 3, not on step 10"""
    from extpom_amd.cases import make_forcing_records, make_lateral_records
    nml = dict(dte=6.0, isplit=60, days=1.0)
    path, _ = written(tmp_path, "seamount", nml, N)

    def start():
        s = fresh("seamount", nml)
        make_forcing_records(s, 4)
        make_lateral_records(s, 6)
        s.cont_bry = 1
        return s
    b = start()
    g = PomGpu(b, libpath=EMU)
    g.read_restart(path)
    assert b.cont_bry == N
    a = start()
    assign_from_file(a, path)
    a.cont_bry = N
    ot = OracleTile(a)
    g.set_forcing_records()
    g.set_lateral_records()
    for n in range(1, 6):
        ot.run(1)
        g.run(1)
        g.download()
        assert not diff(a, b) and same_bits(a.bdry, b.bdry), f"step {n}: {diff(a, b)}"
    g.close()
    c = start()                                                 # the same without the shift differs: the records did matter
    assign_from_file(c, path)
    c.cont_bry = 0
    OracleTile(c).run(5)
    assert not same_bits(c.bdry, a.bdry)


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_untouched(tmp_path):
    restart_expect.refusals_leave_the_state_untouched(tmp_path, libpath=EMU)


# ---- 7: tiles -------------------------------------------------------------------------------------------------------------------
KB_T, GRID_T, ISPLIT_T = 11, (97, 59), 7        # 3x2 tiles of 34 x 31, the east ones 33 wide, the north ones 30 high; w = 7 + 4 fits


def _tiles_run(nx, ny, case, work, library_exchange=False, wide=False, isplit=ISPLIT_T):
    """the rank threads of test_kernels_emulated_tiles.run_tiles with `work(r, tile, st, g, board)` in place of its fixed step loop"""
    import test_kernels_emulated_tiles as T
    world = nx * ny
    iml, jml = decomp.local_size(*GRID_T, nx, ny)
    board, errs = T.Board(world), []
    tiles = [decomp.make_tile(r, *GRID_T, iml, jml, n_proc=world) for r in range(world)]

    def rank(r):
        try:
            tile = tiles[r]
            st = make_case(case, *GRID_T, KB_T, tile=tile, dte=6.0, isplit=isplit)
            g = PomGpu(st, libpath=EMU)
            if library_exchange:
                g.set_transport(tile, lambda *a: T.transport(board, tile, *a), agree=lambda mine: board.allmin(r, mine))
                if wide:
                    assert g.set_wide_external(True, min(t.im for t in tiles), min(t.jm for t in tiles))
            else:
                g.set_exchange(lambda ptrs, nzs: T.exchange(board, tile, [T.view(p, nz, tile) for p, nz in zip(ptrs, nzs)]))
                g.set_order_exchange(lambda *a: T.order(board, tile, *a))

            def dens(s, a, b, c):
                g.upload(s); g.call("dens", a, b, c); g.download(s)

            def baropg(s):
                g.upload(s); g.call("baropg_mcc" if int(s.npg) == 2 else "baropg"); g.download(s)
            finish_initial(st, dens, baropg)
            g.upload(st)
            work(r, tile, st, g, board)
            g.close()
        except Exception as e:
            errs.append(e)
            board.barrier.abort()
    threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    return tiles


@pytest.mark.parametrize("case", ["island", "archipelago"])
def test_tiles_write_one_file_and_read_their_patches(tmp_path, case):
    """2x2 tiles run 3 steps and write ONE file (rank 0 lays it out, the others write in any order): byte for byte the single tile's
    file, because after 3 steps the ghost cells of every restart field equal the single tile's.  Then 3x2 tiles of a fresh initial
    state -- the east and north ones trimmed, im < im_local -- each read their patch and run M steps: owned cells equal the single
    tile's continuation under the oracle, and the padding of the trimmed tiles keeps its initial values across the read."""
    steps, cont = 3, M
    single, _ = written(tmp_path, case, dict(dte=6.0, isplit=ISPLIT_T), steps, grid=(*GRID_T, KB_T), name="single.nc")
    shared = tmp_path / "tiles.nc"

    def write(r, tile, st, g, board):
        g.run(steps)
        if r == 0:
            g.write_file("restart", shared, title=case, time_start="2000-01-01 00:00:00 +00:00", im_global=GRID_T[0], jm_global=GRID_T[1], create=True)
        board.barrier.wait()
        if r != 0:
            g.write_file("restart", shared, title=case, time_start="2000-01-01 00:00:00 +00:00", im_global=GRID_T[0], jm_global=GRID_T[1], create=False)
        g.io_wait()
    _tiles_run(2, 2, case, write)
    assert open(shared, "rb").read() == open(single, "rb").read()

    want = expected_state(case, *GRID_T, KB_T, dict(dte=6.0, isplit=ISPLIT_T), shared)
    OracleTile(want).run(cont)
    for library_exchange in (False, True):
        out = {}

        def read(r, tile, st, g, board):
            init = st.copy()
            g.read_restart(shared, im_global=GRID_T[0], jm_global=GRID_T[1])
            g.download()
            for n in BLK2D + BLK3D:                             # beyond (im, jm): untouched
                assert same_bits(st.field(n)[..., tile.jm:, :], init.field(n)[..., tile.jm:, :]), n
                assert same_bits(st.field(n)[..., :, tile.im:], init.field(n)[..., :, tile.im:]), n
            board.barrier.wait()
            g.run(cont)
            g.download()
            out[r] = (tile, st)
        tiles = _tiles_run(3, 2, case, read, library_exchange=library_exchange, wide=library_exchange)
        assert any(t.im < t.im_local for t in tiles) and any(t.jm < t.jm_local for t in tiles)
        bad = []
        for r, (tile, st) in out.items():
            io, jo, im, jm = tile.i_off, tile.j_off, tile.im, tile.jm
            sl_j = slice(0 if jo == 0 else 1, jm if jo + jm == GRID_T[1] else jm - 1)
            sl_i = slice(0 if io == 0 else 1, im if io + im == GRID_T[0] else im - 1)
            for n in BLK2D + BLK3D:
                if n not in SCRATCH and not same_bits(want.field(n)[..., jo:jo + jm, io:io + im][..., sl_j, sl_i], st.field(n)[..., :jm, :im][..., sl_j, sl_i]):
                    bad.append((r, n))
        assert not bad, (library_exchange, bad)


# ---- 8: the fp32 host builds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_round_the_3d_fields_as_an_upload_does(tmp_path, variant):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    lib = os.path.join(ROOT, "tests", f"_emu_{variant}", f"libpomgpu_emu_{variant}.so")
    path, a = written(tmp_path, "archipelago", {}, 2)
    b = fresh("archipelago", {})
    g = PomGpu(b, libpath=lib)
    g.read_restart(path)
    g.download()
    for n in RESTART_3D:
        assert same_bits(b.field(n), a.field(n).astype(np.float32).astype(np.float64)), n
    for n in RESTART_2D:
        assert same_bits(b.field(n), a.field(n)), n
    assert same_bits(b.d, b.h + a.el) and same_bits(b.dt, b.h + a.et) and b.time0 == a.time
    g.close()
