"""Host-side logic that needs no GPU: namelist, decomposition arithmetic, case generator on tiles,
COMMON-block layout, C-ABI symbol table, 2-rank halo exchange over gloo."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from extpom_amd import decomp, namelist
from extpom_amd.cases import cut_tile, make_case
from extpom_amd.layout import BLK2D, BLK3D, CON_DTYPE, P2, P3, PomState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_sizes_match_reference_common_blocks():
    # sizes verified with nm -S on the flang object (SURVEY 8a "types"): 73 2-D, 40 3-D arrays, blkcon 376 B
    assert len(BLK2D) == 73 and len(BLK3D) == 40 and CON_DTYPE.itemsize == 376
    assert (P3["aam"], P3["zflux"], P2["aam2d"], P2["wvsurff"]) == (0, 39, 0, 72)
    st = PomState(142, 306, 40)
    assert st.blk3d.nbytes == 556185600 and st.blk2d.nbytes == 73 * 142 * 306 * 8 and st.blk1d.nbytes == 1280
    assert st.u.shape == (40, 306, 142) and st.u.ctypes.data == st.blk3d.ctypes.data + P3["u"] * 8 * 142 * 306 * 40


def test_namelist_defaults_and_derived_constants(tmp_path):
    nml = tmp_path / "pom.nml"
    nml.write_text("&pom_nml\n  title = 'x' ! c\n  mode = 3\n  nadv = 2\n  dte = 2.\n  isplit = 30\n  days = 1\n  prtd1 = 0.1\n"
                   "  write_rst = 1.0\n  swtch = 9999.\n  netcdf_file = 'nonetcdf'\n/\n! trailing doc\n")
    c = namelist.read_namelist_file(str(nml))
    assert c["dti"] == 60.0 and c["dte2"] == 4.0 and c["dti2"] == 120.0
    assert c["iend"] == 1440 and c["iprint"] == 144 and c["irestart"] == 1440
    assert c["ispi"] == 1.0 / 30.0 and c["isp2i"] == 1.0 / 60.0
    assert (c["horcon"], c["tprni"], c["smoth"], c["nbct"], c["ispadv"]) == (0.1, 0.1, 0.1, 1, 1)
    with pytest.raises(ValueError):
        namelist.parse_namelist("&pom_nml\n bogus = 1\n/\n")


def test_decomposition_matches_distribute_mpi():
    # pom.h_dist's own example: 282x306 in tiles of 142x306 -> 2x1
    assert decomp.tile_grid(282, 306, 142, 306) == (2, 1)
    t0, t1 = decomp.make_tile(0, 282, 306, 142, 306), decomp.make_tile(1, 282, 306, 142, 306)
    assert (t0.n_west, t0.n_east, t1.n_west, t1.n_east) == (-1, 1, 0, -1)
    assert t1.i_off == 140 and t0.im == t1.im == 142      # neighbours share 2 columns
    # BASELINE configs: 1024x1024 on 2x4 -> 513x258 (north row trimmed to 256), 2048x1536 -> 1025x386 (384)
    assert decomp.local_size(1024, 1024, 2, 4) == (513, 258)
    assert decomp.make_tile(7, 1024, 1024, 513, 258).jm == 256
    assert decomp.local_size(2048, 1536, 2, 4) == (1025, 386)
    assert decomp.make_tile(6, 2048, 1536, 1025, 386).jm == 384
    with pytest.raises(ValueError):
        decomp.make_tile(0, 282, 306, 100, 306, n_proc=2)   # "im_local or jm_local is too low"
    for n in (1, 2, 4, 8):
        nx, ny = decomp.choose_tile_grid(n, 2048, 1536)
        assert (nx, ny) == (1, n)                           # whole rows while the tiles stay tall enough (profiles/round3_tile_grids.txt)
    assert decomp.choose_tile_grid(4, 65, 49) == (2, 2)


@pytest.mark.parametrize("case", ["seamount", "island", "basin", "archipelago"])
def test_tile_generation_equals_cut_of_global(case):
    g = make_case(case, 65, 49, 21, dte=6.0, isplit=30)
    for r in range(4):
        t = decomp.make_tile(r, 65, 49, 34, 26)
        a, b = make_case(case, 65, 49, 21, tile=t, dte=6.0, isplit=30), cut_tile(g, t)
        assert not [n for n in BLK2D + BLK3D if not np.array_equal(a.field(n), b.field(n))]
        for (x, y), (p, q) in zip(a.restore_records, b.restore_records):
            assert np.array_equal(x, p) and np.array_equal(y, q)


# ---- the archipelago case: what it must have, on every grid (and tile split) a test runs it on ---------------------------------------
# (im, jm, kb, [(nx, ny, isplit of the wide-halo run or None)]): tests/test_kernels_emulated*.py, test_gpu_parity.py, test_gpu_multitile.py
ARCHIPELAGO_GRIDS = [
    (65, 49, 21, [(2, 2, 10)]), (66, 50, 21, []), (128, 12, 21, []), (64, 48, 70, []), (256, 192, 50, [(2, 4, 30)]), (128, 96, 21, []),
    (200, 30, 21, []), (200, 93, 11, []), (2050, 20, 50, []), (1024, 1024, 40, []),
    (41, 35, 11, [(2, 1, None), (1, 2, None), (2, 2, None), (3, 2, None), (1, 3, None)]),
    (67, 59, 11, [(2, 2, 7), (2, 1, 7), (1, 2, 7)]), (97, 59, 11, [(3, 2, 7), (2, 2, 7)]), (41, 101, 11, [(1, 3, 7)]),
    (43, 75, 11, [(2, 4, 7)]), (59, 53, 11, [(3, 3, 7)]),
    (97, 61, 16, [(2, 1, 10), (1, 2, 10), (2, 2, 10)]), (72, 150, 12, [(1, 4, 10)]),
]


def _shift(a, dj, di):
    """a(j+dj, i+di), False beyond the grid"""
    out = np.zeros_like(a)
    jm, im = a.shape
    out[max(0, -dj):jm - max(0, dj), max(0, -di):im - max(0, di)] = a[max(0, dj):jm + min(0, dj), max(0, di):im + min(0, di)]
    return out


def _runs(mask):
    """longest run of True along the last axis"""
    best = run = np.zeros(mask.shape[0], dtype=int)
    for i in range(mask.shape[1]):
        run = np.where(mask[:, i], run + 1, 0)
        best = np.maximum(best, run)
    return int(best.max())


@pytest.mark.parametrize("im,jm,kb,splits", ARCHIPELAGO_GRIDS, ids=[f"{g[0]}x{g[1]}x{g[2]}" for g in ARCHIPELAGO_GRIDS])
def test_archipelago_has_what_the_other_cases_lack(im, jm, kb, splits):
    """The properties the parity tests on this case lean on, asserted on the generated state: a case smoothed
    later turns this test red, not the kernels' tests blind.  A 12- or 20-row grid is too short for the straits and lakes; the rest
    is demanded there too."""
    if im * jm * kb > 4.0e6:
        kb = 4                                                   # the horizontal properties do not depend on kb
    st = make_case("archipelago", im, jm, kb, dte=6.0, isplit=30)
    dx, dy, cor, h = st.dx, st.dy, st.cor, st.h
    # grid: the differences behind the curvature terms, and the cross-direction neighbours, are not zero
    assert np.abs(dy[:, 2:] - dy[:, :-2]).max() > 0 and np.abs(dx[2:, :] - dx[:-2, :]).max() > 0
    assert np.abs(cor[:, 1:] - cor[:, :-1]).max() > 0 and np.abs(cor[1:, :] - cor[:-1, :]).max() > 0
    assert np.isclose(float(st.period), 2.0 * np.pi / abs(cor[jm // 2 - 1, im // 2 - 1]) / 86400.0, rtol=1e-14, atol=0)     # initialize.f:357
    assert np.array_equal(st.art, dx * dy)
    assert np.array_equal(st.aru[1:, 1:], 0.25 * (dx[1:, 1:] + dx[1:, :-1]) * (dy[1:, 1:] + dy[1:, :-1]))
    assert np.array_equal(st.arv[1:, 1:], 0.25 * (dx[1:, 1:] + dx[:-1, 1:]) * (dy[1:, 1:] + dy[:-1, 1:]))
    assert np.array_equal(st.aru[:, 0], st.aru[:, 1]) and np.array_equal(st.arv[0, :], st.arv[1, :])
    # land: 3-6 % of the cells, h = 1 there, masks as io_pnetcdf.F:2243-2256
    land = st.fsm == 0.0
    assert 0.03 <= land.mean() <= 0.06, land.mean()
    assert (h[land] == 1.0).all() and (h[~land] >= 10.0).all()
    dum, dvm = (~land).astype(float), (~land).astype(float)
    dum[:, 1:][land[:, :-1]] = 0.0
    dvm[1:, :][land[:-1, :]] = 0.0
    assert np.array_equal(st.dum, dum) and np.array_equal(st.dvm, dvm)
    wet = ~land
    n4 = lambda a: _shift(a, 0, 1) & _shift(a, 0, -1) & _shift(a, 1, 0) & _shift(a, -1, 0)
    n8 = lambda a: n4(a) & _shift(a, 1, 1) & _shift(a, 1, -1) & _shift(a, -1, 1) & _shift(a, -1, -1)
    assert (land & n8(wet)).any()                                                # a one-cell island
    # land on each of the four open edges and in a domain corner; at the end of the first wavefront / of a wide row
    assert land[1:-1, 0].any() and land[1:-1, -1].any() and land[0, 1:-1].any() and land[-1, 1:-1].any() and land[-1, -1]
    if im == 65:
        assert land[:, 63].any() and land[:, 64].any()
    if im >= 2047:
        assert land[:, 2046:].any()
    if jm >= 40:
        pair = land & _shift(land, 0, 1) & ~_shift(land, 0, -1) & ~_shift(land, 0, 2)
        alone = ~_shift(land, 1, 0) & ~_shift(land, -1, 0) & ~_shift(land, 1, 1) & ~_shift(land, -1, 1)
        assert (pair & alone).any()                                              # a 2 x 1 island
        diag = land & _shift(land, 1, 1) & ~_shift(land, 0, 1) & ~_shift(land, 1, 0)
        assert diag.any()                                                        # two cells touching at a corner only
        strait_j = wet & _shift(land, 0, -1) & _shift(land, 0, 1)                # one wet cell between two land cells ...
        strait_i = wet & _shift(land, -1, 0) & _shift(land, 1, 0)
        assert _runs(strait_j.T) >= 10 and _runs(strait_i) >= 10                 # ... ten times in a row, in each direction
        assert (wet & n8(land)).any()                                            # a lake of one cell
        q = wet & _shift(wet, 0, 1) & _shift(wet, 1, 0) & _shift(wet, 1, 1)      # a 2 x 2 lake: its twelve neighbours are land
        ring = np.ones_like(land)
        for dj in (-1, 0, 1, 2):
            for di in (-1, 0, 1, 2):
                if not (dj in (0, 1) and di in (0, 1)):
                    ring &= _shift(land, dj, di)
        assert (q & ring).any()
    # bottom roughness, T / S away from the climatology, forcing: all live, all masked
    r = np.abs(h[:, 1:] / h[:, :-1] - 1.0)[wet[:, 1:] & wet[:, :-1]]
    assert np.median(r) > 0.05
    assert np.abs(st.tb - st.tclim).max() > 0.01 and np.abs(st.sb - st.sclim).max() > 0.005
    for n in ("wusurf", "wvsurf", "wtsurf", "wssurf", "swrad", "vfluxf", "e_atmos"):
        f = st.field(n)
        assert (f[land] == 0.0).all() and np.unique(f[wet]).size > wet.sum() // 2, n
    for n in ("ele", "elw", "eln", "els"):
        assert np.abs(st.field(n)).max() > 0 and st.field(n).min() < 0 < st.field(n).max(), n
    for f, edge in ((st.uab, (slice(None), 1)), (st.uab, (slice(None), -1)), (st.vab, (1, slice(None))), (st.vab, (-1, slice(None)))):
        assert f[edge].min() < 0 < f[edge].max()                                 # both signs of the normal velocity on every edge
    # tiles: land on a line two neighbours share (the owned edge line of one is the ghost line of the other) at some seam, and in
    # the rim of w = isplit + 4 cells by which the wide-halo mode extends a tile
    for nx, ny, isplit in splits:
        iml, jml = decomp.local_size(im, jm, nx, ny)
        edge = ghost = rim = False
        for rk in range(nx * ny):
            t = decomp.make_tile(rk, im, jm, iml, jml, n_proc=nx * ny)
            tl = land[t.j_off:t.j_off + t.jm, t.i_off:t.i_off + t.im]
            if t.n_east >= 0:
                edge, ghost = edge or tl[1:-1, -2].any(), ghost or tl[1:-1, -1].any()
            if t.n_west >= 0:
                edge, ghost = edge or tl[1:-1, 1].any(), ghost or tl[1:-1, 0].any()
            if t.n_north >= 0:
                edge, ghost = edge or tl[-2, 1:-1].any(), ghost or tl[-1, 1:-1].any()
            if t.n_south >= 0:
                edge, ghost = edge or tl[1, 1:-1].any(), ghost or tl[0, 1:-1].any()
            if isplit:
                w = isplit + 4
                j0, j1, i0, i1 = max(0, t.j_off - w), min(jm, t.j_off + t.jm + w), max(0, t.i_off - w), min(im, t.i_off + t.im + w)
                ext = land[j0:j1, i0:i1].sum() - tl.sum()
                rim = rim or ext > 0
        assert edge and ghost and (rim or not isplit), (nx, ny, edge, ghost, rim)


@pytest.mark.parametrize("im,jm,kb,steps,nml", [(65, 49, 21, 100, {}), (65, 49, 21, 100, dict(nadv=1)), (65, 49, 21, 100, dict(nitera=2)),
                                                (65, 49, 21, 100, dict(npg=2)), (65, 49, 21, 100, dict(nbct=2)), (65, 49, 21, 100, dict(mode=2)),
                                                (65, 49, 21, 20, dict(mode=4)), (65, 49, 21, 20, dict(nbct=3, nbcs=3)), (65, 49, 21, 20, dict(nbct=4)),
                                                (66, 50, 21, 12, {}), (256, 192, 50, 10, {}), (67, 59, 21, 12, {}), (64, 48, 70, 3, {}), (128, 12, 21, 12, {})])
def test_archipelago_is_stable_under_the_oracle(im, jm, kb, steps, nml):
    """stability is a condition of the case, not of the code under test: every COMMON array and bdry finite, error_status = 0 and
    vamax < 1 (vmaxl = 100) under the CPU oracle; after the three warm-up steps the normal velocity has both signs on each open edge"""
    from oracle.pyoracle import OracleTile, oracle_finish_initial
    st = make_case("archipelago", im, jm, kb, dte=6.0, isplit=30, **nml)
    oracle_finish_initial(st)
    ot = OracleTile(st)
    ot.run(3)
    wet_u, wet_v = st.dum != 0, st.dvm != 0
    for f, m, edge in ((st.ua, wet_u, (slice(None), 1)), (st.ua, wet_u, (slice(None), -1)), (st.va, wet_v, (1, slice(None))), (st.va, wet_v, (-1, slice(None)))):
        assert f[edge][m[edge]].min() < 0 < f[edge][m[edge]].max()
    if int(st.mode) != 2:
        for f, edge in ((st.u[0], (slice(None), 1)), (st.u[0], (slice(None), -1)), (st.v[0], (1, slice(None))), (st.v[0], (-1, slice(None)))):
            assert f[edge].min() < 0 < f[edge].max()
    ot.run(steps - 3)
    assert all(np.isfinite(st.field(n)).all() for n in BLK2D + BLK3D) and np.isfinite(st.bdry).all()
    assert int(st.error_status) == 0 and 0.0 < ot.vamax[0] < 1.0, ot.vamax


def test_c_abi_library_exports_every_declared_symbol():
    """libpomgpu.so loads without a GPU and exports exactly what include/pomgpu.h declares"""
    import re
    import __graft_entry__ as ge
    so = ge.build_hip()
    lib = ctypes.CDLL(so)
    hdr = open(os.path.join(ROOT, "include", "pomgpu.h")).read()
    declared = sorted(set(re.findall(r"\b(pomgpu_[a-z0-9_]+)\s*\(", hdr)) - {"pomgpu_exchange_fn"})
    assert len(declared) >= 45
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in pomgpu.h but not exported"
    from extpom_amd import lib as binding
    assert set(binding.EXPORTS) <= set(declared)
    # the fp32-storage study variant (BASELINE configs[4], same sources with -DPOMGPU_STORE_F32) exports the same C ABI
    lib32 = ctypes.CDLL(ge.build_hip(f32=True))
    for name in declared:
        assert hasattr(lib32, name), f"{name} missing from libpomgpu_f32.so"
    lib32.pomgpu_version.restype = lib.pomgpu_version.restype = ctypes.c_char_p
    assert b"fp32-storage" in lib32.pomgpu_version() and b"fp32" not in lib.pomgpu_version()
    # no device here: context creation must refuse, not fall back
    from extpom_amd.lib import Dims
    h = ctypes.c_void_p()
    d = Dims(65, 49, 21, 65, 49, -1, -1, -1, -1)
    lib.pomgpu_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(Dims), ctypes.c_int, ctypes.c_void_p]
    import torch
    if not torch.cuda.is_available():
        assert lib.pomgpu_create(ctypes.byref(h), ctypes.byref(d), 0, None) == -4   # POMGPU_ENODEV


def test_two_rank_halo_exchange_is_decomposition_invariant():
    """world_size-2 gloo run: the CPU oracle on a 2x1 (and 1x2) split, with extpom_amd.halo doing
    every exchange, must equal the single-tile run bit for bit"""
    for split in ("x", "y", "xy"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "halo_worker.py"), split],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "HALO-OK" in r.stdout, r.stdout + r.stderr


def test_order_exchange_of_baropg_mcc_is_decomposition_invariant():
    """npg = 2: the 4th-order pressure gradient needs one more ghost column / row (order2d_mpi,
    order3d_mpi); 2x2 split over gloo against the single-tile run"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "halo_worker.py"), "xy", "npg2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "HALO-OK" in r.stdout, r.stdout + r.stderr


def test_domain_stats_partial_sums_add_up_over_tiles():
    """sums_only: the tile-local sums of a 2x2 split (what sum0d_mpi would add) equal the single-tile sums"""
    import ctypes
    import numpy as np
    from extpom_amd import decomp
    from extpom_amd.cases import cut_tile, make_case
    from oracle.pyoracle import OracleTile, oracle_finish_initial
    g = make_case("island", 41, 35, 11, dte=6.0, isplit=10)
    oracle_finish_initial(g)
    OracleTile(g).run(3)

    def sums(st):
        out = (ctypes.c_double * 8)()
        OracleTile(st).call("domain_stats", out, ctypes.c_int(1))
        return np.array(list(out))

    whole = sums(g)
    iml, jml = decomp.local_size(41, 35, 2, 2)
    parts = sum(sums(cut_tile(g, decomp.make_tile(r, 41, 35, iml, jml, n_proc=4))) for r in range(4))
    np.testing.assert_allclose(parts, whole, rtol=1e-12, atol=0)


def test_host_libm_is_the_one_the_pow_clone_restates(tmp_path):
    """bit-parity with the reference leans on glibc's (not correctly rounded) pow: `dens` calls it for abs(sr)**1.5 and the
    HIP kernel restates glibc 2.35's algorithm (THIRD_PARTY_NOTICES.md).  A host with another libm changes what "the
    reference" computes -- so (i) the libc version is pinned here and stated on the bench line, (ii) the restatement
    (tools/check_glibc_pow_clone.c, the same code as gpow15 in k_adv.hip) equals this host's pow() on 2.2e7 arguments."""
    import ctypes
    libc = ctypes.CDLL("libc.so.6")
    libc.gnu_get_libc_version.restype = ctypes.c_char_p
    ver = libc.gnu_get_libc_version().decode()
    assert ver.startswith("2.35"), f"glibc {ver}: the pow tables were read out of 2.35 -- re-run tools/dump_glibc_pow_tables.py and the parity tests"
    exe = tmp_path / "chkpow"
    subprocess.check_call(["gcc", "-O2", "-mfma", "-ffp-contract=off", os.path.join(ROOT, "tools", "check_glibc_pow_clone.c"), "-o", str(exe), "-lm"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300).stdout
    assert "x**1.5: 0 mismatches" in out and "general x**y: 0 mismatches" in out, out


def _bench_selftest(plan, gpus, extra=(), limit="10"):
    """bench.py --gpus N with stand-in ranks (POM_BENCH_SELFTEST: no GPU; what the rank SUPERVISORS make of passes that
    complete, hang or die is what runs here -- the real code path of the launcher, the supervisors and their rendezvous)"""
    import json
    env = dict(os.environ, POM_BENCH_REHEARSE="1", POM_BENCH_SELFTEST=json.dumps(plan), POM_BENCH_PASS_LIMIT=limit)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "2", "--warmup", "1", *extra],
                       capture_output=True, text=True, timeout=600, env=env)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, [json.loads(l) for l in lines]


def test_bench_multi_gpu_passes_survive_a_hang_and_a_dead_rank():
    """north_star's multi-GPU line must not be losable: the ranks' supervisors run a pass with every round on one stream, a
    pass with the second stream and communicator, and a pass on the alternate tile grid, each as fresh child processes.  A
    pass whose rank hangs (here: rank 1 of the overlapped pass never posts) is ended at its limit and named, a pass whose rank
    dies (rank 2 of the alternate-grid pass) ends at once on every rank -- and the line still carries the passes that completed,
    ONE line, with the tile grids BASELINE names (2x4 beside 1x8 would be --gpus 8: four ranks here)."""
    # (limit: a healthy stand-in pass is four python processes importing torch and meeting on gloo -- 2-3 s on an idle box, more on a busy one)
    r, lines = _bench_selftest({"hang": [1, 1], "fail": [2, 2]}, 4, ["--workload", "basin2048"], limit="15")
    assert r.returncode == 0 and len(lines) == 1, r.stdout + r.stderr
    out = lines[0]
    ps = out["passes"]
    assert [(p["tiles"], p["overlap"], p["ok"]) for p in ps] == [("1x4", False, True), ("1x4", True, False), ("2x2", False, False)], ps
    assert out["config"]["tiles"] == "1x4" and out["config"]["tiles_primary"] == "1x4" and ps[0]["primary"]
    assert out["config"]["no_overlap_env"] == "1"                       # pass 0 ran with POMGPU_NO_OVERLAP=1
    assert "no result within" in ps[1]["failed"]["first"] and set(ps[1]["failed"]["phase_by_rank"].values()) == {"connect"}
    assert ps[2]["failed"]["why_by_rank"]["2"] == "exit code 9" and ps[2]["wall_s"] < 12.0     # the dead rank ended the pass at once, not at the limit (15 s)
    # everything healthy: the faster pass (overlap on, in the stand-in's numbers) is the line's value, the alternate grid under it
    r, lines = _bench_selftest({}, 2, ["--workload", "basin1024", "--tiles", "2x1"])
    assert r.returncode == 0 and len(lines) == 1, r.stdout + r.stderr
    out = lines[0]
    assert [(p["tiles"], p["overlap"], p["ok"]) for p in out["passes"]] == [("2x1", False, True), ("2x1", True, True), ("1x2", True, True)]
    assert out["config"]["overlap"] is True and out["ms_per_step"] == 8.0 and out["passes"][1]["primary"]
    # nothing completes: no line, non-zero exit
    r, lines = _bench_selftest({"fail": [0, 0]}, 2, ["--only-pass", "0"])
    assert r.returncode != 0 and not lines


def test_bench_tile_grids_follow_baseline_configs():
    """configs[2] names "2x4 tile decomposition on 8 GPUs" for 1024x1024x40; configs[3] (2048x1536x50) names none: whole rows
    there.  The other grid is always measured beside the primary (parallel_mpi.f:54-65 leaves the split to im_local, jm_local)."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.tile_grids("basin1024", 8) == ("2x4", "1x8")
    assert bench.tile_grids("basin2048", 8) == ("1x8", "2x4")
    assert bench.tile_grids("basin2048", 8, "2x4") == ("2x4", "1x8")
    assert bench.tile_grids("basin2048", 4) == ("1x4", "2x2") and bench.tile_grids("basin2048", 2)[0] == "1x2"
    with pytest.raises(SystemExit):
        bench.tile_grids("basin2048", 8, "3x3")


def test_bench_dump_outputs_writes_the_restart_list_within_64_mb(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every restart-list array as <name>.npy in float64, whole where it is small, else the same seeded
    sample in every run; at the flagship grid (2048x1536x50) the files stay under 64 MB in all"""
    sys.path.insert(0, ROOT)
    import bench
    from extpom_amd.layout import RESTART_2D, RESTART_3D
    names = RESTART_2D + RESTART_3D
    assert len(names) * (bench.DUMP_VALUES_PER_ARRAY * 8 + 128) < 64e6
    st = make_case("seamount", 65, 49, 21)
    bench.dump_outputs(st, str(tmp_path / "whole"))
    for n in names:
        a = np.load(tmp_path / "whole" / f"{n}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, st.field(n)), n
    monkeypatch.setattr(bench, "DUMP_VALUES_PER_ARRAY", 1000)
    for d in ("s1", "s2"):
        bench.dump_outputs(st, str(tmp_path / d))
    for n in names:
        a, b = np.load(tmp_path / "s1" / f"{n}.npy"), np.load(tmp_path / "s2" / f"{n}.npy")
        assert a.dtype == np.float64 and a.shape == (1000,) and np.array_equal(a, b), n
        assert np.isin(a, st.field(n)).all(), n
    assert sorted(p.name for p in (tmp_path / "s1").iterdir()) == sorted(n + ".npy" for n in names)


@pytest.mark.parametrize("extra", [["--steps", "0"], ["--gpus", "2", "--dump-outputs", "x"]])
def test_bench_refuses_what_it_cannot_measure(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and not r.stdout and "error" in r.stderr, r.stdout + r.stderr


def test_short_wave_term_in_double_double_equals_the_quad_evaluation(tmp_path):
    """csrc/dd_exp.h (what the proft kernels evaluate for solver.f:1608-1611) against the REAL(16) expression as libquadmath
    evaluates it, on arguments of proft's ranges (tools/check_dd_exp.cpp; 2e7 arguments there, 3e5 here): no result may differ."""
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "check_dd_exp")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "check_dd_exp.cpp"), "-lquadmath"])
    r = subprocess.run([exe, "300000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 results differ" in r.stdout, r.stdout[-500:]


def test_header_parser_survives_damaged_headers_under_sanitizers(tmp_path):
    """csrc/cdf_io.hpp's host part (read_header, check_var: what every file reader of the library runs before it touches the state) as a
    stand-alone program under AddressSanitizer and UBSan (tools/check_cdf_header.cpp): the three classic files of tests/golden/
    (tests/golden/make_cdf_header_fixtures.py) intact, with every header word overwritten by 0xffffffff in turn and cut to every prefix of
    their headers.  Refusals are expected; a crash or a sanitizer report fails the run."""
    import shutil
    if not shutil.which("g++"):
        pytest.skip("no g++")
    san = ["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(san + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed")
    exe = str(tmp_path / "check_cdf_header")
    build = subprocess.run(san + ["-I" + os.path.join(ROOT, "extpom_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "check_cdf_header.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    files = [os.path.join(ROOT, "tests", "golden", f"cdf_header_{n}.nc") for n in ("grid", "clim", "restart")]
    r = subprocess.run([exe, *files], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CDF-HEADER-OK" in r.stdout and r.stdout.count("damaged words") == 3, r.stdout[-1000:] + r.stderr[-3000:]


@pytest.mark.bg_oracle("seamount", 33, 29, 9, 2)
def test_background_oracle_leaves_the_digests_of_an_in_process_run(bg_oracle):
    """tests/oracle_bg.py + tests/conftest.py: the child process that computes the full-size oracle steps beside the GPU tests
    (test_config4_2048x1536x50_full_size joins it) -- on a small grid its per-array digests after every step are those of the
    same oracle run made here, and a changed bit (the sign of a zero) changes a digest"""
    from oracle_bg import NML, digests
    from extpom_amd.cases import make_case
    from oracle.pyoracle import OracleTile, oracle_finish_initial
    a = make_case("seamount", 33, 29, 9, **NML)
    oracle_finish_initial(a)
    assert bg_oracle.step(0)["digests"] == digests(a)
    oc = OracleTile(a)
    for n in (1, 2):
        oc.run(1)
        want = bg_oracle.step(n, timeout=120)
        assert want["iint"] == n and want["digests"] == digests(a)
    a.field("el")[0, 0] = -0.0 if a.field("el")[0, 0] == 0 else -a.field("el")[0, 0]
    assert digests(a)["el"] != want["digests"]["el"]
