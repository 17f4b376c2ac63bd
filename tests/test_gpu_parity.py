"""Parity of the HIP path (through the C ABI, libpomgpu.so) with the CPU oracle and with the golden
vectors generated from the REFERENCE ITSELF.  fp64 throughout; the measured difference on MI355X is
exactly zero (see DESIGN.md "Parity"), so the asserts below demand bit-identity where the inputs
are identical, and 1e-10 relative (north_star's bar) for the 1000-step run.

scratch arrays of the reference (tps, fluxua, fluxva, zflux: SURVEY appendix A.3) are not
materialised by the fused kernels and are excluded."""
import ctypes
import hashlib

import numpy as np
import pytest

from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D, PROGNOSTIC
from golden_files import golden_file

pytestmark = pytest.mark.gpu
SCRATCH = {"tps", "fluxua", "fluxva", "zflux"}


def _gpu(st):
    from extpom_amd.model import PomGpu
    return PomGpu(st, device=0)


def _oracle():
    from oracle.pyoracle import OracleTile, oracle_finish_initial
    return OracleTile, oracle_finish_initial


def same_bits(x, y):
    """bit for bit: unlike array_equal this sees the sign of a zero (and takes equal NaN patterns for equal)"""
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


def diff(a, b):
    return [n for n in BLK2D + BLK3D if n not in SCRATCH and not same_bits(a.field(n), b.field(n))]


def _against_background_oracle(st, bg, steps, beat=lambda msg: None):
    """steps 1..steps of the HIP path from `st` against the oracle's, which a child process has been computing since the session
    began (tests/oracle_bg.py, tests/conftest.py): per COMMON array that is not scratch one xxh3-128 digest of its 64-bit patterns
    on either side -- equal digests, equal bits.  Step 0 shows that both sides start from identical inputs."""
    from oracle_bg import digests
    want = bg.step(0)
    assert want["digests"] == digests(st), "the background oracle and this test did not start from the same state"
    g = _gpu(st)
    for step in range(1, steps + 1):
        g.run(1)
        g.download()
        beat(f"device step {step} downloaded")
        got = digests(st)
        want = bg.step(step)
        beat(f"oracle step {step} there (it took the child {want['seconds']} s from its start)")
        bad = [n for n in got if got[n] != want["digests"][n]]
        assert not bad, f"step {step} differs from the oracle: {bad}"
        assert want["iint"] == step and st.iint == step
    g.close()


def reldiff(a, b, fields):
    return {f: float(np.abs(a.field(f) - b.field(f)).max() / max(np.abs(a.field(f)).max(), 1e-300)) for f in fields}


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


def _reproduces(gold, name):
    """the initial state and every restart-list field after every checkpoint hash to what the REFERENCE produced"""
    OracleTile, oracle_finish_initial = _oracle()
    cfg = gold["configs"][name]
    im, jm, kb = gold["grid"]
    st = make_case(cfg["case"], im, jm, kb, **cfg["nml"])
    oracle_finish_initial(st)
    bad = [f for f in gold["fields"] if _digest(st.field(f)) != cfg["init"][f]]
    assert not bad, f"{name}: initial state: {bad}"
    g = _gpu(st)
    done = 0
    for step in sorted(int(s) for s in cfg["steps"]):
        g.run(step - done)
        done = step
        g.download()
        bad = [f for f in gold["fields"] if _digest(st.field(f)) != cfg["steps"][str(step)][f]]
        assert not bad, f"{name}: step {step}: {bad} differ from the reference"
    g.close()
    assert st.error_status == 0


def test_native_library_is_the_one_running():
    from extpom_amd import lib
    L = lib.load()
    assert L._name.endswith("extpom_amd/csrc/libpomgpu.so")
    assert b"gfx950" in L.pomgpu_version()


@pytest.mark.parametrize("name", ["seamount_default", "seamount_nadv1", "seamount_nitera2", "seamount_mode2",
                                  "seamount_mode4", "seamount_nbc3", "island_default", "basin_default", "basin_alpha",
                                  "seamount_npg2", "island_npg2"])
def test_gpu_reproduces_reference_digests(golden, name):
    """every restart-list field after every checkpoint hashes to what the REFERENCE produced"""
    _reproduces(golden, name)


def test_gpu_initialisation_matches_reference(golden):
    """dens + baropg of the initialisation sequence, run through the C ABI"""
    from extpom_amd.model import gpu_finish_initial
    cfg = golden["configs"]["seamount_default"]
    im, jm, kb = golden["grid"]
    st = make_case(cfg["case"], im, jm, kb, **cfg["nml"])
    gpu_finish_initial(st, device=0)
    bad = [f for f in golden["fields"] if _digest(st.field(f)) != cfg["init"][f]]
    assert not bad, bad


@pytest.mark.parametrize("nbct", [2, 4])
def test_short_wave_penetration_carries_the_references_bits(golden_planes, nbct):
    """nbct = 2 / 4 with swrad != 0: the reference evaluates proft's radiation term in REAL(16) and rounds once (solver.f:1608-1611;
    the oracle does the same with libquadmath).  The kernels return that double from double-double arithmetic (csrc/dd_exp.h;
    tools/check_dd_exp.cpp: 0 of 2e7 values differ from the REAL(16) evaluation).  An fp64 exp differed in 0.6 % of the values by
    an ulp, and the flow amplifies an ulp by ~1e11 in 1000 steps (round 4, tools/swrad_drift.py with the fp64 exp: equal for 20
    steps, u off by 4e-10 after 100 and by 8e-4 after 1000).  Now: every field bit-identical after 5, 100 and 1000 internal steps (nbct = 4, whose
    fp64-exp run first differed after step 100: 400 steps) -- north_star's 1000-step bar for runs with short-wave penetration."""
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30, nbct=nbct)
    a.swrad[...] = -5.0e-5 * a.fsm
    oracle_finish_initial(a)
    b = a.copy()
    oa, g = OracleTile(a), _gpu(b)
    done = 0
    for n in ((5, 100, 1000) if nbct == 2 else (5, 100, 400)):   # (the oracle's libquadmath exp makes 1000 steps 80 s of CPU: once)
        oa.run(n - done)
        g.run(n - done)
        done = n
        g.download()
        bad = diff(a, b)
        assert not bad, f"nbct = {nbct}, step {n}: {bad}"
    g.close()


ROUTINES = [
    ("advave", (), ()), ("advct", (), ()), ("advu", (), ()), ("advv", (), ()), ("baropg", (), ()), ("baropg_mcc", (), ()), ("profq", (), ()),
    ("profu", (), ()), ("profv", (), ()), ("vertvl", (), ()), ("realvertvl", (), ()), ("lateral_viscosity", (), ()),
    ("mode_interaction", (), ()), ("mode_external", (), ()), ("mode_internal", (), ()),
    ("advq", ("q2b", "q2", "uf"), ()), ("advt1", ("tb", "t", "tclim", "uf"), ()), ("advt2", ("sb", "s", "sclim", "vf"), ()),
    ("dens", ("s", "t", "rho"), ()), ("proft", ("uf", "wtsurf", "tsurf"), (1,)), ("proft", ("vf", "wssurf", "ssurf"), (3,)),
    ("bcond", (), (1,)), ("bcond", (), (2,)), ("bcond", (), (4,)), ("bcond", (), (5,)), ("bcond", (), (6,)),
    ("bcondorl", (), (3,)), ("bcondorl", (), (5,)), ("restore_interior", (), ()),
]


# island: no land at all (dum = dvm = fsm = 1), no curvature; archipelago: every mask, the curvature terms and cor(i-1,j) live, and
# proft's short-wave branches on a non-uniform swrad.  (The island ids stay as they were.)
ROUTINES_ARCHIPELAGO = ROUTINES + [("proft", ("uf", "wtsurf", "tsurf"), (2,)), ("proft", ("uf", "wtsurf", "tsurf"), (4,))]
_rid = lambda r: f"{r[0]}{''.join(map(str, r[2]))}"


@pytest.mark.parametrize("case,name,fields,ints", [("island",) + r for r in ROUTINES] + [("archipelago",) + r for r in ROUTINES_ARCHIPELAGO],
                         ids=[_rid(r) for r in ROUTINES] + ["archipelago-" + _rid(r) for r in ROUTINES_ARCHIPELAGO])
def test_each_routine_bit_identical_to_oracle(case, name, fields, ints):
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case(case, 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    OracleTile(a).run(3)
    a.iint, a.iext = 4, 7
    b = a.copy()
    ot = OracleTile(a)
    ot.call(name, *[ot.a3(f) for f in fields], *[ctypes.c_int(i) for i in ints])
    g = _gpu(b)
    g.call(name, *fields, *ints)
    g.download()
    assert not diff(a, b) and same_bits(a.bdry, b.bdry), f"{name}: {diff(a, b)}"


@pytest.mark.parametrize("name", ["archipelago_default", "archipelago_nadv1", "archipelago_nitera2", "archipelago_npg2", "archipelago_mode2",
                                  "archipelago_mode4", "archipelago_nbct2", "archipelago_nbc3"])
def test_gpu_reproduces_reference_digests_archipelago(name):
    """the fourth case against digests of the REFERENCE's own state (tests/golden/archipelago_65x49x21.json): steps 1, 2, 3, 10, 100 of the
    default namelist, 3 and 20 of the others.  The lane shifts and LDS slabs that carry masks, cor and the curvature coefficients between
    lanes and rows exist on the device only: no emulated test stands in for this one."""
    _reproduces(golden_file("archipelago_65x49x21"), name)


@pytest.mark.parametrize("name", ["archipelago50_default", "archipelago50_npg2"])
def test_gpu_reproduces_reference_digests_archipelago_kb50(name):
    """256x192x50 (tests/golden/archipelago_256x192x50.json): the <50> instantiations, rows of four wavefronts"""
    _reproduces(golden_file("archipelago_256x192x50"), name)


def test_check_velocity_wavefront_reduction():
    """max |vaf| and the LAST arg-max in scan order, incl. ties and an all-zero field (advance.f:619-629)"""
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    rng = np.random.default_rng(1)
    for trial in range(4):
        if trial == 0:
            a.vaf[...] = 0.0
        else:
            a.vaf[...] = rng.standard_normal(a.vaf.shape)
        if trial == 2:
            a.vaf[7, 11] = a.vaf[30, 40] = -9.0     # a tie: the later (j,i) wins
        if trial == 3:
            a.vaf[20, 20] = 1000.0                  # > vmaxl -> error_status
        ot = OracleTile(a)
        ot.call("check_velocity")
        b = a.copy()
        g = _gpu(b)
        assert g.check_velocity() == ot.vamax
        g.get_con()
        assert b.error_status == (1 if trial == 3 else 0)
        a.error_status = 0


def test_surface_and_lateral_forcing_on_device_across_record_changes():
    """wind / heat / surface (bounds_forcing.f:871-983) and lateral_bc (:593-868) with the records in HBM, called
    by advance itself (advance.f:14-18); dti = 360 s puts the record changes of the surface fields at steps 30 and
    60 and those of the lateral boundary values at every tenth step"""
    from extpom_amd.cases import make_forcing_records, make_lateral_records
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=60, days=1.0)
    oracle_finish_initial(a)
    make_forcing_records(a, 4)
    make_lateral_records(a, 8)
    b = a.copy()
    ot = OracleTile(a)
    g = _gpu(b)
    g.set_forcing_records()
    g.set_lateral_records()
    for n in range(1, 63):
        if n % 10 == 0:
            g.set_lateral_records(first=n // 10 + 2, count=1)      # the record lateral_bc asks for at this step
        ot.run(1)
        g.run(1)
        if n in (1, 2, 10, 11, 30, 31, 60, 61, 62):
            g.download()
            assert not diff(a, b) and np.array_equal(a.bdry, b.bdry), f"step {n}: {diff(a, b)}"
    g.close()


def test_output_and_restart_files_without_pnetcdf(tmp_path):
    """write_output_pnetcdf / write_restart_pnetcdf (io_pnetcdf.F:57-410, :1661-2083) as plain CDF-2 files: read back
    with scipy's NetCDF reader -- dimensions, variable names, order, dimensions per variable and attribute texts as
    the reference defines them, values equal to the state on the device"""
    from scipy.io import netcdf_file
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    g = _gpu(a)
    g.run(3)
    g.write_file("output", tmp_path / "out.nc", title="seamount test", time_start="2000-01-01 00:00:00 +00:00")
    g.write_file("restart", tmp_path / "rst.nc", title="seamount test", time_start="2000-01-01 00:00:00 +00:00")
    stats = g.domain_stats()
    g.download()
    g.close()
    kb = 21
    # the WHOLE header of both files -- format version, global attributes, dimensions, every variable in definition order with
    # its type, dimensions and every attribute text -- against tests/golden/cdf_schema.json, which make_cdf_schema.py reads out
    # of the reference's own source (io_pnetcdf.F:6-40, :57-410, :1661-2083), not out of this repository
    from cdf_check import check_header
    for kind, name in (("output", "out.nc"), ("restart", "rst.nc")):
        check_header(tmp_path / name, kind, "seamount test", "2000-01-01 00:00:00 +00:00", kb, 65, 49)
    with netcdf_file(str(tmp_path / "out.nc"), "r", mmap=False) as f:
        assert f.version_byte == 2 and f.title == b"seamount test" and f.description == b"output file"
        assert {k: v for k, v in f.dimensions.items()} == dict(time=1, z=kb, zz=kb - 1, y=49, x=65)
        assert list(f.variables) == ["time", "vtot", "mtot", "tavg", "savg", "eavg", "ekin", "z", "zz", "dx", "dy", "east_u", "east_v",
                                     "east_e", "east_c", "north_u", "north_v", "north_e", "north_c", "rot", "h", "fsm", "dum", "dvm", "uab",
                                     "vab", "elb", "u", "v", "t", "s", "rho", "w"]
        v = f.variables
        assert v["u"].dimensions == ("time", "zz", "y", "x") and v["w"].dimensions == ("time", "z", "y", "x")
        assert v["elb"].dimensions == ("time", "y", "x") and v["h"].dimensions == ("y", "x") and v["zz"].dimensions == ("zz",)
        assert v["u"].long_name == b"x-velocity" and v["u"].units == b"metre/sec" and v["u"].coordinates == b"east_u north_u zz"
        assert v["time"].units == b"days since 2000-01-01 00:00:00 +00:00" and v["z"].formula_terms == b"sigma: z eta: elb depth: h"
        assert v["t"].data.dtype == np.dtype(">f8")
        assert float(v["time"][0]) == a.time
        assert [float(v[n][0]) for n in ("vtot", "mtot", "tavg", "savg", "eavg", "ekin")] == [stats[0], stats[2], stats[4], stats[5], stats[6], stats[7]]
        assert np.array_equal(v["z"][:], a.z) and np.array_equal(v["zz"][:], a.zz[:kb - 1])
        for n in ("dx", "east_c", "rot", "h", "fsm", "dvm"):
            assert np.array_equal(v[n][:], a.field(n)), n
        for n in ("uab", "vab", "elb"):
            assert np.array_equal(v[n][0], a.field(n)), n
        for n in ("u", "v", "t", "s", "rho"):
            assert np.array_equal(v[n][0], a.field(n)[:kb - 1]), n
        assert np.array_equal(v["w"][0], a.w)
    with netcdf_file(str(tmp_path / "rst.nc"), "r", mmap=False) as f:
        assert f.version_byte == 2 and f.description == b"restart file"
        assert {k: v for k, v in f.dimensions.items()} == dict(time=1, z=kb, y=49, x=65)
        from extpom_amd.layout import RESTART_2D, RESTART_3D
        names = list(f.variables)
        assert names[:2] == ["iint", "time"] and sorted(names[2:]) == sorted(RESTART_2D + RESTART_3D)
        assert f.variables["iint"].dimensions == () and float(f.variables["iint"].getValue()) == 3.0
        assert f.variables["q2l"].long_name == b"q2 x l" and f.variables["advua"].long_name == b"sum of 2nd, 3rd and 4th terms in eq (18)"
        for n in RESTART_2D + RESTART_3D:
            assert np.array_equal(f.variables[n][:], a.field(n)), n


def test_files_written_with_the_callers_statistics_see_the_current_state(tmp_path):
    """as tests/test_kernels_emulated.py: the writer's snapshot after an odd number of fused external substeps, with the caller's
    own statistics (no pomgpu_domain_stats call inside), through the asynchronous path"""
    from scipy.io import netcdf_file
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=7)
    oracle_finish_initial(a)
    g = _gpu(a)
    g.run(3)
    g.write_file("output", tmp_path / "out.nc", title="t", time_start="s", stats=(1., 2., 3., 4., 5., 6., 7., 8.))
    g.write_file("restart", tmp_path / "rst.nc", title="t", time_start="s", stats=(1., 2., 3., 4., 5., 6., 7., 8.))
    g.io_wait()
    g.download()
    g.close()
    with netcdf_file(str(tmp_path / "out.nc"), "r", mmap=False) as f:
        assert float(f.variables["vtot"][0]) == 1.0 and float(f.variables["ekin"][0]) == 8.0
        for n in ("uab", "vab", "elb"):
            assert np.array_equal(f.variables[n][0], a.field(n)), n
    with netcdf_file(str(tmp_path / "rst.nc"), "r", mmap=False) as f:
        for n in ("ua", "va", "el", "elb", "uab", "vab", "rho"):
            assert np.array_equal(f.variables[n][:], a.field(n)), n


def test_a_failed_file_write_surfaces_as_a_status():
    """the writers return once the file is laid out; the arrays are written behind the model's back by a host thread.  An I/O
    error there (here: /dev/full, every pwrite fails with ENOSPC) must not be lost: pomgpu_io_wait / pomgpu_sync / the next
    write return it and error_status is 1, as after the reference's handle_error_pnetcdf (io_pnetcdf.F:43-54)"""
    from extpom_amd.lib import PomGpuError
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    g = _gpu(a)
    g.run(1)
    g.write_file("restart", "/dev/full", title="t", time_start="s", create=False)     # laid out by "another rank": only the patch is written
    with pytest.raises(PomGpuError):
        g.io_wait()
    g.get_con()
    assert a.error_status == 1
    a.error_status = 0
    g.set_con(error_status=0)
    g.write_file("output", "/dev/full", title="t", time_start="s", create=False)
    with pytest.raises(PomGpuError):
        g.sync()                                              # sync joins the writer too
    with pytest.raises(PomGpuError):
        g.write_file("output", "/dev/full", title="t", time_start="s", create=True)   # the header itself cannot be written: at once
    g.close()


def test_domain_stats_on_device():
    """print_section's sums (advance.f:644-756) reduced on the device: equal to the oracle to rounding,
    and the same bits every time (fixed reduction tree, no atomics)"""
    import ctypes
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("island", 130, 97, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    b = a.copy()
    ot = OracleTile(a)
    ot.run(4)
    g = _gpu(b)
    g.run(4)
    for sums_only in (0, 1):
        out = (ctypes.c_double * 8)()
        ot.call("domain_stats", out, ctypes.c_int(sums_only))
        got = np.array(g.domain_stats(sums_only=bool(sums_only)))
        np.testing.assert_allclose(got, np.array(list(out)), rtol=1e-12, atol=0)
        assert got.tolist() == list(g.domain_stats(sums_only=bool(sums_only)))
    g.close()


def test_1000_internal_steps_within_1e_10():
    """north_star's bar: all prognostic fields within 1e-10 relative after 1000 internal steps"""
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    b = a.copy()
    OracleTile(a).run(1000)
    g = _gpu(b)
    g.run(1000)
    g.download()
    r = reldiff(a, b, PROGNOSTIC)
    assert max(r.values()) <= 1e-10, r
    assert a.error_status == b.error_status == 0


def test_config2_seamount_256x256x30_matches_oracle():
    """BASELINE config 2 at full size against the oracle (seconds of CPU time per step)"""
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("seamount", 256, 256, 30, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    b = a.copy()
    OracleTile(a).run(6)
    g = _gpu(b)
    g.run(6)
    g.download()
    assert not diff(a, b), diff(a, b)


SWITCH_SETS = [("POMGPU_THOMAS_SCRATCH", "POMGPU_NO_PAIR", "POMGPU_EXT_SPLIT", "POMGPU_ADVQ_SINGLE", "POMGPU_ADVT2_SINGLE",
                "POMGPU_REALVERTVL_CELLS", "POMGPU_BAROPG_CELLS", "POMGPU_VERTVL_CELLS"), ("POMGPU_ADVAVE_SEPARATE", "POMGPU_EXT_RIM_KERNEL"),
               ("POMGPU_EXT_LOOP",), ("POMGPU_RHO_ROUNDTRIP", "POMGPU_TAU_ARRAYS", "POMGPU_IO_SYNC"),
               ("POMGPU_PROFQ_ROWS8", "POMGPU_COL_STRIP", "POMGPU_EXT_MARCH"), ("POMGPU_PROFQ_ROWS2", "POMGPU_PROFQ_NOPACE", "POMGPU_EXT_NOMARCH", "POMGPU_NO_LIN", "POMGPU_EXT_TWO_SETS")]


@pytest.mark.parametrize("switches", SWITCH_SETS)
def test_general_kernels_behind_the_fast_paths(monkeypatch, switches):
    """the scratch-vector / one-column-per-lane / split kernels that serve kb > 64, odd im_local and
    multi-tile runs, selected through the library's developer switches, on an even and an odd grid; second set: the
    external substep with advave and the rim cells as kernels of their own; third: all external substeps in one launch with
    a grid-wide barrier (k_ext_loop, opt-in); fourth: rho's round trip as a kernel of its own, taurstr read from its arrays;
    fifth / sixth: k_profq's 8-row paced workgroups (the large-grid shape) on grids whose last workgroup row is ragged and the
    strip order of the row-sharing column kernels (width 1), and k_profq's 2-row shape without the pacing barrier, the banded XCD
    order of the row-sharing kernels on these ragged grids (the default there is the balanced one); the first set also takes baropg and
    vertvl back to one thread per column"""
    OracleTile, oracle_finish_initial = _oracle()
    for v in switches:
        monkeypatch.setenv(v, "1")
    for im, jm in ((65, 49), (128, 96)):
        a = make_case("seamount", im, jm, 21, dte=6.0, isplit=30)
        oracle_finish_initial(a)
        b = a.copy()
        OracleTile(a).run(3)
        g = _gpu(b)
        g.run(3)
        g.download()
        g.close()
        assert not diff(a, b), (im, jm, diff(a, b))


@pytest.mark.parametrize("switches", SWITCH_SETS)
def test_general_kernels_behind_the_fast_paths_archipelago(monkeypatch, switches):
    """the six switch sets of the test above on the fourth case, 65x49 and 128x96: the general kernels see interior land and a curved grid"""
    OracleTile, oracle_finish_initial = _oracle()
    for v in switches:
        monkeypatch.setenv(v, "1")
    for im, jm in ((65, 49), (128, 96)):
        a = make_case("archipelago", im, jm, 21, dte=6.0, isplit=30)
        oracle_finish_initial(a)
        b = a.copy()
        OracleTile(a).run(3)
        g = _gpu(b)
        g.run(3)
        g.download()
        g.close()
        assert not diff(a, b), (im, jm, diff(a, b))


def test_kb_above_the_register_kernels_bound_archipelago():
    """kb = 70 on the fourth case, short-wave penetration (nbct = 2) on its non-uniform swrad included"""
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("archipelago", 64, 48, 70, dte=6.0, isplit=30, nbct=2)
    oracle_finish_initial(a)
    b = a.copy()
    OracleTile(a).run(3)
    g = _gpu(b)
    g.run(3)
    g.download()
    g.close()
    assert not diff(a, b), diff(a, b)


@pytest.mark.bg_oracle("archipelago", 1024, 1024, 40, 3)
def test_archipelago_1024x1024x40_matches_the_background_oracle(bg_oracle):
    """the default kernel shapes of a large grid (paced k_profq rows, banded XCD order) with land and curvature: steps 1, 2 and 3 on every
    COMMON array that is not scratch against the oracle a child process computes beside the other tests (tests/oracle_bg.py)"""
    OracleTile, oracle_finish_initial = _oracle()
    e = make_case("archipelago", 1024, 1024, 40, dte=6.0, isplit=30)
    oracle_finish_initial(e)
    _against_background_oracle(e, bg_oracle, 3, beat=lambda msg: print(msg, flush=True))


def test_kb_above_the_register_kernels_bound():
    """kb = 70 > 64: the column kernels with private work vectors take over from the unrolled ones"""
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("basin", 64, 48, 70, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    b = a.copy()
    OracleTile(a).run(2)
    g = _gpu(b)
    g.run(2)
    g.download()
    g.close()
    assert not diff(a, b), diff(a, b)


@pytest.mark.bg_oracle("basin", 1024, 1024, 40, 3)
def test_restart_and_determinism_properties_1024x1024x40(bg_oracle):
    """config 3's grid on one GPU, size-independent properties: (i) two runs give identical bits,
    (ii) run(2n) == run(n) + download/upload + run(n) (the restart property), (iii) land stays
    masked, nothing non-finite, (iv) closed basin conserves volume: the area integral of et does
    not drift, (v) steps 1, 2 AND 3 equal the oracle's on every field (3 = the first with every branch warm): at iint = 1 with time0 = 0 mode_internal skips its 3-D
    body (advance.f:362), so step 2 is the first one in which advq / profq / advt2 / proft / advu / advv / profu / profv and
    the filters run, on the default (fast) kernel shapes of this grid."""
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("basin", 1024, 1024, 40, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    b = a.copy()
    vol0 = float((a.et * a.art * a.fsm).sum())
    ga = _gpu(a)
    ga.run(6)
    ga.download()
    ga.close()
    gb = _gpu(b)
    gb.run(3)
    gb.download()
    gb.upload(b)
    gb.run(3)
    gb.download()
    gb.close()
    assert not diff(a, b), diff(a, b)
    for f in PROGNOSTIC + ["q2", "km", "rho", "w"]:
        x = a.field(f)
        assert np.isfinite(x).all(), f
    for f in ("t", "s", "el", "et"):
        x = a.field(f)
        assert not np.any((x if x.ndim == 2 else x[:39]) * (1.0 - a.fsm)), f
    area = float((a.art * a.fsm).sum())
    assert abs(float((a.et * a.art * a.fsm).sum()) - vol0) / area < 1e-12
    e = make_case("basin", 1024, 1024, 40, dte=6.0, isplit=30)
    oracle_finish_initial(e)
    _against_background_oracle(e, bg_oracle, 3)


# ---- the instantiations bench.py runs: kb = 50 and 2048-wide rows ---------------------------------------------------
@pytest.mark.parametrize("name", ["basin50_default", "basin50_nadv1", "basin50_npg2", "seamount50_default"])
def test_gpu_reproduces_reference_digests_kb50(golden_kb50, name):
    """256x192x50: the <50> instantiations of k_proft_reg2 / k_profuv_reg2 / k_uv_filter_reg2 / k_int_uvmean_reg2 (what the
    2048x1536x50 bench dispatches) against digests of the REFERENCE's own state (oracle/_ref/libpomref_256x192x50.so,
    tests/golden/make_golden.py kb50)"""
    _reproduces(golden_kb50, name)


@pytest.mark.parametrize("name", ["basin50_default", "seamount50_default"])
def test_1000_internal_steps_kb50_hash_to_the_reference(name):
    """north_star's bar -- all prognostic fields after 1000 internal steps -- at the benchmark's level count, pinned to the
    REFERENCE ITSELF: digests of every restart-list field after 100 / 500 / 1000 steps of oracle/_ref/libpomref_256x192x50.so
    (tests/golden/kb50_1000steps_<name>.json, make_golden.py kb50long; ten minutes of one core each in the build container).
    north_star asks for 1e-10 relative; equal digests mean the difference is exactly zero."""
    gold = golden_file(f"kb50_1000steps_{name}")
    im, jm, kb = gold["grid"]
    assert kb == 50 and sorted(int(s) for s in gold["configs"][name]["steps"]) == [100, 500, 1000]
    _reproduces(gold, name)


@pytest.mark.parametrize("case,kb,nml", [("basin", 50, {}), ("basin", 50, dict(nadv=1)), ("basin", 50, dict(npg=2)), ("island", 50, {}),
                                         ("basin", 5, {}), ("basin", 6, {}), ("seamount", 7, {}), ("seamount", 24, {}), ("basin", 25, {}), ("seamount", 32, {}),
                                         ("basin", 33, {}), ("basin", 40, {}), ("seamount", 41, {}), ("seamount", 44, {}), ("basin", 45, {}), ("seamount", 56, {}), ("basin", 57, {}),
                                         ("seamount", 64, {}),
                                         ("archipelago", 24, {}), ("archipelago", 25, {}), ("archipelago", 50, {}), ("archipelago", 64, {})])
def test_every_register_kernel_instantiation_matches_oracle(case, kb, nml):
    """ALL fields after 3 steps array_equal to the oracle at the level counts either side of every template bound of
    the register-resident column kernels (k_vert.hip launchers: 24, 32, 40, 44, 50, 56, 64) and at the smallest kb they take"""
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case(case, 64, 48, kb, dte=6.0, isplit=30, **nml)
    oracle_finish_initial(a)
    b = a.copy()
    OracleTile(a).run(3)
    g = _gpu(b)
    g.run(3)
    g.download()
    g.close()
    assert not diff(a, b), (case, kb, nml, diff(a, b))


@pytest.mark.parametrize("case,im,jm,kb", [("basin", 2048, 24, 12), ("seamount", 2050, 20, 50), ("basin", 2047, 16, 8),
                                           ("archipelago", 2050, 20, 50)])                       # land in the last columns of the row
def test_wide_rows_band_geometry_matches_oracle(case, im, jm, kb):
    """iml >= 2047: the launch geometry of the bench grid's rows (set_band_geometry picks 4-row bands, 33-34 workgroups
    per block-row in HALO_XCD_DECODE), all fields after 2 steps array_equal to the oracle"""
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case(case, im, jm, kb, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    b = a.copy()
    OracleTile(a).run(2)
    g = _gpu(b)
    g.run(2)
    g.download()
    g.close()
    assert not diff(a, b), diff(a, b)


def test_100_internal_steps_256x192x50_within_1e_10():
    """north_star's 1e-10 bar on a grid with the bench's level count: 100 internal steps (3000 external) of the basin
    case at 256x192x50 against the oracle; observed difference is zero"""
    OracleTile, oracle_finish_initial = _oracle()
    a = make_case("basin", 256, 192, 50, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    b = a.copy()
    OracleTile(a).run(100)
    g = _gpu(b)
    g.run(100)
    g.download()
    g.close()
    r = reldiff(a, b, PROGNOSTIC)
    assert max(r.values()) <= 1e-10, r
    assert not diff(a, b), diff(a, b)
    assert a.error_status == b.error_status == 0


@pytest.mark.bg_oracle("basin", 2048, 1536, 50, 3)
def test_config4_2048x1536x50_full_size(bg_oracle):
    """BASELINE configs[3]'s grid -- the one bench.py reports -- at full size on one GPU, default (fast) kernel shapes:
    (i) steps 1, 2 AND 3, every field equal to the oracle bit for bit (step 3: the first with every branch warm).  Step 1 (iint = 1, time0 = 0) skips mode_internal's 3-D body
    (advance.f:362); step 2 is the first in which k_profq<1,1,8>, k_advt2_col<2>, k_advq_col<2>, k_advct_col, k_advuv_col in
    strip order, k_ts_update and the <50> register kernels run AT THE BENCHMARKED LAUNCH GEOMETRY -- it is compared with the
    oracle directly.  The oracle's three steps (about three minutes of one CPU core) are computed by a child process from the
    start of the session, beside the other tests (tests/oracle_bg.py); (ii) land stays masked, nothing non-finite.
    (Fast against general kernel shapes over the whole horizon at this size: tools/fullsize_1000.py,
    profiles/round4_fullsize_1000_steps_fast_against_general_kernels.txt; the multi-tile path over 50 steps:
    test_full_size_decomposition_invariance_whole_rows_and_baselines_2x4.)  ~50 GB per host copy of the state."""
    import os
    import time
    OracleTile, oracle_finish_initial = _oracle()
    os.makedirs("gpurun_out", exist_ok=True)
    t0 = time.time()

    def beat(msg):                                   # the GPU box's watchdog looks for signs of life under gpurun_out/
        with open("gpurun_out/fullsize_progress.log", "a") as f:
            f.write(f"{time.time() - t0:7.1f} s  {msg}\n")

    a = make_case("basin", 2048, 1536, 50, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    beat("case built")
    _against_background_oracle(a, bg_oracle, 3, beat)    # step 3: the first with every branch warm (leapfrog levels, filters, restore records)
    for f in PROGNOSTIC + ["q2", "km", "rho", "w"]:
        assert np.isfinite(a.field(f)).all(), f
    for f in ("t", "s", "el", "et"):
        x = a.field(f)
        assert not np.any((x if x.ndim == 2 else x[:49]) * (1.0 - a.fsm)), f
    assert a.error_status == 0
    beat("done")


def test_gpu_equals_the_references_own_advance_with_file_forcing():
    """the HIP path (pomgpu_advance with the forcing and lateral records in HBM) against digests of the reference's OWN
    `advance` subroutine (tests/golden/forced_advance_65x49x21.json, make_golden.py forced)"""
    import json
    import os
    from extpom_amd.cases import make_forcing_records, make_lateral_records
    OracleTile, oracle_finish_initial = _oracle()
    here = os.path.dirname(os.path.abspath(__file__))
    gold = json.load(open(os.path.join(here, "golden", "forced_advance_65x49x21.json")))
    cfg = gold["config"]
    im, jm, kb = gold["grid"]
    st = make_case(cfg["case"], im, jm, kb, **cfg["nml"])
    oracle_finish_initial(st)
    make_forcing_records(st, cfg["forcing_records"])
    make_lateral_records(st, cfg["lateral_records"])
    g = _gpu(st)
    g.set_forcing_records()
    g.set_lateral_records()
    checkpoints = sorted(int(s) for s in cfg["steps"])
    for n in range(1, checkpoints[-1] + 1):
        if n % 10 == 0:
            g.set_lateral_records(first=n // 10 + 2, count=1)      # the record lateral_bc asks for at this step
        g.run(1)
        if n in checkpoints:
            g.download()
            want = cfg["steps"][str(n)]
            bad = [f for f in gold["fields"] if _digest(st.field(f)) != want[f]]
            assert not bad and _digest(st.bdry) == want["bdry"], f"step {n}: {bad}"
    g.close()


def test_fp32_storage_variant_tracks_the_fp64_path_within_its_stated_drift():
    """BASELINE configs[4]'s study variant (libpomgpu_f32.so: the same sources with -DPOMGPU_STORE_F32 -- 3-D arrays stored
    as fp32, arithmetic and the 2-D external mode fp64).  It is NOT a parity path: the flow amplifies rounding-level
    differences (profiles/round2_fp32_storage_study_gpu.txt: 1.5e-8 in u after one step, 2.7e-4 after 10, 5e-2 after 100).
    Asserted: it runs, it is the variant, and it stays inside that envelope for 1 and 10 steps; the output writer is
    refused there (tiles: test_fp32_storage_variant_on_tiles)."""
    from extpom_amd import lib as L
    from extpom_amd.lib import PomGpuError
    from extpom_amd.model import PomGpu, gpu_finish_initial
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30)
    gpu_finish_initial(a, device=0)
    b = a.copy()
    g64, g32 = PomGpu(a, device=0), PomGpu(b, device=0, libpath=L.LIBPATH_F32)
    assert b"fp32-storage" in g32.L.pomgpu_version() and b"fp32" not in g64.L.pomgpu_version()
    for steps, bound in ((1, 2e-7), (10, 2e-3)):
        g64.run(steps - (0 if steps == 1 else 1)); g32.run(steps - (0 if steps == 1 else 1))
        g64.download(); g32.download()
        r = reldiff(a, b, PROGNOSTIC)
        assert max(r.values()) <= bound, (steps, r)
        assert max(r.values()) > 0 or steps == 0              # it really is another precision
        assert a.error_status == b.error_status == 0
    with pytest.raises(PomGpuError):
        g32.write_file("output", "/tmp/should_not_exist.nc")
    g64.close(); g32.close()


@pytest.mark.gpu
def test_fp32_storage_variant_at_the_benchmarks_level_count():
    """the drift envelope of the fp32-storage variant at kb = 50 (256x192x50, the bench's level count and the <50> register
    kernels): after 1 internal step the prognostic fields sit at fp32 rounding level of the fp64 path, after 10 steps inside
    the envelope the 65x49x21 study found (the flow amplifies rounding-level differences: DESIGN.md section 8)"""
    from extpom_amd import lib as L
    from extpom_amd.model import PomGpu, gpu_finish_initial
    # the seamount case: its 0.2 m/s inflow gives every field a magnitude of its own (in the basin at rest the flow IS the response
    # to a 1e-3 K perturbation, of which fp32 rounding of T is 1e-3: u differs by 1e-2 of its tiny maximum after the first 3-D step)
    a = make_case("seamount", 256, 192, 50, dte=6.0, isplit=30)
    gpu_finish_initial(a, device=0)
    b = a.copy()
    g64, g32 = PomGpu(a, device=0), PomGpu(b, device=0, libpath=L.LIBPATH_F32)
    seen = {}
    for steps, bound in ((2, 2e-5), (10, 1e-2)):     # step 1 skips the 3-D body (advance.f:362): 2 is the first step that stores fp32
        g64.run(steps - (0 if steps == 2 else 2)); g32.run(steps - (0 if steps == 2 else 2))
        g64.download(); g32.download()
        r = reldiff(a, b, PROGNOSTIC)
        seen[steps] = max(r.values())
        assert 0 < max(r.values()) <= bound, (steps, r)
        assert a.error_status == b.error_status == 0
    print("fp32-storage drift at 256x192x50:", seen)
    g64.close(); g32.close()


@pytest.mark.gpu
def test_fp32_storage_drift_envelope_on_the_configs_own_grid():
    """BASELINE configs[4] names 2048x1536x50: both builds from identical initial states of the bench grid in one process (60 + 30 GB of
    the 288), 10 internal steps, every prognostic field within the envelope measured at this size (profiles/round5_fp32_drift_basin2048.json,
    tools/fp32_study_gpu.py --full-drift: 1 / 10 / 100 steps) -- T and S at fp32 rounding level, the velocities and the elevation within per
    cents of maxima that are themselves tiny (the basin starts at rest: its flow IS the response to a 1e-3 K perturbation) -- and the
    fp32-storage run is really another run (T differs)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    from fp32_drift import full_size_drift
    d = full_size_drift([10])
    r = d["steps"]["10"]
    bound = {"t": 4e-6, "s": 2e-6, "el": 2e-2, "et": 2e-2, "ua": 5e-3, "va": 5e-2, "u": 2e-3, "v": 2e-2}   # measured x ~4
    print("fp32-storage drift at 2048x1536x50 after 10 steps:", {f: float(f"{r[f]:.2e}") for f in bound})
    assert r["error_status"] == [0, 0], r
    assert all(r[f] <= bound[f] for f in bound), {f: (r[f], bound[f]) for f in bound if r[f] > bound[f]}
    assert r["t"] > 1e-9 and r["s"] > 1e-9, r


@pytest.mark.gpu
def test_fp32_storage_variant_on_tiles():
    """configs[4]'s other half: the fp32-storage variant under the library's exchange and the wide-halo external mode (its
    halos travel as doubles: a stored fp32 value widens exactly and rounds back to itself).  1 x 4 whole-row tiles of
    256x192x50 against the single tile, both in fp32 storage, GPU against GPU.  Unlike the product the variant is NOT
    decomposition-invariant bit for bit (a fused kernel integrates the fp64 values it holds where the tile path's edge-line
    kernels re-read fp32-rounded ones): asserted is that T, S, rho, the velocities and the elevation stay within the
    fp32-storage envelope of the single tile, and that the run completes with its message rounds (the script prints the
    largest difference per field).  The stated cause is asserted too (second run below)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_tiles_threads.py"), "256x192x50", "4", "6", "f32"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "TILES-THREADS-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    # the cause, asserted: with the q2 / q2l filter and the vertical integrals working from the STORED arrays on both sides (POMGPU_QFILTER_SPLIT,
    # POMGPU_SUM2D_OFF: the places where a tile's edge-line kernels re-read fp32-rounded values that the single tile's fused kernels hold
    # unrounded) one tile and four tiles of the fp32-storage variant carry the SAME bits on every owned cell of every array
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_tiles_threads.py"), "256x192x50", "4", "6", "f32", "stored_only"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "TILES-THREADS-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("canonical", [True, False])
def test_marching_external_substep_with_and_without_canonical_areas(monkeypatch, canonical):
    """k_ext_march forced onto a small grid with a ragged last segment (its default use is the full-size test): art, aru, arv
    formed from dx, dy where the arrays ARE initialize.f:361-367's formulas (k_check_areas decides on the device), read from
    memory where the host's arrays differ in the last bit on a few cells -- all fields equal to the oracle's either way"""
    OracleTile, oracle_finish_initial = _oracle()
    monkeypatch.setenv("POMGPU_EXT_MARCH", "1")
    monkeypatch.setenv("POMGPU_EXT_ROWS", "6")
    a = make_case("seamount", 200, 93, 11, dte=6.0, isplit=10)
    oracle_finish_initial(a)
    if not canonical:
        for name in ("aru", "art", "arv"):
            f = a.field(name)
            f[5:80:3, 7:190:5] = np.nextafter(f[5:80:3, 7:190:5], np.inf)
    b = a.copy()
    OracleTile(a).run(2)
    g = _gpu(b)
    g.run(2)
    g.download()
    g.close()
    assert not diff(a, b), diff(a, b)


@pytest.mark.parametrize("case,im,jm,kb,isplit,rows2", [("seamount", 200, 93, 11, 10, "6"), ("island", 130, 97, 9, 7, "5"), ("seamount", 65, 49, 21, 30, None),
                                                        ("basin", 257, 64, 6, 8, "30"), ("seamount", 121, 60, 8, 4, "2"),
                                                        ("archipelago", 200, 93, 11, 10, "6")])
def test_two_external_substeps_per_pass(monkeypatch, case, im, jm, kb, isplit, rows2):
    """k_ext_march2 (two substeps per pass over memory: the second generation marches one row behind the first, the rim's
    intermediate generation through a third buffer set) forced onto small grids -- its default use is the full-size test:
    ragged last segments and wavefronts, segments of 2 to 30 rows, an odd isplit (the last substep alone), the etf weights
    of the last three substeps falling on either half of a pair, open (seamount), island and closed (basin) rims.  All fields
    bit for bit equal to the oracle's."""
    OracleTile, oracle_finish_initial = _oracle()
    monkeypatch.setenv("POMGPU_EXT_PAIR", "1")
    if rows2:
        monkeypatch.setenv("POMGPU_EXT_ROWS2", rows2)
    a = make_case(case, im, jm, kb, dte=6.0, isplit=isplit)
    oracle_finish_initial(a)
    b = a.copy()
    OracleTile(a).run(3)
    g = _gpu(b)
    g.prof_begin()
    g.run(3)
    prof = g.prof_end()
    g.download()
    g.close()
    assert prof.get("k_ext_pair", (0, 0))[0] == 3 * (isplit // 2), prof.keys()     # the path under test did run
    assert not diff(a, b), diff(a, b)


def test_reference_call_sequence_pairs_its_external_substeps(monkeypatch):
    """the Fortran host's way (advance.f:6-59 routine by routine: isplit calls of pomgpu_mode_external): an odd substep of a tile that
    takes two substeps per pass waits for the next call and the two run as ONE pass; a download in between (here after substep 3
    of step 2) makes the waiting substep run alone first.  Same bits as the oracle either way."""
    OracleTile, oracle_finish_initial = _oracle()
    monkeypatch.setenv("POMGPU_EXT_PAIR", "1")
    isplit = 8
    a = make_case("seamount", 96, 80, 9, dte=6.0, isplit=isplit)
    oracle_finish_initial(a)
    b = a.copy()
    OracleTile(a).run(3)
    g = _gpu(b)
    g.prof_begin()
    for n in range(1, 4):
        g.set_con(iint=n)
        g.call("get_time")
        g.get_con()
        g.call("lateral_viscosity")
        g.call("mode_interaction")
        for iext in range(1, isplit + 1):
            g.set_con(iext=iext)
            g.call("mode_external")
            if n == 2 and iext == 3:
                g.download()                                  # substep 3 was waiting for substep 4: it runs alone now
                g.set_con(iext=iext)
        g.set_con(iext=isplit + 1)
        g.call("mode_internal")
        g.check_velocity()
    prof = g.prof_end()
    g.download()
    g.close()
    assert prof.get("k_ext_pair", (0, 0))[0] == 3 * (isplit // 2) - 1, {k: v[0] for k, v in prof.items() if "ext" in k}
    assert not diff(a, b), diff(a, b)


@pytest.mark.gpu
def test_bench_cpu_workers_never_open_the_gpu():
    """bench.py's all-cores CPU leg starts one oracle process per core; the GPU boxes end a job in which more than a handful of
    processes hold the device open (round 4: the default bench died of it -- torch.distributed.barrier() on a gloo group
    initialises the GPU runtime; tools/diag/kfd_open.py).  Two workers of the smallest workload, on a box that HAS a GPU: neither
    may have /dev/kfd or a render node open when it is done."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1",
                   POM_TILE_GRID="1x2", POM_BENCH_REPORT_DEVICE_FDS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "bench.py"), "--cpu-tiles-worker", "--workload", "seamount65"],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    for r, o in enumerate(outs):
        assert f"DEVICE-FDS rank {r}: []" in o, o[-2000:]



@pytest.mark.gpu
def test_tune_placement_moves_the_arrays_and_keeps_the_bits(monkeypatch):
    """pomgpu_tune_placement (include/pomgpu.h): blk3d and the 3-D scratch arrays move into one allocation and are tried at several
    start offsets with real steps in between.  Where an array lives must not show in any result: after two steps, the trials (forced
    on this small grid: POMGPU_TUNE_FORCE) and three more steps every field equals the oracle's after as many steps, bit for bit;
    a second call re-uses the allocation."""
    OracleTile, oracle_finish_initial = _oracle()
    monkeypatch.setenv("POMGPU_TUNE_FORCE", "1")
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    b = a.copy()
    oa, g = OracleTile(a), _gpu(b)
    g.run(2)
    r = g.tune_placement(2, 5)
    assert r["tried"] == 5 and len(set(r["front_mib"])) >= 1 and 0 <= r["kept"] < 5, r
    g.run(1)
    r2 = g.tune_placement(1, 3)
    assert r2["tried"] == 3, r2
    g.run(2)
    g.download()
    oa.run(2 + 5 * (2 + 1) + 1 + 3 * (1 + 1) + 2)                # every trial: one untimed step after the move, then the timed ones
    bad = diff(a, b)
    assert not bad, bad
    assert a.iint == b.iint
    g.close()


@pytest.mark.gpu
def test_tune_placement_refuses_once_a_3d_address_has_been_handed_out(monkeypatch):
    """pomgpu_tune_placement moves blk3d and frees the allocations it lived in: an address obtained from pomgpu_device_3d before would
    dangle (a host's device pointer, a torch tensor wrapped around it, an exchange hook's cache).  The call therefore refuses from
    the first pomgpu_device_3d on (include/pomgpu.h), the state is untouched, and the context goes on stepping with the oracle's bits."""
    from extpom_amd.lib import PomGpuError
    OracleTile, oracle_finish_initial = _oracle()
    monkeypatch.setenv("POMGPU_TUNE_FORCE", "1")
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    b = a.copy()
    oa, g = OracleTile(a), _gpu(b)
    g.run(2)
    assert g.device_ptr("aam") != 0
    with pytest.raises(PomGpuError, match="pomgpu_device_3d"):
        g.tune_placement(1, 2)
    g.run(2)                                          # (the refusal also raised error_status, the reference's convention; the arrays are what they were)
    g.download()
    oa.run(4)
    assert int(b.error_status) == 1 and not diff(a, b), diff(a, b)
    g.close()



@pytest.mark.gpu
def test_bench_dump_outputs_hold_the_state_after_the_warm_up_profiled_and_timed_steps(tmp_path):
    """bench.py --dump-outputs: what the timed path computed in its last step.  The placement trials (forced on this small grid:
    POMGPU_TUNE_FORCE) advance the model by as many steps as layouts fit in free memory; the bench starts its warm-up from the
    initial state again, so the dump is the oracle's state after exactly warm-up + one profiled + K timed steps, bit for bit."""
    import json
    import os
    import subprocess
    import sys
    from extpom_amd import dist as pdist
    from extpom_amd.layout import RESTART_2D, RESTART_3D
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    OracleTile, oracle_finish_initial = _oracle()
    env = dict(os.environ, POMGPU_TUNE_FORCE="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "seamount65", "--steps", "3", "--warmup", "2",
                        "--no-cpu-baseline", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["error_status"] == 0, line
    assert line["config"]["placement"]["tried"] > 0, line["config"]["placement"]
    sys.path.insert(0, root)
    import bench
    a = bench.build_state("seamount65", pdist.tile_for_rank(0, 1, 65, 49))
    oracle_finish_initial(a)
    OracleTile(a).run(2 + 1 + 3)
    bad = [n for n in RESTART_2D + RESTART_3D if not same_bits(np.load(tmp_path / f"{n}.npy"), a.field(n))]
    assert not bad, bad


@pytest.mark.gpu
def test_bench_plain_run_leaves_the_cpu_baselines_to_full():
    """bench.py without --full does what its headline figure needs: no CPU leg runs and none is on the line.  --full measures
    them as before -- THE cpu_baseline (the oracle on the bench's own grid, one core) and the sample beside it (the grid itself on
    the smallest workload) -- and --no-cpu-baseline still leaves them out of a --full run."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def line(*extra):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "seamount65", "--steps", "2", "--warmup", "1", *extra],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])

    cpu_legs = lambda out: sorted(k for k in out if k.startswith("cpu_baseline"))
    plain = line()
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["error_status"] == 0, plain
    assert plain["dtype"] == "f64" and plain["unit"] == "cell-updates/s" and plain["higher_is_better"] is True, plain
    assert cpu_legs(plain) == [], cpu_legs(plain)
    full = line("--full")
    assert full["cpu_baseline"]["kind"] == "port" and full["cpu_baseline"]["value"] > 0, full.get("cpu_baseline")
    assert full["cpu_baseline_sample_port"]["value"] > 0, cpu_legs(full)
    assert cpu_legs(line("--full", "--no-cpu-baseline")) == []
