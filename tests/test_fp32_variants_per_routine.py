"""The two fp32 study builds routine by routine against the fp64 oracle, on the host (tests/emu builds the unmodified kernel
sources of libpomgpu_f32.so and libpomgpu_f32a.so for the CPU).  Every case starts from a warm state whose 3-D arrays hold fp32
values, so the oracle and the variants see the same inputs and only the rounding of the results can differ.

(a) fp32 storage (-DPOMGPU_STORE_F32): every routine of ROUTINES gives fp32(oracle) bit for bit in every 3-D array and the
    oracle itself in every 2-D array, signed zeros included -- but for the pairs of EXEMPT, each with its cause and a per-cell
    bound in fp32 ulps of the reference.
(b) fp32 arithmetic (-DPOMGPU_STORE_F32 -DPOMGPU_COMPUTE_F32): every routine outside the fp32 kernels gives the storage
    variant's bits.
(c) The fp32 kernels per cell against fp32(oracle): advt2 and advq within a few ulps of the cell's own value, advct and
    lateral_viscosity within C u32 S + 1 ulp, S the per-cell condition scale of advct_scale().  Also on seeded O(1) noise in
    place of the advected fields, where a wrong neighbour or a dropped term cannot hide under |T| ~ 15.
(d) The fp32 kernels that run only inside mode_internal, against the kernels the developer switches put in their place:
    k_advt2x2_col / k_advq2_col against the single kernels (same bits), k_advuv_col against the fp64 k_advu_profu /
    k_advv_profv (POMGPU_THOMAS_SCRATCH; same bits in fp32 storage, bounded per cell in fp32 arithmetic), and k_ts_update's
    rho against the oracle's dens of the variant's own t and s (same bits).
DESIGN.md section 7 states the bounds.  tests/test_gpu_fp32_variants_per_routine.py runs the same checks on the device."""
import concurrent.futures
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from extpom_amd.cases import make_case
from extpom_amd.layout import BLK2D, BLK3D
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_kernels_emulated import ROUTINES, SCRATCH  # noqa: E402

EMU_F32 = os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so")
EMU_F32A = os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")
U32 = 2.0 ** -24                                              # unit roundoff of fp32

# grids: (case, im, jm, kb, namelist).  Odd and even im (the two-columns-per-lane kernels), a narrow 128 x 12 island, kb = 50
# (the <50> register kernels) and kb = 70 (above the register kernels' bound: the column kernels with work vectors)
SHAPES = {
    "island": ("island", 65, 49, 21, {}),
    "seamount": ("seamount", 65, 49, 21, {}),
    "even66x50": ("seamount", 66, 50, 21, {}),
    "island128x12": ("island", 128, 12, 21, {}),
    "kb50": ("seamount", 65, 49, 50, {}),
    "kb70": ("basin", 64, 48, 70, {}),
}
# the branches the variants treat differently: the fp64 advt1 (nadv = 1), advt2's fp64 iterations (nitera > 1), baropg_mcc
# (npg = 2), no internal mode (mode = 2) and no tracer step (mode = 4)
BRANCHES = {
    "nadv1": ("seamount", 65, 49, 21, dict(nadv=1)),
    "nitera2": ("island", 65, 49, 21, dict(nitera=2)),
    "nitera3": ("seamount", 65, 49, 21, dict(nitera=3, sw=1.0)),
    "npg2": ("island", 65, 49, 21, dict(npg=2)),
    "mode2": ("seamount", 65, 49, 21, dict(mode=2)),
    "mode4": ("seamount", 65, 49, 21, dict(mode=4)),
}
BRANCH_ROUTINES = {"nadv1": ("advt1", "mode_internal"), "nitera2": ("advt2", "mode_internal"), "nitera3": ("advt2", "mode_internal"),
                   "npg2": ("baropg_mcc", "mode_internal"), "mode2": ("mode_external", "mode_internal"),
                   "mode4": ("mode_external", "mode_internal")}
# the grids of tests/test_gpu_fp32_variants_per_routine.py (256 x 192 x 50: the bench's level count)
GPU_SHAPES = {"gpu_island": ("island", 65, 49, 21, {}), "gpu_seamount256x192x50": ("seamount", 256, 192, 50, {})}
# seeded O(1) noise in place of the advected fields (the geometry, masks and velocities of the warm state stay)
NOISE = {"island+noise": "island", "seamount+noise": "seamount", "even66x50+noise": "even66x50"}
NOISE_FIELDS = ("t", "tb", "tclim", "s", "sb", "sclim", "q2", "q2b", "q2l", "q2lb")
NOISE_ROUTINES = ("advq", "advt2")                            # (advct reads no advected field)

# (a): the routine-array pairs of the storage variant that are not fp32(oracle) bit for bit -- why, and for which grids: a function of
# the case name giving the largest distance from fp32(oracle) any cell may have, in fp32 ulps of the reference (2x what that case
# measures, or less), or None where the pair must be exact.
def _kb(cfg):
    return (SHAPES | BRANCHES | GPU_SHAPES)[NOISE.get(cfg, cfg)][3]


def _nitera(cfg):
    return (SHAPES | BRANCHES | GPU_SHAPES)[NOISE.get(cfg, cfg)][4].get("nitera", 1)


EXEMPT = {
    ("profq", "uf"): ("k_profq keeps its elimination vectors in memory -- gg1, gg2 in uf, vf in place, ee1, ee2 in the scratch arrays "
                      "s3[4], s3[5] -- which are fp32 in this build: the back substitution reads rounded ee, gg.  The error of the "
                      "recurrence grows with the column: measured at most 3 ulps up to kb = 50, 105 at kb = 70",
                      lambda cfg: 6 if _kb(cfg) <= 50 else 210),
    ("profq", "vf"): ("as profq/uf; measured at most 3 ulps up to kb = 50, 39 at kb = 70", lambda cfg: 6 if _kb(cfg) <= 50 else 78),
    ("advt2", "vf"): ("nitera > 1 only: the Smolarkiewicz iterations hand ff from k_advt2_step to k_smol, to the next iteration (s3[3]) "
                      "and to k_advt2_diff through memory, fp32 in this build.  Measured 1 ulp; nitera = 1 (k_advt2_col) is exact",
                      lambda cfg: 2 if _nitera(cfg) > 1 else None),
}
# mode_internal: the step path passes its intermediates (advq's and profq's q2 / q2l in uf / vf, the tracer forecast in uf / vf,
# advx / advy, the velocity forecast, ...) through fp32 arrays where the oracle keeps fp64, and k_ts_update's dens takes the
# unrounded t, s: every array it writes differs.  Near-zero cells make ulps of the cell's own value meaningless here (w, wr), so
# the bound is in fp32 ulps of the largest |value| of the cell's level: 2x the largest measured over SHAPES, BRANCHES and GPU_SHAPES
# (host build; the device gives the same maxima at 256 x 192 x 50).
MODE_INTERNAL_LEVEL_ULPS = {"q2b": 22, "q2": 78, "q2lb": 2, "q2l": 38, "rho": 24, "tb": 2, "t": 22, "sb": 2, "s": 34,
                            "ub": 2, "uf": 22, "u": 22, "vb": 2, "vf": 30, "v": 30, "w": 530, "wr": 141}
# ... and the bottom stresses profu / profv leave (2-D): in u32 of the array's largest |value| (measured 9.8 and 16)
MODE_INTERNAL_2D_U32 = {"wubot": 19.5, "wvbot": 32}
# (c): per-cell bounds of the fp32 kernels in fp32 ulps of the reference (largest measured: advt2 2.0, advq 5.0 at kb = 50) ...
CELL_ULPS = {"advt2": 4.0, "advq": 6.0}
# ... on the noise input in ulps of the level's largest |value| (a forecast of O(1) noise is near zero in many cells; measured
# advt2 4, advq 2) ...
NOISE_LEVEL_ULPS = {"advt2": 8.0, "advq": 4.0}
# ... and C of |got - ref| <= C u32 S + ulp32(ref) for advct's advx, advy (largest measured: 2.9 on the host grids, kb = 50;
# 3.4 on the device at 256 x 192 x 50)
ADVCT_C = 4.0


@pytest.fixture(scope="module", autouse=True)
def emu_variants():
    for v in ("f32", "f32a"):
        subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), v], stdout=subprocess.DEVNULL)


# ---- states and runs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _warm(cfg):
    """the 65x49x21-style warm state of test_kernels_emulated.warm_state at cfg, 3-D arrays rounded to fp32 (read-only: copy it)"""
    if cfg in NOISE:
        a = _warm(NOISE[cfg]).copy()
        rng = np.random.default_rng(sum(map(ord, cfg)))
        for n in NOISE_FIELDS:
            a.field(n)[...] = rng.uniform(-1.0, 1.0, a.field(n).shape).astype(np.float32)
        for n in ("q2", "q2b", "q2l", "q2lb"):                  # turbulence quantities stay positive
            a.field(n)[...] = np.abs(a.field(n)) + 0.5
        a.blk3d[...] = a.blk3d.astype(np.float32)               # (the sums above are fp64: held as fp32 values like every input)
        return a
    case, im, jm, kb, nml = (SHAPES | BRANCHES | GPU_SHAPES)[cfg]
    a = make_case(case, im, jm, kb, dte=6.0, isplit=30, **nml)
    oracle_finish_initial(a)
    OracleTile(a).run(3)
    a.iint = 4
    a.iext = 7
    a.blk3d[...] = a.blk3d.astype(np.float32)
    return a


def run_routine(lib, st, name, fields=(), ints=(), switches=()):
    """a copy of st after routine `name` of the oracle (lib None) or of the library at lib"""
    b = st.copy()
    if lib is None:
        ot = OracleTile(b)
        ot.call(name, *[ot.a3(f) for f in fields], *[ctypes.c_int(i) for i in ints])
        return b
    g = PomGpu(b, libpath=lib)
    for s in switches:
        g.switch(s, 1)
    g.call(name, *fields, *ints)
    g.download()
    g.close()
    return b


_POOL = concurrent.futures.ThreadPoolExecutor(3)                # ctypes lets go of the GIL: the three runs side by side


@functools.lru_cache(maxsize=2)
def _runs(cfg, name, fields, ints, libs=(EMU_F32, EMU_F32A)):
    """(oracle, fp32 storage, fp32 arithmetic) after one routine from cfg's warm state"""
    a0 = _warm(cfg)
    futs = [_POOL.submit(run_routine, lib, a0, name, fields, ints) for lib in (None,) + tuple(libs)]
    return tuple(f.result() for f in futs)


# ---- comparisons --------------------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x).astype(np.float32)


def bits32(x):
    return f32(x).view(np.uint32)


def ulp32(ref):
    """fp32 ulp of each cell's reference value (as float64)"""
    return np.spacing(np.abs(f32(ref))).astype(np.float64)


def ulps(got, ref):
    """|got - ref| in fp32 ulps of ref, per cell (both rounded to fp32 first)"""
    g, r = f32(got).astype(np.float64), f32(ref).astype(np.float64)
    return np.abs(g - r) / ulp32(ref)


def level_ulps(got, ref):
    """|got - ref| in fp32 ulps of the largest |ref| of the cell's level"""
    g, r = f32(got).astype(np.float64), f32(ref).astype(np.float64)
    top = np.abs(r).max(axis=tuple(range(1, r.ndim)), keepdims=True)
    return np.abs(g - r) / np.maximum(ulp32(top), np.finfo(np.float32).tiny)


def rel_u32(got, ref):
    """largest |got - ref| in u32 of the largest |ref| (fp64 arrays)"""
    return float(np.abs(got - ref).max() / (U32 * max(float(np.abs(ref).max()), 1e-300)))


def same_zeros(got, ref):
    """the zero pattern and the sign of every zero agree"""
    g, r = f32(got), f32(ref)
    return np.array_equal(g == 0, r == 0) and np.array_equal(np.signbit(g[r == 0]), np.signbit(r[r == 0]))


def arrays3():
    return [n for n in BLK3D if n not in SCRATCH]


def arrays2():
    return [n for n in BLK2D if n not in SCRATCH]


def storage_mismatches(o, s, name, cfg):
    """[(array, cells, largest ulps)] of every array of the storage variant s that is not what (a) asks of it at cfg"""
    bad = []
    for n in arrays3():
        if np.array_equal(bits32(o.field(n)), bits32(s.field(n))):
            continue
        if name == "mode_internal":
            d, exempt = level_ulps(s.field(n), o.field(n)), MODE_INTERNAL_LEVEL_ULPS.get(n)
        else:
            d, exempt = ulps(s.field(n), o.field(n)), EXEMPT[name, n][1](cfg) if (name, n) in EXEMPT else None
        if exempt is None or not np.isfinite(d).all() or d.max() > exempt:
            bad.append((n, int((bits32(o.field(n)) != bits32(s.field(n))).sum()), float(d.max())))
    for n in arrays2():
        if not np.array_equal(o.field(n).view(np.uint64), s.field(n).view(np.uint64)):
            r = rel_u32(s.field(n), o.field(n))
            if name != "mode_internal" or r > MODE_INTERNAL_2D_U32.get(n, -1):
                bad.append((n, int((o.field(n) != s.field(n)).sum()), r))
    return bad


def identical_arrays(x, y, skip=()):
    """the arrays in which two runs differ (every bit of the stored value, 2-D arrays included)"""
    return [n for n in arrays3() + arrays2() if n not in skip and not np.array_equal(x.field(n).view(np.uint64), y.field(n).view(np.uint64))]


def fixed_cells(st, kb_level=True):
    """land cells, the outermost line on every side and level kb: what the fp32 stencils do not compute (must be exact)"""
    kb, jm, im = st.kb, st.jm, st.im
    m = np.zeros((kb, jm, im), bool)
    m[:, st.fsm[:jm, :im] == 0] = True
    m[:, [0, -1], :] = True
    m[:, :, [0, -1]] = True
    if kb_level:
        m[-1] = True
    return m


def advct_scale(st):
    """(Sx, Sy): advct's advx, advy evaluated on |operands| with every difference turned into a sum -- the sum of the absolute
    values of the terms and of the intermediate sums each cell's result is made of (oracle/pom_oracle.c pomo_advct, solver.f:
    206-405).  An fp32 evaluation of any order of those operations is within a small multiple of u32 * S of the exact result;
    the result itself may be far smaller (it is a difference of fluxes)."""
    kb, jm, im = st.kb, st.jm, st.im
    A = lambda n: np.abs(st.field(n)[:, :jm, :im])                                    # noqa: E731
    dt, dx, dy, aru, arv = (np.abs(st.field(n)[:jm, :im]) for n in ("dt", "dx", "dy", "aru", "arv"))
    u, v, ub, vb, aam = A("u"), A("v"), A("ub"), A("vb"), A("aam")

    def sh(a, di, dj):                                       # a(i+di, j+dj), zero outside the grid
        out = np.zeros_like(a)
        ys, yd = (slice(dj, None), slice(0, -dj or None)) if dj >= 0 else (slice(0, dj), slice(-dj, None))
        xs, xd = (slice(di, None), slice(0, -di or None)) if di >= 0 else (slice(0, di), slice(-di, None))
        out[..., yd, xd] = a[..., ys, xs]
        return out
    dt4 = dt + sh(dt, -1, 0) + sh(dt, 0, -1) + sh(dt, -1, -1)
    dx4 = dx + sh(dx, -1, 0) + sh(dx, 0, -1) + sh(dx, -1, -1)
    dy4 = dy + sh(dy, -1, 0) + sh(dy, 0, -1) + sh(dy, -1, -1)
    aam4 = aam + sh(aam, -1, 0) + sh(aam, 0, -1) + sh(aam, -1, -1)
    dtaam = .25 * dt4 * aam4
    with np.errstate(divide="ignore", invalid="ignore"):
        cross = dtaam * ((ub + sh(ub, 0, -1)) / dy4 + (vb + sh(vb, -1, 0)) / dx4)
        curv = .25 * ((sh(v, 0, 1) + v) * np.abs(sh(dy, 1, 0) - sh(dy, -1, 0)) + (sh(u, 1, 0) + u) * np.abs(sh(dx, 0, 1) - sh(dx, 0, -1))) / (dx * dy)
        xfx = dy * (.125 * ((sh(dt, 1, 0) + dt) * sh(u, 1, 0) + (dt + sh(dt, -1, 0)) * u) * (sh(u, 1, 0) + u) + dt * aam * 2. * (sh(ub, 1, 0) + ub) / dx)
        yfx = .25 * dx4 * (.125 * ((dt + sh(dt, 0, -1)) * v + (sh(dt, -1, 0) + sh(dt, -1, -1)) * sh(v, -1, 0)) * (u + sh(u, 0, -1)) + cross)
        sx = xfx + sh(xfx, -1, 0) + sh(yfx, 0, 1) + yfx + aru * .25 * (curv * dt * (sh(v, 0, 1) + v) + sh(curv * dt * (sh(v, 0, 1) + v), -1, 0))
        xfy = .25 * dy4 * (.125 * ((dt + sh(dt, -1, 0)) * u + (sh(dt, 0, -1) + sh(dt, -1, -1)) * sh(u, 0, -1)) * (v + sh(v, -1, 0)) + cross)
        yfy = dx * (.125 * ((sh(dt, 0, 1) + dt) * sh(v, 0, 1) + (dt + sh(dt, 0, -1)) * v) * (sh(v, 0, 1) + v) + dt * aam * 2. * (sh(vb, 0, 1) + vb) / dy)
        sy = sh(xfy, 1, 0) + xfy + yfy + sh(yfy, 0, -1) + arv * .25 * (curv * dt * (sh(u, 1, 0) + u) + sh(curv * dt * (sh(u, 1, 0) + u), 0, -1))
    return np.nan_to_num(sx, posinf=0.0), np.nan_to_num(sy, posinf=0.0)


MEASURED = {}                                                 # largest per-cell measures of this session, printed with -s


def _note(key, value):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(value))
    print(f"{key}: {value:.3g}")


def check_fp32_kernel(name, a0, o, s, t, noise=False, tag=""):
    """(c) for one fp32 routine: the arithmetic variant t against the reference fp32(oracle o), the storage variant s naming the
    arrays the routine's fp32 kernel writes (everything else must be s's bits)"""
    out = {"advt2": ("vf",), "advq": ("uf",), "advct": ("advx", "advy"), "lateral_viscosity": ("advx", "advy")}[name]
    assert not identical_arrays(s, t, skip=out), (name, identical_arrays(s, t, skip=out))
    for n in out:
        ref, got = o.field(n), t.field(n)
        assert np.isfinite(f32(got)).all(), n
        if name in ("advct", "lateral_viscosity"):
            S = advct_scale(a0)[0 if n == "advx" else 1]
            err = np.abs(f32(got).astype(np.float64) - f32(ref).astype(np.float64))
            with np.errstate(divide="ignore", invalid="ignore"):
                c = np.where(err > ulp32(ref), (err - ulp32(ref)) / (U32 * S), 0.0)
            assert np.isfinite(c).all(), (n, "an error where the condition scale is 0")
            _note(f"{tag}{name}/{n} C", c.max())
            assert c.max() <= ADVCT_C, (n, float(c.max()), np.unravel_index(int(np.argmax(c)), c.shape))
            # where advct computes nothing (outside 2..imm1 x 2..jmm1 and level kb), it writes the oracle's zeros
            fixed = fixed_cells(a0) & ~(a0.fsm[:a0.jm, :a0.im] == 0)[None]
            assert np.array_equal(bits32(got)[fixed], bits32(ref)[fixed]), n
        else:
            d, bound = (level_ulps(got, ref), NOISE_LEVEL_ULPS[name]) if noise else (ulps(got, ref), CELL_ULPS[name])
            _note(f"{tag}{name}/{n} {'level ' if noise else ''}ulps", d.max())
            assert d.max() <= bound, (n, float(d.max()), np.unravel_index(int(np.argmax(d)), d.shape))
            assert same_zeros(got, ref), n
            fixed = fixed_cells(a0)
            assert np.array_equal(bits32(got)[fixed], bits32(ref)[fixed]), (n, int((bits32(got)[fixed] != bits32(ref)[fixed]).sum()))


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _routine_id(r):
    return f"{r[0]}{''.join(map(str, r[2]))}"


def _cases():
    out = []
    for cfg in SHAPES:
        for r in ROUTINES:
            out += [(cfg, r, "storage"), (cfg, r, "arith")]
    for cfg in BRANCHES:
        for r in ROUTINES:
            if r[0] in BRANCH_ROUTINES[cfg]:
                out += [(cfg, r, "storage"), (cfg, r, "arith")]
    for cfg in NOISE:
        for r in ROUTINES:
            if r[0] in NOISE_ROUTINES:
                out += [(cfg, r, "storage"), (cfg, r, "arith")]
    return [c for c in out if not (c[1][0] == "mode_internal" and c[2] == "arith")]   # (d) covers it


@pytest.mark.parametrize("cfg,routine,variant", _cases(), ids=[f"{c}-{_routine_id(r)}-{v}" for c, r, v in _cases()])
def test_variant_routine_against_the_oracle(cfg, routine, variant):
    """(a) storage: fp32(oracle) bit for bit but the pairs of EXEMPT (bounded); (b) arithmetic outside the fp32 kernels: the
    storage variant's bits; (c) arithmetic in advt2 (nitera = 1), advq, advct, lateral_viscosity: per cell within their bounds"""
    name, fields, ints = routine
    o, s, t = _runs(cfg, name, fields, ints)
    check_routine(cfg, name, variant, o, s, t)


def check_routine(cfg, name, variant, o, s, t, tag=""):
    if variant == "storage":
        bad = storage_mismatches(o, s, name, cfg)
        assert not bad, f"{name}: (array, cells, largest ulps) {bad}"
        return
    fp32_kernel = name in ("advct", "advq", "lateral_viscosity") or (name == "advt2" and _nitera(cfg) == 1)
    if not fp32_kernel:
        assert not identical_arrays(s, t), f"{name}: {identical_arrays(s, t)}"
        return
    check_fp32_kernel(name, _warm(cfg), o, s, t, noise=cfg in NOISE, tag=tag)


# ---- (d) the fp32 kernels of the step path -------------------------------------------------------------------------------------
STEP_CFGS = ["island", "seamount", "even66x50", "island128x12", "kb50", "nadv1", "npg2", "island+noise"]
# k_advuv_col + k_profuv_reg against k_advu_profu / k_advv_profv (POMGPU_THOMAS_SCRATCH) after the whole mode_internal.  Not the
# same bits even in fp32 storage: the scratch path keeps the solves' work vectors in 3-D scratch arrays (fp32 there), the register
# kernels in registers.  Per cell, in fp32 ulps of the level's largest |value| (3-D) or u32 of the array's largest |value| (2-D),
# 2x the largest measured (SHAPES, STEP_CFGS and GPU_SHAPES); an array not named here must keep its bits.  The velocity forecast is a sum of tendencies of either
# sign, so per cell it may cancel: the level's scale, not the cell's value.
UV_STORAGE = {"uf": 12, "u": 12, "vf": 5, "v": 5, "ub": 2, "vb": 2, "wr": 4, "wubot": 1.5, "wvbot": 1.8}
UV_ARITH = {"uf": 16, "u": 16, "vf": 29, "v": 29, "ub": 2, "vb": 2, "wr": 16, "wubot": 12, "wvbot": 49}


def _mode_internal(lib, st, switches=()):
    return run_routine(lib, st, "mode_internal", switches=switches)


def _map(fn, args, pool):
    return [q.result() for q in [pool.submit(fn, *a) for a in args]] if pool else [fn(*a) for a in args]


@pytest.mark.parametrize("cfg", STEP_CFGS)
def test_paired_tracer_and_turbulence_kernels_match_the_single_ones(cfg):
    """fp32 arithmetic: k_advt2x2_col and k_advq2_col (the default mode_internal) give the bits of k_advt2_col and k_advq_col
    run one array at a time (POMGPU_ADVT2_SINGLE, POMGPU_ADVQ_SINGLE)"""
    check_paired_kernels(cfg, EMU_F32A, _POOL)


def check_paired_kernels(cfg, lib_a, pool=None):
    a0 = _warm(cfg)
    x, y = _map(_mode_internal, [(lib_a, a0, sw) for sw in ((), ("POMGPU_ADVT2_SINGLE", "POMGPU_ADVQ_SINGLE"))], pool)
    assert not identical_arrays(x, y), identical_arrays(x, y)


@pytest.mark.parametrize("cfg", STEP_CFGS)
def test_advuv_col_against_the_fp64_velocity_kernels(cfg):
    """k_advuv_col (default mode_internal, kb <= 64) against POMGPU_THOMAS_SCRATCH (the fp64 k_advu_profu, k_advv_profv), in
    fp32 storage and in fp32 arithmetic: every array within UV_STORAGE / UV_ARITH, land cells exact"""
    check_advuv(cfg, EMU_F32, EMU_F32A, _POOL)


def check_advuv(cfg, lib_s, lib_a, pool=None, tag=""):
    a0 = _warm(cfg)
    runs = [(lib, a0, sw) for lib in (lib_s, lib_a) for sw in ((), ("POMGPU_THOMAS_SCRATCH",))]
    s_def, s_ts, t_def, t_ts = _map(_mode_internal, runs, pool)
    land = np.broadcast_to(a0.fsm[:a0.jm, :a0.im] == 0, (a0.kb, a0.jm, a0.im))
    for var, got, ref, bound in (("storage", s_def, s_ts, UV_STORAGE), ("arith", t_def, t_ts, UV_ARITH)):
        diff = identical_arrays(got, ref)
        assert set(diff) <= set(bound), (var, diff)
        for n in diff:
            if n in BLK3D:
                d = level_ulps(got.field(n), ref.field(n)).max()
                assert np.array_equal(bits32(got.field(n))[land], bits32(ref.field(n))[land]), (var, n)
            else:
                d = rel_u32(got.field(n), ref.field(n))
            _note(f"{tag}advuv_col {var}/{n}", d)
            assert d <= bound[n], (var, n, float(d))


@pytest.mark.parametrize("cfg", STEP_CFGS)
def test_ts_update_density_is_the_oracles_dens_of_the_variants_own_t_and_s(cfg):
    """k_ts_update keeps dens_point in fp64 on the fp32 t, s it stores: rho(1..kbm1) after the fp32-arithmetic mode_internal is
    fp32 of the oracle's dens applied to that t and s, bit for bit (independent of the fp32 rounding of everything else)"""
    check_ts_update(cfg, EMU_F32A)


def check_ts_update(cfg, lib_a):
    t = _mode_internal(lib_a, _warm(cfg))
    d = run_routine(None, t, "dens", ("s", "t", "rho"))
    kbm1, jm, im = t.kb - 1, t.jm, t.im
    got, ref = t.field("rho")[:kbm1, :jm, :im], d.field("rho")[:kbm1, :jm, :im]
    assert np.array_equal(bits32(got), bits32(ref)), int((bits32(got) != bits32(ref)).sum())
    assert not np.array_equal(t.field("rho"), _warm(cfg).field("rho"))          # the step did write rho
