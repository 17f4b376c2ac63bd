"""tests/test_fp32_variants_per_routine.py on an MI355X: the same assertions against libpomgpu_f32.so and libpomgpu_f32a.so, whose
device code differs from the host build of the same sources (DPP lane shifts, LDS row slabs, k_profq's elimination vectors in LDS,
divi's fp32 quotient), at 65x49x21 and at 256x192x50 (the bench's level count).  The storage variant must give fp32(oracle) bit
for bit but the pairs of EXEMPT, the arithmetic variant must stay within the per-cell bounds measured on the host.  The largest
per-cell measures and the largest difference from the emulated variants (65x49x21) are printed (run with -s).

Each grid's checks run in a child process of their own (this file as a script: `python <this file> <grid> routines|step`) under a
time limit, so a device that hangs ends the test instead of the session."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import test_fp32_variants_per_routine as T  # noqa: E402

GRIDS = list(T.GPU_SHAPES)
CHILD_TIMEOUT = 240                                            # seconds per grid and part (measured: ~20)
OK = "FP32-PER-ROUTINE-OK"


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as ge
    ge.build_hip(f32=True)
    ge.build_hip(f32a=True)
    for v in ("f32", "f32a"):
        subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), v], stdout=subprocess.DEVNULL)


def _child(cfg, part):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), cfg, part], capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0 and OK in r.stdout, (r.returncode, r.stdout[-3000:] + r.stderr[-3000:])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", GRIDS)
def test_gpu_variant_routines_against_the_oracle(libs, cfg):
    """every routine of ROUTINES: (a) the storage variant, (b) / (c) the arithmetic variant, as on the host"""
    _child(cfg, "routines")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", GRIDS)
def test_gpu_step_path_fp32_kernels(libs, cfg):
    """(d) on the device: the paired tracer / turbulence kernels against the single ones, k_advuv_col against the fp64 velocity
    kernels, and k_ts_update's rho against the oracle's dens of the variant's own t, s"""
    _child(cfg, "step")


# ---- the child ------------------------------------------------------------------------------------------------------------------
def _emu_level_ulps(cfg, name, fields, ints, s, t):
    """largest per-cell distance between the device and the host build of each variant, in fp32 ulps of the largest |value| of the
    cell's level (in ulps of the cell's own value a cancelling advct result differs by ~5e5 while both stay within its bound)"""
    out = {}
    for tag, lib, dev in (("storage", T.EMU_F32, s), ("arith", T.EMU_F32A, t)):
        e = T.run_routine(lib, T._warm(cfg), name, fields, ints)
        out[tag] = max((float(T.level_ulps(dev.field(n), e.field(n)).max()) for n in T.arrays3()), default=0.0)
    return out


def routines(cfg):
    from extpom_amd.lib import LIBPATH_F32, LIBPATH_F32A
    from test_kernels_emulated import ROUTINES
    fails, emu = [], {}
    for name, fields, ints in ROUTINES:
        a0 = T._warm(cfg)
        o = T.run_routine(None, a0, name, fields, ints)
        s = T.run_routine(LIBPATH_F32, a0, name, fields, ints)
        t = T.run_routine(LIBPATH_F32A, a0, name, fields, ints)
        if cfg == "gpu_island":
            emu[name + "".join(map(str, ints))] = _emu_level_ulps(cfg, name, fields, ints, s, t)
        for variant in ("storage", "arith"):
            if name == "mode_internal" and variant == "arith":
                continue
            try:
                T.check_routine(cfg, name, variant, o, s, t, tag=f"{cfg} ")
            except AssertionError as e:
                fails.append(f"{name}{''.join(map(str, ints))} {variant}: {str(e)[:300]}")
    for r, d in emu.items():
        if d["storage"] or d["arith"]:
            print(f"{cfg} {r}: device - emulated, largest level ulps: storage {d['storage']:.3g}, arith {d['arith']:.3g}")
    if emu:
        print(f"{cfg} largest device - emulated level ulps over all routines: storage {max(d['storage'] for d in emu.values()):.3g}, "
              f"arith {max(d['arith'] for d in emu.values()):.3g}")
    assert not fails, "\n".join(fails)


def step(cfg):
    from extpom_amd.lib import LIBPATH_F32, LIBPATH_F32A
    T.check_paired_kernels(cfg, LIBPATH_F32A)
    T.check_advuv(cfg, LIBPATH_F32, LIBPATH_F32A, tag=f"{cfg} ")
    T.check_ts_update(cfg, LIBPATH_F32A)


if __name__ == "__main__":
    grid, part = sys.argv[1], sys.argv[2]
    {"routines": routines, "step": step}[part](grid)
    print(OK, grid, part)
