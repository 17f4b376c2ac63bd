"""The fp32-arithmetic variant (libpomgpu_f32a.so, pomgpu_internal.hpp) on an MI355X: the fp64 product, the fp32-storage variant
and the fp32-arithmetic variant from one state; the arithmetic variant's drift from fp64 stays within bounds measured with
tools/fp32_arith_study_gpu.py (profiles/fp32_arith_drift_*.json), x ~4.  Like the storage variant it is NOT a parity path: the
flow amplifies rounding-level differences."""
import os
import subprocess
import sys

import numpy as np
import pytest

from extpom_amd.cases import make_case
from extpom_amd.layout import PROGNOSTIC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b, f):
    x, y = a.field(f), b.field(f)
    return float(np.abs(x - y).max() / max(float(np.abs(x).max()), 1e-300))


# seamount 256x192x50, largest |fp32-arith - fp64| relative to the field's largest magnitude, measured (MI355X):
#   step 2:  el 5.1e-10, et 5.3e-10, ua 1.1e-9, va 1.1e-8, u 4.7e-7, v 2.2e-6, t 4.6e-7, s 9.8e-7
#   step 10: el 3.2e-5, et 3.1e-5, ua 1.9e-6, va 8.8e-6, u 1.5e-3, v 5.5e-4, t 4.5e-6, s 3.7e-6
# (the storage variant after 10 steps: el 2.6e-6, u 4.3e-4, t 1.7e-6, s 3.4e-6)
BOUND = {2: {"el": 2e-9, "et": 2e-9, "ua": 4e-9, "va": 4e-8, "u": 2e-6, "v": 9e-6, "t": 2e-6, "s": 4e-6},
         10: {"el": 1.3e-4, "et": 1.3e-4, "ua": 8e-6, "va": 3.5e-5, "u": 6e-3, "v": 2.2e-3, "t": 1.8e-5, "s": 1.5e-5}}


def test_fp32_arith_variant_drift_at_256x192x50():
    """the three builds from one state of the 256x192x50 seamount; after 2 internal steps (step 1 skips the 3-D body, advance.f:362)
    and 10 the arithmetic variant's drift from fp64 stays within BOUND, T and S within 1e-4 after 10; it really is another run
    (it differs from fp64 and from the storage variant)"""
    from extpom_amd import lib as L
    from extpom_amd.model import PomGpu, gpu_finish_initial
    a = make_case("seamount", 256, 192, 50, dte=6.0, isplit=30)
    gpu_finish_initial(a, device=0)
    b, c = a.copy(), a.copy()
    g64, g32, g32a = PomGpu(a, device=0), PomGpu(b, device=0, libpath=L.LIBPATH_F32), PomGpu(c, device=0, libpath=L.LIBPATH_F32A)
    assert b"fp32-arithmetic" in g32a.L.pomgpu_version() and b"fp32-arithmetic" not in g32.L.pomgpu_version()
    done, seen = 0, {}
    for n in (2, 10):
        for g in (g64, g32, g32a):
            g.run(n - done)
        done = n
        for g in (g64, g32, g32a):
            g.download()
        assert a.error_status == b.error_status == c.error_status == 0
        r = {f: _rel(a, c, f) for f in PROGNOSTIC}
        seen[n] = r
        assert all(np.isfinite(c.field(f)).all() for f in PROGNOSTIC)
        assert all(r[f] <= BOUND[n][f] for f in PROGNOSTIC), (n, {f: (r[f], BOUND[n][f]) for f in PROGNOSTIC if r[f] > BOUND[n][f]})
        assert r["t"] > 0 and max(_rel(b, c, f) for f in PROGNOSTIC) > 0
    assert seen[10]["t"] <= 1e-4 and seen[10]["s"] <= 1e-4, seen[10]
    print("fp32-arith drift at 256x192x50:", {n: {f: float(f"{v:.2e}") for f, v in r.items()} for n, r in seen.items()})
    for g in (g64, g32, g32a):
        g.close()


# 2048x1536x50 basin (bench grid), 10 internal steps, measured: el 1.4e-2, et 1.4e-2, ua 6.1e-3, va 4.8e-2, u 5.1e-4, v 7.1e-3, t 1.5e-6,
# s 6.2e-7 (profiles/fp32_arith_drift_basin2048.json; the basin starts at rest: its flow IS the response to a 1e-3 K perturbation)
FULL_BOUND = {"el": 5.5e-2, "et": 5.5e-2, "ua": 2.5e-2, "va": 0.2, "u": 2e-3, "v": 3e-2, "t": 6e-6, "s": 2.5e-6}


def test_fp32_arith_variant_drift_on_the_configs_own_grid():
    """BASELINE configs[4]'s grid, fp64 and the fp32-arithmetic build from one state in one process (60 + 30 GB of the 288): after 10
    internal steps every prognostic field within FULL_BOUND of fp64, and T differs"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fp32_arith_study_gpu import BUILDS, full_size_drift
    d = full_size_drift([10], builds=(BUILDS[0], BUILDS[2]))
    r = d["steps"]["fp32-arith"]["10"]
    print("fp32-arith drift at 2048x1536x50 after 10 steps:", {f: float(f"{r[f]:.2e}") for f in PROGNOSTIC})
    assert r["error_status"] == [0, 0], r
    assert all(r[f] <= FULL_BOUND[f] for f in PROGNOSTIC), {f: (r[f], FULL_BOUND[f]) for f in PROGNOSTIC if r[f] > FULL_BOUND[f]}
    assert r["t"] > 1e-9, r


def test_fp32_arith_variant_on_tiles():
    """1 x 4 whole-row tiles of 256x192x50 in the fp32-arithmetic variant under the library's exchange and the wide-halo external mode
    (halos travel as doubles) against its own single tile, GPU against GPU: the message rounds complete and every field stays within
    the fp32 envelope of tests/gpu_tiles_threads.py (F32_BOUND)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tiles_threads_f32a.py"), "256x192x50", "4", "6", "f32"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "TILES-THREADS-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "message rounds per step and tile" in r.stdout
