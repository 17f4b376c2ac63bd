"""The fp32-arithmetic variant (libpomgpu_f32a.so: -DPOMGPU_STORE_F32 -DPOMGPU_COMPUTE_F32, pomgpu_internal.hpp) without a GPU:
its device code really computes the stencil kernels in fp32 and stays within the fp32-storage build's registers, it exports the
C ABI, and its kernel logic -- compiled for the host like tests/emu does for the product -- runs the seamount within a stated
envelope of the fp64 oracle, on one tile and on 2 x 1 tiles."""
import concurrent.futures
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from extpom_amd.cases import make_case
from extpom_amd.layout import PROGNOSTIC
from extpom_amd.model import PomGpu
from oracle.pyoracle import OracleTile, oracle_finish_initial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "extpom_amd", "csrc")
EMU_F32A = os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")
STORE = ["-DPOMGPU_STORE_F32"]
ARITH = ["-DPOMGPU_STORE_F32", "-DPOMGPU_COMPUTE_F32"]
# fp64 arithmetic the ISA test counts: the VALU operations of the expressions (conversions and moves are not arithmetic)
F64_OP = re.compile(r"^\s+v_(?:fma|mul|add|div_scale|div_fmas|div_fixup|rcp|max|min)_f64\b")
# the emulated variant against the fp64 oracle, seamount 65x49x21: largest |difference| relative to the field's largest magnitude.
# Measured after 20 internal steps: el 1.3e-4, et 1.3e-4, ua 7.1e-6, va 2.1e-5, u 4.1e-3, v 1.1e-3, t 9.6e-6, s 1.6e-6 (x ~4 below).
ENVELOPE = {"el": 5e-4, "et": 5e-4, "ua": 3e-5, "va": 1e-4, "u": 2e-2, "v": 5e-3, "t": 4e-5, "s": 1e-5}


def _asm(src, defines, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + CSRC, "--cuda-device-only", "-S"] + defines + [os.path.join(CSRC, src), "-o", out])
    return open(out).read()


def kernel_stats(asm):
    """{mangled kernel name: (fp64 arithmetic instructions, VGPRs)}"""
    f64, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            f64[cur] = 0
        elif cur and F64_OP.match(line):
            f64[cur] += 1
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        out[m.group(1)] = (f64.get(m.group(1), 0), int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1)))
    return out


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa")
    jobs = {(src, tag): (src, defs, str(d / f"{src}.{tag}.s")) for src in ("k_tile.hip", "k_adv.hip") for tag, defs in (("store", STORE), ("arith", ARITH))}
    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        futs = {k: ex.submit(_asm, *v) for k, v in jobs.items()}
        return {k: kernel_stats(f.result()) for k, f in futs.items()}


def _pick(stats, name):
    ks = {k: v for k, v in stats.items() if re.search(r"\d" + name + r"(I|\d|2KP)", k)}
    assert ks, name
    return ks


def test_variant_stencil_kernels_compute_in_fp32(isa):
    """no fp64 arithmetic left in the tracer, turbulence and velocity stencils; advct keeps only its fp64 vertical sums; k_ts_update
    keeps only dens_point (k_dens of the same build is dens_point alone); and no kernel needs more registers than in fp32 storage"""
    tile, adv = isa[("k_tile.hip", "arith")], isa[("k_adv.hip", "arith")]
    tile_s, adv_s = isa[("k_tile.hip", "store")], isa[("k_adv.hip", "store")]
    for name in ("k_advt2_col", "k_advq_col", "k_advuv_col"):
        ks = _pick(tile, name)
        assert len(ks) >= (1 if name == "k_advuv_col" else 2)
        for k, (n, _) in ks.items():
            assert n == 0, (k, n)
    ks = _pick(tile, "k_advct_col")
    assert len(ks) == 2
    for k, (n, _) in ks.items():
        assert n <= 40, (k, n)
    dens = _pick(adv, "k_dens")
    (n_dens, _), = dens.values()
    assert n_dens > 50                                      # the glibc pow clone and the UNESCO polynomial: really fp64
    ks = _pick(adv, "k_ts_update")
    assert len(ks) == 2
    for k, (n, _) in ks.items():
        assert n <= n_dens + 10, (k, n, n_dens)
    # the storage-only build of the same kernels still computes in fp64 (what makes the counts above a change)
    for k, (n, _) in _pick(tile_s, "k_advt2_col").items():
        assert n > 300, (k, n)
    for stats, stats_s, names in ((tile, tile_s, ("k_advt2_col", "k_advq_col", "k_advuv_col", "k_advct_col")), (adv, adv_s, ("k_ts_update",))):
        for name in names:
            for k, (_, v) in _pick(stats, name).items():
                assert v <= stats_s[k][1], (k, v, stats_s[k][1])


def test_variant_library_exports_the_c_abi():
    import __graft_entry__ as ge
    lib = ctypes.CDLL(ge.build_hip(f32a=True))
    hdr = open(os.path.join(ROOT, "include", "pomgpu.h")).read()
    declared = sorted(set(re.findall(r"\b(pomgpu_[a-z0-9_]+)\s*\(", hdr)) - {"pomgpu_exchange_fn"})
    assert len(declared) >= 45
    for name in declared:
        assert hasattr(lib, name), f"{name} missing from libpomgpu_f32a.so"
    lib.pomgpu_version.restype = lib.pomgpu_build_id.restype = ctypes.c_char_p
    assert b"fp32-arithmetic" in lib.pomgpu_version() and b"fp32-storage" in lib.pomgpu_version()
    assert lib.pomgpu_build_id().endswith(b"-f32a")
    from extpom_amd import lib as binding
    assert binding.LIBPATH_F32A == os.path.join(CSRC, "libpomgpu_f32a.so")


@pytest.fixture(scope="module")
def emu_f32a():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh")], stdout=subprocess.DEVNULL)
    return EMU_F32A


def _rel(x, y, scale):
    return float(np.abs(x - y).max() / max(float(np.abs(scale).max()), 1e-300))


def test_emulated_variant_runs_the_seamount_within_its_envelope(emu_f32a):
    """20 internal steps (600 external) of the 65x49x21 seamount: no error, every value finite, every prognostic field within
    ENVELOPE of the fp64 oracle -- and not equal to it (the arithmetic really is another)"""
    a = make_case("seamount", 65, 49, 21, dte=6.0, isplit=30)
    oracle_finish_initial(a)
    b = a.copy()
    ot, g = OracleTile(a), PomGpu(b, libpath=emu_f32a)
    assert b"fp32-arithmetic" in g.L.pomgpu_version()
    done = 0
    for n in (2, 20):
        ot.run(n - done); g.run(n - done); done = n
        g.download()
        assert b.error_status == 0 and b.iint == n
        r = {f: _rel(a.field(f), b.field(f), a.field(f)) for f in PROGNOSTIC}
        assert all(np.isfinite(b.field(f)).all() for f in PROGNOSTIC)
        assert all(r[f] <= ENVELOPE[f] for f in PROGNOSTIC), (n, r)
        assert r["t"] > 1e-8 and r["u"] > 1e-8, r
    g.close()


def test_emulated_variant_on_tiles_stays_within_its_single_tile_envelope(emu_f32a, monkeypatch):
    """2 x 1 tiles of the variant under the library's exchange and the wide-halo external mode (halos travel as doubles), against
    the variant's own single tile: the message rounds happen and every owned cell stays within ENVELOPE of it"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_kernels_emulated_tiles as T
    monkeypatch.setattr(T, "EMU", emu_f32a)
    steps = 6
    out = T.run_tiles(2, 1, {}, library_exchange=True, wide=True, grid=T.WIDE_GRID, isplit=T.WIDE_ISPLIT, case="seamount", steps=steps)
    IMg, JMg = T.WIDE_GRID
    one = make_case("seamount", IMg, JMg, T.KB, dte=6.0, isplit=T.WIDE_ISPLIT)
    oracle_finish_initial(one)
    g = PomGpu(one, libpath=emu_f32a)
    g.run(steps); g.download(); g.close()
    assert len(out) == 2
    for r, (tile, st, rounds) in out.items():
        assert rounds >= steps and st.error_status == 0, (r, rounds, st.error_status)
        io, jo, im, jm = tile.i_off, tile.j_off, tile.im, tile.jm
        sl_j = slice(0 if jo == 0 else 1, jm if jo + jm == JMg else jm - 1)
        sl_i = slice(0 if io == 0 else 1, im if io + im == IMg else im - 1)
        for f in PROGNOSTIC:
            ref = one.field(f)[..., jo:jo + jm, io:io + im][..., sl_j, sl_i]
            got = st.field(f)[..., :jm, :im][..., sl_j, sl_i]
            assert np.isfinite(got).all(), (r, f)
            assert _rel(ref, got, one.field(f)) <= ENVELOPE[f], (r, f, _rel(ref, got, one.field(f)))
