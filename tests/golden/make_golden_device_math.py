"""Regenerate tests/golden/device_math_rad_q.npz: seeded arguments of proft's short-wave term and, for each, the 64-bit pattern the
reference's expression has when it is formed in REAL(16) and rounded once,

    real( swrad * ( r*exp(real(x1,16)) + (1.d0-r)*exp(real(x2,16)) ), 8 )        (tools/check_dd_exp.cpp forms it the same way)

evaluated by a small g++ / libquadmath helper that this script writes and builds in a temporary directory.  The helper also runs the
HOST build of proft_rad_q (extpom_amd/csrc/dd_exp.h) on the same arguments: a fixture is written only if the two agree everywhere, so
what the device is held to is what the header computes where libm is the host's.  The tests that read the file need no compiler.

    python tests/golden/make_golden_device_math.py

Stored: `in` (n, 3) = swrad, x1, x2; `ntp` (n) the Jerlov type that gives r and omr = 1 - r; `fam` (n) the family; `bits` (n) the
expected pattern (0 in the family PLAIN, which is held to the plain fp64 formula instead).  |swrad| is in [1e-6, 1] throughout."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "device_math_rad_q.npz")
SEED = 20261019
R = np.array([.58, .62, .67, .77, .78])                      # Jerlov types (initialize.f), as tools/check_dd_exp.cpp lists them
AD1 = np.array([.35, .60, 1.0, 1.5, 1.4])
AD2 = np.array([23., 20., 17., 14., 7.9])
LN2 = 0.6931471805599453
FAMILIES = ["SUBNORMAL", "X1_AT_CUT", "X1_EQ_X2", "TINY", "ZERO_TO_700", "LAST_SUBNORMALS", "JERLOV", "X1_DEAD", "X2_DEAD", "BOTH_DEAD",
            "GAPS", "NAN_X1", "PLAIN"]
FAM = {n: k for k, n in enumerate(FAMILIES)}
N_MAIN = 4096                                                 # each of the first six families

HELPER = r"""
#include <quadmath.h>
#include <stdio.h>
#include <stdlib.h>
#include "dd_exp.h"
int main(int argc, char **argv) {
  FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  double a[5], o[2];
  while (fread(a, sizeof(double), 5, fi) == 5) {               // swrad, r, omr, x1, x2
    const __float128 q = (__float128)a[0] * ((__float128)a[1] * expq((__float128)a[3]) + (__float128)a[2] * expq((__float128)a[4]));
    o[0] = (double)q;
    o[1] = proft_rad_q(a[0], a[1], a[2], a[3], a[4]);
    if (fwrite(o, sizeof(double), 2, fo) != 2) return 3;
  }
  return fclose(fo) ? 4 : 0;
}
"""


def have_compiler():
    return shutil.which("g++") is not None


def inputs():
    """(in (n, 3), ntp (n), fam (n)): the same arrays on every call"""
    g = np.random.default_rng(SEED)
    sw, x1, x2, fam = [], [], [], []

    def swrad(n):                                             # mostly downward (negative, as the model's), |swrad| log-uniform in [1e-6, 1]
        return np.where(g.random(n) < .125, 1., -1.) * 10. ** (-6. * g.random(n))

    def add(name, a, b, s=None):
        sw.append(swrad(a.size) if s is None else s)
        x1.append(a)
        x2.append(b)
        fam.append(np.full(a.size, FAM[name], np.uint8))

    n = N_MAIN
    # results in the subnormal band: the second term alone, with x1 = 20 x2, with a first term that still counts
    b = -760. + 70. * g.random(n)
    a = np.where(np.arange(n) % 3 == 0, -2.e4, np.where(np.arange(n) % 3 == 1, 20. * b, b - 40. * g.random(n)))
    add("SUBNORMAL", a, b)
    a = -11400. + 10. * (g.random(n) - .5)
    a[:8] = [-11400., np.nextafter(-11400., 0.), np.nextafter(-11400., -1e5), -11399.5, -11400.5, -11395., -11405., -11400.]
    add("X1_AT_CUT", a, -700. * g.random(n))
    a = -700. * g.random(n)
    add("X1_EQ_X2", a, a.copy())
    a = np.where(g.random(n) < .5, 1., -1.) * 10. ** (-10. - 20. * g.random(n))
    b = np.where(g.random(n) < .5, 1., -1.) * 10. ** (-10. - 20. * g.random(n))
    a[:6] = [0., -0., 5e-324, -5e-324, 1e-310, -1e-310]
    b[:6] = [0., 0., -5e-324, 0., -1e-310, 1e-10]
    add("TINY", a, b)
    a, b = 700. * g.random(n), 700. * g.random(n)
    a[:4] = [0., 700., 700., 0.]
    b[:4] = [0., 700., 0., 700.]
    add("ZERO_TO_700", a, b)
    b = -745.2 + 1.2 * g.random(n)
    add("LAST_SUBNORMALS", 20. * b, b, -np.ones(n))
    # the Jerlov families of tools/check_dd_exp.cpp: x = z * dh / ad
    n = 1024
    t = g.integers(0, 5, n)
    zdh = -g.random(n) * (5. + g.random(n) * np.where(np.arange(n) % 3 == 0, 60., 6000.))
    jer = (zdh / AD1[t], zdh / AD2[t], -(1e-6 + g.random(n) * 3e-4), t)
    n = 512
    add("X1_DEAD", -11400. - 10. ** (-3. + 7. * g.random(n)), -740. * g.random(n))
    add("X2_DEAD", -740. * g.random(n), -11400. - 10. ** (-3. + 7. * g.random(n)))
    n = 256
    add("BOTH_DEAD", -11400. - 10. ** (-3. + 7. * g.random(n)), -11400. - 10. ** (-3. + 7. * g.random(n)))
    # exponent gaps k1 - k2 (k = nearbyint(x / ln 2)): on both sides of the cut at -240, and where the smaller term still reaches
    # the double (a cut misplaced towards 0 changes results there)
    n = 512
    for lo, hi in ((-243., -237.), (-56., -38.), (-112., -56.)):
        hiarg = -50. * g.random(n)
        loarg = hiarg + (lo + (hi - lo) * g.random(n)) * LN2
        swap = np.arange(n) % 2 == 0
        add("GAPS", np.where(swap, hiarg, loarg), np.where(swap, loarg, hiarg))
    n = 64
    add("NAN_X1", np.full(n, np.nan), -100. * g.random(n))
    # one argument above 700: the plain fp64 formula
    n = 256
    big, other = 700. + 9. * (1. - g.random(n)), -50. + 750. * g.random(n)
    swap = np.arange(n) % 2 == 0
    add("PLAIN", np.where(swap, big, other), np.where(swap, other, big))

    ntp = [g.integers(0, 5, a.size).astype(np.uint8) for a in x1]
    k = FAM["JERLOV"]                                         # in the order of FAMILIES
    sw.insert(k, jer[2]); x1.insert(k, jer[0]); x2.insert(k, jer[1]); ntp.insert(k, jer[3].astype(np.uint8))
    fam.insert(k, np.full(jer[0].size, k, np.uint8))
    arr = np.stack([np.concatenate(sw), np.concatenate(x1), np.concatenate(x2)], axis=1)
    assert np.all((np.abs(arr[:, 0]) >= 1e-6) & (np.abs(arr[:, 0]) <= 1.))
    return np.ascontiguousarray(arr), np.concatenate(ntp), np.concatenate(fam)


def operands(arr, ntp):
    """the five arguments of proft_rad_q: swrad, r, omr = 1 - r in fp64 (as the kernels pass it), x1, x2"""
    r = R[ntp]
    return arr[:, 0].copy(), r, 1. - r, arr[:, 1].copy(), arr[:, 2].copy()


def evaluate(arr, ntp):
    """(quad result rounded once, host proft_rad_q) through the helper"""
    tmp = tempfile.mkdtemp(prefix="device_math_")
    try:
        with open(os.path.join(tmp, "helper.cpp"), "w") as fh:
            fh.write(HELPER)
        exe = os.path.join(tmp, "helper")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "extpom_amd", "csrc"), "-o", exe,
                               os.path.join(tmp, "helper.cpp"), "-lquadmath"])
        np.stack(operands(arr, ntp), axis=1).tofile(os.path.join(tmp, "in.bin"))
        subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")])
        out = np.fromfile(os.path.join(tmp, "out.bin")).reshape(-1, 2)
        assert out.shape[0] == arr.shape[0]
        return out[:, 0].copy(), out[:, 1].copy()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def generate():
    arr, ntp, fam = inputs()
    quad, host = evaluate(arr, ntp)
    exact = fam != FAM["PLAIN"]
    nan = np.isnan(quad)
    bad = exact & ((np.isnan(host) != nan) | (~nan & (host.view(np.uint64) != quad.view(np.uint64))))
    if bad.any():
        k = np.flatnonzero(bad)
        raise SystemExit(f"the host proft_rad_q differs from the REAL(16) evaluation at {k.size} points, first {arr[k[0]]} family "
                         f"{FAMILIES[fam[k[0]]]}: {host[k[0]]!r} against {quad[k[0]]!r} -- no fixture for a header that is not the reference")
    bits = np.where(exact, quad.view(np.uint64), np.uint64(0))
    return {"in": arr, "ntp": ntp, "fam": fam, "bits": bits}


def main():
    d = generate()
    np.savez_compressed(PATH, **d)
    print(f"wrote {PATH}: {d['fam'].size} points, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
