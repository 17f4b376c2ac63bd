// k_float.hpp -- Lagrangian floats (include/pomgpu.h "Lagrangian floats"): the three kernels and their launchers, included by pomgpu_api.hip.
//
// One lane per float, 256 lanes a workgroup; the six arrays of the float state (x y sig: double, status kind id: int) are read and written
// coalesced, everything else is a gather: per stage 8 values of each of u, v, w (four corners on two levels), 8 of dx, 8 of dy and 4 of dt,
// 44 loads whose addresses are all formed before the first of them is used.  The two stages of the midpoint step depend on each other and
// nothing else does.  No lane talks to another: no LDS, no atomics.  Element offsets are 32-bit (an array has fewer than 2^32 elements).
// z and zz are read with a wave-uniform index (F1: scalar loads) in a loop over the levels; the level of a lane is a select in that loop.
// Every coordinate is limited before it becomes an integer and every index after the fractions are formed, so whatever a position or a
// velocity holds -- NaN, infinity, many cells a step -- the loads stay inside the arrays.  Lanes of floats that are not active return before
// their first gather.  The arithmetic is restated, operation by operation and in this association, by tests/float_expect.py.
#pragma once
#include "pomgpu.h"
#include "pomgpu_internal.hpp"

__device__ __forceinline__ double flt_L(double p, double q, double f) { return p + f * (q - p); }   // exact for p == q
__device__ __forceinline__ int flt_clampi(int a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : a); }
__device__ __forceinline__ bool flt_finite(double x) { return fabs(x) <= __DBL_MAX__; }             // false for NaN
// one axis of a field point's cell: the coordinate limited to [0, n + 1], its floor and fraction, the two indices limited to 1..n
__device__ __forceinline__ void flt_axis(double xs, int n, int &i0, int &i1, double &f) {
  xs = fmin(fmax(xs, 0.), (double)(n + 1));
  const double fl = floor(xs);
  f = xs - fl;
  const int a = (int)fl;
  i0 = flt_clampi(a, 1, n);
  i1 = flt_clampi(a + 1, 1, n);
}
// the containing cell along one axis, limited to 1..n
__device__ __forceinline__ int flt_cell(double x, int n) {
  const double xs = fmin(fmax(x + 0.5, 0.), (double)(n + 1));
  return flt_clampi((int)floor(xs), 1, n);
}
// u v t s live on zz: level 1 alone at or above zz(1), level kbm1 alone at or below zz(kbm1), else zz(k) >= sig > zz(k+1)
struct FltLev { int k, k2; double fz; bool alone; };
__device__ __forceinline__ FltLev flt_levels_zz(const KP &P, double sig) {
  const int kbm1 = P.kbm1;
  const double top = F1(zz, 1), bot = F1(zz, kbm1);
  int k = 1;
  double zk = top, zk1 = F1(zz, 2);
  for (int kk = 2; kk <= kbm1 - 1; kk++) {                    // wave-uniform index: the last level that is not below sig
    const double a = F1(zz, kk), b = F1(zz, kk + 1);
    if (a >= sig) { k = kk; zk = a; zk1 = b; }
  }
  FltLev r;
  if (sig >= top) { r.k = r.k2 = 1; r.fz = 0.; r.alone = true; }
  else if (sig <= bot) { r.k = r.k2 = kbm1; r.fz = 0.; r.alone = true; }
  else { r.k = k; r.k2 = k + 1; r.fz = (zk - sig) / (zk - zk1); r.alone = false; }
  return r;
}
// w lives on z: the k in 1..kbm1 with z(k) >= sig > z(k+1); sig = 0 gives k = 1, fz = 0
__device__ __forceinline__ FltLev flt_levels_z(const KP &P, double sig) {
  int k = 1;
  double zk = F1(z, 1), zk1 = F1(z, 2);
  for (int kk = 2; kk <= P.kbm1; kk++) {
    const double a = F1(z, kk), b = F1(z, kk + 1);
    if (a >= sig) { k = kk; zk = a; zk1 = b; }
  }
  FltLev r;
  r.k = k; r.k2 = k + 1; r.fz = (zk - sig) / (zk - zk1); r.alone = false;
  return r;
}
// L in i, then in j
__device__ __forceinline__ double flt_bil(double a00, double a10, double a01, double a11, double fx, double fy) {
  return flt_L(flt_L(a00, a10, fx), flt_L(a01, a11, fx), fy);
}
// the velocity in index space at (x, y, sig): a = U / DXU, b = V / DYV, c = W / D
struct FltV { double a, b, c; };
__device__ __forceinline__ FltV flt_velocity(const KP &P, double x, double y, double sig) {
  const double *u = A3(u), *v = A3(v), *w = A3(w), *dx = A2(dx), *dy = A2(dy), *dt = A2(dt);
  // ---- addresses: u at (i - 0.5, j), v at (i, j - 0.5), w and dt at (i, j); the centre's cell shares v's i and u's j
  int ui0, ui1, vj0, vj1, ci0, ci1, cj0, cj1;
  double ufx, vfy, cfx, cfy;
  flt_axis(x + 0.5, P.im, ui0, ui1, ufx);
  flt_axis(y + 0.5, P.jm, vj0, vj1, vfy);
  flt_axis(x, P.im, ci0, ci1, cfx);
  flt_axis(y, P.jm, cj0, cj1, cfy);
  const unsigned iml = (unsigned)P.iml, n2 = (unsigned)P.n2;
  const unsigned ru0 = (unsigned)(cj0 - 1) * iml, ru1 = (unsigned)(cj1 - 1) * iml;   // rows of u's and the centre's cell
  const unsigned rv0 = (unsigned)(vj0 - 1) * iml, rv1 = (unsigned)(vj1 - 1) * iml;   // rows of v's cell
  const unsigned rvm0 = (unsigned)(flt_clampi(vj0 - 1, 1, P.jm) - 1) * iml, rvm1 = (unsigned)(flt_clampi(vj1 - 1, 1, P.jm) - 1) * iml;
  const unsigned cu0 = (unsigned)(ui0 - 1), cu1 = (unsigned)(ui1 - 1);
  const unsigned cum0 = (unsigned)(flt_clampi(ui0 - 1, 1, P.im) - 1), cum1 = (unsigned)(flt_clampi(ui1 - 1, 1, P.im) - 1);
  const unsigned cc0 = (unsigned)(ci0 - 1), cc1 = (unsigned)(ci1 - 1);
  const FltLev lz = flt_levels_zz(P, sig), lw = flt_levels_z(P, sig);
  const unsigned ka = (unsigned)(lz.k - 1) * n2, kb = (unsigned)(lz.k2 - 1) * n2;
  const unsigned wa = (unsigned)(lw.k - 1) * n2, wb = (unsigned)(lw.k2 - 1) * n2;
  // ---- gathers, all of them before the first use
  const double u00a = u[ka + ru0 + cu0], u10a = u[ka + ru0 + cu1], u01a = u[ka + ru1 + cu0], u11a = u[ka + ru1 + cu1];
  const double u00b = u[kb + ru0 + cu0], u10b = u[kb + ru0 + cu1], u01b = u[kb + ru1 + cu0], u11b = u[kb + ru1 + cu1];
  const double v00a = v[ka + rv0 + cc0], v10a = v[ka + rv0 + cc1], v01a = v[ka + rv1 + cc0], v11a = v[ka + rv1 + cc1];
  const double v00b = v[kb + rv0 + cc0], v10b = v[kb + rv0 + cc1], v01b = v[kb + rv1 + cc0], v11b = v[kb + rv1 + cc1];
  const double w00a = w[wa + ru0 + cc0], w10a = w[wa + ru0 + cc1], w01a = w[wa + ru1 + cc0], w11a = w[wa + ru1 + cc1];
  const double w00b = w[wb + ru0 + cc0], w10b = w[wb + ru0 + cc1], w01b = w[wb + ru1 + cc0], w11b = w[wb + ru1 + cc1];
  const double dx00 = dx[ru0 + cu0], dx10 = dx[ru0 + cu1], dx01 = dx[ru1 + cu0], dx11 = dx[ru1 + cu1];
  const double dxm00 = dx[ru0 + cum0], dxm10 = dx[ru0 + cum1], dxm01 = dx[ru1 + cum0], dxm11 = dx[ru1 + cum1];
  const double dy00 = dy[rv0 + cc0], dy10 = dy[rv0 + cc1], dy01 = dy[rv1 + cc0], dy11 = dy[rv1 + cc1];
  const double dym00 = dy[rvm0 + cc0], dym10 = dy[rvm0 + cc1], dym01 = dy[rvm1 + cc0], dym11 = dy[rvm1 + cc1];
  const double d00 = dt[ru0 + cc0], d10 = dt[ru0 + cc1], d01 = dt[ru1 + cc0], d11 = dt[ru1 + cc1];
  // ---- values: L in i, then in j, per level, then in k
  const double ua = flt_bil(u00a, u10a, u01a, u11a, ufx, cfy), ub = flt_bil(u00b, u10b, u01b, u11b, ufx, cfy);
  const double va = flt_bil(v00a, v10a, v01a, v11a, cfx, vfy), vb = flt_bil(v00b, v10b, v01b, v11b, cfx, vfy);
  const double wva = flt_bil(w00a, w10a, w01a, w11a, cfx, cfy), wvb = flt_bil(w00b, w10b, w01b, w11b, cfx, cfy);
  const double U = lz.alone ? ua : flt_L(ua, ub, lz.fz), V = lz.alone ? va : flt_L(va, vb, lz.fz), W = flt_L(wva, wvb, lw.fz);
  const double DXU = flt_bil(0.5 * (dx00 + dxm00), 0.5 * (dx10 + dxm10), 0.5 * (dx01 + dxm01), 0.5 * (dx11 + dxm11), ufx, cfy);
  const double DYV = flt_bil(0.5 * (dy00 + dym00), 0.5 * (dy10 + dym10), 0.5 * (dy01 + dym01), 0.5 * (dy11 + dym11), cfx, vfy);
  const double D = flt_bil(d00, d10, d01, d11, cfx, cfy);
  FltV r;
  r.a = U / DXU; r.b = V / DYV; r.c = W / D;
  return r;
}
// where a position stands: 0 not finite, 1 outside 2..im-1 x 2..jm-1, 2 on land, 3 in the water
__device__ __forceinline__ int flt_classify(const KP &P, double x, double y, double s) {
  if (!(flt_finite(x) && flt_finite(y) && flt_finite(s))) return 0;
  const double xc = floor(x + 0.5), yc = floor(y + 0.5);
  if (!(xc >= 2. && xc <= (double)(P.im - 1) && yc >= 2. && yc <= (double)(P.jm - 1))) return 1;
  const double *fsm = A2(fsm);
  return fsm[(unsigned)((int)yc - 1) * (unsigned)P.iml + (unsigned)((int)xc - 1)] == 0. ? 2 : 3;
}

// one midpoint step of length dti with the fields frozen, for the active floats
__global__ void __launch_bounds__(256) k_float_step(KP P, int n, double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ fs,
                                                    int *__restrict__ status, const int *__restrict__ kind) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (unsigned)n) return;
  if (status[t] != POMGPU_FLOAT_ACTIVE) return;
  const double x = fx[t], y = fy[t], sig = fs[t], dti = P.dti, hm = 0.5 * dti;
  const bool keeps = kind[t] == 1;
  const FltV v1 = flt_velocity(P, x, y, sig);
  const double xm = x + hm * v1.a, ym = y + hm * v1.b;
  double sm = keeps ? sig : sig + hm * v1.c;
  sm = fmin(fmax(sm, -1.), 0.);
  const FltV v2 = flt_velocity(P, xm, ym, sm);
  const double xn = x + dti * v2.a, yn = y + dti * v2.b, sraw = keeps ? sig : sig + dti * v2.c;
  double sn = sraw;
  if (sn > 0.) sn = -sn;
  if (sn < -1.) sn = -2. - sn;
  sn = fmin(fmax(sn, -1.), 0.);
  const int where = flt_classify(P, xn, yn, sraw);           // sn's finiteness is that of the sum: the limits would hide a NaN
  if (where == 0) { status[t] = POMGPU_FLOAT_LOST; return; } // position kept
  if (where == 2) { fs[t] = sn; return; }                    // land: x, y kept, the float tries again next step
  if (where == 1) status[t] = POMGPU_FLOAT_EXITED;           // this is where it left
  fx[t] = xn; fy[t] = yn; fs[t] = sn;
}

// admission of uploaded positions: not finite or on land LOST, outside EXITED; a float whose `keep` says other than ACTIVE keeps that
__global__ void __launch_bounds__(256) k_float_admit(KP P, int n, const double *__restrict__ fx, const double *__restrict__ fy,
                                                     const double *__restrict__ fs, int *__restrict__ status, const int *__restrict__ keep) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (unsigned)n) return;
  if (keep && keep[t] != POMGPU_FLOAT_ACTIVE) { status[t] = keep[t]; return; }
  const int where = flt_classify(P, fx[t], fy[t], fs[t]);
  status[t] = where == 3 ? POMGPU_FLOAT_ACTIVE : (where == 1 ? POMGPU_FLOAT_EXITED : POMGPU_FLOAT_LOST);
}

// lon lat depth t s of every float, whatever its status: out[q * n + t]
__global__ void __launch_bounds__(256) k_float_sample(KP P, int n, const double *__restrict__ fx, const double *__restrict__ fy,
                                                      const double *__restrict__ fs, double *__restrict__ out) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (unsigned)n) return;
  const double x = fx[t], y = fy[t], sig = fs[t];
  const double *ee = A2(east_e), *ne = A2(north_e), *et = A2(et), *dt = A2(dt), *tt = A3(t), *ss = A3(s);
  int i0, i1, j0, j1;
  double cfx, cfy;
  flt_axis(x, P.im, i0, i1, cfx);
  flt_axis(y, P.jm, j0, j1, cfy);
  const unsigned iml = (unsigned)P.iml, n2 = (unsigned)P.n2;
  const unsigned r0 = (unsigned)(j0 - 1) * iml, r1 = (unsigned)(j1 - 1) * iml, c0 = (unsigned)(i0 - 1), c1 = (unsigned)(i1 - 1);
  const unsigned cell = (unsigned)(flt_cell(y, P.jm) - 1) * iml + (unsigned)(flt_cell(x, P.im) - 1);
  const FltLev lz = flt_levels_zz(P, sig);
  const unsigned ka = (unsigned)(lz.k - 1) * n2 + cell, kb = (unsigned)(lz.k2 - 1) * n2 + cell;
  const double e00 = ee[r0 + c0], e10 = ee[r0 + c1], e01 = ee[r1 + c0], e11 = ee[r1 + c1];
  const double n00 = ne[r0 + c0], n10 = ne[r0 + c1], n01 = ne[r1 + c0], n11 = ne[r1 + c1];
  const double etc = et[cell], dtc = dt[cell], ta = tt[ka], tb = tt[kb], sa = ss[ka], sb = ss[kb];
  const size_t N = (size_t)n;
  out[t] = flt_bil(e00, e10, e01, e11, cfx, cfy);
  out[N + t] = flt_bil(n00, n10, n01, n11, cfx, cfy);
  out[2 * N + t] = etc + sig * dtc;
  out[3 * N + t] = lz.alone ? ta : flt_L(ta, tb, lz.fz);
  out[4 * N + t] = lz.alone ? sa : flt_L(sa, sb, lz.fz);
}

static inline dim3 flt_grid(int n) { return dim3((unsigned)((n + 255) / 256), 1, 1); }
static void launch_float_step(pomgpu_ctx *c) {
  LAUNCH(c, k_float_step, flt_grid(c->nflt), dim3(256), c->P, c->nflt, c->flt_x, c->flt_y, c->flt_s, c->flt_status, (const int *)c->flt_kind);
}
static void launch_float_admit(pomgpu_ctx *c, const int *keep) {
  LAUNCH(c, k_float_admit, flt_grid(c->nflt), dim3(256), c->P, c->nflt, (const double *)c->flt_x, (const double *)c->flt_y, (const double *)c->flt_s, c->flt_status, keep);
}
static void launch_float_sample(pomgpu_ctx *c, double *out) {
  LAUNCH(c, k_float_sample, flt_grid(c->nflt), dim3(256), c->P, c->nflt, (const double *)c->flt_x, (const double *)c->flt_y, (const double *)c->flt_s, out);
}
