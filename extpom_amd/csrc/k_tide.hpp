// k_tide.hpp -- tides (include/pomgpu.h "tides"): the phasor table of a step and the two kernels of the harmonic analysis, with their
// launchers, included by pomgpu_api.hip.  The tide itself enters bcond(2) in k_ext.hip (tide_add).
//
// k_tide_table: the host's phasors of one internal step come as kernel arguments and are stored by vector stores, one double per lane; the
// substeps' kernels behind it on the stream index the table by their iext.  Arguments are copied when the launch is made, so the host's
// buffer is free at once and nothing has to be pinned, recorded or waited for.
// k_harm_accum: one lane per cell of the (iml, jml) plane, 256 lanes a workgroup; per field 1 + 2 nc planes read, added to and written,
// plane-major, every access coalesced; 32-bit element offsets (3 x 17 planes: checked where the accumulators are made).  No lane talks to
// another: no LDS, no atomics.  The phasors are kernel arguments (scalar registers).
// k_harm_solve: the same lanes; the inverse of the normal matrix comes as an argument, coef[p] = sum over q, in the order of q, of
// inv[p][q] * sums[q].
#pragma once
#include "pomgpu.h"
#include "pomgpu_internal.hpp"

#define TIDE_CHUNK 480                                      // doubles per k_tide_table launch: 3840 bytes of the 4096 a launch may carry
struct TideChunk { double v[TIDE_CHUNK]; };
struct HarmB { double cn[POMGPU_TIDEMAX], sn[POMGPU_TIDEMAX]; };
#define HARM_MAXB (1 + 2 * POMGPU_TIDEMAX)
struct HarmInv { double a[HARM_MAXB * HARM_MAXB]; };

__global__ void __launch_bounds__(256) k_tide_table(double *__restrict__ dst, TideChunk ch, int n) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < (unsigned)n) dst[t] = ch.v[t];
}

// acc: 3 x (1 + 2 nc) planes of n2 doubles; elb, uab, vab: where the three fields live now
__global__ void __launch_bounds__(256) k_harm_accum(unsigned n2, int nc, HarmB b, double *__restrict__ acc, const double *__restrict__ elb,
                                                    const double *__restrict__ uab, const double *__restrict__ vab) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n2) return;
  const unsigned np = 1u + 2u * (unsigned)nc;
  const double f[3] = {elb[t], uab[t], vab[t]};
#pragma unroll
  for (int q = 0; q < 3; q++) {
    double *a = acc + (size_t)((unsigned)q * np * n2 + t);
    a[0] = a[0] + f[q];
    for (int c = 0; c < nc; c++) {
      const unsigned p = (1u + 2u * (unsigned)c) * n2;
      a[p] = a[p] + f[q] * b.cn[c];
      a[p + n2] = a[p + n2] + f[q] * b.sn[c];
    }
  }
}

// sums: the 1 + 2 nc planes of one field; coef: as many planes
__global__ void __launch_bounds__(256) k_harm_solve(unsigned n2, int np, HarmInv inv, const double *__restrict__ sums, double *__restrict__ coef) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n2) return;
  for (int p = 0; p < np; p++) {
    double s = inv.a[p * np] * sums[t];
    for (int q = 1; q < np; q++) s = s + inv.a[p * np + q] * sums[(unsigned)q * n2 + t];
    coef[(unsigned)p * n2 + t] = s;
  }
}

// coef: the mean, then C and S of every constituent (k_harm_solve); out: the mean, nc amplitudes hypot(C, S), nc phases g = atan2(S, C) in
// degrees in [0, 360), the g of A cos(omega t - g)
__global__ void __launch_bounds__(256) k_harm_constants(unsigned n2, int nc, const double *__restrict__ coef, double *__restrict__ out) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n2) return;
  out[t] = coef[t];
  for (int c = 0; c < nc; c++) {
    const double C = coef[(1u + 2u * (unsigned)c) * n2 + t], S = coef[(2u + 2u * (unsigned)c) * n2 + t];
    double g = atan2(S, C) * (180. / 3.14159265358979323846);
    if (g < 0.) g = g + 360.;
    if (g >= 360.) g = 0.;
    out[(1u + (unsigned)c) * n2 + t] = hypot(C, S);
    out[(1u + (unsigned)(nc + c)) * n2 + t] = g;
  }
}

// n doubles of the host's table into dst, TIDE_CHUNK per launch
static void launch_tide_table(pomgpu_ctx *c, double *dst, const double *host, size_t n) {
  for (size_t o = 0; o < n; o += TIDE_CHUNK) {
    TideChunk ch;
    const int m = (int)(n - o < (size_t)TIDE_CHUNK ? n - o : (size_t)TIDE_CHUNK);
    for (int e = 0; e < m; e++) ch.v[e] = host[o + e];
    for (int e = m; e < TIDE_CHUNK; e++) ch.v[e] = 0.;
    LAUNCH(c, k_tide_table, dim3((unsigned)((m + 255) / 256), 1, 1), dim3(256), dst + o, ch, m);
  }
}
static void launch_harm_accum(pomgpu_ctx *c, const HarmB &b) {
  const KP &P = c->P;
  LAUNCH(c, k_harm_accum, dim3((unsigned)((P.n2 + 255) / 256), 1, 1), dim3(256), (unsigned)P.n2, c->ntide, b, c->harm_acc, (const double *)P.x2[X2_elb],
         (const double *)P.x2[X2_uab], (const double *)P.x2[X2_vab]);
}
static void launch_harm_constants(pomgpu_ctx *c, const double *coef, double *out) {
  LAUNCH(c, k_harm_constants, dim3((unsigned)((c->P.n2 + 255) / 256), 1, 1), dim3(256), (unsigned)c->P.n2, c->ntide, coef, out);
}
static void launch_harm_solve(pomgpu_ctx *c, const HarmInv &inv, const double *sums, double *coef) {
  const KP &P = c->P;
  LAUNCH(c, k_harm_solve, dim3((unsigned)((P.n2 + 255) / 256), 1, 1), dim3(256), (unsigned)P.n2, 1 + 2 * c->ntide, inv, sums, coef);
}
