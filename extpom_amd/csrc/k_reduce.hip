// k_reduce.hip -- check_velocity (advance.f:611-641): vamax = max |vaf| with the LAST position
// (j outer, i inner scan; `.ge.` at :623) at which the maximum is attained.
//
// A (value, linear index) pair is reduced with the total order "larger value wins, ties go to the
// larger scan index", which is associative and commutative, so the wavefront shuffle tree gives
// exactly the reference's sequential answer.  Two stages: up to 1024 workgroups each reduce a strided
// share (4 wavefronts x __shfl_down tree -> LDS -> first wavefront), one workgroup reduces the partials.
#include "pomgpu_internal.hpp"

struct VelMax { double v; long long n; };
__device__ __forceinline__ VelMax vm_best(VelMax a, VelMax b) {
  return (b.v > a.v || (b.v == a.v && b.n > a.n)) ? b : a;
}
__device__ __forceinline__ VelMax vm_wave(VelMax x) {
  for (int off = 32; off > 0; off >>= 1) {
    VelMax y;
    y.v = __shfl_down(x.v, off, 64);
    y.n = __shfl_down(x.n, off, 64);
    x = vm_best(x, y);
  }
  return x;
}
__device__ __forceinline__ VelMax vm_block(VelMax best, VelMax *part) {   // all threads call; valid in wave 0
  best = vm_wave(best);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[wave] = best;
  __syncthreads();
  VelMax x = (lane < (int)(blockDim.x >> 6)) ? part[lane] : best;
  return vm_wave(x);
}
// stage 1: every workgroup scans a strided share of the plane; partial (value, index) -> pv, pn
__global__ void __launch_bounds__(256) k_check_velocity(KP P, double *pv, double *pn) {
  __shared__ VelMax part[4];
  const long long total = (long long)P.im * P.jm;
  VelMax best;
  best.v = 0.;            // vamax starts at 0 and `>=` lets the last zero win
  best.n = -1;
  for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < total; n += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(n / P.im) + 1, i = (int)(n % P.im) + 1;
    VelMax c;
    c.v = fabs(F2(vaf, i, j));
    c.n = n;
    if (c.v >= best.v) best = vm_best(best, c);
  }
  best = vm_block(best, part);
  if (threadIdx.x == 0) { pv[blockIdx.x] = best.v; pn[blockIdx.x] = (double)best.n; }
}
// stage 2: out[0] = vamax, out[1] = imax, out[2] = jmax (as doubles); err: device error flag
__global__ void __launch_bounds__(256) k_check_velocity_fin(KP P, const double *pv, const double *pn, int nb, double *out, int *err) {
  __shared__ VelMax part[4];
  VelMax best;
  best.v = 0.;
  best.n = -1;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    VelMax c;
    c.v = pv[b];
    c.n = (long long)pn[b];
    if (c.v >= best.v) best = vm_best(best, c);
  }
  best = vm_block(best, part);
  if (threadIdx.x == 0) {
    out[0] = best.v;
    out[1] = (best.n >= 0) ? (double)(best.n % P.im + 1) : 0.;
    out[2] = (best.n >= 0) ? (double)(best.n / P.im + 1) : 0.;
    if (best.v > P.vmaxl) atomicOr(err, POMGPU_DERR_VELOCITY);
  }
}
// ---------------------------------------------------------------------------------------------
// domain_stats (advance.f:644-756): seven masked sums -- vtot, atot, mtot, stot, sum(tb*dvol), sum(et*darea),
// ekin -- as a fixed-shape reduction: a thread sums its water columns level by level, a wavefront
// shuffle tree and the 4 wavefronts of a workgroup follow, one workgroup adds the partials in index
// order.  Same launch, same bits (no atomics); against the reference's SUM intrinsic parity is to
// rounding (its order of additions is the compiler's).  dvol is assigned on 2:imm1 x 2:jmm1 only and
// zero elsewhere (:692-695), so the 3-D sums -- edge additions included -- cover the interior; atot and
// the elevation sum include the physical edges without corners (:666-677).
#define NSTAT 7
__device__ __forceinline__ double ds_wave(double x) {
  for (int off = 32; off > 0; off >>= 1) x = x + __shfl_down(x, off, 64);
  return x;
}
__device__ __forceinline__ void ds_block(double (&a)[NSTAT], double (*part)[NSTAT]) {   // result in thread 0
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NSTAT; q++) a[q] = ds_wave(a[q]);
  if (lane == 0)
    for (int q = 0; q < NSTAT; q++) part[wave][q] = a[q];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 0; q < NSTAT; q++) a[q] = part[0][q] + part[1][q] + part[2][q] + part[3][q];
}
__global__ void __launch_bounds__(256) k_domain_stats(KP P, double *partial) {
  __shared__ double part[4][NSTAT];
  double a[NSTAT] = {0., 0., 0., 0., 0., 0., 0.};           // vtot atot mtot stot tsum esum ekin
  const long long total = (long long)P.im * P.jm;
  for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < total; n += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(n / P.im) + 1, i = (int)(n % P.im) + 1;
    const bool ii = (i >= 2 && i <= P.imm1), jj = (j >= 2 && j <= P.jmm1);
    const bool edge = (jj && ((P.W && i == 1) || (P.E && i == P.im))) || (ii && ((P.S && j == 1) || (P.N && j == P.jm)));
    if (!(ii && jj) && !edge) continue;
    const double darea = F2(dx, i, j) * F2(dy, i, j) * F2(fsm, i, j);
    a[1] = a[1] + darea;
    a[5] = a[5] + F2(et, i, j) * darea;
    if (ii && jj) {
      const double dtc = F2(dt, i, j);
      for (int k = 1; k <= P.kbm1; k++) {
        const double dvol = darea * dtc * F1(dz, k);
        const double dmass = dvol * (F3(rho, i, j, k) * P.rhoref + 1000.);
        a[0] = a[0] + dvol;
        a[2] = a[2] + dmass;
        a[3] = a[3] + F3(sb, i, j, k) * dvol;
        a[4] = a[4] + F3(tb, i, j, k) * dvol;
        const double uu = F3(u, i, j, k), vv = F3(v, i, j, k);
        a[6] = a[6] + .5 * (dmass * (uu * uu + vv * vv));
      }
    }
  }
  ds_block(a, part);
  if (threadIdx.x == 0)
    for (int q = 0; q < NSTAT; q++) partial[(size_t)blockIdx.x * NSTAT + q] = a[q];
}
__global__ void __launch_bounds__(256) k_domain_stats_fin(const double *partial, int nb, double *out) {
  __shared__ double part[4][NSTAT];
  double a[NSTAT] = {0., 0., 0., 0., 0., 0., 0.};
  for (int b = threadIdx.x; b < nb; b += blockDim.x)
    for (int q = 0; q < NSTAT; q++) a[q] = a[q] + partial[(size_t)b * NSTAT + q];
  ds_block(a, part);
  if (threadIdx.x == 0)
    for (int q = 0; q < NSTAT; q++) out[q] = a[q];
}
void launch_domain_stats(pomgpu_ctx *c, double *out_dev) {
  const long long total = (long long)c->P.im * c->P.jm;
  int nb = (int)((total + 255) / 256);
  if (nb > 2048) nb = 2048;
  if (nb < 1) nb = 1;
  LAUNCH(c, k_domain_stats, dim3(nb), dim3(256), c->P, c->P.s2[7]);          // 2048 x 7 partials fit one 2-D scratch plane (>= 25 cells checked at create)
  LAUNCH(c, k_domain_stats_fin, dim3(1), dim3(256), (const double *)c->P.s2[7], nb, out_dev);
}
// ---------------------------------------------------------------------------------------------
// pomgpu_tracer_stats (include/pomgpu.h): the inventory of every registered tracer in ONE pass over the columns, in the shape of
// k_domain_stats -- a strided share of the columns per lane, the wavefront shuffle tree, four partials in LDS, one finishing workgroup, no
// atomics: same launch, same bits.  Per tracer tot = sum trb * dvol with domain_stats' dvol = dx*dy*fsm * dt * dz(k) on its cells
// (2:imm1 x 2:jmm1, k = 1..kbm1), so that tile sums add up under the host's rank reduction as sum(tb*dvol) does, and min / max of tr over
// the cells of (1:im, 1:jm, 1:kbm1) with fsm != 0, which are exact whatever the tree's shape.  vtot comes out of the same pass:
// avg = tot / vtot.  A value's place q says how it is combined: 0 vtot (sum); 1 + 3t, 2 + 3t, 3 + 3t: tot (sum), min, max of tracer t.
// The loops over the tracers are unrolled to POMGPU_TRMAX with the count as a predicate: every value stays in a register.
#define TRS_NV (1 + 3 * POMGPU_TRMAX)
struct TrStatTab { const double *trb[POMGPU_TRMAX], *tr[POMGPU_TRMAX]; int ntr; };
__device__ __forceinline__ double trs_op(int q, double x, double y) {
  const int kind = q == 0 ? 0 : (q - 1) % 3;
  return kind == 0 ? x + y : (kind == 1 ? (y < x ? y : x) : (y > x ? y : x));
}
__device__ __forceinline__ double trs_unit(int q) { return (q == 0 || (q - 1) % 3 == 0) ? 0. : ((q - 1) % 3 == 1 ? __DBL_MAX__ : -__DBL_MAX__); }
__device__ __forceinline__ void trs_block(double (&a)[TRS_NV], double (*part)[TRS_NV]) {   // result in thread 0
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < TRS_NV; q++)
    for (int off = 32; off > 0; off >>= 1) a[q] = trs_op(q, a[q], __shfl_down(a[q], off, 64));
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < TRS_NV; q++) part[wave][q] = a[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < TRS_NV; q++) a[q] = trs_op(q, trs_op(q, trs_op(q, part[0][q], part[1][q]), part[2][q]), part[3][q]);
  }
}
__global__ void __launch_bounds__(256) k_tracer_stats(KP P, TrStatTab T, double *partial) {
  __shared__ double part[4][TRS_NV];
  double a[TRS_NV];
#pragma unroll
  for (int q = 0; q < TRS_NV; q++) a[q] = trs_unit(q);
  const unsigned total = (unsigned)P.im * (unsigned)P.jm;       // a level's cells: 32 bits hold them (pomgpu_create: an array is under 4 GiB)
  for (unsigned n = blockIdx.x * blockDim.x + threadIdx.x; n < total; n += gridDim.x * blockDim.x) {
    const int j = (int)(n / (unsigned)P.im) + 1, i = (int)(n % (unsigned)P.im) + 1;
    const bool inner = i >= 2 && i <= P.imm1 && j >= 2 && j <= P.jmm1;
    const double fs = F2(fsm, i, j);
    const bool wet = fs != 0.;
    if (!inner && !wet) continue;
    const double darea = F2(dx, i, j) * F2(dy, i, j) * fs, dtc = F2(dt, i, j);
    if (inner)
      for (int k = 1; k <= P.kbm1; k++) a[0] = a[0] + darea * dtc * F1(dz, k);
    // tracer by tracer down the column: two of the sixteen array addresses are in use at a time
#pragma unroll
    for (int t = 0; t < POMGPU_TRMAX; t++)
      if (t < T.ntr) {
        const double *pb = T.trb[t] + IX2(i, j), *px = T.tr[t] + IX2(i, j);
        double tot = a[1 + 3 * t], mn = a[2 + 3 * t], mx = a[3 + 3 * t];
        for (int k = 1; k <= P.kbm1; k++) {
          const double dvol = darea * dtc * F1(dz, k);
          const size_t e = (size_t)(k - 1) * P.n2;
          if (inner) tot = tot + pb[e] * dvol;
          if (wet) {
            const double x = px[e];
            mn = x < mn ? x : mn;
            mx = x > mx ? x : mx;
          }
        }
        a[1 + 3 * t] = tot; a[2 + 3 * t] = mn; a[3 + 3 * t] = mx;
      }
  }
  trs_block(a, part);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < TRS_NV; q++) partial[(size_t)blockIdx.x * TRS_NV + q] = a[q];
  }
}
__global__ void __launch_bounds__(256) k_tracer_stats_fin(const double *partial, int nb, int ntr, double *out) {
  __shared__ double part[4][TRS_NV];
  double a[TRS_NV];
#pragma unroll
  for (int q = 0; q < TRS_NV; q++) a[q] = trs_unit(q);
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
#pragma unroll
    for (int q = 0; q < TRS_NV; q++) a[q] = trs_op(q, a[q], partial[(size_t)b * TRS_NV + q]);
  }
  trs_block(a, part);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int t = 0; t < POMGPU_TRMAX; t++)
      if (t < ntr) {
        out[4 * t] = a[1 + 3 * t];
        out[4 * t + 1] = a[0] != 0. ? a[1 + 3 * t] / a[0] : 0.;
        out[4 * t + 2] = a[2 + 3 * t];
        out[4 * t + 3] = a[3 + 3 * t];
      }
  }
}
void launch_tracer_stats(pomgpu_ctx *c, double *out_dev) {
  const long long total = (long long)c->P.im * c->P.jm;
  int nb = (int)((total + 255) / 256);
  if (nb > 2048) nb = 2048;
  if (nb < 1) nb = 1;
  TrStatTab T;
  for (int t = 0; t < POMGPU_TRMAX; t++) { T.trb[t] = t < c->ntr ? c->trc[t].trb : NULL; T.tr[t] = t < c->ntr ? c->trc[t].tr : NULL; }
  T.ntr = c->ntr;
  // nb x 25 partials fit one 2-D scratch plane: nb = 1 needs 25 cells (checked at create), beyond that 25 per 256 cells
  LAUNCH(c, k_tracer_stats, dim3(nb), dim3(256), c->P, T, c->P.s2[7]);
  LAUNCH(c, k_tracer_stats_fin, dim3(1), dim3(256), (const double *)c->P.s2[7], nb, c->ntr, out_dev);
}
void launch_check_velocity(pomgpu_ctx *c) {
  const long long total = (long long)c->P.im * c->P.jm;
  int nb = (int)((total + 256 * 8 - 1) / (256 * 8));
  if (nb > 1024) nb = 1024;
  if (nb < 1) nb = 1;
  LAUNCH(c, k_check_velocity, dim3(nb), dim3(256), c->P, c->P.s2[5], c->P.s2[6]);
  LAUNCH(c, k_check_velocity_fin, dim3(1), dim3(256), c->P, (const double *)c->P.s2[5], (const double *)c->P.s2[6], nb, c->d_vel, c->d_err);
}
