// pomgpu_api.hip -- the C ABI of include/pomgpu.h: context, COMMON-block mirrors in HBM, and the
// orchestration of the reference's advance.f as sequences of fused kernel launches on ONE HIP
// stream.  Host code here only enqueues work; nothing synchronises except the calls documented
// to do so (upload/download, check_velocity, sync).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "pomgpu.h"
#include "pomgpu_internal.hpp"
#include "k_float.hpp"
#include "k_tide.hpp"

struct ProfPair { int slot; hipEvent_t a, b; };
struct ProfState { std::vector<ProfPair> pending; std::vector<ProfPair> free_; char filter[64]; };
static ProfState *PS(pomgpu_ctx *c) { return (ProfState *)c->prof_state; }

#define SLOT2(c, n) ((c)->P.b2 + (size_t)(n) * (c)->P.n2)
#define SLOT3(c, n) ((c)->P.b3 + (size_t)(n) * (c)->P.a3)
#define D2(c, name) SLOT2(c, P2_##name)
#define D3(c, name) SLOT3(c, P3_##name)
// level lev + 1 of a 3-D array, as a handle: in the fp32-storage variant the levels are n2 FLOATS apart
#define LEV3(c, p, lev) ((double *)((pomgpu_st *)(p) + (size_t)(lev) * (c)->P.n2))

int pomgpu_fail(pomgpu_ctx *c, int code, const char *fmt, ...) {
  if (c && c->parent) c = c->parent;
  if (c) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof c->err, fmt, ap);
    va_end(ap);
    c->con.error_status = 1;   // the reference's error convention (advance.f:118,637)
    fprintf(stderr, "pomgpu: %s\n", c->err);
  }
  return code;
}
#define fail pomgpu_fail
#define HIPCHK(c, call)                                                                  \
  do {                                                                                   \
    hipError_t _e = (call);                                                              \
    if (_e != hipSuccess) return fail((c), POMGPU_EHIP, "%s: %s", #call, hipGetErrorString(_e)); \
  } while (0)

void pomgpu_launch_check(pomgpu_ctx *c, const char *name) {
  const hipError_t e = hipGetLastError();
  if (c->parent) c = c->parent;
  if (e == hipSuccess || c->launch_err) return;
  c->launch_err = (int)e;
  (void)fail(c, POMGPU_EHIP, "launch of %s refused: %s", name, hipGetErrorString(e));
}

// ---- profiling ---------------------------------------------------------------------------------
int pomgpu_prof_slot(pomgpu_ctx *c, const char *name) {
  if (c->parent) c = c->parent;
  ProfState *ps = PS(c);
  if (ps->filter[0] && strcmp(ps->filter, name) != 0) return -1;
  for (int k = 0; k < c->nprof; k++)
    if (c->prof[k].name == name || strcmp(c->prof[k].name, name) == 0) return k;
  if (c->nprof >= (int)(sizeof c->prof / sizeof c->prof[0])) return -1;
  c->prof[c->nprof].name = name;
  c->prof[c->nprof].launches = 0;
  c->prof[c->nprof].ms = 0.;
  return c->nprof++;
}
void pomgpu_prof_pre(pomgpu_ctx *c) {
  const hipStream_t st = c->cur;                              // the stream the bracketed work goes to
  if (c->parent) c = c->parent;
  ProfState *ps = PS(c);
  ProfPair p;
  if (!ps->free_.empty()) { p = ps->free_.back(); ps->free_.pop_back(); }
  else { (void)hipEventCreate(&p.a); (void)hipEventCreate(&p.b); }
  p.slot = -1;
  (void)hipEventRecord(p.a, st);
  ps->pending.push_back(p);
}
void pomgpu_prof_post(pomgpu_ctx *c, int slot) {
  const hipStream_t st = c->cur;
  if (c->parent) c = c->parent;
  ProfState *ps = PS(c);
  ProfPair &p = ps->pending.back();
  p.slot = slot;
  (void)hipEventRecord(p.b, st);
}
// Phases: brackets that contain other brackets (a whole step, its external substeps).  Not subject to the kernel filter, so
// that a timed region which brackets one kernel only still yields K-step means of the step and of its external mode.
static int prof_phase_open(pomgpu_ctx *c) {
  if (!c->prof_on) return -1;
  pomgpu_prof_pre(c);
  return (int)PS(c)->pending.size() - 1;
}
static void prof_phase_close(pomgpu_ctx *c, int idx, const char *name) {
  if (idx < 0 || !c->prof_on) return;
  ProfState *ps = PS(c);
  int slot = -1;
  for (int k = 0; k < c->nprof; k++) if (strcmp(c->prof[k].name, name) == 0) slot = k;
  if (slot < 0 && c->nprof < (int)(sizeof c->prof / sizeof c->prof[0])) {
    slot = c->nprof++;
    c->prof[slot].name = name; c->prof[slot].launches = 0; c->prof[slot].ms = 0.;
  }
  ps->pending[idx].slot = slot;
  (void)hipEventRecord(ps->pending[idx].b, c->stream);
}
static void prof_drain(pomgpu_ctx *c) {
  ProfState *ps = PS(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->side) (void)hipStreamSynchronize(c->side);
  for (size_t n = 0; n < ps->pending.size(); n++) {
    ProfPair &p = ps->pending[n];
    float ms = 0.f;
    if (p.slot >= 0 && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      c->prof[p.slot].launches += 1;
      c->prof[p.slot].ms += (double)ms;
    }
    ps->free_.push_back(p);
  }
  ps->pending.clear();
}
extern "C" int pomgpu_prof_begin(pomgpu_ctx *c) {
  if (!c) return POMGPU_EINVAL;
  c->nprof = 0;
  c->prof_on = true;
  if (c->wide.x) c->wide.x->prof_on = true;
  return POMGPU_OK;
}
// restrict event bracketing to one kernel (by name, e.g. "k_profq"); NULL or "" = every kernel
extern "C" int pomgpu_prof_filter(pomgpu_ctx *c, const char *kernel_name) {
  if (!c) return POMGPU_EINVAL;
  ProfState *ps = PS(c);
  snprintf(ps->filter, sizeof ps->filter, "%s", kernel_name ? kernel_name : "");
  return POMGPU_OK;
}
extern "C" int pomgpu_prof_end(pomgpu_ctx *c) {
  if (!c) return POMGPU_EINVAL;
  prof_drain(c);
  c->prof_on = false;
  if (c->wide.x) c->wide.x->prof_on = false;
  return POMGPU_OK;
}
extern "C" int pomgpu_prof_count(pomgpu_ctx *c) { return c ? c->nprof : 0; }
extern "C" int pomgpu_prof_get(pomgpu_ctx *c, int k, const char **name, long *launches, double *total_ms) {
  if (!c || k < 0 || k >= c->nprof) return POMGPU_EINVAL;
  if (name) *name = c->prof[k].name;
  if (launches) *launches = c->prof[k].launches;
  if (total_ms) *total_ms = c->prof[k].ms;
  return POMGPU_OK;
}

// ---- scalars -----------------------------------------------------------------------------------
static void sync_scalars(pomgpu_ctx *c) {
  KP &P = c->P;
  const pom_blkcon &k = c->con;
  P.alpha = k.alpha; P.dte = k.dte; P.dti = k.dti; P.dti2 = k.dti2; P.dte2 = k.dte2; P.grav = k.grav;
  P.kappa = k.kappa; P.ramp = k.ramp; P.rfe = k.rfe; P.rfn = k.rfn; P.rfs = k.rfs; P.rfw = k.rfw;
  P.rhoref = k.rhoref; P.sbias = k.sbias; P.small_ = k.small; P.tbias = k.tbias; P.tprni = k.tprni;
  P.umol = k.umol; P.horcon = k.horcon; P.ispi = k.ispi; P.isp2i = k.isp2i; P.smoth = k.smoth; P.sw = k.sw;
  P.time = k.time; P.vmaxl = k.vmaxl;
  P.mode = k.mode; P.ntp = k.ntp; P.nadv = k.nadv; P.nbct = k.nbct; P.nbcs = k.nbcs; P.nitera = k.nitera;
  P.npg = k.npg; P.isplit = k.isplit; P.iext = k.iext; P.iint = k.iint; P.iend = k.iend;
  // loop invariants the reference evaluates with libm pow at run time (solver.f:1273, :1297);
  // 15.8 and 2./3. are REAL(4) literals there
  P.const1_profq = pow(16.6, 2. / 3.) * 1.;
  P.cb_profq = pow((double)15.8f * 100., (double)(2.f / 3.f));
}

static void tracers_free(pomgpu_ctx *c);
static void floats_free(pomgpu_ctx *c);
static void tides_free(pomgpu_ctx *c);
static int tide_table(pomgpu_ctx *c);
static int tide_widen(pomgpu_ctx *c);
static int harm_accumulate(pomgpu_ctx *c);
// ---- life cycle -------------------------------------------------------------------------------
// a digest of the library's sources, put in by the build (__graft_entry__.build_hip): measurements kept in profiles/ carry it, and
// bench.py only quotes a stored counter value (roofline.traffic) for the build it was taken from
#ifndef POMGPU_BUILD_ID
#define POMGPU_BUILD_ID "unknown"
#endif
extern "C" const char *pomgpu_build_id(void) { return POMGPU_BUILD_ID; }
#ifdef POMGPU_STORE_F32
#ifdef POMGPU_COMPUTE_F32   // the stencil kernels of the internal mode also compute in fp32 (pomgpu_internal.hpp); same context layout
extern "C" const char *pomgpu_version(void) { return "extpom_amd pomgpu 0.2 (gfx950) fp32-storage fp32-arithmetic variant"; }
#else
extern "C" const char *pomgpu_version(void) { return "extpom_amd pomgpu 0.2 (gfx950) fp32-storage variant"; }
#endif
#define F32_REFUSE(c, what) return fail(c, POMGPU_EINVAL, what ": not in the fp32-storage variant (3-D arrays are not doubles there)")
#else
extern "C" const char *pomgpu_version(void) { return "extpom_amd pomgpu 0.2 (gfx950)"; }
#define F32_REFUSE(c, what)
#endif
// host <-> device copies of one 3-D array.  fp64 (the product): a plain copy.  fp32-storage variant: through a staging
// array of doubles (a scratch slot: n3 * 8 bytes) and a conversion kernel, so that the C ABI moves doubles either way.
#ifdef POMGPU_STORE_F32
__global__ void k_cvt_to_st(pomgpu_st *dst, const double *src, size_t n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[t] = (pomgpu_st)src[t];
}
__global__ void k_cvt_from_st(double *dst, const pomgpu_st *src, size_t n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[t] = (double)src[t];
}
#endif
static int copy3_h2d(pomgpu_ctx *c, double *slot, const double *host) {
  const size_t n3 = c->P.n3;
#ifdef POMGPU_STORE_F32
  double *stage = c->P.s3[POMGPU_NSCR3 - 1];
  HIPCHK(c, hipMemcpyAsync(stage, host, sizeof(double) * n3, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_cvt_to_st, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, c->stream, (pomgpu_st *)slot, (const double *)stage, n3);
#else
  HIPCHK(c, hipMemcpyAsync(slot, host, sizeof(double) * n3, hipMemcpyHostToDevice, c->stream));
#endif
  return POMGPU_OK;
}
static int copy3_d2h(pomgpu_ctx *c, double *host, const double *slot) {
  const size_t n3 = c->P.n3;
#ifdef POMGPU_STORE_F32
  double *stage = c->P.s3[POMGPU_NSCR3 - 1];
  hipLaunchKernelGGL(k_cvt_from_st, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, c->stream, stage, (const pomgpu_st *)slot, n3);
  HIPCHK(c, hipMemcpyAsync(host, stage, sizeof(double) * n3, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));                 // the staging array is reused by the next copy
#else
  HIPCHK(c, hipMemcpyAsync(host, slot, sizeof(double) * n3, hipMemcpyDeviceToHost, c->stream));
#endif
  return POMGPU_OK;
}

// ---- the two generations of ua, va, d, el, elb (fused external step, k_ext.hip) -------------------
// ext_parity == 0: the current generation is in the blk2d arrays; == 1: in alt2.  KP.x2 (read) and
// KP.y2 (write) both point at the current generation, so every kernel works in place; only
// launch_ext_step gets a KP whose y2 is the other set.  ext_canonical() moves the current generation
// back into blk2d; every entry point except pomgpu_mode_external calls it first (a no-op after an
// even number of fused substeps).
static const int X2_SLOT[POMGPU_NGEN] = {P2_ua, P2_va, P2_d, P2_el, P2_elb, P2_uab, P2_vab};
static void ext_buffers(pomgpu_ctx *c) {
  KP &P = c->P;
  for (int n = 0; n < POMGPU_NGEN; n++) P.x2[n] = P.y2[n] = c->ext_parity ? c->alt2[n] : P.b2 + (size_t)X2_SLOT[n] * P.n2;
}
// trstr, srstr, taurstr of the last internal step, if k_ts_update skipped them
// rho's deferred round trip (levels 1..kbm1; level kb was done when it was deferred)
static void rho_materialize(pomgpu_ctx *c) {
  if (!c->rho_rt_pending || (c->flags & POMGPU_CTX_2D)) return;
  c->rho_rt_pending = c->rho_rt_cols = 0;
  launch_roundtrip(c, SLOT3(c, P3_rho), SLOT3(c, P3_rmean), 2);
}
static void side_join(pomgpu_ctx *c);
static void side_begin(pomgpu_ctx *c);
static void side_end(pomgpu_ctx *c, hipEvent_t ev);
static int rim_side(pomgpu_ctx *c);
static void early_invalidate(pomgpu_ctx *c);
// wr of the last completed step, if mode_internal left it pending (one tile).  Valid anywhere between the end of one mode_internal
// and the 3-D part of the next: nothing in lateral_viscosity, mode_interaction, mode_external, surface_forcing or lateral_bc writes
// w, u, v, dt, et or etb, and et holds the bits etf had when the reference calls realvertvl (advance.f:525-534) -- etf itself is
// rewritten by the next step's last external substeps (:298-314), so the kernel reads et in its place.
void pomgpu_wr_materialize(pomgpu_ctx *c) {
  if (!c->wr_pending) return;
  c->wr_pending = 0;
  (void)hipSetDevice(c->device);
  if (!(c->flags & POMGPU_CTX_2D)) launch_realvertvl(c, 1);
}
// may mode_internal leave wr to whoever asks for it?  Only where forming it needs no message round (a round is collective and cannot
// happen on one rank's demand) and every read of the mirrors goes through the library
static bool wr_on_demand(const pomgpu_ctx *c) {
  return !c->exch && !c->tp.on && !c->wide.on && !c->parent && !(c->flags & POMGPU_CTX_2D) && !c->wr_eager && !SW(c, WR_NODEFER);
}
// may mode_internal end in k_profuv_filter_reg2 and leave the interior of uf, vf pending?  One tile whose mirrors only the library reads
// (as for wr), a grid with an interior, and the register kernels' range of kb
static bool uv_fused(const pomgpu_ctx *c) {
  const KP &P = c->P;
  return !c->exch && !c->tp.on && !c->wide.on && !c->parent && !(c->flags & POMGPU_CTX_2D) && !c->wr_eager && pomgpu_reg_kb(c) &&
         P.im >= 8 && P.jm >= 8 && !SW(c, UV_NOFUSE);
}
// may mode_internal form w inside the q2 / q2l advection march (k_advq_col<2, true>) instead of launching vertvl in front of it?  One
// tile with no exchange of any kind (on tiles w has a message round of its own, Rw, between the two kernels) and the one-pass q2 / q2l
// path.  No lazy state comes with it: w is in memory, final, when the kernel ends.  The fp32-arithmetic variant has no such kernel
// (POMGPU_W_FUSE) and keeps the pair
static bool w_fused(const pomgpu_ctx *c) {
  return POMGPU_W_FUSE && !c->exch && !c->tp.on && !c->wide.on && !(c->flags & POMGPU_CTX_2D) && !SW(c, ADVQ_SINGLE) && !SW(c, ADVQ_EXCHANGE) &&
         !SW(c, VERTVL_CELLS) && !SW(c, W_NOFUSE);
}
// may mode_internal leave u, v raw in memory and have every kernel between the external mode and the velocity filter apply the
// depth-mean correction (advance.f:365-393) to what it loads, instead of launching k_int_uvmean?  Where all those kernels are the ones
// that know how (uvm_fix, pomgpu_internal.hpp): the fused q2 / q2l march that also forms w, the one-pass tracer advection or none
// (mode 4), k_advuv_col and the fused profu / profv / filter tail -- and where k_advct_col has left the depth sums of the u, v that
// are in memory now (uvm_valid).  POMGPU_UVMEAN_PASS (read here, at launch time) keeps the pass.  No lazy state survives the step: the
// filter that ends the 3-D body overwrites u, v.  The fp32-arithmetic variant keeps the pass at build time (POMGPU_UVM_ONLOAD)
static bool uvm_onload(const pomgpu_ctx *c) {
  const pom_blkcon &k = c->con;
  return POMGPU_UVM_ONLOAD && w_fused(c) && uv_fused(c) && c->uvm_valid && !SW(c, UVMEAN_PASS) &&
         (k.mode == 4 || (k.nadv == 2 && c->P.nitera == 1 && !SW(c, ADVT2_SINGLE))) &&
         // passive tracers are advected in mode 4 too, and with nadv 1 or nitera > 1 by kernels that read u, v as they are in memory
         (!c->ntr || (k.nadv == 2 && c->P.nitera == 1));
}
// may a round trip be read only where it changes bits (rt_words, rt_cols)?  One tile alone: no exchange hook, no transport, no wide halo,
// no parent, not 2-D -- and no address handed out (pomgpu_device_2d / _3d: writes the library cannot see, as for wr).  POMGPU_RT_LOAD is
// read where the consumers are launched
static bool rt_one_tile(const pomgpu_ctx *c) { return !c->exch && !c->tp.on && !c->wide.on && !c->parent && !(c->flags & POMGPU_CTX_2D) && !c->wr_eager; }
// may k_profq of a step that another step of the same pomgpu_run follows keep l and dtef out of memory (launch_profq, store_ld = 0)?
// Nothing on the device reads them back and the next step's profq rewrites both whole, so the question is only who can look between
// the two: nobody on one tile whose mirrors only the library reads (as for wr).  No lazy state comes with it -- they cannot be formed
// afterwards, l = |q2lb / q2b| takes the OLD q2b, q2lb, which the fused filter overwrites on the way up -- the last step of every
// call stores them, and after every call that returns the arrays are those of the last completed step.  POMGPU_LD_EAGER (read here,
// at launch time) stores in every step
static bool ld_on_demand(const pomgpu_ctx *c) {
  return !c->exch && !c->tp.on && !c->wide.on && !c->parent && !(c->flags & POMGPU_CTX_2D) && !c->wr_eager && !SW(c, LD_EAGER);
}
// will the step after this one ask for a forcing or lateral record (pomgpu_wind / _heat / _surface / _lateral_bc: steps whose iint +
// cont_bry is a multiple of the record interval; pomgpu_water: steps whose iint alone is a multiple of a day's)?  That is where a pomgpu_run ends early for a reason outside the device -- a record the
// file or the host does not have -- and surface_forcing / lateral_bc come first in a step: the step in front of it stores l, dtef, so
// that such a run leaves the whole state of its last completed step.  (One step per record interval, 1/24 day: every 20th at dti = 180 s.)
static bool next_step_fetches_record(const pomgpu_ctx *c) {
  if (!c->frc_on && !c->lat_on && !c->wat_on) return false;
  const pom_blkcon &k = c->con;
  const int isrf = (int)(.125 * 86400. / k.dti), ibc = (int)((double)(1.f / 24.f) * 86400. / k.dti), iwater = (int)(86400. / k.dti);
  const int next = k.iint + 1 + k.cont_bry;
  // water's own condition (pomgpu_water): once a day, without cont_bry
  return (c->frc_on && (isrf < 1 || next % isrf == 0)) || (c->lat_on && (ibc < 1 || next % ibc == 0)) ||
         (c->wat_on && (iwater < 1 || (k.iint + 1) % iwater == 0));
}
// ---- the two homes of aam (k_advct_col<*, true>, k_tile.hip) ----------------------------------------
// aam_parity == 0: the current aam is in its blk3d slot; == 1: its levels 1..kbm1 are in aam_spare (level kb and whatever the march
// does not write are never read from the spare).  KP::aamc names the current one for the column kernels of mode_internal
// (k_advq_col, k_advt2_col) and the next k_advct_col; aam_canonical() copies it back into the slot for everybody else.
static void aam_buffers(pomgpu_ctx *c) {
  KP &P = c->P;
  P.aamc = (c->aam_parity && c->aam_spare) ? c->aam_spare : (P.b3 ? P.b3 + (size_t)P3_aam * P.a3 : NULL);
}
static void aam_canonical(pomgpu_ctx *c) {
  if (!c->aam_parity) return;
  (void)hipSetDevice(c->device);
  launch_aam_copy(c, SLOT3(c, P3_aam), c->aam_spare);
  c->aam_parity = 0;
  aam_buffers(c);
}
// may lateral_viscosity form aam and aam2d inside advct's march instead of launching k_aam_pair / k_aam and k_vint?  One tile whose mirrors
// only the library reads (as for wr), with the 3-D part on (mode 2 has no aam).  POMGPU_AAM_NOFUSE (read here, at launch time) keeps the
// pair; the fp32-arithmetic variant keeps it at build time (POMGPU_AAM_FUSE).  The spare array is allocated here the first time
static bool aam_fused(pomgpu_ctx *c) {
  if (!POMGPU_AAM_FUSE || c->exch || c->tp.on || c->wide.on || c->parent || (c->flags & POMGPU_CTX_2D) || c->wr_eager || c->P.mode == 2 ||
      SW(c, AAM_NOFUSE) || c->aam_spare_failed)
    return false;
  if (!c->aam_spare) {
    const size_t bytes = c->P.n3 * sizeof(pomgpu_st);
    if (hipMalloc((void **)&c->aam_spare, bytes) != hipSuccess) { (void)hipGetLastError(); c->aam_spare = NULL; c->aam_spare_failed = 1; return false; }
    (void)hipMemsetAsync(c->aam_spare, 0, bytes, c->stream);
  }
  return true;
}
static void uvf_materialize(pomgpu_ctx *c) {
  if (!c->uvf_pending) return;
  c->uvf_pending = 0;
  launch_uvf_copy(c);
}
static void restore_materialize(pomgpu_ctx *c) {
  c->uvm_valid = 0;                                           // whoever asks for materialised state may write u, v next (uploads, handed-out addresses, stand-alone entry points)
  side_join(c);                                               // whoever asks for materialised state also waits for the side stream
  rho_materialize(c);
  pomgpu_wr_materialize(c);
  uvf_materialize(c);
  aam_canonical(c);
  if (!c->rst_pending) return;
  c->rst_pending = 0;
  launch_restore_fields(c, c->rst_fold, c->rst_fnew);
}
static void ext_flush_deferred(pomgpu_ctx *c);
static void ext_canonical(pomgpu_ctx *c) {
  ext_flush_deferred(c);                                      // a substep pomgpu_mode_external is holding back for its partner
  if (!c->ext_parity) return;
  KP &P = c->P;
  for (int n = 0; n < POMGPU_NGEN; n++) launch_copy2(c, P.b2 + (size_t)X2_SLOT[n] * P.n2, c->alt2[n]);
  c->ext_parity = 0;
  ext_buffers(c);
}
static int ctx_create(pomgpu_ctx **out, const pomgpu_dims *d, int device, void *stream, int flags);
extern "C" int pomgpu_create(pomgpu_ctx **out, const pomgpu_dims *d, int device, void *stream) {
  return ctx_create(out, d, device, stream, 0);
}
static int ctx_create(pomgpu_ctx **out, const pomgpu_dims *d, int device, void *stream, int flags) {
  if (!out || !d) return POMGPU_EINVAL;
  *out = NULL;
  if (d->kb < 4 || d->kb > POMGPU_KBMAX || d->im < 5 || d->jm < 5 || d->im > d->im_local || d->jm > d->jm_local) {
    fprintf(stderr, "pomgpu_create: unsupported extents im=%d jm=%d kb=%d (need im,jm>=5, 4<=kb<=%d)\n", d->im, d->jm,
            d->kb, POMGPU_KBMAX);
    return POMGPU_EINVAL;
  }
  if ((size_t)d->im_local * d->jm_local * d->kb * sizeof(double) >= ((size_t)1 << 32)) {
    fprintf(stderr, "pomgpu_create: a 3-D array of this tile has %zu bytes; the column kernels address a level with 32-bit offsets "
                    "(< 4 GiB per array): split the domain into more tiles\n", (size_t)d->im_local * d->jm_local * d->kb * sizeof(double));
    return POMGPU_EINVAL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    fprintf(stderr, "pomgpu_create: no usable HIP device (count=%d, asked %d); the hot path has no CPU fallback\n", ndev,
            device);
    return POMGPU_ENODEV;
  }
  pomgpu_ctx *c = (pomgpu_ctx *)calloc(1, sizeof(pomgpu_ctx));
  if (!c) return POMGPU_ENOMEM;
  c->device = device;
  c->flags = flags;
  c->lbry_sides = POMGPU_SIDE_EAST | POMGPU_SIDE_SOUTH;
  if (hipSetDevice(device) != hipSuccess) { free(c); return POMGPU_EHIP; }
  KP &P = c->P;
  P.im = d->im; P.jm = d->jm; P.kb = d->kb; P.imm1 = d->im - 1; P.jmm1 = d->jm - 1; P.kbm1 = d->kb - 1; P.kbm2 = d->kb - 2;
  P.iml = d->im_local; P.jml = d->jm_local;
  P.W = d->n_west == -1; P.E = d->n_east == -1; P.S = d->n_south == -1; P.N = d->n_north == -1;
  P.n2 = (size_t)P.iml * P.jml; P.n3 = P.n2 * P.kb;
  // The arrays of blk3d are n3 doubles apart on the host.  On the device a padding may be put between them
  // (POMGPU_PAD3 = 4-KiB pages): at the benchmark size the arrays are an exact multiple of 16 MiB apart, so that the ~10
  // arrays a kernel reads at one (i,j,k) sit at the same offset of the memory interleave; upload / download copy
  // array by array then
  pomgpu_switches_read(c->sw);                                // the developer switches: once per context, never on the launch path
  {
    const long pages = SW(c, PAD3) ? SWV(c, PAD3) : 0;
    P.a3 = P.n3 + (pages > 0 ? (size_t)pages * 512 : 0);
  }
  set_band_geometry(P, c->sw);
  size_t off = 0; int s = 0;
#define BD_(name, shape) P.bdoff[s++] = off; off += BDN_##shape;
#define BDN_J ((size_t)P.jml)
#define BDN_I ((size_t)P.iml)
#define BDN_JK ((size_t)P.jml * P.kb)
#define BDN_IK ((size_t)P.iml * P.kb)
  POM_BDRY(BD_)
#undef BD_
  const size_t nbd = off;
  c->con.error_status = 0;
  if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
  else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { free(c); return POMGPU_EHIP; }
    c->own_stream = true;
  }
  c->cur = c->stream;
  c->prof_state = new ProfState();
  PS(c)->filter[0] = 0;
  bool ok = true;
  auto alloc = [&](double **p, size_t n) {
    if (!ok) return;
    if (hipMalloc((void **)p, n * sizeof(double)) != hipSuccess) { ok = false; *p = NULL; return; }
    if (hipMemsetAsync(*p, 0, n * sizeof(double), c->stream) != hipSuccess) ok = false;
  };
  alloc(&P.b1, (size_t)POM_NBLK1D * P.kb);
  alloc(&P.r1, (size_t)POM_NBLK1D * P.kb);
  alloc(&P.b2, (size_t)POM_NBLK2D * P.n2);
  const bool only2d = (flags & POMGPU_CTX_2D) != 0;
  if (!only2d) alloc(&P.b3, (size_t)POM_NBLK3D * P.a3);
  alloc(&P.bd, nbd);
  for (int n = 0; n < POMGPU_NSCR3 && !only2d; n++) alloc(&P.s3[n], P.n3);
  for (int n = 0; n < POMGPU_NSCR2; n++) alloc(&P.s2[n], P.n2);
  for (int n = 0; n < 2 && !only2d; n++) alloc(&c->uvb_bot[n], P.n2);
  if (!only2d) {                                              // round trips read only where bits change: 8 bytes per (level <= kbm1, row, 62 columns), 4 per column
    double *m = NULL; alloc(&m, (size_t)(P.kb > 1 ? P.kb - 1 : 1) * P.jml * RT_NBX(P)); c->rt_words = (unsigned long long *)m;
    m = NULL; alloc(&m, (P.n2 + 1) / 2); c->rt_cols = (unsigned *)m;
  }
  for (int n = 0; n < POMGPU_NCOEF2; n++) alloc(&P.c2[n], P.n2);
  alloc(&c->alt2[0], (size_t)POMGPU_NGEN * P.n2);              // ONE block: a kernel reaches the whole set through one buffer descriptor (k_ext_march2)
  for (int n = 1; n < POMGPU_NGEN && ok; n++) c->alt2[n] = c->alt2[0] + (size_t)n * P.n2;
  { double *m = NULL; alloc(&m, (P.n2 + 7) / 8 + 1); P.m8 = (unsigned char *)m; }
  for (int n = 0; n < 2; n++) {
    const size_t len = (size_t)(P.kb + 1) * (n == 0 ? P.jml : P.iml);
    alloc(&c->ord_send[n], len);
    alloc(&c->ord_recv[n], len);
  }
  if (ok) { P.g4[2] = c->ord_recv[0]; P.g4[0] = c->ord_recv[0] + P.jml; P.g4[3] = c->ord_recv[1]; P.g4[1] = c->ord_recv[1] + P.iml; }
  alloc(&c->d_vel, 4);
  alloc(&c->d_stats, 8);
  if (ok && hipMalloc((void **)&c->d_err, sizeof(int)) != hipSuccess) ok = false;
  if (ok && hipMalloc((void **)&c->d_areas, sizeof(int)) != hipSuccess) ok = false;
  if (ok && hipMemsetAsync(c->d_areas, 0, sizeof(int), c->stream) != hipSuccess) ok = false;
  if (ok && hipMemsetAsync(c->d_err, 0, sizeof(int), c->stream) != hipSuccess) ok = false;
  if (SW(c, DEBUG_ALLOC))
    fprintf(stderr, "pomgpu_create: b1 %p r1 %p b2 %p b3 %p bd %p s3[0] %p s3[4] %p s2[0] %p c2[0] %p\n", (void *)P.b1, (void *)P.r1, (void *)P.b2,
            (void *)P.b3, (void *)P.bd, (void *)P.s3[0], (void *)P.s3[4], (void *)P.s2[0], (void *)P.c2[0]);
  if (!ok) {
    fprintf(stderr, "pomgpu_create: device allocation failed (%zu MB per 3-D array)\n", P.n3 * 8 >> 20);
    pomgpu_destroy(c);
    return POMGPU_ENOMEM;
  }
  c->ext_parity = 0;
  c->rst_pending = 0;
  ext_buffers(c);
  aam_buffers(c);
  (void)hipStreamSynchronize(c->stream);
  *out = c;
  return POMGPU_OK;
}

static void wide_free(pomgpu_ctx *c);
extern "C" void pomgpu_destroy(pomgpu_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->side) (void)hipStreamSynchronize(c->side);
  if (pomgpu_io_wait(c) != POMGPU_OK)                          // nobody is left to hand the status to: say it (error_status dies with the context)
    fprintf(stderr, "pomgpu_destroy: the output / restart file still being written could not be completed -- call pomgpu_io_wait (or pomgpu_sync) "
                    "before pomgpu_destroy to get its status\n");
  wide_free(c);
  pomgpu_tp_free(c);
  pomgpu_ff_free(c);
  KP &P = c->P;
  (void)hipFree(P.r1);
  if (c->tune_block) {                                        // pomgpu_tune_placement: blk3d and the scratch arrays are pieces of one allocation
    (void)hipFree(c->tune_block);
    c->tune_block = NULL; P.b3 = NULL;
    for (int n = 0; n < POMGPU_NSCR3; n++) P.s3[n] = NULL;
  }
  (void)hipFree(P.b1); (void)hipFree(P.b2); (void)hipFree(P.b3); (void)hipFree(P.bd);
  for (int n = 0; n < POMGPU_NSCR3; n++) (void)hipFree(P.s3[n]);
  for (int n = 0; n < POMGPU_NSCR2; n++) (void)hipFree(P.s2[n]);
  (void)hipFree(c->uvb_bot[0]); (void)hipFree(c->uvb_bot[1]);
  (void)hipFree(c->rt_words); (void)hipFree(c->rt_cols);
  (void)hipFree(c->aam_spare);
  for (int n = 0; n < POMGPU_NCOEF2; n++) (void)hipFree(P.c2[n]);
  (void)hipFree(c->alt2[0]); (void)hipFree(c->alt3[0]);         // one block each
  (void)hipFree(P.m8);
  for (int n = 0; n < 2; n++) { (void)hipFree(c->ord_send[n]); (void)hipFree(c->ord_recv[n]); }
  for (int n = 0; n <= POMGPU_MAXREC; n++) { (void)hipFree(c->rec_t[n]); (void)hipFree(c->rec_s[n]); (void)hipFree(c->rec_tau[n]); }
  (void)hipFree(c->d_vel); (void)hipFree(c->d_err); (void)hipFree(c->d_areas); (void)hipFree(c->d_stats); (void)hipFree(c->ext_bar);
  for (int k = 0; k < 3; k++) for (int sl = 0; sl < 4; sl++) { (void)hipFree(c->frc_dev[k][sl][0]); (void)hipFree(c->frc_dev[k][sl][1]); }
  for (int sl = 0; sl < 4; sl++) { (void)hipFree(c->lat_dev[sl]); (void)hipFree(c->wat_dev[sl]); }
  (void)hipFree(c->mean_acc);
  tracers_free(c);
  floats_free(c);
  tides_free(c);
  ProfState *ps = PS(c);
  if (ps) {
    for (auto &p : ps->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto &p : ps->free_) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    delete ps;
  }
  if (c->side) {
    (void)hipEventDestroy(c->ev_fork); (void)hipEventDestroy(c->ev_early);
    for (auto &e : c->side_ev) (void)hipEventDestroy(e.ev);
    (void)hipStreamDestroy(c->side);
  }
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  free(c);
}

// One developer switch of one context, after its creation (pomgpu_internal.hpp: POMGPU_SWITCHES).  name with or without the
// "POMGPU_" prefix; value NULL clears it, anything else sets it (numbers are read with atol).  For tools and tests only.
extern "C" int pomgpu_debug_switch(pomgpu_ctx *c, const char *name, const char *value) {
  if (!c || !name) return POMGPU_EINVAL;
  if (strncmp(name, "POMGPU_", 7) == 0) name += 7;
  for (int n = 0; n < SW__count; n++)
    if (strcmp(POMGPU_SW_NAMES[n], name) == 0) {
      pomgpu_ctx *two[2] = {c, c->wide.x};
      for (pomgpu_ctx *t : two)
        if (t) { t->sw.on[n] = value ? 1 : 0; t->sw.val[n] = value ? atol(value) : 0; }
      if (n == SW_AAM_NOFUSE) aam_canonical(c);               // the pair reads and writes aam in its slot
      return POMGPU_OK;
    }
  return fail(c, POMGPU_EINVAL, "debug_switch: no switch named %s", name);
}
extern "C" const char *pomgpu_last_error(const pomgpu_ctx *c) { return c ? c->err : "null context"; }
extern "C" void *pomgpu_stream(pomgpu_ctx *c) { return c ? (void *)c->stream : NULL; }
extern "C" void *pomgpu_current_stream(pomgpu_ctx *c) { return c ? (void *)c->cur : NULL; }

static int pull_err(pomgpu_ctx *c) {
  if (c->launch_err) return POMGPU_EHIP;                      // message already in last_error
  int e = 0;
  HIPCHK(c, hipMemcpyAsync(&e, c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (e) c->con.error_status = 1;
  if (e & POMGPU_DERR_BARRIER) {
    // k_ext_loop (opt-in) gave up at its grid barrier.  Its abort word is sticky and its arrival counter is out of step then:
    // clear both and keep this context off that path (a shared or oversubscribed GPU does not guarantee that all workgroups
    // are resident, which the barrier needs).  A velocity violation (POMGPU_DERR_VELOCITY) leaves that path alone.
    pomgpu_ctx *two[2] = {c, c->wide.x};
    for (pomgpu_ctx *t : two)
      if (t && t->ext_bar) {
        (void)hipMemsetAsync(t->ext_bar, 0, 2 * sizeof(unsigned), c->stream);
        t->ext_bar_base = 0;
        t->ext_loop_off = 1;
      }
  }
  return POMGPU_OK;
}
extern "C" int pomgpu_sync(pomgpu_ctx *c) {
  if (!c) return POMGPU_EINVAL;
  side_join(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  { const int rio = pomgpu_io_wait(c); if (rio) return rio; }
  return c->launch_err ? POMGPU_EHIP : POMGPU_OK;
}

// ---- state transfer ----------------------------------------------------------------------------
extern "C" int pomgpu_set_con(pomgpu_ctx *c, const pom_blkcon *con, int lramp) {
  if (!c || !con) return POMGPU_EINVAL;
  if (c->wr_pending && con->dti2 != c->P.dti2) pomgpu_wr_materialize(c);   // the pending wr is the old dti2's
  c->con = *con;
  c->lramp = lramp;
  sync_scalars(c);
  return POMGPU_OK;
}
extern "C" int pomgpu_get_con(pomgpu_ctx *c, pom_blkcon *con) {
  if (!c || !con) return POMGPU_EINVAL;
  int rc = pull_err(c);
  if (rc) return rc;
  *con = c->con;
  return POMGPU_OK;
}
// masks must be exactly 0 or 1: the kernels fold repeated mask multiplies (k_bc.hip)
static int check_masks(pomgpu_ctx *c, const double *blk2d) {
  const int slots[3] = {P2_fsm, P2_dum, P2_dvm};
  for (int s = 0; s < 3; s++) {
    const double *m = blk2d + (size_t)slots[s] * c->P.n2;
    for (size_t n = 0; n < c->P.n2; n++)
      if (m[n] != 0. && m[n] != 1.) return fail(c, POMGPU_EINVAL, "mask array (blk2d slot %d) holds a value other than 0/1", slots[s]);
  }
  return POMGPU_OK;
}
static void refresh_coefs(pomgpu_ctx *c);
extern "C" int pomgpu_upload(pomgpu_ctx *c, const double *b1, const double *b2, const double *b3, const double *bd,
                             const pom_blkcon *con, int lramp) {
  if (!c) return POMGPU_EINVAL;
  KP &P = c->P;
  HIPCHK(c, hipSetDevice(c->device));
  ext_canonical(c);
  restore_materialize(c);
  c->wide.static_done = 0;                                    // the extended tile's copy of the grid metrics is stale
  early_invalidate(c);                                        // ... and so is whatever an early gather has already moved
  if (b2) { int rc = check_masks(c, b2); if (rc) return rc; }
  if (b1) HIPCHK(c, hipMemcpyAsync(P.b1, b1, sizeof(double) * POM_NBLK1D * P.kb, hipMemcpyHostToDevice, c->stream));
  if (b2) HIPCHK(c, hipMemcpyAsync(P.b2, b2, sizeof(double) * POM_NBLK2D * P.n2, hipMemcpyHostToDevice, c->stream));
  if (b3) {
    pomgpu_tau_touched(c, 0); pomgpu_tau_touched(c, 1);         // taurstrb, taurstrf are the caller's now
#ifndef POMGPU_STORE_F32
    if (P.a3 == P.n3) HIPCHK(c, hipMemcpyAsync(P.b3, b3, sizeof(double) * POM_NBLK3D * P.n3, hipMemcpyHostToDevice, c->stream));
    else
#endif
    for (int n = 0; n < POM_NBLK3D; n++) {
      const int rc3 = copy3_h2d(c, SLOT3(c, n), b3 + (size_t)n * P.n3);
      if (rc3) return rc3;
#ifdef POMGPU_STORE_F32
      HIPCHK(c, hipStreamSynchronize(c->stream));             // one staging array
#endif
    }
  }
  if (bd) {
    const size_t nbd = P.bdoff[PB__count - 1] + (size_t)P.iml * P.kb;
    HIPCHK(c, hipMemcpyAsync(P.bd, bd, sizeof(double) * nbd, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (con) {
    pomgpu_set_con(c, con, lramp);
    HIPCHK(c, hipMemsetAsync(c->d_err, 0, sizeof(int), c->stream));
  }
  if (b2) refresh_coefs(c);
  return POMGPU_OK;
}
extern "C" int pomgpu_download(pomgpu_ctx *c, double *b1, double *b2, double *b3, double *bd, pom_blkcon *con) {
  if (!c) return POMGPU_EINVAL;
  KP &P = c->P;
  HIPCHK(c, hipSetDevice(c->device));
  ext_canonical(c);
  restore_materialize(c);
  if (b1) HIPCHK(c, hipMemcpyAsync(b1, P.b1, sizeof(double) * POM_NBLK1D * P.kb, hipMemcpyDeviceToHost, c->stream));
  if (b2) HIPCHK(c, hipMemcpyAsync(b2, P.b2, sizeof(double) * POM_NBLK2D * P.n2, hipMemcpyDeviceToHost, c->stream));
  if (b3) {
#ifndef POMGPU_STORE_F32
    if (P.a3 == P.n3) HIPCHK(c, hipMemcpyAsync(b3, P.b3, sizeof(double) * POM_NBLK3D * P.n3, hipMemcpyDeviceToHost, c->stream));
    else
#endif
    for (int n = 0; n < POM_NBLK3D; n++) {
      const int rc3 = copy3_d2h(c, b3 + (size_t)n * P.n3, SLOT3(c, n));
      if (rc3) return rc3;
    }
  }
  if (bd) {
    const size_t nbd = P.bdoff[PB__count - 1] + (size_t)P.iml * P.kb;
    HIPCHK(c, hipMemcpyAsync(bd, P.bd, sizeof(double) * nbd, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (con) return pomgpu_get_con(c, con);
  return POMGPU_OK;
}
// derived 2-D coefficient arrays follow the uploaded metrics / depths
static void refresh_coefs(pomgpu_ctx *c) {
  c->areas_checked = 0;                                       // dx, dy, art, aru, arv may have changed
  launch_coef_static(c);
  launch_coef_dt(c);
  launch_coef_eta(c);
}
#define SLOTCHK(c, s, n) if (!(c) || (s) < 0 || (s) >= (n)) return POMGPU_EINVAL; ext_canonical(c); restore_materialize(c)
static bool wide_travels_every_step(int slot2d);
extern "C" int pomgpu_upload_2d(pomgpu_ctx *c, int s, const double *h) {
  SLOTCHK(c, s, POM_NBLK2D);
  if (s == P2_fsm || s == P2_dum || s == P2_dvm)               // the kernels fold mask multiplies: 0/1 only, as io_pnetcdf.F derives them
    for (size_t n = 0; n < c->P.n2; n++)
      if (h[n] != 0. && h[n] != 1.) return fail(c, POMGPU_EINVAL, "mask array (blk2d slot %d) holds a value other than 0/1", s);
  HIPCHK(c, hipMemcpyAsync(SLOT2(c, s), h, sizeof(double) * c->P.n2, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!wide_travels_every_step(s)) c->wide.static_done = 0;   // e.g. forcing fields uploaded every step are gathered every step anyway
  early_invalidate(c);
  refresh_coefs(c);
  return POMGPU_OK;
}
extern "C" int pomgpu_upload_3d(pomgpu_ctx *c, int s, const double *h) {
  SLOTCHK(c, s, POM_NBLK3D);
  if (s == P3_taurstrb) pomgpu_tau_touched(c, 0);
  if (s == P3_taurstrf) pomgpu_tau_touched(c, 1);
  { const int rc3 = copy3_h2d(c, SLOT3(c, s), h); if (rc3) return rc3; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return POMGPU_OK;
}
extern "C" int pomgpu_download_2d(pomgpu_ctx *c, int s, double *h) {
  SLOTCHK(c, s, POM_NBLK2D);
  HIPCHK(c, hipMemcpyAsync(h, SLOT2(c, s), sizeof(double) * c->P.n2, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return POMGPU_OK;
}
extern "C" int pomgpu_download_3d(pomgpu_ctx *c, int s, double *h) {
  SLOTCHK(c, s, POM_NBLK3D);
  { const int rc3 = copy3_d2h(c, h, SLOT3(c, s)); if (rc3) return rc3; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return POMGPU_OK;
}
extern "C" double *pomgpu_device_2d(pomgpu_ctx *c, int s) {
  if (!c || s < 0 || s >= POM_NBLK2D) return NULL;
  ext_canonical(c);
  pomgpu_wr_materialize(c);                                   // a pending wr reads et, etb, dt: the caller may write them through the address it gets
  c->wr_eager = 1;
  c->areas_checked = 0;                                       // the caller may write through the address it gets
  return SLOT2(c, s);
}
extern "C" double *pomgpu_device_3d(pomgpu_ctx *c, int s) {
  if (!c || s < 0 || s >= POM_NBLK3D) return NULL;
  restore_materialize(c);
  c->wr_eager = 1;                                            // reads of wr (and writes of w, u, v) the library no longer sees: realvertvl ends every step from now on
  c->dev3_handed = 1;                                         // pomgpu_tune_placement would leave this address dangling: it refuses from now on (pomgpu.h)
  if (s == P3_taurstrb || s == P3_taurstrf) {                 // the caller may write the rate through the address at any time: k_ts_update reads both arrays from now on
    c->tau_handed = 1;
    pomgpu_tau_touched(c, s == P3_taurstrf);
  }
  return SLOT3(c, s);
}
extern "C" int pomgpu_bind_host(pomgpu_ctx *c, const double *h2, const double *h3) {
  if (!c) return POMGPU_EINVAL;
  c->host2 = h2;
  c->host3 = h3;
  return POMGPU_OK;
}
extern "C" int pomgpu_set_restore_record(pomgpu_ctx *c, int n, const double *tr, const double *sr) {
  if (!c || n < 1 || n > POMGPU_MAXREC || !tr || !sr) return POMGPU_EINVAL;
  if (pomgpu_ff_has(c, 2)) return fail(c, POMGPU_EINVAL, "set_restore_record: the restore records come from a file (pomgpu_set_forcing_files)");
  const size_t cnt = (size_t)c->P.im * c->P.jm * c->P.kb;
  if (!c->rec_t[n]) {
    HIPCHK(c, hipMalloc((void **)&c->rec_t[n], cnt * sizeof(double)));
    HIPCHK(c, hipMalloc((void **)&c->rec_s[n], cnt * sizeof(double)));
  }
  HIPCHK(c, hipMemcpyAsync(c->rec_t[n], tr, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->rec_s[n], sr, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return POMGPU_OK;
}
extern "C" int pomgpu_set_restore_rate_record(pomgpu_ctx *c, int n, const double *tau) {
  if (!c || n < 1 || n > POMGPU_MAXREC || !tau) return POMGPU_EINVAL;
  if (pomgpu_ff_has(c, 3)) return fail(c, POMGPU_EINVAL, "set_restore_rate_record: the restore rate comes from a file (pomgpu_set_restore_rate_file)");
  const size_t cnt = (size_t)c->P.im * c->P.jm * c->P.kb;
  if (!c->rec_tau[n]) HIPCHK(c, hipMalloc((void **)&c->rec_tau[n], cnt * sizeof(double)));
  HIPCHK(c, hipMemcpyAsync(c->rec_tau[n], tau, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->tau_gen++;                                               // what an array was made from under this number before is not this record
  return POMGPU_OK;
}
extern "C" int pomgpu_set_exchange(pomgpu_ctx *c, pomgpu_exchange_fn fn, void *user) {
  if (c && fn) { F32_REFUSE(c, "set_exchange"); }
  if (!c) return POMGPU_EINVAL;
  if (fn) pomgpu_wr_materialize(c);                           // while forming it still needs no message round
  c->exch = fn;
  c->exch_user = user;
  return POMGPU_OK;
}
extern "C" int pomgpu_set_order_exchange(pomgpu_ctx *c, pomgpu_order_fn fn, void *user) {
  if (!c) return POMGPU_EINVAL;
  c->order = fn;
  c->order_user = user;
  return POMGPU_OK;
}

extern "C" int pomgpu_halo_pack(pomgpu_ctx *c, double *const *dev, const int *nz, int count, int dir, double *to_lo, double *to_hi) {
  if (!c || !dev || !nz || (dir != 0 && dir != 1)) return POMGPU_EINVAL;
  return launch_halo_pack(c, dev, nz, count, dir, to_lo, to_hi) ? fail(c, POMGPU_EINVAL, "halo_pack: bad array list") : POMGPU_OK;
}
extern "C" int pomgpu_halo_unpack(pomgpu_ctx *c, double *const *dev, const int *nz, int count, int dir, const double *from_lo,
                                  const double *from_hi) {
  if (!c || !dev || !nz || (dir != 0 && dir != 1)) return POMGPU_EINVAL;
  return launch_halo_unpack(c, dev, nz, count, dir, from_lo, from_hi) ? fail(c, POMGPU_EINVAL, "halo_unpack: bad array list") : POMGPU_OK;
}
extern "C" int pomgpu_halo_pack8(pomgpu_ctx *c, double *const *dev, const int *nz, int count, double *const *to) {
  if (!c || !dev || !nz || !to) return POMGPU_EINVAL;
  return launch_halo_pack8(c, dev, nz, count, to) ? fail(c, POMGPU_EINVAL, "halo_pack8: bad array list") : POMGPU_OK;
}
extern "C" int pomgpu_halo_unpack8(pomgpu_ctx *c, double *const *dev, const int *nz, int count, const double *const *from) {
  if (!c || !dev || !nz || !from) return POMGPU_EINVAL;
  return launch_halo_unpack8(c, dev, nz, count, from) ? fail(c, POMGPU_EINVAL, "halo_unpack8: bad array list") : POMGPU_OK;
}

// host address of a COMMON array -> device mirror (Fortran passes array actuals by reference)
static double *dev3(pomgpu_ctx *c, const double *host) {
  if (!c->host3 || !host) return NULL;
  const ptrdiff_t off = host - c->host3;
  if (off < 0 || (size_t)off >= (size_t)POM_NBLK3D * c->P.n3 || (size_t)off % c->P.n3) return NULL;
  // an array argument of a stand-alone entry point may be written (ztosig's t, dens's rhoo, advt's ff ...): a rate array among them is no longer the library's
  if ((size_t)off / c->P.n3 == P3_taurstrb) pomgpu_tau_touched(c, 0);
  if ((size_t)off / c->P.n3 == P3_taurstrf) pomgpu_tau_touched(c, 1);
  return SLOT3(c, (size_t)off / c->P.n3);
}
static double *dev2(pomgpu_ctx *c, const double *host) {
  if (!c->host2 || !host) return NULL;
  const ptrdiff_t off = host - c->host2;
  if (off < 0 || (size_t)off >= (size_t)POM_NBLK2D * c->P.n2 || (size_t)off % c->P.n2) return NULL;
  return c->P.b2 + off;
}

// ---- halo exchange points ---------------------------------------------------------------------
static void xch(pomgpu_ctx *c, int count, ...) {
  if (!c->exch) return;   // single tile: every neighbour is -1 (parallel_mpi.f:171)
  double *ptr[8];
  int nz[8];
  va_list ap;
  va_start(ap, count);
  for (int n = 0; n < count; n++) { ptr[n] = va_arg(ap, double *); nz[n] = va_arg(ap, int); }
  va_end(ap);
  c->exch(c->exch_user, ptr, nz, count);
}

// ---- sequences (each mirrors one reference subroutine) ----------------------------------------
static void seq_advave(pomgpu_ctx *c) {                       // solver.f:6-198
  KP &P = c->P;
  if (!c->exch && P.mode != 2) { launch_advave_fused(c); return; }   // one tile: nothing to exchange, the fluxes stay in registers
  launch_advave_a(c);
  xch(c, 2, P.s2[0], 1, P.s2[1], 1);                          // :60-61
  launch_advave_b(c);
  xch(c, 3, D2(c, advua), 1, D2(c, fluxua), 1, D2(c, fluxva), 1);   // :70, :111-112
  launch_advave_c(c);
  xch(c, 1, D2(c, advva), 1);                                 // :121
  if (P.mode == 2) {
    launch_advave_m2a(c);
    xch(c, 1, P.s2[2], 1);                                    // :153
    launch_advave_m2b(c);
  }
}
static void seq_advct(pomgpu_ctx *c, int sum2d = 0, int defer_xch = 0, double *aam_w = NULL) {   // solver.f:201-408
  KP &P = c->P;
  if (!c->exch) {                                             // one tile: nothing to exchange, fluxes stay in registers
    launch_advct_col(c, sum2d, aam_w);                        // aam_w (lateral_viscosity): the new aam and aam2d as well
    c->uvm_valid = POMGPU_UVM_ONLOAD && !c->tp.on && !c->wide.on && !(c->flags & POMGPU_CTX_2D);   // ... and the depth sums of u, v are left for mode_internal
    return;
  }
  if (c->tp.on && !SW(c, ADVCT_SPLIT)) {            // tiles, the library's own exchange: see k_advct_edge
    pomgpu_transport &T = c->tp;
    const size_t ne = 2 * (size_t)P.kbm1 * P.jm, nn = 2 * (size_t)P.kbm1 * P.im;
    const size_t sc[8] = {0, T.nbr[1] >= 0 ? ne : 0, 0, T.nbr[3] >= 0 ? nn : 0, 0, 0, 0, 0};
    const size_t rc[8] = {T.nbr[0] >= 0 ? ne : 0, 0, T.nbr[2] >= 0 ? nn : 0, 0, 0, 0, 0, 0};
    // rim round R1: the lines and their round on the side stream, beside the column kernel (which does not read them); the side
    // stream's staging buffers hold them until k_advct_fix has run (the next side round forks off the main stream behind it)
    const bool side = rim_side(c);                            // (pomgpu_set_wide_external sized the side stream's buffers for any exchange point)
    double *const *snd = side ? T.send2 : T.send, *const *rcv = side ? T.recv2 : T.recv;
    if (side) side_begin(c);
    launch_advct_edge(c, T.nbr[1] >= 0 ? snd[1] : NULL, T.nbr[3] >= 0 ? snd[3] : NULL);
    const int rcm = side ? pomgpu_tp_move_side(c, sc, rc) : pomgpu_tp_move(c, sc, rc);
    if (side) side_end(c, c->side_ev[SIDE_R1].ev);
    if (rcm) return;
    launch_advct_col(c, sum2d);
    if (side) (void)hipStreamWaitEvent(c->stream, c->side_ev[SIDE_R1].ev, 0);
    launch_advct_fix(c, T.nbr[0] >= 0 ? rcv[0] : NULL, T.nbr[2] >= 0 ? rcv[2] : NULL);
    if (sum2d) launch_advct_fix2d(c, T.nbr[0] >= 0, T.nbr[2] >= 0);
    if (!defer_xch) xch(c, 2, D3(c, advx), P.kb, D3(c, advy), P.kb);   // :315, :405
    return;
  }
  launch_advct_a(c);
  xch(c, 2, P.s3[0], P.kbm1, P.s3[1], P.kbm1);                // :229, :279
  launch_advct_b(c);
  xch(c, 2, D3(c, advx), P.kb, P.s3[4], P.kbm1);              // :315, :369
  launch_advct_c(c);
  xch(c, 1, D3(c, advy), P.kb);                               // :405
}
// defer_rt (pomgpu_advance, mode 3): the in-place round trip rho = rho - rmean ... rho = rho + rmean (:854 + :937) changes
// the stored rho by a rounding.  Before dens rewrites rho at the end of the same step only profq reads it, so the three
// array passes of k_roundtrip are replaced by one extra read of rmean inside k_profq; level kb, which dens does not
// write, makes its round trip here.  Anything else that wants rho first gets it materialised (rho_materialize).
// cols: k_baropg_rs has just written the column plane for this rho, rmean (rt_cols)
static void seq_rho_roundtrip(pomgpu_ctx *c, int defer_rt, int cols = 0) {
  if (defer_rt) {
    launch_roundtrip_level(c, D3(c, rho), D3(c, rmean), c->P.kb);
    c->rho_rt_pending = 1;
    c->rho_rt_cols = cols;
  } else {
    launch_roundtrip(c, D3(c, rho), D3(c, rmean), 0);
  }
}
static void seq_baropg(pomgpu_ctx *c, int sum2d = 0, int defer_rt = 0) {        // solver.f:848-940
  const int cols = launch_baropg(c, sum2d, (defer_rt && rt_one_tile(c)) ? c->rt_cols : NULL);
  seq_rho_roundtrip(c, defer_rt, cols);                       // :854 + :937
}
static void seq_baropg_mcc(pomgpu_ctx *c, int sum2d = 0, int defer_rt = 0) {    // solver.f:943-1159
  KP &P = c->P;
  if (c->order) {                                             // :958-959 order2d_mpi(d), order3d_mpi(rho - rmean), one message per neighbour
    launch_order_pack(c, c->ord_send[0], c->ord_send[1]);
    c->order(c->order_user, c->ord_send[0], (P.kb + 1) * P.jml, c->ord_send[1], (P.kb + 1) * P.iml, c->ord_recv[0], c->ord_recv[1]);
  }
  launch_baropg_mcc(c, sum2d);
  seq_rho_roundtrip(c, defer_rt);                             // :954 + :1164
}
static void seq_advq(pomgpu_ctx *c, double *qb, double *q, double *qf, int pair, int zero_else) {   // solver.f:411-477
  KP &P = c->P;
  if (!c->exch) { launch_coef_eta(c); launch_advq_col(c, q, qb, qf, zero_else); return; }
  double *xf = P.s3[pair ? 2 : 0], *yf = P.s3[pair ? 3 : 1];
  launch_advq_flux(c, q, qb, xf, yf);
  xch(c, 2, xf, P.kbm1, yf, P.kbm1);                          // :458-459
  launch_advq_step(c, q, qb, qf, xf, yf, zero_else);
}
static void seq_profq(pomgpu_ctx *c, int fuse_filter = 0, int with_w = 0, int store_ld = 1) {   // solver.f:1212-1538
  KP &P = c->P;
  launch_profq_bc(c);
  double *ufkb = LEV3(c, D3(c, uf), P.kb - 1);
  const int lines = c->exch && c->tp.on && !SW(c, PROD_FULL);   // tiles, the library's own exchange
  if (lines) {
    // the production term's lines (k_profq_prod_lines) depend on nothing profq_bc or the exchange below delivers:
    // :1289-1290, :1374 (and advance.f:400 for w) travel in ONE round
    launch_profq_prod(c, 1, c->rho_rt_pending);
    if (with_w) xch(c, 4, P.s2[4], 1, ufkb, 1, LEV3(c, P.s3[0], 1), P.kbm2, D3(c, w), P.kb);
    else xch(c, 3, P.s2[4], 1, ufkb, 1, LEV3(c, P.s3[0], 1), P.kbm2);
    launch_profq(c, 2, fuse_filter, c->rho_rt_pending);       // owned columns form prod inside the solve
    return;
  }
  if (with_w) xch(c, 3, P.s2[4], 1, ufkb, 1, D3(c, w), P.kb);   // :1289-1290 + advance.f:400
  else xch(c, 2, P.s2[4], 1, ufkb, 1);                        // :1289-1290
  if (!c->exch) { launch_profq(c, 1, fuse_filter, c->rho_rt_pending, 0, -1, store_ld); return; }  // one tile: prod is formed inside the solve kernel
  launch_profq_prod(c, 0, c->rho_rt_pending);
  xch(c, 1, LEV3(c, P.s3[0], 1), P.kbm2);                          // :1374
  launch_profq(c, 0, fuse_filter, c->rho_rt_pending);
}
static void seq_fb_fix(pomgpu_ctx *c, double *fb, const double *fclim) {
  launch_copy_kb(c, fb);                                      // solver.f:496 / :618
  launch_roundtrip(c, fb, fclim, 0);                          // :511+:532 / :691+:715
}
static void seq_advt1(pomgpu_ctx *c, double *fb, double *f, const double *fclim, double *ff) {   // solver.f:480-574
  launch_advt1(c, fb, f, fclim, ff);
  seq_fb_fix(c, fb, fclim);
}
static void seq_advt2(pomgpu_ctx *c, double *fb, double *f, const double *fclim, double *ff, bool defer_roundtrip = false) {   // solver.f:577-731
  KP &P = c->P;
  if (P.nitera == 1) {
    launch_coef_eta(c);                                       // etb/etf are final once the external mode is done
    launch_advt2_rows(c, fb, f, fclim, ff);
  } else {
    launch_advt2_mass(c);
    const double *fbmem = fb, *eta = D2(c, etb);
    for (int itera = 1; itera <= P.nitera; itera++) {
      launch_advt2_step(c, fbmem, f, eta, ff, itera);
      xch(c, 1, ff, P.kbm1);                                  // :679
      launch_mask3(c, ff, D2(c, fsm));                        // :1898-1900
      launch_smol(c, ff);                                     // :1903-1964
      eta = D2(c, etf);                                       // :684-685
      launch_copy3(c, P.s3[3], ff);
      fbmem = P.s3[3];
    }
    launch_advt2_diff(c, fb, fclim, ff);                      // :691-726
  }
  xch(c, 1, ff, P.kbm1);                                      // :728
  if (defer_roundtrip) launch_copy_kb(c, fb);                 // :618; the round trip :691,:715 rides in k_ts_update
  else seq_fb_fix(c, fb, fclim);
}
// host half of restore_interior: record reads/shifts; returns the interpolation weights
static int restore_prepare(pomgpu_ctx *c, double *fold_out, double *fnew_out) {   // bounds_forcing.f:1034-1087
  const pom_blkcon &k = c->con;
  const double trst = 30.;
  const int irst = (int)(trst * 86400. / k.dti);
  const int ntime = (int)(k.time / trst);
  // One load of record n: "taurstrf = 1./trst" over the whole padded array as ever, then the rate that goes with T/S record n -- (a) a rate
  // file: record n's window mapped by k_ztosig straight into taurstrf, (b) a rate record n: taurstrf(1:im,1:jm,1:kb) = tau, (c) neither.
  // Whether every record is there is settled before a slot or a mirror is written.
  auto load = [&](int n) -> int {
    const int rfile = pomgpu_ff_has(c, 3), steady = rfile && pomgpu_ff_rate_steady(c);
    if (rfile) { const int rc = pomgpu_ff_rate_have(c, n); if (rc) return rc; }
    const double *tr, *sr;
    if (pomgpu_ff_has(c, 2)) {                                  // read_restore_ts_interior_pnetcdf(n, ...) from the file
      const int rc = pomgpu_ff_fetch_restore(c, n);
      if (rc) return rc;
      tr = c->rec_t[0]; sr = c->rec_s[0];
    } else {
      if (n < 1 || n > POMGPU_MAXREC || !c->rec_t[n])
        return fail(c, POMGPU_EINVAL, "restore_interior: record %d was not supplied (pomgpu_set_restore_record)", n);
      tr = c->rec_t[n]; sr = c->rec_s[n];
    }
    const double *taur = !rfile && n >= 1 && n <= POMGPU_MAXREC ? c->rec_tau[n] : NULL;
    const int keep = steady && c->rate_in_f && !c->tau_handed;  // the file's one record is in taurstrf already: the same bits
    launch_restore_load(c, tr, sr, 1. / trst, taur, !keep);
    if (rfile) {
      c->tau_known[1] = 0;
      if (!keep) {
        c->rate_in_f = 0; c->tau_id[1] = 0;
        const int rc = pomgpu_ff_fetch_rate(c, n);
        if (rc) return rc;
        c->rate_in_f = steady;
        c->tau_id[1] = (c->tau_gen << 32) | (long)(steady ? 1 : n + 1);
      }
    } else if (taur) {
      c->tau_known[1] = 0; c->rate_in_f = 0;
      c->tau_id[1] = (c->tau_gen << 32) | (long)(n + 1);
    } else {
      c->tau_known[1] = 1; c->tau_val[1] = 1. / trst;             // "taurstrf = 1./trst", the whole array
      c->tau_id[1] = 0; c->rate_in_f = 0;
    }
    return POMGPU_OK;
  };
  auto same = [&]() { c->tau_same = !c->tau_handed && !c->tau_known[0] && !c->tau_known[1] && c->tau_id[0] && c->tau_id[0] == c->tau_id[1]; };
  if (k.iint == 2) { c->tau_same = 0; int rc = load((k.iint / irst) + 1); if (rc) return rc; }
  if (k.iint == 2 || (irst > 0 && k.iint % irst == 0)) {
    c->tau_same = 0;
    launch_restore_shift(c);
    c->tau_known[0] = c->tau_known[1]; c->tau_val[0] = c->tau_val[1]; c->tau_id[0] = c->tau_id[1];
    if (k.iint != k.iend) { int rc = load((k.iint + irst) / irst + 1); if (rc) return rc; }
    same();
  }
  *fnew_out = k.time / trst - ntime;
  *fold_out = 1. - *fnew_out;
  return POMGPU_OK;
}
static int seq_restore_interior(pomgpu_ctx *c) {              // bounds_forcing.f:1023-1121
  double fold, fnew;
  const int rc = restore_prepare(c, &fold, &fnew);            // record reads / shifts, interpolation weights
  if (rc) return rc;
  launch_restore(c, fold, fnew);
  return POMGPU_OK;
}

// ---- the side stream --------------------------------------------------------------------------------------------------
// side_begin: what is enqueued from here on goes to the side stream, after everything the main stream holds so far;
// side_end(ev): back to the main stream; `ev` marks the end of the side work.  side_post(r): side_end on round r's event, and the main
// stream owes it a wait; side_wait(r): the main stream waits for round r if it still owes that.  side_join: ... for all of them.
static void side_begin(pomgpu_ctx *c) {
  (void)hipEventRecord(c->ev_fork, c->stream);
  (void)hipStreamWaitEvent(c->side, c->ev_fork, 0);
  c->cur = c->side;
  if (c->wide.x) c->wide.x->cur = c->side;
}
static void side_end(pomgpu_ctx *c, hipEvent_t ev) {
  (void)hipEventRecord(ev, c->side);
  c->cur = c->stream;
  if (c->wide.x) c->wide.x->cur = c->stream;
}
static void side_post(pomgpu_ctx *c, side_round r) {
  side_end(c, c->side_ev[r].ev);
  c->side_ev[r].pending = 1;
}
static void side_wait(pomgpu_ctx *c, side_round r) {
  if (!c->side_ev[r].pending) return;
  (void)hipStreamWaitEvent(c->stream, c->side_ev[r].ev, 0);
  c->side_ev[r].pending = 0;
}
// "The early part of this step's wide exchange has been posted" (early_started) is a fact about the MESSAGE PATTERN of the step:
// wide_begin posts the late part only while it holds, and every rank must post alike.  Joining the side stream therefore only
// waits; the flag falls when wide_begin has used it, or when something rewrites the arrays the early part carried (an upload:
// early_invalidate -- to be called on all ranks alike, like the upload itself).
static void side_join(pomgpu_ctx *c) {                        // everything the side stream holds, before the main stream goes on
  if (c->early_started) (void)hipStreamWaitEvent(c->stream, c->ev_early, 0);
  for (int r = 0; r < SIDE__count; r++) side_wait(c, (side_round)r);
}
// ---- rim rounds: exchange points on the side stream, beside the kernels of the main stream ------------------------------------------
// north_star: "halo exchange ... overlapped with interior stencil compute on a second HIP stream".  Four of the step's exchange points
// have a consumer that either does not need the ghost cells at once or needs them on the ghost lines only; their pack -> message round
// -> unpack run on the side stream over its own communicator and staging buffers, and the main stream waits for an event where the
// first reader of those ghost cells starts:
//   R1  advct's edge lines (seq_advct)                     beside k_advct_col; k_advct_fix waits
//   R2  advx, advy, aam (advance.f:137, solver.f:315,405)  beside the vertical integrals, the wide exchange and the whole external mode;
//                                                          mode_internal's 3-D part waits (aam2d's ghost lines follow the round, k_vint)
//   R7  wubot, wvbot, uf, vf (advance.f:466-467)           beside the Asselin filter, which leaves the ghost lines alone: there it ends in
//                                                          u = uf, v = vf (:511-514), written from the same message
//   R8  ub, vb, level kb of u, uf, v, vf (:516-521)        beside the 2-D tail, check_velocity and the NEXT step's baropg, which moves
//                                                          in front of advct for it; advct (the next reader of u, v) waits
// Three more exchange points of mode_internal have a consumer that needs the exchanged values on its GHOST lines only -- profq, proft and the
// Asselin filters run over all i, j, ghost lines included (solver.f:1650-1661, advance.f:416-421,444-449), each column from its own operands --
// and what they leave on a ghost line is what the neighbour computes on the line it owns: the same arithmetic on the same operands (that is
// the reference's own invariant; every operand of those columns is either exchanged or was computed this way before).  Instead of
// exchanging the INPUTS in front of the kernel (w + utau2 + uf(kb) + prod: solver.f:1289-1290,1374, advance.f:400; q2f / q2lf: :411-412;
// tf / sf: solver.f:728, advance.f:436-437) the RESULTS travel behind it:
//   Rw   w (advance.f:400)                                   beside advq and profq; the tracer advection (its first reader) waits
//   Rq   q2, q2b, q2l, q2lb, km, kh, kq, l, dtef             beside the tracer step; profu / profv (km of the neighbour line) wait
//   Rts  t, tb, s, sb, rho                                   beside advu ... the end of the step; the next step's baropg waits
// The kernels run on every line as before; what they make of a ghost line's stale operands is overwritten by the round.  k_profq forms
// its production term as on one tile (no lines kernel, no prod exchange).  More bytes (9 + 5 arrays x kb instead of ~6 x kb lines per
// neighbour), no round between kernels: of a full step's ten rounds only the late part of the wide exchange stays on the kernels' stream.
// POMGPU_RIM_RESULTS_MAIN keeps the reference's three input exchanges (on the kernels' stream).
// All ranks post the same rounds in the same order on either communicator: whether this path is taken depends on nothing but the
// agreed side stream (pomgpu_tp_side_ok) and the collective switch set (POMGPU_RIM_MAIN keeps the four rounds on the main stream).
// Each round's event and "the main stream has not waited yet" are entry SIDE_<round> of pomgpu_ctx::side_ev (R7 uses R8's event).
static int rim_side(pomgpu_ctx *c) { return c->tp.on && c->exch && c->wide.on && c->wide.split && !SW(c, RIM_MAIN); }
// One exchange point: pack8 towards the eight neighbours -> one message round -> unpack8 (parallel_mpi.f:154-351), all on one stream.
// side = 0: the main stream, the transport's first set of staging buffers.  side = 1: the side stream and its own set (the caller has
// called side_begin).  `dev2`, if given, is a second list of arrays of the same shapes that receive the same ghost values (u, v behind uf, vf)
static int round8(pomgpu_ctx *c, int side, double *const *dev, const int *nz, int count, double *const *dev2 = NULL) {
  const KP &P = c->P;
  pomgpu_transport &T = c->tp;
  const char *what = side ? "exchange (side stream)" : "exchange";
  double *const *snd = side ? T.send2 : T.send, *const *rcv = side ? T.recv2 : T.recv;
  const size_t *cap = side ? T.cap2 : T.cap;
  size_t total = 0;
  for (int a = 0; a < count; a++) total += (size_t)nz[a];
  const size_t len[8] = {(size_t)P.jm, (size_t)P.jm, (size_t)P.im, (size_t)P.im, 1, 1, 1, 1};
  size_t cnt[8];
  for (int d = 0; d < 8; d++) {
    cnt[d] = T.nbr[d] >= 0 ? total * len[d] : 0;
    if (cnt[d] > cap[d]) return fail(c, POMGPU_EINVAL, "%s: %zu doubles exceed the staging buffer", what, cnt[d]);
  }
  if (launch_halo_pack8(c, dev, nz, count, snd)) return fail(c, POMGPU_EINVAL, "%s: bad array list", what);
  const int rc = side ? pomgpu_tp_move_side(c, cnt, cnt) : pomgpu_tp_move(c, cnt, cnt);
  if (rc) return rc;
  (void)launch_halo_unpack8(c, dev, nz, count, rcv);
  if (dev2) (void)launch_halo_unpack8(c, dev2, nz, count, rcv);
  return POMGPU_OK;
}
// one rim round: the exchange point on the side stream, behind everything the main stream holds so far; the main stream owes side_wait(c, r)
static int rim_round(pomgpu_ctx *c, side_round r, double *const *dev, const int *nz, int count, double *const *dev2 = NULL) {
  side_begin(c);
  const int rc = round8(c, 1, dev, nz, count, dev2);
  side_post(c, r);
  return rc;
}
static void early_invalidate(pomgpu_ctx *c) {
  if (c->early_started) { (void)hipStreamWaitEvent(c->stream, c->ev_early, 0); c->early_started = 0; }
}
// the side stream and its events, created on first use; 1 = they exist
int pomgpu_side_stream(pomgpu_ctx *c) {
  if (c->side) return 1;
  if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess) { c->side = NULL; return 0; }
  bool ok = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&c->ev_early, hipEventDisableTiming) == hipSuccess;
  for (auto &e : c->side_ev) ok = ok && hipEventCreateWithFlags(&e.ev, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    (void)hipStreamDestroy(c->side);
    c->side = NULL;
    return 0;
  }
#ifdef POMGPU_EMU
  emu_stream_defer(c->side);                                  // tests: the side stream's work at the LATEST moment the device could run it (tests/emu/hip/hip_runtime.h)
#endif
  return 1;
}
#define NEED_RAW(c) if (!(c)) return POMGPU_EINVAL; if ((c)->broken) return POMGPU_EHIP; (void)hipSetDevice((c)->device)
static void wide_flush(pomgpu_ctx *c);
#define NEED_HOT(c) NEED_RAW(c); ext_canonical(c); wide_flush(c)   /* the entry points pomgpu_advance strings together */
#define NEED(c) NEED_HOT(c); side_join(c); restore_materialize(c)

// every lazily kept array brought up to date in the COMMON-block mirrors (the second generation of the external mode's arrays,
// the extended tile's 2-D state, work on the side stream, rho's deferred round trip, the restore fields): what anything that
// reads the mirrors directly -- the file writers' snapshot -- must call first
int pomgpu_materialize(pomgpu_ctx *c) {
  NEED(c);
  return POMGPU_OK;
}
// pomgpu_read_restart (cdf_in.hip) has written 2-D and 3-D mirrors with its own kernel: what pomgpu_upload_2d invalidates for
// those slots (none of them is a mask or a taurstr array; upload_3d invalidates nothing else)
void pomgpu_mirrors_written(pomgpu_ctx *c) {
  c->uvm_valid = 0;                                           // u, v are the file's now
  c->rho_rt_cols = 0;                                         // ... and rho (the reader has materialised a pending round trip before it wrote: no plane can be valid here)
  c->wide.static_done = 0;
  early_invalidate(c);
  refresh_coefs(c);
}
// pomgpu_cold_start (cdf_in.hip) has filled the grid, tb sb t s and tclim sclim: the rest of initial_conditions and update_initial
// (initialize.f:416-425, :472-518) in the reference's order, with the launchers the stand-alone entry points use; the two kernels of
// cdf_in.hip come in as functions.  Then what pomgpu_upload of all blocks invalidates.  The caller has vetted npg
void pomgpu_cold_tail(pomgpu_ctx *c, void (*update_initial)(pomgpu_ctx *), void (*sums)(pomgpu_ctx *)) {
  launch_dens(c, D3(c, sclim), D3(c, tclim), D3(c, rmean));
  launch_dens(c, D3(c, sb), D3(c, tb), D3(c, rho));
  update_initial(c);
  if (c->con.npg == 2) seq_baropg_mcc(c); else seq_baropg(c);
  sums(c);
  pomgpu_tau_touched(c, 0); pomgpu_tau_touched(c, 1);         // taurstrb, taurstrf are zero arrays now, not the library's value
  pomgpu_mirrors_written(c);
}
extern "C" int pomgpu_get_time(pomgpu_ctx *c) {               // advance.f:62-75
  NEED_HOT(c);
  pom_blkcon &k = c->con;
  k.time = k.dti * (double)(float)k.iint / 86400. + k.time0;
  if (k.iint >= k.iswtch) k.iprint = (int)lround(k.prtd2 * 24. * 3600. / k.dti);
  if (c->lramp) { k.ramp = k.time / k.period; if (k.ramp > 1.) k.ramp = 1.; }
  else k.ramp = 1.;
  sync_scalars(c);
  return POMGPU_OK;
}
// sum2d (pomgpu_advance on one tile): advct and baropg leave the vertical integrals that mode_interaction
// would otherwise gather by reading advx, advy, drhox, drhoy again (advance.f:152-168)
static int lateral_viscosity(pomgpu_ctx *c, int sum2d, int defer_rt = 0) {      // advance.f:96-141
  NEED_HOT(c);
  side_wait(c, SIDE_RTS);                                     // rho's ghost lines (rim round Rts of the step before; posted ahead of R8 on the same stream)
  rho_materialize(c);                                         // a deferred round trip no step has consumed (baropg reads rho)
  KP &P = c->P;
  c->aam2d_done = 0;
  if (P.mode != 2) {
    const bool lib_x = c->tp.on && c->exch && !SW(c, ADVCT_SPLIT);
    auto pressure_gradient = [&]() {
      if (P.npg == 1) seq_baropg(c, sum2d, defer_rt);
      else if (P.npg == 2) seq_baropg_mcc(c, sum2d, defer_rt);
      else {                                                  // advance.f:117-120
        fprintf(stderr, "\nError: invalid value for npg\n");
        c->con.error_status = 1;
      }
    };
    // rim round R8 of the step before (the ghost cells of u, v, ub, vb) may still be in flight: baropg reads none of them and
    // shares nothing with advct, so it goes first and advct waits
    const bool pg_first = c->side_ev[SIDE_R8].pending != 0;
    if (pg_first) pressure_gradient();
    side_wait(c, SIDE_R8);
    // aam and aam2d out of advct's march (one tile, inside a whole step: sum2d; the routine-by-routine entry points keep the pair).  The
    // march reads the current aam and writes the other buffer; the parity flips behind it
    const bool fuse = sum2d && aam_fused(c);
    if (!fuse) aam_canonical(c);                              // k_advct_col<*, false>, advct_a/b/c, k_aam_pair / k_aam work on the slot
    seq_advct(c, sum2d, lib_x, fuse ? (c->aam_parity ? SLOT3(c, P3_aam) : c->aam_spare) : NULL);   // lib_x: advx, advy travel with aam below
    if (!pg_first) pressure_gradient();
    if (fuse) { c->aam_parity ^= 1; aam_buffers(c); c->aam2d_done = 1; }
    else launch_aam(c);
    if (lib_x && sum2d && rim_side(c)) {                      // rim round R2: solver.f:315,405 + :137 on the side stream
      double *arr[3] = {D3(c, advx), D3(c, advy), D3(c, aam)};
      const int nz[3] = {P.kb, P.kb, P.kbm1};
      side_begin(c);                                          // (rim_round by hand: one more launch behind the round)
      const int rc2 = round8(c, 1, arr, nz, 3);
      if (!rc2) launch_vint(c, 1, -1);                        // aam2d on the ghost lines (advance.f:158-168), from the aam that has just arrived
      side_post(c, SIDE_R2);
      if (rc2) return rc2;
    }
    else if (lib_x) xch(c, 3, D3(c, advx), P.kb, D3(c, advy), P.kb, D3(c, aam), P.kbm1);   // solver.f:315,405 + :137 in one round
    else xch(c, 1, D3(c, aam), P.kbm1);                       // :137
  }
  return POMGPU_OK;
}
static int wide_early_start(pomgpu_ctx *c);
// The reference's own sequence (advance.f:14-21: surface_forcing, lateral_bc, lateral_viscosity, mode_interaction) gets the
// early part of the wide exchange beside lateral_viscosity like pomgpu_advance does: the step's forcing is in place when the
// host calls this.  What the early part has moved is NOT moved again: between this call and pomgpu_mode_interaction the host leaves the
// 2-D state alone (pomgpu.h says so); the two calls that may come in between -- pomgpu_upload, pomgpu_upload_2d, made by every rank
// alike -- end the early part's validity themselves (early_invalidate) and wide_begin then gathers everything in one round.
extern "C" int pomgpu_lateral_viscosity(pomgpu_ctx *c) {
  NEED_HOT(c);
  const int rc = wide_early_start(c);
  // rho's round trip stays a flag as in pomgpu_advance (same condition): k_profq of the pomgpu_mode_internal that follows applies it to
  // what it loads and dens rewrites rho; a caller that does anything else first gets it stored (rho_materialize: every NEED, the next call of this)
  const pom_blkcon &k0 = c->con;
  const int defer_rt = k0.mode == 3 && (k0.iint != 1 || k0.time0 != 0.) && !SW(c, RHO_ROUNDTRIP);
  return rc ? rc : lateral_viscosity(c, 0, defer_rt);
}
static int wide_begin(pomgpu_ctx *c);
static int mode_interaction(pomgpu_ctx *c, int sums_done) {   // advance.f:144-202
  NEED_HOT(c);
  if (c->wide.on) {                                           // one wide exchange instead of ~180 narrow ones
    // :152-168; while rim round R2 is in flight aam's ghost lines are not there yet: this launch leaves aam2d's alone, the side stream
    // fills them behind the round (lateral_viscosity)
    if (c->P.mode != 2) { aam_canonical(c); launch_vint(c, sums_done, sums_done && c->side_ev[SIDE_R2].pending ? 1 : 0); }
    return wide_begin(c);                                     // :170-199 on the extended tile
  }
  if (c->P.mode != 2) {
    // :152-168.  aam2d_done: this step's march has left all five integrals (lateral_viscosity); whoever comes here without it reads aam in its slot
    if (!(sums_done && c->aam2d_done)) { aam_canonical(c); launch_vint(c, sums_done); }
    seq_advave(c);
  }
  c->aam2d_done = 0;
  launch_modeint_tail(c);
  xch(c, 2, D2(c, utf), 1, D2(c, vtf), 1);                    // :198-199
  return POMGPU_OK;
}
// store_f: write elf, uaf, vaf on every substep (the public entry point: the caller may look at them);
// pomgpu_advance stores them on the last substep only -- nothing reads them in between
// Rows [1 + lo, jm - hi] of a tile as a tile of its own, same leading dimension: every blk2d array, the scratch and coefficient
// arrays, both generations, the mask bytes and the j-indexed boundary values begin `lo` rows later.
static KP row_window(const KP &P, int lo, int hi) {
  KP Q = P;
  const size_t sh = (size_t)lo * P.iml;
  Q.b2 += sh;
  for (int n = 0; n < POMGPU_NSCR2; n++) if (Q.s2[n]) Q.s2[n] += sh;
  for (int n = 0; n < POMGPU_NCOEF2; n++) if (Q.c2[n]) Q.c2[n] += sh;
  for (int n = 0; n < POMGPU_NGEN; n++) { Q.x2[n] += sh; Q.y2[n] += sh; }
  if (Q.m8) Q.m8 += sh;
  if (Q.tide_j) Q.tide_j += lo;                               // the tide's j-indexed lines, like the boundary values below
  int s = 0;
#define BD_(name, shape) Q.bdoff[s++] += BDW_##shape;
#define BDW_J ((size_t)lo)
#define BDW_I 0
#define BDW_JK 0
#define BDW_IK 0
  POM_BDRY(BD_)
#undef BD_
  Q.jm = P.jm - lo - hi; Q.jmm1 = Q.jm - 1; Q.jml = Q.jm;
  return Q;
}
static int mode_external(pomgpu_ctx *c, int store_f) {        // advance.f:205-353
  NEED_RAW(c);
  if (c->wide.on && c->wide.pending) {                        // the substep runs on the extended tile (wide_begin)
    pomgpu_ctx *x = c->wide.x;
    x->con.iext = c->con.iext;
    const int last = c->con.iext == c->con.isplit;
    const int rc = mode_external(x, store_f || last);
    if (last) wide_flush(c);                                  // the tile's arrays, ghost cells included, are current again
    return rc;
  }
  KP &P = c->P;
  P.iext = c->con.iext;
  if (!c->exch && !SW(c, EXT_SPLIT)) {              // one tile: one kernel per substep, two buffer generations
    // advave every substep (ispadv = 1 is hard-coded in the reference, initialize.f:156): it rides in the substep's kernel
    const int fuse_adv = c->con.ispadv == 1 && P.mode != 2 && !SW(c, ADVAVE_SEPARATE);
    if (!fuse_adv && c->con.ispadv > 0 && c->con.iext % c->con.ispadv == 0) seq_advave(c);   // :235 (reads ua, va, d of the current generation)
    KP Q = P;
    for (int n = 0; n < POMGPU_NGEN; n++) Q.y2[n] = c->ext_parity ? P.b2 + (size_t)X2_SLOT[n] * P.n2 : c->alt2[n];
    // once per internal step (and after any upload): are art, aru, arv what initialize.f:361-367 makes of dx, dy?  Then
    // k_ext_march forms them in registers instead of reading three arrays per substep.  On the device, no host round trip.
    if (fuse_adv && !c->areas_checked) { launch_check_areas(c); c->areas_checked = 1; }   // dx, dy, art, aru, arv change with an upload only (refresh_coefs)
    if (c->parent && !SW(c, WIDE_FULL)) {
      // The extended tile of the wide-halo mode: its stale rim grows by one line per substep (see "How far stale cells spread"
      // below), so substep n need not compute the n - 1 outermost rows of an extended side at all -- they are wrong already and
      // nobody reads them again.  The window's own outermost row is "the row an exchange would have filled", as the extended
      // tile's was.  (Rows only: a window in i would need a width apart from the leading dimension.)
      const pomgpu_wide &Wd = c->parent->wide;
      int cut = P.iext - 1 < Wd.w - 5 ? P.iext - 1 : Wd.w - 5;
      if (cut < 0) cut = 0;
      const int lo = Wd.oy > 0 ? cut : 0, hi = P.jm - c->parent->P.jm - Wd.oy > 0 ? cut : 0;
      if (lo + hi > 0 && P.jm - lo - hi >= 16) Q = row_window(Q, lo, hi);
    }
    launch_ext_step(c, Q, store_f || P.iext == P.isplit, fuse_adv);   // :211-347
    c->ext_parity ^= 1;
    ext_buffers(c);
    return POMGPU_OK;
  }
  ext_canonical(c);
  launch_ext_elf(c);                                          // :211-231
  xch(c, 1, D2(c, elf), 1);                                   // :233
  if (c->con.ispadv > 0 && c->con.iext % c->con.ispadv == 0) seq_advave(c);   // :235
  launch_ext_uvaf(c, 1);                                      // :237-290
  xch(c, 2, D2(c, uaf), 1, D2(c, vaf), 1);                    // :292-293
  launch_ext_update(c);                                       // :295-347
  if (P.iext != P.isplit) xch(c, 2, D2(c, utf), 1, D2(c, vtf), 1);   // :348-349
  return POMGPU_OK;
}
// Substeps iext and iext + 1 in one pass over memory (k_ext_march2, k_ext.hip): one tile -- or the extended tile of the wide-halo
// mode -- large enough for the marching kernels, inside pomgpu_advance only (the public pomgpu_mode_external leaves elf, uaf, vaf
// of EVERY substep in memory for its caller).  1 = both substeps done (c->con.iext = iext + 1), 0 = not applicable.
static int ext_pair_ok(pomgpu_ctx *c, int iext) {             // may substeps iext, iext + 1 share a pass?
  pomgpu_ctx *t = c;
  if (c->wide.on) { if (!c->wide.pending) return 0; t = c->wide.x; }
  else if (c->exch) return 0;
  if (iext < 1 || iext + 1 > c->con.isplit || SW(c, EXT_SPLIT) || c->con.ispadv != 1 || t->P.mode == 2 || SW(c, ADVAVE_SEPARATE)) return 0;
  return launch_ext_pair_ok(c->sw, t->P);
}
static int ext_pair(pomgpu_ctx *c, int iext, int store_f = 0) {
  if (!ext_pair_ok(c, iext)) return 0;
  pomgpu_ctx *t = c->wide.on ? c->wide.x : c;
  const int isplit = c->con.isplit;
  KP &P = t->P;
  if (!t->alt3[0]) {
    if (hipMalloc((void **)&t->alt3[0], (size_t)POMGPU_NGEN * P.n2 * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); t->alt3[0] = NULL; return 0; }
    for (int n = 1; n < POMGPU_NGEN; n++) t->alt3[n] = t->alt3[0] + (size_t)n * P.n2;
    (void)hipMemsetAsync(t->alt3[0], 0, (size_t)POMGPU_NGEN * P.n2 * sizeof(double), c->stream);
  }
  t->con.iext = iext; t->con.isplit = isplit;
  P.iext = iext;
  if (!t->areas_checked) { launch_check_areas(t); t->areas_checked = 1; }
  KP Q = P;
  // Every launch moves the current generation to the other buffer set; the loop should end in the blk2d arrays (else ext_canonical
  // copies seven arrays back: 0.09 ms at 2048x1536).  If the launches still to come (pairs, and a last single substep of an odd
  // rest) would leave it in alt2, ONE pair goes alt2 -> alt3 with the stale blk2d arrays as its scratch set, and the two sets
  // swap names: 15 pairs = blk2d -> alt2 -> alt3 (now called alt2) -> blk2d -> ...
  const int rest = isplit - iext + 1, launches = rest / 2 + (rest & 1);
  const bool stay = t->ext_parity == 1 && !(launches & 1) && !SW(c, EXT_TWO_SETS);
  double *canon[POMGPU_NGEN];
  for (int n = 0; n < POMGPU_NGEN; n++) canon[n] = P.b2 + (size_t)X2_SLOT[n] * P.n2;
  for (int n = 0; n < POMGPU_NGEN; n++) Q.y2[n] = stay ? t->alt3[n] : t->ext_parity ? canon[n] : t->alt2[n];
  double *third[POMGPU_NGEN];
  for (int n = 0; n < POMGPU_NGEN; n++) third[n] = stay ? canon[n] : t->alt3[n];
  if (t->parent && !SW(c, WIDE_FULL)) {
    // the extended tile shrinks as it goes stale (mode_external above): both substeps of the pair run on the window of the FIRST one
    // (the second one's is a row smaller on every extended side: a subset)
    const pomgpu_wide &Wd = t->parent->wide;
    int cut = iext - 1 < Wd.w - 5 ? iext - 1 : Wd.w - 5;
    if (cut < 0) cut = 0;
    const int lo = Wd.oy > 0 ? cut : 0, hi = P.jm - t->parent->P.jm - Wd.oy > 0 ? cut : 0;
    if (lo + hi > 0 && P.jm - lo - hi >= 16) {
      Q = row_window(Q, lo, hi);
      for (int n = 0; n < POMGPU_NGEN; n++) third[n] += (size_t)lo * P.iml;
    }
  }
  if (!launch_ext_pair(t, Q, third, store_f || iext + 1 == isplit)) return 0;
  if (stay) for (int n = 0; n < POMGPU_NGEN; n++) { double *x = t->alt2[n]; t->alt2[n] = t->alt3[n]; t->alt3[n] = x; }
  else t->ext_parity ^= 1;                                    // two substeps, one change of buffer sets
  ext_buffers(t);
  c->con.iext = iext + 1; t->con.iext = iext + 1; P.iext = iext + 1; c->P.iext = iext + 1;
  if (c->wide.on && iext + 1 == isplit) wide_flush(c);        // the tile's arrays, ghost cells included, are current again
  return 1;
}
// every external substep of the step in one launch (k_ext_loop): one tile -- or the extended tile of the wide-halo mode --
// whose workgroups are all resident at once; 0 = not applicable, the caller loops over mode_external
static int ext_loop_all(pomgpu_ctx *c) {
  pomgpu_ctx *t = c;
  if (c->wide.on) { if (!c->wide.pending) return 0; t = c->wide.x; t->con.isplit = c->con.isplit; }
  else if (c->exch) return 0;
  KP &P = t->P;
  const int isplit = c->con.isplit;
  if (SW(c, EXT_SPLIT) || c->con.ispadv != 1 || P.mode == 2 || SW(c, ADVAVE_SEPARATE) || isplit < 2) return 0;
  P.iext = 1;
  KP Q = P;
  for (int n = 0; n < POMGPU_NGEN; n++) Q.y2[n] = t->ext_parity ? P.b2 + (size_t)X2_SLOT[n] * P.n2 : t->alt2[n];
  if (!launch_ext_loop(t, Q, 1, isplit)) return 0;
  if (isplit & 1) t->ext_parity ^= 1;                         // one generation swap per substep
  ext_buffers(t);
  c->con.iext = isplit; t->con.iext = isplit; P.iext = isplit; c->P.iext = isplit;
  if (c->wide.on) wide_flush(c);                              // the tile's arrays, ghost cells included, are current again
  return 1;
}
// ---- the library's own exchange (include/pomgpu.h "transport") -----------------------------------------------
// every exchange point: round8 on the stream (the hook has no return value: a failed round has set error_status)
static void tp_exchange(void *user, double *const *dev, const int *nz, int count) { (void)round8((pomgpu_ctx *)user, 0, dev, nz, count); }
// order2d_mpi / order3d_mpi (parallel_mpi.f:353-480): eastward and northward only
static void tp_order(void *user, const double *send_e, int n_e, const double *send_n, int n_n, double *recv_w, double *recv_s) {
  pomgpu_ctx *c = (pomgpu_ctx *)user;
  const pomgpu_transport &T = c->tp;
  const double *snd[8] = {NULL, send_e, NULL, send_n, NULL, NULL, NULL, NULL};
  double *rcv[8] = {recv_w, NULL, recv_s, NULL, NULL, NULL, NULL, NULL};
  size_t sc[8] = {0, T.nbr[1] >= 0 ? (size_t)n_e : 0, 0, T.nbr[3] >= 0 ? (size_t)n_n : 0, 0, 0, 0, 0};
  size_t rc[8] = {T.nbr[0] >= 0 ? (size_t)n_e : 0, 0, T.nbr[2] >= 0 ? (size_t)n_n : 0, 0, 0, 0, 0, 0};
  (void)pomgpu_tp_move_ptr(c, snd, sc, rcv, rc);
}
static int tp_install(pomgpu_ctx *c, const int *nbr8) {
  int rc = pomgpu_tp_setup(c, nbr8);
  if (rc) return rc;
  bool any = false;
  for (int d = 0; d < 8; d++) any = any || c->tp.nbr[d] >= 0;
  // a tile without neighbours keeps the single-tile (fused) kernels: every exchange is a no-op (parallel_mpi.f:171)
  c->exch = any ? tp_exchange : NULL; c->exch_user = c;
  c->order = any ? tp_order : NULL; c->order_user = c;
  return POMGPU_OK;
}
extern "C" int pomgpu_set_transport(pomgpu_ctx *c, const int *nbr8, pomgpu_transport_fn fn, void *user) {
  NEED_HOT(c);
  wide_free(c);
  pomgpu_tp_free(c);
  if (!fn) {                                                  // no mover: back to the hooks / a single tile
    c->exch = NULL; c->order = NULL;
    return POMGPU_OK;
  }
  c->tp.fn = fn; c->tp.user = user;
  return tp_install(c, nbr8);
}
extern "C" int pomgpu_rccl_init(pomgpu_ctx *c, const void *id128, int rank, int nranks, const int *nbr8, const char *librccl_path) {
  NEED_HOT(c);
  wide_free(c);
  pomgpu_tp_free(c);
  int rc = pomgpu_tp_rccl(c, id128, rank, nranks, librccl_path);
  if (rc) return rc;
  return tp_install(c, nbr8);
}

// ---- wide-halo external mode (include/pomgpu.h: pomgpu_set_wide_external) --------------------------------------
// How far stale cells spread (advance.f:211-347, solver.f:16-121).  The outermost line of the extended tile is
// never computed (in the reference it comes from an exchange).  uaf(i) reads ua(i-1..i+1), el(i-1) and, through
// fluxua(i-1) inside advua, d(i-2); elf(i) reads ua(i..i+1), d(i-1..i+1).  If ua is wrong up to column a and el, d
// up to column b, the next substep leaves ua wrong up to max(a+1, b+2) and el up to a: starting from a=2, b=1 the
// front moves ONE column per substep (ua wrong up to n+1, el up to n after n substeps; the other three sides
// alike).  advave and the tail of mode_interaction, run once before the loop on the same extended tile, add two
// columns at most.  With w = isplit + 4 extra cells the tile and its ghost cells are never reached
// (tests/test_kernels_emulated_tiles.py shows exact ghost cells with this w and owned cells going wrong below
// isplit - 1).
// Arrays that travel.  HALO: read by the 2-D part of the step with a stencil or by a substep's pointwise formulas
// in cells beyond the tile -- they need the neighbours' cells.  LOCAL: written by the 2-D part; the extended tile
// starts from the tile's own values so that cells no kernel writes (e.g. utf(1,j) on a physical edge) stay what they
// are.  BACK: what the 2-D part writes -- copied back, ghost cells included.
static const int WIDE_HALO[] = {P2_adx2d, P2_ady2d, P2_drx2d, P2_dry2d, P2_aam2d, P2_ua, P2_va, P2_uab, P2_vab, P2_el, P2_elb,
                                P2_d, P2_vfluxf, P2_e_atmos, P2_wusurf, P2_wvsurf, P2_wubot, P2_wvbot};
static const int WIDE_LOCAL[] = {P2_advua, P2_advva, P2_elf, P2_uaf, P2_vaf, P2_egf, P2_utf, P2_vtf, P2_etf};
static const int WIDE_BACK[] = {P2_adx2d, P2_ady2d, P2_advua, P2_advva, P2_elf, P2_uaf, P2_vaf, P2_ua, P2_va, P2_el, P2_elb, P2_d,
                                P2_uab, P2_vab, P2_egf, P2_utf, P2_vtf, P2_etf, P2_wubot, P2_wvbot};
// open-boundary values bcond(2) reads (bounds_forcing.f:43-83): indexed by j on the west / east edge, by i on the
// south / north edge; a tile on such an edge continues them from its neighbours along the edge
static const int WIDE_BD_J[] = {PB_uabw, PB_elw, PB_vabw, PB_uabe, PB_ele, PB_vabe};
static const int WIDE_BD_I[] = {PB_vabs, PB_els, PB_uabs, PB_vabn, PB_eln, PB_uabn};
// The same HALO list in two parts.  LATE: what lateral_viscosity and the vertical integrals of mode_interaction produce in
// THIS step (advance.f:96-168).  EARLY: everything else -- final when the step starts (the external mode and mode_internal
// of the step before wrote them; surface_forcing / lateral_bc, if they run, come first) -- most of the bytes.
static const int WIDE_HALO_LATE[] = {P2_adx2d, P2_ady2d, P2_drx2d, P2_dry2d, P2_aam2d};
static const int WIDE_HALO_EARLY[] = {P2_ua, P2_va, P2_uab, P2_vab, P2_el, P2_elb, P2_d, P2_vfluxf, P2_e_atmos, P2_wusurf, P2_wvsurf, P2_wubot,
                                      P2_wvbot};
#define NEL(a) ((int)(sizeof(a) / sizeof((a)[0])))
static bool wide_travels_every_step(int slot2d) {
  for (int n = 0; n < NEL(WIDE_HALO); n++) if (WIDE_HALO[n] == slot2d) return true;
  for (int n = 0; n < NEL(WIDE_LOCAL); n++) if (WIDE_LOCAL[n] == slot2d) return true;
  return false;
}

struct JobList {
  std::vector<RectJob> jobs;
  std::vector<RectGroup> groups;
  void begin() { RectGroup g = {(int)jobs.size(), 0, 0, 0}; groups.push_back(g); }
  void add(const double *src, int ld_s, double *dst, int ld_d, int ni, int nj) {
    if (ni <= 0 || nj <= 0) return;
    RectJob j = {src, dst, ld_s, ld_d, ni, nj};
    jobs.push_back(j);
    RectGroup &g = groups.back();
    g.count++;
    if (ni > g.mni) g.mni = ni;
    if (nj > g.mnj) g.mnj = nj;
  }
};
static int table_upload(pomgpu_ctx *c, const JobList &L, RectTable &T) {
  T.dev = NULL; T.ngroups = 0;
  if (L.jobs.empty()) return POMGPU_OK;
  if (hipMalloc((void **)&T.dev, L.jobs.size() * sizeof(RectJob)) != hipSuccess) return fail(c, POMGPU_ENOMEM, "wide: job table");
  HIPCHK(c, hipMemcpyAsync(T.dev, L.jobs.data(), L.jobs.size() * sizeof(RectJob), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));                 // L.jobs is the caller's temporary
  for (size_t n = 0; n < L.groups.size() && T.ngroups < 8; n++)
    if (L.groups[n].count) T.g[T.ngroups++] = L.groups[n];
  return POMGPU_OK;
}
static void table_run(pomgpu_ctx *c, const RectTable &T) {
  for (int n = 0; n < T.ngroups; n++) launch_rect_jobs(c, T.dev + T.g[n].first, T.g[n].count, T.g[n].mni, T.g[n].mnj);
}
static void table_free(RectTable &T) { (void)hipFree(T.dev); T.dev = NULL; T.ngroups = 0; }
static void wide_free(pomgpu_ctx *c) {
  pomgpu_wide &Wd = c->wide;
  table_free(Wd.gather_pack); table_free(Wd.gather_unpack); table_free(Wd.scatter);
  table_free(Wd.early_pack); table_free(Wd.early_unpack); table_free(Wd.late_pack); table_free(Wd.late_unpack);
  Wd.split = 0;
  c->early_started = 0;
  if (Wd.x) { pomgpu_destroy(Wd.x); Wd.x = NULL; }
  Wd.on = 0;
}
// the block of the tile that neighbour d needs (sx,sy: its first cell, tile indices) and where the block that
// neighbour d sends lands in the extended tile (rx,ry: tile indices, i.e. before + ox / + oy); both ni x nj
static void wide_rect(const KP &P, int w, int d, int &sx, int &sy, int &rx, int &ry, int &ni, int &nj) {
  static const int DX[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, DY[8] = {0, 0, -1, 1, -1, -1, 1, 1};
  const int lox = P.W ? 1 : 2, hix = P.E ? P.im : P.imm1, loy = P.S ? 1 : 2, hiy = P.N ? P.jm : P.jmm1;
  if (DX[d] < 0) { sx = 2; rx = 1 - w; ni = w + 1; }
  else if (DX[d] > 0) { sx = P.im - 1 - w; rx = P.im; ni = w + 1; }
  else { sx = rx = lox; ni = hix - lox + 1; }
  if (DY[d] < 0) { sy = 2; ry = 1 - w; nj = w + 1; }
  else if (DY[d] > 0) { sy = P.jm - 1 - w; ry = P.jm; nj = w + 1; }
  else { sy = ry = loy; nj = hiy - loy + 1; }
}
// Job lists for one set of arrays: `halo` slots get the tile's own cells and the neighbours' blocks, `local` slots
// the tile's own cells only; with_bd adds the open-boundary lines.  pack/unpack go around one message round.
static void wide_jobs(pomgpu_ctx *c, const int *halo, int nhalo, const int *local, int nlocal, bool with_bd, JobList &pack,
                      JobList &unpack, size_t *scount, size_t *rcount, double *const *snd = NULL, double *const *rcv = NULL) {
  const KP &P = c->P;
  const pomgpu_wide &Wd = c->wide;
  const KP &X = Wd.x->P;
  const pomgpu_transport &T = c->tp;
  if (!snd) { snd = T.send; rcv = T.recv; }
  auto tile = [&](int s, int i, int j) { return P.b2 + (size_t)s * P.n2 + (size_t)(j - 1) * P.iml + (size_t)(i - 1); };
  auto ext = [&](int s, int i, int j) { return X.b2 + (size_t)s * X.n2 + (size_t)(j + Wd.oy - 1) * X.iml + (size_t)(i + Wd.ox - 1); };
  pack.begin();                                               // own cells, ghost cells included
  for (int n = 0; n < nhalo; n++) pack.add(tile(halo[n], 1, 1), P.iml, ext(halo[n], 1, 1), X.iml, P.im, P.jm);
  for (int n = 0; n < nlocal; n++) pack.add(tile(local[n], 1, 1), P.iml, ext(local[n], 1, 1), X.iml, P.im, P.jm);
  if (with_bd) {
    pack.begin();
    for (int n = 0; n < NEL(WIDE_BD_J); n++) pack.add(P.bd + P.bdoff[WIDE_BD_J[n]], P.jml, X.bd + X.bdoff[WIDE_BD_J[n]] + Wd.oy, X.jml, P.jm, 1);
    for (int n = 0; n < NEL(WIDE_BD_I); n++) pack.add(P.bd + P.bdoff[WIDE_BD_I[n]], P.iml, X.bd + X.bdoff[WIDE_BD_I[n]] + Wd.ox, X.iml, P.im, 1);
  }
  for (int cls = 0; cls < 3; cls++) {                         // W/E blocks, S/N blocks, corners: one launch each
    pack.begin(); unpack.begin();
    for (int d = (cls == 0 ? 0 : (cls == 1 ? 2 : 4)); d < (cls == 0 ? 2 : (cls == 1 ? 4 : 8)); d++) {
      scount[d] = rcount[d] = 0;
      if (T.nbr[d] < 0) continue;
      int sx, sy, rx, ry, ni, nj;
      wide_rect(P, Wd.w, d, sx, sy, rx, ry, ni, nj);
      size_t o = 0;
      for (int n = 0; n < nhalo; n++) {
        pack.add(tile(halo[n], sx, sy), P.iml, snd[d] + o, ni, ni, nj);
        unpack.add(rcv[d] + o, ni, ext(halo[n], rx, ry), X.iml, ni, nj);
        o += (size_t)ni * nj;
      }
      if (with_bd && cls == 1)                                // from S / N: the continuation of the west / east edge lines
        for (int n = 0; n < NEL(WIDE_BD_J); n++) {
          pack.add(P.bd + P.bdoff[WIDE_BD_J[n]] + (sy - 1), nj, snd[d] + o, nj, nj, 1);
          unpack.add(rcv[d] + o, nj, X.bd + X.bdoff[WIDE_BD_J[n]] + (ry + Wd.oy - 1), nj, nj, 1);
          o += (size_t)nj;
        }
      if (with_bd && cls == 0)                                // from W / E: the continuation of the south / north edge lines
        for (int n = 0; n < NEL(WIDE_BD_I); n++) {
          pack.add(P.bd + P.bdoff[WIDE_BD_I[n]] + (sx - 1), ni, snd[d] + o, ni, ni, 1);
          unpack.add(rcv[d] + o, ni, X.bd + X.bdoff[WIDE_BD_I[n]] + (rx + Wd.ox - 1), ni, ni, 1);
          o += (size_t)ni;
        }
      scount[d] = rcount[d] = o;
    }
  }
}
static void refresh_coefs(pomgpu_ctx *c);
// grid metrics, masks, Coriolis ... : every blk2d array once (and again after an upload), in chunks that fit
// the staging buffers
static int wide_static(pomgpu_ctx *c) {
  pomgpu_wide &Wd = c->wide;
  const int chunk = NEL(WIDE_HALO);
  for (int s0 = 0; s0 < POM_NBLK2D; s0 += chunk) {
    int slots[64], n = 0;
    for (int s = s0; s < POM_NBLK2D && n < chunk; s++) slots[n++] = s;
    JobList pk, up;
    size_t sc[8], rc[8];
    wide_jobs(c, slots, n, NULL, 0, false, pk, up, sc, rc);
    RectTable tp_, tu_;
    int e;
    if ((e = table_upload(c, pk, tp_)) || (e = table_upload(c, up, tu_))) return e;
    table_run(c, tp_);
    if ((e = pomgpu_tp_move(c, sc, rc))) return e;
    table_run(c, tu_);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    table_free(tp_); table_free(tu_);
  }
  HIPCHK(c, hipMemcpyAsync(Wd.x->P.b1, c->P.b1, (size_t)POM_NBLK1D * c->P.kb * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  refresh_coefs(Wd.x);
  Wd.static_done = 1;
  return POMGPU_OK;
}
extern "C" int pomgpu_set_wide_external(pomgpu_ctx *c, int on, int min_im, int min_jm) {
  NEED_HOT(c);
  wide_free(c);
  if (!on) return POMGPU_OK;
  pomgpu_transport &T = c->tp;
  if (!T.on) return fail(c, POMGPU_EINVAL, "wide external mode: set a transport first");
  const KP &P = c->P;
  // the width follows the number of external substeps per internal step: the state (blkcon) must have been uploaded
  if (c->con.isplit < 1) return fail(c, POMGPU_EINVAL, "wide external mode: isplit = %d -- upload the state (pomgpu_upload / pomgpu_set_con) first", c->con.isplit);
  int w = c->con.isplit + 4;
  if (SW(c, WIDE_W)) w = (int)SWV(c, WIDE_W);   // developer switch: shows that fewer cells are not enough
  if (w < 1 || min_im < w + 3 || min_jm < w + 3 || P.im < w + 3 || P.jm < w + 3) {
    snprintf(c->err, sizeof c->err, "wide external mode: tiles of %d x %d cells are narrower than w + 3 = %d", min_im, min_jm, w + 3);
    return POMGPU_EINVAL;                                     // not an error of the run: the per-point exchanges stay in use
  }
  bool any = false;
  for (int d = 0; d < 8; d++) any = any || T.nbr[d] >= 0;
  if (!any) return POMGPU_OK;                                 // one tile: nothing to widen
  pomgpu_wide &Wd = c->wide;
  Wd.w = w;
  Wd.ox = T.nbr[0] >= 0 ? w : 0;
  Wd.oy = T.nbr[2] >= 0 ? w : 0;
  pomgpu_dims d;
  d.im = P.im + Wd.ox + (T.nbr[1] >= 0 ? w : 0);
  d.jm = P.jm + Wd.oy + (T.nbr[3] >= 0 ? w : 0);
  d.kb = P.kb;
  d.im_local = d.im + (d.im & 1);                             // even: the two-columns-per-lane advave kernel applies
  d.jm_local = d.jm;
  d.n_west = T.nbr[0]; d.n_east = T.nbr[1]; d.n_south = T.nbr[2]; d.n_north = T.nbr[3];
  int rc = ctx_create(&Wd.x, &d, c->device, (void *)c->stream, POMGPU_CTX_2D);
  if (rc) return fail(c, rc, "wide external mode: cannot create the %d x %d extended tile", d.im, d.jm);
  Wd.x->parent = c;
  Wd.x->sw = c->sw;                                           // the extended tile runs under its tile's switches
  set_band_geometry(Wd.x->P, Wd.x->sw);
  // staging buffers: the per-step arrays of one neighbour block (w+1 lines of the tile's edge; corners (w+1)^2)
  size_t need[8];
  const size_t per = (size_t)NEL(WIDE_HALO) * (w + 1), edge = (size_t)NEL(WIDE_BD_J) * (w + 1);
  need[0] = need[1] = per * P.jm + edge;
  need[2] = need[3] = per * P.im + edge;
  need[4] = need[5] = need[6] = need[7] = per * (w + 1);
  if ((rc = pomgpu_tp_reserve(c, need))) { wide_free(c); return rc; }
  JobList pk, up, sc;
  wide_jobs(c, WIDE_HALO, NEL(WIDE_HALO), WIDE_LOCAL, NEL(WIDE_LOCAL), true, pk, up, Wd.scount, Wd.rcount);
  const KP &X = Wd.x->P;
  sc.begin();
  for (int n = 0; n < NEL(WIDE_BACK); n++)
    sc.add(X.b2 + (size_t)WIDE_BACK[n] * X.n2 + (size_t)Wd.oy * X.iml + Wd.ox, X.iml, P.b2 + (size_t)WIDE_BACK[n] * P.n2, P.iml, P.im, P.jm);
  if ((rc = table_upload(c, pk, Wd.gather_pack)) || (rc = table_upload(c, up, Wd.gather_unpack)) || (rc = table_upload(c, sc, Wd.scatter))) {
    wide_free(c);
    return rc;
  }
  // the two-part gather on two streams: where EVERY rank can serve a second stream (pomgpu_tp_side_ok: the ranks' agreement,
  // taken by pomgpu_rccl_init over the communicator or handed in by the host of a callback mover; never a rank's own choice)
  if (pomgpu_tp_side_ok(c)) {
    size_t need2[8];
    const size_t per2 = (size_t)NEL(WIDE_HALO_EARLY) * (w + 1);
    need2[0] = need2[1] = per2 * P.jm + edge;
    need2[2] = need2[3] = per2 * P.im + edge;
    need2[4] = need2[5] = need2[6] = need2[7] = per2 * (w + 1);
    // the wr exchange of the end of the step shares these buffers (same stream, so never at the same time)
    const size_t wrn[8] = {(size_t)P.kb * P.jm, (size_t)P.kb * P.jm, (size_t)P.kb * P.im, (size_t)P.kb * P.im, (size_t)P.kb, (size_t)P.kb, (size_t)P.kb, (size_t)P.kb};
    for (int d8 = 0; d8 < 8; d8++) if (need2[d8] < wrn[d8]) need2[d8] = wrn[d8];
    // ... and so do the rim rounds (the exchange points that run on the side stream): what an ordinary exchange point may need (pomgpu_tp_setup)
    for (int d8 = 0; d8 < 8; d8++) if (need2[d8] < 10 * wrn[d8]) need2[d8] = 10 * wrn[d8];   // (the largest: nine arrays of kb levels)
    if ((rc = pomgpu_tp_reserve2(c, need2))) { wide_free(c); return rc; }
    JobList epk, eup, lpk, lup;
    wide_jobs(c, WIDE_HALO_EARLY, NEL(WIDE_HALO_EARLY), WIDE_LOCAL, NEL(WIDE_LOCAL), true, epk, eup, Wd.e_scount, Wd.e_rcount, T.send2, T.recv2);
    wide_jobs(c, WIDE_HALO_LATE, NEL(WIDE_HALO_LATE), NULL, 0, false, lpk, lup, Wd.l_scount, Wd.l_rcount);
    if ((rc = table_upload(c, epk, Wd.early_pack)) || (rc = table_upload(c, eup, Wd.early_unpack)) || (rc = table_upload(c, lpk, Wd.late_pack)) ||
        (rc = table_upload(c, lup, Wd.late_unpack))) {
      wide_free(c);
      return rc;
    }
    Wd.split = 1;
  }
  Wd.static_done = 0;
  if ((rc = tide_widen(c))) { wide_free(c); return rc; }      // the extended tile's stretch of the tide's lines, cut from the global ones
  Wd.on = 1;
  return POMGPU_OK;
}
// The early part of the gather, on the side stream: called by pomgpu_advance once the step's forcing is in place, so that
// its pack kernels, its message round and its unpack kernels run beside lateral_viscosity (advance.f:96-141) on the main
// stream.  Nothing between here and wide_begin touches the arrays of WIDE_HALO_EARLY / WIDE_LOCAL / the boundary lines,
// nor the extended tile.
static int wide_early_start(pomgpu_ctx *c) {
  pomgpu_wide &Wd = c->wide;
  if (!Wd.on || !Wd.split || Wd.pending || c->early_started) return POMGPU_OK;
  int rc;
  if (!Wd.static_done && (rc = wide_static(c))) return rc;
  side_begin(c);
  table_run(c, Wd.early_pack);
  rc = pomgpu_tp_move_side(c, Wd.e_scount, Wd.e_rcount);
  if (!rc) table_run(c, Wd.early_unpack);
  side_end(c, c->ev_early);
  c->early_started = 1;
  return rc;
}
// The 2-D part of one internal step on the extended tile.  wide_begin: the rest of mode_interaction after the
// vertical integrals (advance.f:170-199); the isplit calls of mode_external then work on the extended tile
// (mode_external above); wide_end after the last one copies the result back.  Any other entry point that finds
// the 2-D state still out there fetches it first (wide_flush in NEED_HOT).
static int wide_begin(pomgpu_ctx *c) {
  pomgpu_wide &Wd = c->wide;
  pomgpu_ctx *x = Wd.x;
  int rc;
  if (c->con.isplit + 4 > Wd.w && !SW(c, WIDE_W))     // the stale rim grows by one cell per substep (see above)
    return fail(c, POMGPU_EINVAL, "wide external mode: isplit = %d now, the extended tile was made for isplit <= %d -- call pomgpu_set_wide_external again", c->con.isplit, Wd.w - 4);
  if (!Wd.static_done && (rc = wide_static(c))) return rc;
  if (c->early_started) {                                     // the rest of the gather here, then wait for the part that ran beside
    table_run(c, Wd.late_pack);
    if ((rc = pomgpu_tp_move(c, Wd.l_scount, Wd.l_rcount))) return rc;
    table_run(c, Wd.late_unpack);
    (void)hipStreamWaitEvent(c->stream, c->ev_early, 0);
    c->early_started = 0;
  } else {
    table_run(c, Wd.gather_pack);
    if ((rc = pomgpu_tp_move(c, Wd.scount, Wd.rcount))) return rc;
    table_run(c, Wd.gather_unpack);
  }
  x->con = c->con; x->lramp = c->lramp;
  sync_scalars(x);
  if (x->P.mode != 2) seq_advave(x);                          // advance.f:170 (the extended tile has no exchange: fused kernels)
  launch_modeint_tail(x);                                     // :172-196; the exchange of utf, vtf (:198-199) is not needed
  Wd.pending = 1;
  return POMGPU_OK;
}
static void wide_flush(pomgpu_ctx *c) {
  pomgpu_wide &Wd = c->wide;
  if (!Wd.on || !Wd.pending) return;
  side_join(c);                                               // a deferred realvertvl on the side stream reads the etf this scatter rewrites
  ext_canonical(Wd.x);
  table_run(c, Wd.scatter);
  Wd.pending = 0;
}

extern "C" int pomgpu_mode_interaction(pomgpu_ctx *c) { return mode_interaction(c, 0); }
// the substep pomgpu_mode_external holds back, alone after all (its partner did not come: another entry point, a download ...)
static void ext_flush_deferred(pomgpu_ctx *c) {
  if (!c->ext_deferred) return;
  const int now = c->con.iext;
  c->con.iext = c->ext_deferred;
  c->ext_deferred = 0;
  if (mode_external(c, 1)) c->con.error_status = 1;           // the held substep failed: the context says so at the next entry point / get_con (pomgpu.h)
  c->con.iext = now;
  c->P.iext = now;
}
// The reference calls mode_external isplit times in a row (advance.f:27-29) and looks at nothing in between.  An ODD substep of a tile
// that takes two substeps per pass (k_ext_march2) is therefore held back until the next call: if that is the following substep, the
// two run as one pass (elf, uaf, vaf of the second are stored, as the caller of this entry point may expect of every call); anything
// else that touches the state first -- any other entry point, a download -- makes it run alone before (ext_canonical).
extern "C" int pomgpu_mode_external(pomgpu_ctx *c) {
  NEED_RAW(c);
  const int iext = c->con.iext;
  if (c->ntide) {                                             // the step's phasors, once per iint; the table has isplit substeps
    if (iext < 1 || iext > c->con.isplit) return fail(c, POMGPU_EINVAL, "mode_external with a tide: iext = %d is not a substep of 1..%d", iext, c->con.isplit);
    const int rct = tide_table(c);
    if (rct) return rct;
  }
  if (c->ext_deferred) {
    if (iext == c->ext_deferred + 1) {
      const int first = c->ext_deferred;
      c->ext_deferred = 0;
      if (ext_pair(c, first, 1)) return POMGPU_OK;
      c->con.iext = first;                                    // the pass was refused after all: the two substeps one by one
      int rc = mode_external(c, 1);
      c->con.iext = iext;
      return rc ? rc : mode_external(c, 1);
    }
    ext_flush_deferred(c);
  }
  if ((iext & 1) && ext_pair_ok(c, iext)) { c->ext_deferred = iext; return POMGPU_OK; }
  return mode_external(c, 1);
}
// wr (solver.f:2024-2067) and its exchange (:2055) on the side stream: nobody on the hot path reads wr (a diagnostic for the
// output file), so realvertvl itself may run there as well (with_kernel: beside the NEXT step's external substeps, below)
// ---- passive tracers (include/pomgpu.h) ---------------------------------------------------------------------------
// The stage mode_internal runs between dens (advance.f:454) and advu (:459) while tracers are registered: per tracer the lines the
// reference runs for T -- advt1 / advt2, the exchange of :436, proft, bcond(4), the filter and rotation -- plus a source / decay term
// behind the advection.  It reads u v w aam kh etb etf as they stand there (u, v through the UM forms while KP::uvm is up) and writes
// nothing but the tracers' own arrays.  With the one-pass advection (nadv 2, nitera 1) tracers 2p-1, 2p share k_advt2_col<2>, one lane of
// proft where launch_proft2 takes the pair, k_tr_edges<2> and k_tr_update<2>; an odd one, nadv 1 and nitera > 1 go one by one
// (POMGPU_TR_NOPAIR, read here: every tracer one by one).  fb's round trip (solver.f:691,715) is deferred to k_tr_update as k_ts_update
// does for T and S; k_tr_source, which reads trb in between, applies it to what it loads.
// Message rounds, the library's own exchange (lib_x): the one-pass advection's solver.f:728 and advance.f:436 have nothing written on a
// ghost line in between that the neighbour does not write alike (the source is pointwise and runs on ghost lines too), so ONE round
// carries trf of all tracers (xch takes eight arrays); nitera > 1 adds smol_adif's nitera rounds and :728 per tracer (seq_advt2).
static void xchv(pomgpu_ctx *c, double *const *ptr, const int *nz, int count) {
  if (c->exch) c->exch(c->exch_user, ptr, nz, count);
}
static int tracer_stage(pomgpu_ctx *c, bool lib_x) {
  KP &P = c->P;
  const pom_blkcon &k = c->con;
  const int ntr = c->ntr;
  if (k.nadv != 1 && k.nadv != 2) return fail(c, POMGPU_EINVAL, "Error: invalid value for nadv");
  const bool one_pass = k.nadv == 2 && P.nitera == 1;
  const bool pairs = one_pass && !SW(c, ADVT2_SINGLE) && !SW(c, TR_NOPAIR);
  const int rt = k.nadv == 2;                                 // advt2's round trip of trb rides in k_tr_update
  // 1. the advection
  for (int n = 0; n < ntr;) {
    pomgpu_ctx::pomgpu_tracer &a = c->trc[n];
    if (pairs && n + 1 < ntr) {
      pomgpu_ctx::pomgpu_tracer &b = c->trc[n + 1];
      launch_advt2x2_col(c, a.trb, a.tr, a.clim, a.trf, b.trb, b.tr, b.clim, b.trf);
      if (!lib_x) { xch(c, 1, a.trf, P.kbm1); xch(c, 1, b.trf, P.kbm1); }   // solver.f:728
      launch_copy_kb(c, a.trb, b.trb);                        // :618
      n += 2;
      continue;
    }
    if (k.nadv == 1) seq_advt1(c, a.trb, a.tr, a.clim, a.trf);
    else if (one_pass) {
      launch_advt2_rows(c, a.trb, a.tr, a.clim, a.trf);       // (HEA, HFA: mode_internal's launch_coef_eta)
      if (!lib_x) xch(c, 1, a.trf, P.kbm1);                   // :728
      launch_copy_kb(c, a.trb);                               // :618
    } else seq_advt2(c, a.trb, a.tr, a.clim, a.trf, true);
    n += 1;
  }
  // 2. source and decay
  for (int n = 0; n < ntr; n++) {
    const pomgpu_ctx::pomgpu_tracer &a = c->trc[n];
    if (a.q || a.lam != 0.) launch_tr_source(c, a.trf, a.trb, rt ? a.clim : NULL, a.q, a.lam);
  }
  // 3. advance.f:436
  {
    double *ptr[POMGPU_TRMAX];
    int nz[POMGPU_TRMAX];
    for (int n = 0; n < ntr; n++) { ptr[n] = c->trc[n].trf; nz[n] = P.kbm1; }
    xchv(c, ptr, nz, ntr);
  }
  side_wait(c, SIDE_RQ);                                      // proft's ghost columns need kh of the ghost lines
  // 4. - 6. proft, bcond(4), the filter and rotation
  for (int n = 0; n < ntr;) {
    const pomgpu_ctx::pomgpu_tracer &a = c->trc[n];
    const int nf = (pairs && n + 1 < ntr) ? 2 : 1;
    const pomgpu_ctx::pomgpu_tracer &b = c->trc[n + nf - 1];
    if (nf == 1 || !launch_proft2(c, a.trf, a.wsurf, a.surf, a.nbc, b.trf, b.wsurf, b.surf, b.nbc)) {
      launch_proft(c, a.trf, a.wsurf, a.surf, a.nbc);
      if (nf == 2) launch_proft(c, b.trf, b.wsurf, b.surf, b.nbc);
    }
    const TrEdge e[2] = {{a.trf, a.tr, a.bd[0], a.bd[1], a.bd[2], a.bd[3]}, {b.trf, b.tr, b.bd[0], b.bd[1], b.bd[2], b.bd[3]}};
    launch_tr_edges(c, e, nf);
    const TrUpd u[2] = {{a.trf, a.clim, a.tr, a.trb}, {b.trf, b.clim, b.tr, b.trb}};
    launch_tr_update(c, u, nf, rt);
    n += nf;
  }
  return POMGPU_OK;
}
static int wr_on_side(pomgpu_ctx *c, int with_kernel) {
  const KP &P = c->P;
  side_wait(c, SIDE_WR);                                      // at most one piece of side work outstanding per event
  side_begin(c);
  if (with_kernel) launch_realvertvl(c);
  double *arr[1] = {D3(c, wr)};
  const int nz[1] = {P.kbm1};
  const int rcw = round8(c, 1, arr, nz, 1);                   // (kbm1 lines fit the side stream's buffers: pomgpu_set_wide_external sized them for kb)
  side_post(c, SIDE_WR);
  return rcw;                                                 // a failed round is the step's failure (error_status is set)
}
// defer_wr (pomgpu_run, every step but the last of the call): realvertvl and wr's exchange are left to the next step, which runs
// them on the side stream beside its external substeps (wr_deferred) -- on a tile those are ~30 small dependent launches on the
// extended tile's own arrays that leave most of the chip idle, while realvertvl is a plain pass over five 3-D arrays.  Its
// operands (w, u, v, dt, et, etb, etf of the tile) are written next by the scatter that ends the external mode (wide_flush: etf)
// and by the 3-D part of mode_internal: wide_flush joins the side stream first.
static int mode_internal(pomgpu_ctx *c, int defer_wr) {       // advance.f:356-537
  NEED_HOT(c);
  KP &P = c->P;
  const pom_blkcon &k = c->con;
  side_wait(c, SIDE_R2);                                      // advx, advy, aam: ghost cells from the side stream (advq, advt2 read aam's)
  side_wait(c, SIDE_R8);                                      // (a step whose lateral_viscosity did not run: nothing else has waited)
  if ((k.iint != 1 || k.time0 != 0.) && k.mode != 2) {
    c->uvf_pending = 0;                                       // u, v change now and advq rewrites uf, vf whole: nobody has asked for the copy
    // the row-sharing column kernels (k_advq_col, k_advt2_col) read the current aam wherever it lives (KP::aamc); the other advection
    // kernels -- advt1, smol_adif's advt2, the flux / step pair of ADVQ_EXCHANGE -- read the slot
    if (!(k.nadv == 2 && P.nitera == 1) || (c->exch && SW(c, ADVQ_EXCHANGE))) aam_canonical(c);
    // :365-393 as a pass over u, v -- or applied by every kernel below to what it loads of them, u, v staying raw in memory until the
    // filter overwrites them (uvm_onload; KP::uvm tells the kernels, and is down again when this function returns)
    struct UvmScope { pomgpu_ctx *c; ~UvmScope() { c->P.uvm = 0; c->uvm_valid = 0; } } uvm_scope{c};
    P.uvm = uvm_onload(c) ? 1 : 0;
    if (!P.uvm) launch_int_uvmean(c);                         // :365-393
    const bool wf = w_fused(c);                               // :396-398 inside advq's march below
    if (!wf) launch_vertvl(c, 1);                             // :396-398
    // :400 exchange3d_mpi(w): nothing reads w's ghost cells before advt / advu (advq takes w at the cell's own
    // column only), so on tiles it travels with profq's bottom-boundary exchange below -- one round less
    const bool lib_x = c->tp.on && c->exch;                   // the library's own exchange: rounds may be merged
    // rim rounds Rw, Rq, Rts (see "rim rounds" above): results behind the kernels instead of inputs in front of them
    const bool rimr = lib_x && rim_side(c) && !SW(c, RIM_RESULTS_MAIN) && !SW(c, ADVQ_EXCHANGE) && !SW(c, PROD_FULL);
    if (rimr) {
      double *aw[1] = {D3(c, w)};
      const int nw[1] = {P.kb};
      const int rcw = rim_round(c, SIDE_RW, aw, nw, 1);       // :400
      if (rcw) return rcw;
    }
    else if (!lib_x) xch(c, 1, D3(c, w), P.kb);
    // :403-409 (uf = vf = 0 is folded into the advq step kernels)
    launch_coef_eta(c, P.uvm);                                // etb/etf are final once the external mode is done (and utf, vtf: the means u, v are corrected to)
    // advq's exchange of xflux, yflux (solver.f:458-459) hands a tile the neighbour's xflux(2,j) as its
    // xflux(im,j): the same formula on the same operands the tile holds in its own ghost cells (q, qb, u, dt, aam
    // have all been exchanged), i.e. the value it computes itself.  The fused flux+step kernel therefore serves
    // tiles as well, without that exchange.  (pomgpu_advq, the stand-alone entry point, keeps the reference's form.)
    if (!c->exch || !SW(c, ADVQ_EXCHANGE)) {
      if (SW(c, ADVQ_SINGLE)) {
        launch_advq_col(c, D3(c, q2), D3(c, q2b), D3(c, uf), 1);
        launch_advq_col(c, D3(c, q2l), D3(c, q2lb), D3(c, vf), 1);
#if POMGPU_W_FUSE
      } else if (wf) {
        launch_advq2w_col(c, D3(c, q2), D3(c, q2b), D3(c, uf), D3(c, q2l), D3(c, q2lb), D3(c, vf), 1);  // ... and w, formed on the way down
#endif
      } else {
        launch_advq2_col(c, D3(c, q2), D3(c, q2b), D3(c, uf), D3(c, q2l), D3(c, q2lb), D3(c, vf), 1);   // q2 and q2l in one pass
      }
    } else {
      double *x0 = P.s3[0], *y0 = P.s3[1], *x1 = P.s3[2], *y1 = P.s3[3];
      launch_advq_flux(c, D3(c, q2), D3(c, q2b), x0, y0);
      launch_advq_flux(c, D3(c, q2l), D3(c, q2lb), x1, y1);
      xch(c, 4, x0, P.kbm1, y0, P.kbm1, x1, P.kbm1, y1, P.kbm1);
      launch_advq_step(c, D3(c, q2), D3(c, q2b), D3(c, uf), x0, y0, 1);
      launch_advq_step(c, D3(c, q2l), D3(c, q2lb), D3(c, vf), x1, y1, 1);
    }
    const int qfuse = !SW(c, QFILTER_SPLIT);
    if (rimr) {
      launch_profq_bc(c);
      // the production term as on one tile.  Ghost ROWS are left out (Rq fills them: 24 instead of 25 row blocks on a 2048x194 tile, three
      // full rounds of workgroups instead of three and a nearly empty fourth); ghost COLUMNS are computed from stale operands and overwritten.
      launch_profq(c, 1, qfuse, c->rho_rt_pending, P.S ? 1 : 2, P.N ? P.jm : P.jmm1);
    } else {
      // with the interior's Asselin filter (:416-421) on its way up; l, dtef reach memory in a step somebody can look after (ld_on_demand)
      seq_profq(c, qfuse, lib_x, !(defer_wr && ld_on_demand(c) && !next_step_fetches_record(c)));
      xch(c, 2, LEV3(c, D3(c, uf), 1), P.kbm2, LEV3(c, D3(c, vf), 1), P.kbm2);   // :411-412
    }
    launch_bcond6_edges(c);                                   // :414
    if (qfuse) launch_q_filter_rim(c);                        // :416-421, edge lines
    else launch_q_filter(c, 1);
    if (rimr) {
      double *aq[9] = {D3(c, q2), D3(c, q2b), D3(c, q2l), D3(c, q2lb), D3(c, km), D3(c, kh), D3(c, kq), D3(c, l), D3(c, dtef)};
      const int nq[9] = {P.kb, P.kb, P.kb, P.kb, P.kb, P.kb, P.kb, P.kb, P.kb};
      const int rcq = rim_round(c, SIDE_RQ, aq, nq, 9);
      if (rcq) return rcq;
    }
    side_wait(c, SIDE_RW);                                    // the tracer advection and advu / advv read w's ghost lines
    if (k.mode != 4) {
      bool ts_flags = false;                                  // rt_words are this step's: the one-pass T / S advection alone writes them
      if (k.nadv == 1) {
        seq_advt1(c, D3(c, tb), D3(c, t), D3(c, tclim), D3(c, uf));
        seq_advt1(c, D3(c, sb), D3(c, s), D3(c, sclim), D3(c, vf));
      } else if (k.nadv == 2) {
        if (P.nitera == 1 && !SW(c, ADVT2_SINGLE)) {   // T and S in one pass (HEA, HFA: launch_coef_eta above -- etb, etf have not changed since)
          ts_flags = rt_one_tile(c);                            // ... and says where the round trip of tb, sb changes bits, for k_ts_update below
          launch_advt2x2_col(c, D3(c, tb), D3(c, t), D3(c, tclim), D3(c, uf), D3(c, sb), D3(c, s), D3(c, sclim), D3(c, vf), ts_flags ? c->rt_words : NULL);
          // solver.f:728 exchanges T, then S; advance.f:436-437 below exchanges both again with nothing written
          // in between: the library's own exchange serves the three points in that one round
          if (!lib_x) xch(c, 1, D3(c, uf), P.kbm1);             // solver.f:728 (T)
          if (!lib_x) xch(c, 1, D3(c, vf), P.kbm1);             // :728 (S)
          launch_copy_kb(c, D3(c, tb), D3(c, sb));              // :618 for T and S in one launch (level kb of tb, sb: no exchange reads it)
        } else {
          seq_advt2(c, D3(c, tb), D3(c, t), D3(c, tclim), D3(c, uf), true);
          seq_advt2(c, D3(c, sb), D3(c, s), D3(c, sclim), D3(c, vf), true);
        }
      } else {
        return fail(c, POMGPU_EINVAL, "Error: invalid value for nadv");
      }
      // rim round Rts: T and S leave the tracer advection with stale ghost lines; proft, bcond(4) and the filter run on them as on any line
      // and the round behind k_ts_update replaces what they made of them -- valid for the one-pass advection, whose own exchange is this one
      const bool rts = rimr && k.nadv == 2 && P.nitera == 1 && !SW(c, ADVT2_SINGLE);
      // (without Rts but with Rq: uf(:,:,kb) still holds profq's bottom boundary value, which the reference exchanges at solver.f:1290 and
      // later copies into t(:,:,kb) with `t = uf` -- Rq does not carry it, so it rides here)
      if (!rts) xch(c, 2, D3(c, uf), rimr ? P.kb : P.kbm1, D3(c, vf), P.kbm1);   // :436-437
      if (!rts) side_wait(c, SIDE_RQ);                        // ... and proft's ghost columns, which nothing will replace, need kh of the ghost lines
      if (!launch_proft2(c, D3(c, uf), D2(c, wtsurf), D2(c, tsurf), k.nbct, D3(c, vf), D2(c, wssurf), D2(c, ssurf), k.nbcs)) {   // :439-440, T and S in one launch
        launch_proft(c, D3(c, uf), D2(c, wtsurf), D2(c, tsurf), k.nbct);
        launch_proft(c, D3(c, vf), D2(c, wssurf), D2(c, ssurf), k.nbcs);
      }
      launch_bcond4_edges(c);                                 // :442
      double fold, fnew;
      int rc = restore_prepare(c, &fold, &fnew);              // :452 (record handling)
      if (rc) return rc;
      launch_ts_update(c, fold, fnew, k.nadv == 2, 0, ts_flags && !SW(c, RT_LOAD));   // :444-454 in one pass; trstr/srstr/taurstr on demand
      c->rho_rt_pending = c->rho_rt_cols = 0;                 // dens has rewritten rho(1..kbm1)
      c->rst_pending = 1; c->rst_fold = fold; c->rst_fnew = fnew;
      if (rts) {
        double *at[5] = {D3(c, t), D3(c, tb), D3(c, s), D3(c, sb), D3(c, rho)};
        const int nt[5] = {P.kb, P.kb, P.kb, P.kb, P.kb};
        const int rct = rim_round(c, SIDE_RTS, at, nt, 5);
        if (rct) return rct;
      }
    }
    if (c->ntr) {                                             // the passive tracers: behind :454, in front of :459, mode 3 and mode 4 alike
      const int rct = tracer_stage(c, lib_x);
      if (rct) return rct;
    }
    side_wait(c, SIDE_RQ);                                    // profu / profv average km with the neighbour line's
    const bool fuse = uv_fused(c);                            // :461-462 and the interior of :469-514 in one kernel (one tile)
    if (pomgpu_reg_kb(c)) {
      launch_advuv_col(c);                                    // :459-460 advu, advv in one pass
      if (fuse) launch_profuv_filter_reg(c, c->uvb_bot[0], c->uvb_bot[1]);
      else launch_profuv_reg(c);                              // :461-462 profu, profv with register-resident elimination vectors
    } else {
      launch_advu_profu(c, 1, 1);                             // :459-462
      launch_advv_profv(c, 1, 1);
    }
    if (!lib_x) xch(c, 2, D2(c, wubot), 1, D2(c, wvbot), 1);  // solver.f:1777, :1874
    launch_bcondorl3(c);                                      // :464 (does not read wubot, wvbot)
    const bool rim78 = lib_x && rim_side(c);
    if (rim78) {
      // rim rounds R7 and R8: both of the step's last velocity exchanges on the side stream.  R7 brings uf, vf (and wubot, wvbot); the
      // filter below runs on the cells this tile OWNS and leaves the ghost lines alone -- there :469-514 ends in u = uf, v = vf
      // (levels 1..kbm1; ub, vb and level kb of the ghost lines come with R8 as before), which R7's message writes as well.
      const int top = P.kb - 1;
      double *a7[4] = {D2(c, wubot), D2(c, wvbot), D3(c, uf), D3(c, vf)}, *b7[4] = {D2(c, wubot), D2(c, wvbot), D3(c, u), D3(c, v)};
      const int n7[4] = {1, 1, P.kbm1, P.kbm1};
      side_begin(c);                                          // (R7 records R8's event without owing a wait: R8 below records it again)
      const int rc7 = round8(c, 1, a7, n7, 4, b7);            // solver.f:1777,1874 + :466-467
      side_end(c, c->side_ev[SIDE_R8].ev);
      launch_uv_filter(c, 1);                                 // :469-514 on owned cells, beside R7
      double *a8[6] = {D3(c, ub), D3(c, vb), LEV3(c, D3(c, u), top), LEV3(c, D3(c, uf), top), LEV3(c, D3(c, v), top), LEV3(c, D3(c, vf), top)};
      const int n8[6] = {P.kb, P.kb, 1, 1, 1, 1};
      if (rc7) { side_begin(c); side_post(c, SIDE_R8); return rc7; }   // a failed R7: what it left on the side stream is still waited for
      const int rc8 = rim_round(c, SIDE_R8, a8, n8, 6);       // :516-521, behind the filter: R8 sends what it wrote
      if (rc8) return rc8;
    } else {
      if (lib_x) xch(c, 4, D2(c, wubot), 1, D2(c, wvbot), 1, D3(c, uf), P.kbm1, D3(c, vf), P.kbm1);   // solver.f:1777,1874 + :466-467
      else xch(c, 2, D3(c, uf), P.kbm1, D3(c, vf), P.kbm1);   // :466-467
      if (fuse) { launch_uv_filter_rim(c); c->uvf_pending = 1; }   // :469-514 on the frame; the interior's uf, vf stay a flag
      else launch_uv_filter(c);                               // :469-514
      if (lib_x) {
        // :516-521 exchange all kb levels of ub, u, uf, vb, v, vf.  For u, uf, v, vf the levels 1..kbm1 are redundant: uf, vf
        // were exchanged at :466-467 and not written since, and u = uf, v = vf are copies.  What is not valid in a ghost
        // column is their level kb (profu / profv write it on owned columns only).  ub, vb are needed in full: the filter
        // (:469-509) runs on ghost columns too, but from a u whose western / southern ghost cells missed the depth-mean
        // correction (:365-393 starts at i = 2, j = 2 and is not followed by an exchange).  2 x kb + 4 planes instead of 6 x kb.
        const int top = P.kb - 1;
        xch(c, 6, D3(c, ub), P.kb, D3(c, vb), P.kb, LEV3(c, D3(c, u), top), 1, LEV3(c, D3(c, uf), top), 1, LEV3(c, D3(c, v), top), 1, LEV3(c, D3(c, vf), top), 1);
      } else {
        xch(c, 6, D3(c, ub), P.kb, D3(c, u), P.kb, D3(c, uf), P.kb, D3(c, vb), P.kb, D3(c, v), P.kb, D3(c, vf), P.kb);   // :516-521
      }
    }
  }
  launch_int_tail(c);                                         // :525-531, and the derived coefficients of the new dt (k_coef_dt's) in the same pass
  const bool side_wr = c->tp.on && c->exch && c->wide.split && c->tp.wr_side;   // wr_side: no rank asked for POMGPU_WR_MAIN (agreed with side_agreed)
  if (side_wr && defer_wr && c->wide.on && !SW(c, WR_NODEFER)) {
    c->wr_deferred = 1;                                       // :534 and solver.f:2055 beside the next step's external substeps
    return POMGPU_OK;
  }
  // one tile: wr is a diagnostic for the output file that no routine of the step reads; it stays a flag until somebody looks at the
  // mirrors (pomgpu_wr_materialize) -- in a run of steps nobody does, and the next step's end simply sets the flag again
  if (wr_on_demand(c)) { c->wr_pending = 1; return POMGPU_OK; }
  c->wr_pending = 0;
  side_wait(c, SIDE_R8);                                      // realvertvl reads u, v of the eastern / northern ghost line
  launch_realvertvl(c);                                       // :534
  // solver.f:2055 on the side stream: the round runs beside check_velocity and the next step's lateral_viscosity; the next
  // step's early gather follows it on the same stream, and whoever looks at the state waits for it (side_join)
  if (side_wr) return wr_on_side(c, 0);
  xch(c, 1, D3(c, wr), P.kbm1);                               // solver.f:2055
  return POMGPU_OK;
}
extern "C" int pomgpu_mode_internal(pomgpu_ctx *c) { return mode_internal(c, 0); }
// Reads vaf alone (k_reduce.hip), a blk2d array outside the external mode's two generations: it needs the extended tile's 2-D state
// back and the side stream joined, not the lazily kept 3-D arrays (rho's round trip, the restore fields, wr) -- a host that steps
// routine by routine calls this after every mode_internal (advance.f:57) and would otherwise pay for all three every step
extern "C" int pomgpu_check_velocity(pomgpu_ctx *c, double *vamax, int *imax, int *jmax) {   // advance.f:611-641
  NEED_HOT(c);
  side_join(c);
  launch_check_velocity(c);
  double out[3];
  HIPCHK(c, hipMemcpyAsync(out, c->d_vel, sizeof out, hipMemcpyDeviceToHost, c->stream));
  int rc = pull_err(c);
  if (rc) return rc;
  if (vamax) *vamax = out[0];
  if (imax) *imax = (int)out[1];
  if (jmax) *jmax = (int)out[2];
  if (out[0] > c->con.vmaxl) {
    fprintf(stderr, "Error: velocity condition violated\n iint =%8d vamax =%12.3e   imax,jmax =%5d%5d\n", c->con.iint, out[0],
            (int)out[1], (int)out[2]);
    c->con.error_status = 1;
  }
  return POMGPU_OK;
}
// ---- surface forcing -- advance.f:77-93, bounds_forcing.f:871-983 ---------------------------------
extern "C" int pomgpu_set_forcing_record(pomgpu_ctx *c, int kind, int n, const double *a, const double *b) {
  NEED(c);
  if (kind < 0 || kind > 2 || n < 1 || !a || !b) return fail(c, POMGPU_EINVAL, "set_forcing_record: kind 0..2, n >= 1, two (im,jm) fields");
  if (pomgpu_ff_has(c, 0)) return fail(c, POMGPU_EINVAL, "set_forcing_record: the surface records come from a file (pomgpu_set_forcing_files)");
  const int sl = n % 4;
  const size_t bytes = sizeof(double) * (size_t)c->P.im * c->P.jm;
  for (int f = 0; f < 2; f++) {
    if (!c->frc_dev[kind][sl][f]) HIPCHK(c, hipMalloc((void **)&c->frc_dev[kind][sl][f], bytes));
    HIPCHK(c, hipMemcpyAsync(c->frc_dev[kind][sl][f], f ? b : a, bytes, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));                 // the caller may reuse its buffers
  c->frc_n[kind][sl] = n;
  c->frc_on = 1;
  return POMGPU_OK;
}
static int frc_read(pomgpu_ctx *c, int kind, int n, double *xf, double *yf) {   // what read_*_pnetcdf(n, ...) delivers
  const int sl = ((n % 4) + 4) % 4;
  if (pomgpu_ff_has(c, 0)) { const int rc = pomgpu_ff_fetch_surface(c, kind, n); if (rc) return rc; }   // the file's record n, into the slot the setter fills
  else if (n < 1 || c->frc_n[kind][sl] != n)
    return fail(c, POMGPU_EINVAL, "%s: record %d was not supplied (pomgpu_set_forcing_record)", kind == 0 ? "wind" : kind == 1 ? "heat" : "surface", n);
  launch_frc_load(c, c->frc_dev[kind][sl][0], c->frc_dev[kind][sl][1], xf, yf);
  return POMGPU_OK;
}
// wind and heat: two fields, a record every `tint` days, linear in time
static int frc_interp(pomgpu_ctx *c, int kind, double tint, int x, int xb, int xf, int y, int yb, int yf) {
  const pom_blkcon &k = c->con;
  const int istep = (int)(tint * 86400. / k.dti);
  if (istep < 1) return fail(c, POMGPU_EINVAL, "surface forcing: dti is longer than the record interval");
  int rc;
  if (k.iint == 1 && (rc = frc_read(c, kind, (k.iint + k.cont_bry) / istep + 1, SLOT2(c, xf), SLOT2(c, yf)))) return rc;   // :884-888
  if (k.iint == 1 || (k.iint + k.cont_bry) % istep == 0) {                                                                   // :890-902
    launch_copy2(c, SLOT2(c, xb), SLOT2(c, xf));
    launch_copy2(c, SLOT2(c, yb), SLOT2(c, yf));
    if (k.iint != k.iend && (rc = frc_read(c, kind, (k.iint + k.cont_bry + istep) / istep + 1, SLOT2(c, xf), SLOT2(c, yf)))) return rc;
  }
  const int ntime = (int)(k.time / tint);                                                                                    // :905-907
  const double fnew = k.time / tint - ntime, fold = 1. - fnew;
  launch_frc_interp(c, fold, fnew, SLOT2(c, x), SLOT2(c, xb), SLOT2(c, xf), SLOT2(c, y), SLOT2(c, yb), SLOT2(c, yf));
  return POMGPU_OK;
}
extern "C" int pomgpu_wind(pomgpu_ctx *c) {                   // bounds_forcing.f:871-912, twind = .125
  NEED_HOT(c);
  return frc_interp(c, 0, .125, P2_wusurf, P2_wusurfb, P2_wusurff, P2_wvsurf, P2_wvsurfb, P2_wvsurff);
}
extern "C" int pomgpu_heat(pomgpu_ctx *c) {                   // bounds_forcing.f:915-960, theat = .125
  NEED_HOT(c);
  return frc_interp(c, 1, .125, P2_wtsurf, P2_wtsurfb, P2_wtsurff, P2_swrad, P2_swradb, P2_swradf);
}
extern "C" int pomgpu_surface(pomgpu_ctx *c) {                // bounds_forcing.f:963-983: SST, no interpolation
  NEED_HOT(c);
  const pom_blkcon &k = c->con;
  const int isrf = (int)(.125 * 86400. / k.dti);
  if (isrf < 1) return fail(c, POMGPU_EINVAL, "surface forcing: dti is longer than the record interval");
  // pomgpu_set_surface_sss: ":979 ssurf(1:im,1:jm) = sss", which the reference keeps commented, as the load's second target
  if (k.iint == 1 || (k.iint + k.cont_bry) % isrf == 0)
    return frc_read(c, 2, (k.iint + k.cont_bry) / isrf + 1, SLOT2(c, P2_tsurf), c->sss_on ? SLOT2(c, P2_ssurf) : NULL);
  return POMGPU_OK;
}
// ---- water -- bounds_forcing.f:986-1020, the call advance.f:89 keeps commented ----------------------
extern "C" int pomgpu_set_water_record(pomgpu_ctx *c, int n, const double *w) {
  NEED(c);
  if (n < 0 || !w) return fail(c, POMGPU_EINVAL, "set_water_record: n >= 0, one (im,jm) field");
  if (pomgpu_ff_has_water(c)) return fail(c, POMGPU_EINVAL, "set_water_record: the water records come from a file (pomgpu_set_water_files)");
  const int sl = n % 4;
  const size_t bytes = sizeof(double) * (size_t)c->P.im * c->P.jm;
  if (!c->wat_dev[sl]) HIPCHK(c, hipMalloc((void **)&c->wat_dev[sl], bytes));
  HIPCHK(c, hipMemcpyAsync(c->wat_dev[sl], w, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));                 // the caller may reuse its buffer
  c->wat_n[sl] = n + 1;
  c->wat_on = 1;
  return POMGPU_OK;
}
extern "C" int pomgpu_set_water(pomgpu_ctx *c, int on) {
  NEED_RAW(c);
  c->wat_on = on ? 1 : 0;
  return POMGPU_OK;
}
extern "C" int pomgpu_set_surface_sss(pomgpu_ctx *c, int on) {
  NEED_RAW(c);
  c->sss_on = on ? 1 : 0;
  return POMGPU_OK;
}
// what read_water_pnetcdf(n, wssurff) delivers; shift: "wssurfb = wssurff" (:1001-1005) goes in front of it, in the same launch.  A
// record that cannot be had fails the step before any mirror is written: the shift is not made either
static int wat_have(pomgpu_ctx *c, int n) {                   // record n in its slot: the file's, fetched now, or the setter's
  if (pomgpu_ff_has_water(c)) return pomgpu_ff_fetch_water(c, n);
  if (n < 0 || c->wat_n[n % 4] != n + 1) return fail(c, POMGPU_EINVAL, "water: record %d was not supplied (pomgpu_set_water_record)", n);
  return POMGPU_OK;
}
static void wat_load(pomgpu_ctx *c, int n, int shift) {
  launch_frc_load1(c, c->wat_dev[n % 4], SLOT2(c, P2_wssurff), shift ? SLOT2(c, P2_wssurfb) : NULL);
}
// Not wind's schedule: no cont_bry, no "+ 1" on the record number (the files count from 0) and no "iint /= iend" around the second
// read -- a run whose last step is a multiple of iwater needs one more record
extern "C" int pomgpu_water(pomgpu_ctx *c) {
  NEED_HOT(c);
  const pom_blkcon &k = c->con;
  const double twater = 1.;                                   // "twater=1.": days
  const int iwater = (int)(twater * 86400. / k.dti);          // :994
  if (iwater < 1) return fail(c, POMGPU_EINVAL, "surface forcing: dti is longer than the record interval");
  const bool first = k.iint == 1, next = first || k.iint % iwater == 0;
  const int n0 = k.iint / iwater, n1 = (k.iint + iwater) / iwater;   // (n1 = n0 + 1 at iint == 1: two slots)
  int rc;
  if (first && (rc = wat_have(c, n0))) return rc;             // both records are had before either is loaded
  if (next && (rc = wat_have(c, n1))) return rc;
  if (first) wat_load(c, n0, 0);                                                                 // :998
  if (next) wat_load(c, n1, 1);                                                                  // :1000-1007
  const int ntime = (int)(k.time / twater);                                                      // :1010-1012
  const double fnew = k.time / twater - ntime, fold = 1. - fnew;
  launch_frc_interp1(c, fold, fnew, SLOT2(c, P2_wssurf), SLOT2(c, P2_wssurfb), SLOT2(c, P2_wssurff));
  return POMGPU_OK;
}
extern "C" int pomgpu_surface_forcing(pomgpu_ctx *c) {        // advance.f:77-93
  int rc;
  if ((rc = pomgpu_wind(c))) return rc;
  if ((rc = pomgpu_heat(c))) return rc;
  if (c->wat_on && (rc = pomgpu_water(c))) return rc;         // advance.f:89, where the reference keeps the call commented
  return pomgpu_surface(c);
}
// ---- lateral_bc -- bounds_forcing.f:593-868 --------------------------------------------------------
extern "C" int pomgpu_set_lateral_record(pomgpu_ctx *c, int n, const double *const *a) {
  NEED(c);
  if (n < 1 || !a) return fail(c, POMGPU_EINVAL, "set_lateral_record: n >= 1 and 20 arrays");
  if (pomgpu_ff_has(c, 1)) return fail(c, POMGPU_EINVAL, "set_lateral_record: the lateral records come from a file (pomgpu_set_forcing_files)");
  const KP &P = c->P;
  const size_t njk = (size_t)P.jml * P.kb, nik = (size_t)P.iml * P.kb;
  const size_t total = 8 * njk + 8 * nik + 2 * (size_t)P.jml + 2 * (size_t)P.iml;
  const int sl = n % 4;
  if (!c->lat_dev[sl]) HIPCHK(c, hipMalloc((void **)&c->lat_dev[sl], total * sizeof(double)));
  size_t off = 0;
  for (int q = 0; q < 20; q++) {
    const size_t len = q < 8 ? njk : (q < 16 ? nik : (q < 18 ? (size_t)P.jml : (size_t)P.iml));
    if (!a[q]) return fail(c, POMGPU_EINVAL, "set_lateral_record: array %d is NULL", q);
    HIPCHK(c, hipMemcpyAsync(c->lat_dev[sl] + off, a[q], len * sizeof(double), hipMemcpyHostToDevice, c->stream));
    off += len;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->lat_n[sl] = n;
  c->lat_on = 1;
  return POMGPU_OK;
}
static int lat_read(pomgpu_ctx *c, int n) {
  const int sl = ((n % 4) + 4) % 4;
  if (pomgpu_ff_has(c, 1)) { const int rc = pomgpu_ff_fetch_lateral(c, n); if (rc) return rc; }
  else if (n < 1 || c->lat_n[sl] != n) return fail(c, POMGPU_EINVAL, "lateral_bc: record %d was not supplied (pomgpu_set_lateral_record)", n);
  launch_lat(c, 0, c->lat_dev[sl], 0., 0.);
  return POMGPU_OK;
}
extern "C" int pomgpu_lateral_bc(pomgpu_ctx *c) {
  NEED_HOT(c);
  const pom_blkcon &k = c->con;
  const double tbc = (double)(1.f / 24.f);                    // "tbc=1./24.": a REAL(4) constant (:602)
  const int ibc = (int)(tbc * 86400. / k.dti);
  if (ibc < 1) return fail(c, POMGPU_EINVAL, "lateral_bc: dti is longer than the record interval");
  const int ntime = (int)(k.time / tbc);
  int rc;
  if (k.iint == 1 && (rc = lat_read(c, (k.iint + k.cont_bry) / ibc + 1))) return rc;           // :607-636
  if (k.iint == 1 || (k.iint + k.cont_bry) % ibc == 0) {                                       // :740-772
    launch_lat(c, 1, NULL, 0., 0.);
    if (k.iint != k.iend && (rc = lat_read(c, (k.iint + k.cont_bry + ibc) / ibc + 1))) return rc;
  }
  const double fnew = k.time / tbc - (double)ntime, fold = 1. - fnew;                          // :774-775
  launch_lat(c, 2, NULL, fold, fnew);
  return POMGPU_OK;
}
extern "C" int pomgpu_domain_stats(pomgpu_ctx *c, double *out, int sums_only) {   // advance.f:644-756
  NEED(c);
  if (!out) return POMGPU_EINVAL;
  launch_domain_stats(c, c->d_stats);
  double s[7];                                                // vtot atot mtot stot sum(tb*dvol) sum(et*darea) ekin
  HIPCHK(c, hipMemcpyAsync(s, c->d_stats, sizeof s, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double tavg = s[4], savg = 0., eavg = s[5];
  if (!sums_only) {                                           // what my_task 0 does after sum0d_mpi (:680-686, :728-736)
    eavg = (s[1] != 0) ? s[5] / s[1] : 0.;
    if (s[0] != 0) { tavg = s[4] / s[0]; savg = s[3] / s[0]; } else { tavg = 0.; savg = 0.; }
  }
  out[0] = s[0]; out[1] = s[1]; out[2] = s[2]; out[3] = s[3]; out[4] = tavg; out[5] = savg; out[6] = eavg; out[7] = s[6];
  return POMGPU_OK;
}
// ---- the time-mean output (include/pomgpu.h; the kernels and the mean file: cdf_out.hip) ------------------------------------------------
// The step's accumulation: acc = acc + x with x what pomgpu_download would show now, read from wherever it lives.  uab, vab, elb come from
// the CURRENT generation of the external mode's arrays (KP::x2) -- no ext_canonical, whose seven copies a step that ends in the other
// buffer set would otherwise pay every step; u v t s rho w are final in their mirrors when mode_internal returns (the depth-mean
// correction is stored by the filter, dens has rewritten rho, w has no lazy form); wr, uf / vf and the restore fields, which the step
// keeps lazily, are not among the nine and stay lazy.  On tiles the ghost lines of u, v (R8) and t, s, rho (Rts) are still travelling on
// the side stream: the main stream waits for those two events here -- which the next step's first kernels would do a few launches later
// -- and posts no round of its own.  The wide-halo mode has scattered the 2-D result back when the last substep ended (wide_flush).
// What only a host that calls this out of the step's order can leave behind -- a held substep, the extended tile's 2-D state, rho's round
// trip -- is completed first: correct values come first.
static int mean_accumulate(pomgpu_ctx *c) {
  ext_flush_deferred(c);
  wide_flush(c);
  side_wait(c, SIDE_RW); side_wait(c, SIDE_R8); side_wait(c, SIDE_RTS);
  rho_materialize(c);
  const KP &P = c->P;
  const double *x[9] = {P.x2[X2_uab], P.x2[X2_vab], P.x2[X2_elb], D3(c, u), D3(c, v), D3(c, t), D3(c, s), D3(c, rho), D3(c, w)};
  launch_mean_accum(c, x);
  c->mean_count += 1;
  if (c->trmean_acc) {                                        // the tracers: tr is final when mode_internal returns (k_tr_update), its ghost
    launch_tracer_mean_accum(c);                              // lines travelled on this stream.  ONE more launch of k_mean_accum per step
    c->trmean_count += 1;
  }
  return POMGPU_OK;
}
extern "C" int pomgpu_mean_accumulate(pomgpu_ctx *c) {
  NEED_RAW(c);
  if (!c->mean_acc) return fail(c, POMGPU_EINVAL, "mean_accumulate: the time-mean output is off (pomgpu_set_mean_output)");
  return mean_accumulate(c);
}
extern "C" int pomgpu_mean_count(pomgpu_ctx *c) { return c && c->mean_acc ? c->mean_count : -1; }
// The tracers' accumulators exist if and only if the mean is on and tracers are registered: both switches end here.  They are created
// anew at +0.0 with count 0 -- pomgpu_set_mean_output(1) zeroes every sum, pomgpu_set_tracers(n > 0) zeroes the tracers themselves -- and
// the nine fields' accumulators and count are not looked at
static void trmean_free(pomgpu_ctx *c) {
  if (c->trmean_acc) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->trmean_acc); }
  c->trmean_acc = NULL; c->trmean_stride = 0; c->trmean_count = 0;
}
static int trmean_reset(pomgpu_ctx *c) {
  trmean_free(c);
  if (!c->mean_acc || !c->ntr) return POMGPU_OK;
  const size_t stride = c->P.n3 + (c->P.n3 & 1), total = stride * (size_t)c->ntr;
  double *acc = NULL;
  if (hipMalloc((void **)&acc, total * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return fail(c, POMGPU_ENOMEM, "no memory for the tracers' mean accumulators (%zu MB)", total * sizeof(double) >> 20); }
  c->trmean_acc = acc; c->trmean_stride = stride;
  HIPCHK(c, hipMemsetAsync(acc, 0, total * sizeof(double), c->stream));
  return POMGPU_OK;
}
extern "C" int pomgpu_set_mean_output(pomgpu_ctx *c, int on) {
#ifdef POMGPU_STORE_F32
  if (c) return fail(c, POMGPU_EINVAL, "set_mean_output: not in the fp32-storage variant (download and write from the host)");
#endif
  NEED_RAW(c);
  if (c->flags & POMGPU_CTX_2D) return fail(c, POMGPU_EINVAL, "set_mean_output: a context with 3-D arrays");
  const KP &P = c->P;
  if (!on) {
    if (c->mean_acc) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->mean_acc); }
    c->mean_acc = NULL; c->mean_count = 0;
    trmean_free(c);
    return POMGPU_OK;
  }
  // nine accumulators in one allocation, each n2 / n3 doubles: a 3-D one starts on a 16-byte boundary exactly where its mirror does
  // (k_mean_accum's 16-byte form), a 2-D one where its blk2d array does
  static const int is3d[9] = {0, 0, 0, 1, 1, 1, 1, 1, 1};
  const double *mirror[9] = {D2(c, uab), D2(c, vab), D2(c, elb), D3(c, u), D3(c, v), D3(c, t), D3(c, s), D3(c, rho), D3(c, w)};
  size_t off[9], cur = 0;
  for (int q = 0; q < 9; q++) {
    if ((cur & 1) != (((size_t)mirror[q] >> 3) & 1)) cur++;
    off[q] = cur;
    cur += is3d[q] ? P.n3 : P.n2;
  }
  if (!c->mean_acc) {
    double *acc = NULL;
    if (hipMalloc((void **)&acc, cur * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return fail(c, POMGPU_ENOMEM, "set_mean_output: no memory for the accumulators (%zu MB)", cur * sizeof(double) >> 20); }
    c->mean_acc = acc;
  }
  for (int q = 0; q < 9; q++) c->mean_off[q] = off[q];
  c->mean_count = 0;
  HIPCHK(c, hipMemsetAsync(c->mean_acc, 0, cur * sizeof(double), c->stream));   // +0.0 everywhere, behind whatever still accumulates
  return trmean_reset(c);                                     // and the tracers registered now
}
// ---- passive tracers: the state (include/pomgpu.h; the stage: tracer_stage above) ---------------------------------------------------------
static void tracers_free(pomgpu_ctx *c) {
  for (int n = 0; n < POMGPU_TRMAX; n++) {
    pomgpu_ctx::pomgpu_tracer &t = c->trc[n];
    (void)hipFree(t.trb); (void)hipFree(t.tr); (void)hipFree(t.trf); (void)hipFree(t.q); (void)hipFree(t.wsurf); (void)hipFree(t.surf);
    if (t.clim != c->tr_zero3) (void)hipFree(t.clim);
    for (int d = 0; d < 4; d++) (void)hipFree(t.bd[d]);
    memset(&t, 0, sizeof t);
  }
  (void)hipFree(c->tr_zero3);
  c->tr_zero3 = NULL;
  c->ntr = 0;
  trmean_free(c);
  (void)hipFree(c->d_trstats);
  c->d_trstats = NULL;
}
// doubles of array `which` of a tracer (enum pomgpu_tracer_array), 0 = no such array
static size_t tracer_len(const pomgpu_ctx *c, int which) {
  const KP &P = c->P;
  switch (which) {
    case POMGPU_TR_TRB: case POMGPU_TR_TR: case POMGPU_TR_CLIM: case POMGPU_TR_SOURCE: return P.n3;
    case POMGPU_TR_WSURF: case POMGPU_TR_SURF: return P.n2;
    case POMGPU_TR_BE: case POMGPU_TR_BW: return (size_t)P.kb * P.jml;
    case POMGPU_TR_BN: case POMGPU_TR_BS: return (size_t)P.kb * P.iml;
    default: return 0;
  }
}
static double **tracer_slot(pomgpu_ctx *c, int n, int which) {
  pomgpu_ctx::pomgpu_tracer &t = c->trc[n - 1];
  switch (which) {
    case POMGPU_TR_TRB: return &t.trb;
    case POMGPU_TR_TR: return &t.tr;
    case POMGPU_TR_CLIM: return &t.clim;
    case POMGPU_TR_SOURCE: return &t.q;
    case POMGPU_TR_WSURF: return &t.wsurf;
    case POMGPU_TR_SURF: return &t.surf;
    case POMGPU_TR_BE: return &t.bd[0];
    case POMGPU_TR_BW: return &t.bd[1];
    case POMGPU_TR_BN: return &t.bd[2];
    default: return &t.bd[3];
  }
}
static int tracer_zeros(pomgpu_ctx *c, double **p, size_t n) {
  if (!*p && hipMalloc((void **)p, n * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    *p = NULL;
    return fail(c, POMGPU_ENOMEM, "set_tracers: no memory for a tracer array (%zu MB)", n * sizeof(double) >> 20);
  }
  HIPCHK(c, hipMemsetAsync(*p, 0, n * sizeof(double), c->stream));
  return POMGPU_OK;
}
extern "C" int pomgpu_tracer_count(pomgpu_ctx *c) { return c ? c->ntr : 0; }
extern "C" int pomgpu_set_tracers(pomgpu_ctx *c, int n) {
  if (c) { F32_REFUSE(c, "set_tracers"); }
  NEED_RAW(c);
  if (c->flags & POMGPU_CTX_2D) return fail(c, POMGPU_EINVAL, "set_tracers: a context with 3-D arrays");
  if (n < 0 || n > POMGPU_MAXTRACERS) return fail(c, POMGPU_EINVAL, "set_tracers: %d tracers asked for, 0..%d are possible", n, POMGPU_MAXTRACERS);
  if (c->ntr) HIPCHK(c, hipStreamSynchronize(c->stream));     // arrays are about to be freed: behind the steps that still use them
  if (n != c->ntr) tracers_free(c);                           // another number: the arrays go
  if (!n) return POMGPU_OK;
  int rc;
  if ((rc = tracer_zeros(c, &c->tr_zero3, c->P.n3))) { tracers_free(c); return rc; }
  for (int t = 1; t <= n; t++) {
    pomgpu_ctx::pomgpu_tracer &T = c->trc[t - 1];
    if (T.clim && T.clim != c->tr_zero3) (void)hipFree(T.clim);   // a kept allocation: an own clim or q goes back to the default
    (void)hipFree(T.q);
    T.clim = c->tr_zero3; T.q = NULL; T.nbc = 1; T.lam = 0.;
    static const int own[] = {POMGPU_TR_TRB, POMGPU_TR_TR, POMGPU_TR_WSURF, POMGPU_TR_SURF, POMGPU_TR_BE, POMGPU_TR_BW, POMGPU_TR_BN, POMGPU_TR_BS};
    for (int q = 0; q < 8; q++)
      if ((rc = tracer_zeros(c, tracer_slot(c, t, own[q]), tracer_len(c, own[q])))) { tracers_free(c); return rc; }
    if ((rc = tracer_zeros(c, &T.trf, c->P.n3))) { tracers_free(c); return rc; }
  }
  c->ntr = n;
  return trmean_reset(c);                                     // with the mean on: sums of +0.0 and count 0 for the tracers that are +0.0 now
}
static int tracer_args(pomgpu_ctx *c, const char *what, int n, int which, bool has_which = true) {
  if (!c->ntr) return fail(c, POMGPU_EINVAL, "%s: no tracers are registered (pomgpu_set_tracers)", what);
  if (n < 1 || n > c->ntr) return fail(c, POMGPU_EINVAL, "%s: tracer %d, 1..%d are registered", what, n, c->ntr);
  if (has_which && !tracer_len(c, which)) return fail(c, POMGPU_EINVAL, "%s: %d names no tracer array (enum pomgpu_tracer_array)", what, which);
  return POMGPU_OK;
}
extern "C" int pomgpu_tracer_set(pomgpu_ctx *c, int n, int nbc, double lam) {
  if (c) { F32_REFUSE(c, "tracer_set"); }
  NEED_RAW(c);
  int rc = tracer_args(c, "tracer_set", n, 0, false);
  if (rc) return rc;
  if (nbc != 1 && nbc != 3)
    return fail(c, POMGPU_EINVAL, "tracer_set: nbc = %d; a tracer takes 1 (the flux wtrsurf) or 3 (the value trsurf), the short-wave forms 2 and 4 are T's", nbc);
  c->trc[n - 1].nbc = nbc; c->trc[n - 1].lam = lam;
  return POMGPU_OK;
}
extern "C" int pomgpu_tracer_upload(pomgpu_ctx *c, int n, int which, const double *host) {
  if (c) { F32_REFUSE(c, "tracer_upload"); }
  NEED_RAW(c);
  int rc = tracer_args(c, "tracer_upload", n, which);
  if (rc) return rc;
  double **slot = tracer_slot(c, n, which);
  const size_t len = tracer_len(c, which);
  const bool opt = which == POMGPU_TR_CLIM || which == POMGPU_TR_SOURCE;
  if (!host && !opt) return fail(c, POMGPU_EINVAL, "tracer_upload: no host array");
  if (opt) {                                                  // own array on first upload; NULL: back to the default
    double *def = which == POMGPU_TR_CLIM ? c->tr_zero3 : NULL;
    if (!host) {
      if (*slot != def) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(*slot); *slot = def; }
      return POMGPU_OK;
    }
    if (*slot == def) {
      double *p = NULL;
      if (hipMalloc((void **)&p, len * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return fail(c, POMGPU_ENOMEM, "tracer_upload: no memory for the array (%zu MB)", len * sizeof(double) >> 20); }
      *slot = p;
    }
  }
  HIPCHK(c, hipMemcpyAsync(*slot, host, len * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));                 // the host array is the caller's again
  return POMGPU_OK;
}
extern "C" int pomgpu_tracer_download(pomgpu_ctx *c, int n, int which, double *host) {
  if (c) { F32_REFUSE(c, "tracer_download"); }
  NEED_RAW(c);
  int rc = tracer_args(c, "tracer_download", n, which);
  if (rc) return rc;
  if (!host) return fail(c, POMGPU_EINVAL, "tracer_download: no host array");
  const double *src = *tracer_slot(c, n, which);
  const size_t len = tracer_len(c, which);
  if (!src) { memset(host, 0, len * sizeof(double)); return POMGPU_OK; }   // no source array: zeros
  HIPCHK(c, hipMemcpyAsync(host, src, len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return POMGPU_OK;
}
extern "C" int pomgpu_tracer_get(pomgpu_ctx *c, int n, int *nbc, double *lam) {
  if (c) { F32_REFUSE(c, "tracer_get"); }
  NEED_RAW(c);
  int rc = tracer_args(c, "tracer_get", n, 0, false);
  if (rc) return rc;
  if (nbc) *nbc = c->trc[n - 1].nbc;
  if (lam) *lam = c->trc[n - 1].lam;
  return POMGPU_OK;
}
// the inventory: tot avg min max per tracer (k_reduce.hip: k_tracer_stats, two launches for all tracers).  The host emulation has no lanes
// to shuffle between and forms the same four numbers here, the sums in scan order
extern "C" int pomgpu_tracer_stats(pomgpu_ctx *c, double *out) {
  if (c) { F32_REFUSE(c, "tracer_stats"); }
  NEED(c);
  if (!c->ntr) return fail(c, POMGPU_EINVAL, "tracer_stats: no tracers are registered (pomgpu_set_tracers)");
  if (!out) return fail(c, POMGPU_EINVAL, "tracer_stats: no host array");
  if (!c->d_trstats && hipMalloc((void **)&c->d_trstats, 4 * POMGPU_TRMAX * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    c->d_trstats = NULL;
    return fail(c, POMGPU_ENOMEM, "tracer_stats: no memory for the result");
  }
#ifndef POMGPU_EMU
  launch_tracer_stats(c, c->d_trstats);
#else
  {
    const KP &P = c->P;
    for (int t = 0; t < c->ntr; t++) {
      double vt = 0., tot = 0., mn = __DBL_MAX__, mx = -__DBL_MAX__;
      for (int j = 1; j <= P.jm; j++)
        for (int i = 1; i <= P.im; i++) {
          const bool inner = i >= 2 && i <= P.imm1 && j >= 2 && j <= P.jmm1;
          const double fs = F2(fsm, i, j), darea = F2(dx, i, j) * F2(dy, i, j) * fs, dtc = F2(dt, i, j);
          for (int k = 1; k <= P.kbm1; k++) {
            const double dvol = darea * dtc * F1(dz, k), x = c->trc[t].tr[IX3(i, j, k)];
            if (inner) { vt = vt + dvol; tot = tot + c->trc[t].trb[IX3(i, j, k)] * dvol; }
            if (fs != 0.) { mn = x < mn ? x : mn; mx = x > mx ? x : mx; }
          }
        }
      c->d_trstats[4 * t] = tot; c->d_trstats[4 * t + 1] = vt != 0. ? tot / vt : 0.; c->d_trstats[4 * t + 2] = mn; c->d_trstats[4 * t + 3] = mx;
    }
  }
#endif
  HIPCHK(c, hipMemcpyAsync(out, c->d_trstats, 4 * (size_t)c->ntr * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return POMGPU_OK;
}
extern "C" int pomgpu_tracer_mean_count(pomgpu_ctx *c) { return c && c->trmean_acc ? c->trmean_count : -1; }
extern "C" int pomgpu_tracer_mean_download(pomgpu_ctx *c, int n, double *host) {
  if (c) { F32_REFUSE(c, "tracer_mean_download"); }
  NEED_RAW(c);
  int rc = tracer_args(c, "tracer_mean_download", n, 0, false);
  if (rc) return rc;
  if (!host) return fail(c, POMGPU_EINVAL, "tracer_mean_download: no host array");
  if (!c->trmean_acc) return fail(c, POMGPU_EINVAL, "tracer_mean_download: the time-mean output is off (pomgpu_set_mean_output)");
  if (c->trmean_count < 1) return fail(c, POMGPU_EINVAL, "tracer_mean_download: no step has been accumulated since the switch, pomgpu_set_tracers or the last mean file");
  const size_t len = c->P.n3;
  HIPCHK(c, hipMemcpyAsync(host, c->trmean_acc + (size_t)(n - 1) * c->trmean_stride, len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const double cnt = (double)c->trmean_count;
  for (size_t e = 0; e < len; e++) host[e] = host[e] / cnt;    // the division k_mean_snapshot makes
  return POMGPU_OK;
}
// ---- Lagrangian floats (include/pomgpu.h; the kernels: k_float.hpp) -------------------------------------------------------------------------
// The step reads u v w dt dx dy fsm z zz as pomgpu_download would show them: what mean_accumulate completes first is what this stage needs
// complete, and in the step's own order it finds nothing to do.  No lazily kept array is formed: wr, uf / vf, the restore fields and aam's
// spare home are not among the operands
static void float_stage(pomgpu_ctx *c) {
  ext_flush_deferred(c);
  wide_flush(c);
  side_wait(c, SIDE_RW); side_wait(c, SIDE_R8); side_wait(c, SIDE_RTS);
  launch_float_step(c);
}
static void floats_free(pomgpu_ctx *c) {
  (void)hipFree(c->flt_x); (void)hipFree(c->flt_y); (void)hipFree(c->flt_s); (void)hipFree(c->flt_smp);
  (void)hipFree(c->flt_status); (void)hipFree(c->flt_kind); (void)hipFree(c->flt_id);
  c->flt_x = c->flt_y = c->flt_s = c->flt_smp = NULL;
  c->flt_status = c->flt_kind = c->flt_id = NULL;
  c->nflt = 0;
}
// what pomgpu_float_upload and pomgpu_read_floats (cdf_in.hip) share: every refusal, then the new arrays, then the old ones go.  status:
// a float whose entry is not ACTIVE keeps it over the admission's verdict (a checkpoint); NULL: the admission decides alone
int pomgpu_float_register(pomgpu_ctx *c, const char *what, int n, const double *x, const double *y, const double *sig, const int *kind, const int *id,
                          const int *status) {
  NEED_RAW(c);
  if (n < 0 || n > POMGPU_MAXFLOATS) return fail(c, POMGPU_EINVAL, "%s: %d floats asked for, 0..%d are possible", what, n, POMGPU_MAXFLOATS);
  if (n && (!x || !y || !sig)) return fail(c, POMGPU_EINVAL, "%s: no host array for x, y or sig", what);
  const KP &P = c->P;
  if (!(P.W && P.E && P.S && P.N) || c->parent)
    return fail(c, POMGPU_EINVAL, "%s: this context is a tile with neighbours; floats live on a single tile, moving them between ranks takes a message round a step that the library does not have", what);
  if (c->flags & POMGPU_CTX_2D) return fail(c, POMGPU_EINVAL, "%s: a context with 3-D arrays", what);
  if (c->nflt) HIPCHK(c, hipStreamSynchronize(c->stream));     // the steps that still use the old arrays
  if (!n) { floats_free(c); return POMGPU_OK; }
  const size_t N = (size_t)n;
  double *d[3] = {NULL, NULL, NULL};
  int *q[3] = {NULL, NULL, NULL}, *keep = NULL;
  bool ok = true;
  for (int a = 0; a < 3 && ok; a++) ok = hipMalloc((void **)&d[a], N * sizeof(double)) == hipSuccess && hipMalloc((void **)&q[a], N * sizeof(int)) == hipSuccess;
  if (ok && status) ok = hipMalloc((void **)&keep, N * sizeof(int)) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    for (int a = 0; a < 3; a++) { (void)hipFree(d[a]); (void)hipFree(q[a]); }
    (void)hipFree(keep);
    return fail(c, POMGPU_ENOMEM, "%s: no memory for %d floats", what, n);
  }
  floats_free(c);                                             // from here on the float set changes
  c->flt_x = d[0]; c->flt_y = d[1]; c->flt_s = d[2]; c->flt_status = q[0]; c->flt_kind = q[1]; c->flt_id = q[2];
  c->nflt = n;
  std::vector<int> iota;
  if (!id) { iota.resize(N); for (size_t e = 0; e < N; e++) iota[e] = (int)e; id = iota.data(); }
  int rc = POMGPU_OK;
  auto put = [&](void *dst, const void *src, size_t bytes) { if (!rc && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = POMGPU_EHIP; };
  put(c->flt_x, x, N * sizeof(double)); put(c->flt_y, y, N * sizeof(double)); put(c->flt_s, sig, N * sizeof(double));
  put(c->flt_id, id, N * sizeof(int));
  if (kind) put(c->flt_kind, kind, N * sizeof(int));
  else if (hipMemsetAsync(c->flt_kind, 0, N * sizeof(int), c->stream) != hipSuccess) rc = POMGPU_EHIP;
  if (keep) put(keep, status, N * sizeof(int));
  if (!rc) launch_float_admit(c, keep);
  if (hipStreamSynchronize(c->stream) != hipSuccess) rc = POMGPU_EHIP;   // the host arrays are the caller's again
  (void)hipFree(keep);
  if (rc) { floats_free(c); return fail(c, POMGPU_EHIP, "%s: a HIP call failed while the floats were copied; none are registered", what); }
  return POMGPU_OK;
}
extern "C" int pomgpu_float_upload(pomgpu_ctx *c, int n, const double *x, const double *y, const double *sig, const int *kind, const int *id) {
  if (c) { F32_REFUSE(c, "float_upload"); }
  return pomgpu_float_register(c, "float_upload", n, x, y, sig, kind, id, NULL);
}
extern "C" int pomgpu_float_count(pomgpu_ctx *c) { return c ? c->nflt : 0; }
extern "C" int pomgpu_float_download(pomgpu_ctx *c, double *x, double *y, double *sig, int *status, int *kind, int *id) {
  if (c) { F32_REFUSE(c, "float_download"); }
  NEED_RAW(c);
  if (!c->nflt) return POMGPU_OK;
  const size_t N = (size_t)c->nflt;
  if (x) HIPCHK(c, hipMemcpyAsync(x, c->flt_x, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (y) HIPCHK(c, hipMemcpyAsync(y, c->flt_y, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (sig) HIPCHK(c, hipMemcpyAsync(sig, c->flt_s, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (status) HIPCHK(c, hipMemcpyAsync(status, c->flt_status, N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (kind) HIPCHK(c, hipMemcpyAsync(kind, c->flt_kind, N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (id) HIPCHK(c, hipMemcpyAsync(id, c->flt_id, N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return POMGPU_OK;
}
extern "C" int pomgpu_float_step(pomgpu_ctx *c) {
  if (c) { F32_REFUSE(c, "float_step"); }
  NEED_RAW(c);
  if (!c->nflt) return fail(c, POMGPU_EINVAL, "float_step: no floats are registered (pomgpu_float_upload)");
  float_stage(c);
  return POMGPU_OK;
}
extern "C" int pomgpu_float_sample(pomgpu_ctx *c, double *out) {
  if (c) { F32_REFUSE(c, "float_sample"); }
  NEED_RAW(c);
  if (!c->nflt) return fail(c, POMGPU_EINVAL, "float_sample: no floats are registered (pomgpu_float_upload)");
  if (!out) return fail(c, POMGPU_EINVAL, "float_sample: no host array");
  const size_t bytes = 5 * (size_t)c->nflt * sizeof(double);
  if (!c->flt_smp && hipMalloc((void **)&c->flt_smp, bytes) != hipSuccess) {
    (void)hipGetLastError();
    c->flt_smp = NULL;
    return fail(c, POMGPU_ENOMEM, "float_sample: no memory for the result (%zu MB)", bytes >> 20);
  }
  { const int rcm = pomgpu_materialize(c); if (rcm) return rcm; }   // t s et dt as pomgpu_download would show them
  launch_float_sample(c, c->flt_smp);
  HIPCHK(c, hipMemcpyAsync(out, c->flt_smp, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return POMGPU_OK;
}
// ---- tides (include/pomgpu.h "tides"; tide_add in k_ext.hip, the other kernels: k_tide.hpp) -------------------------------------------------
static void tide_phasors(const pomgpu_ctx *c, double t, double *out) {
  for (int q = 0; q < c->ntide; q++) { out[2 * q] = cos(c->tide_omega[q] * t); out[2 * q + 1] = sin(c->tide_omega[q] * t); }
}
static double tide_time(const pom_blkcon &k, int iint, int iext) {
  return (k.time0 * 86400. + k.dti * (double)(iint - 1)) + k.dte * (double)iext;
}
// the coefficient lines of context t (the tile, or its extended tile `off` cells further west / south) cut out of the global lines and put on
// the device; KP's members set.  0 or a pomgpu_status; nothing changes on failure
static int tide_cut(pomgpu_ctx *c, pomgpu_ctx *t, int ox, int oy, int sides) {
  KP &P = t->P;
  const int nc = c->ntide, ldj = P.jml, ldi = P.iml;
  const size_t nj = (size_t)2 * nc * 4 * ldj, ni = (size_t)2 * nc * 4 * ldi;
  std::vector<double> h(nj + ni, 0.);
  for (int side = 0; side < 4; side++) {
    const bool alongj = side < 2;
    const int ld = alongj ? ldj : ldi, len = alongj ? P.jm : P.im, ng = alongj ? c->tide_g[1] : c->tide_g[0];
    const int g0 = (alongj ? c->tide_g[3] - oy : c->tide_g[2] - ox) - 1;      // global index (0-based) of the context's point 1
    for (int q = 0; q < 4; q++) {
      const double *src = c->tide_host[side][q];
      if (!src) continue;
      for (int k = 0; k < nc; k++) {
        double *dst = h.data() + (alongj ? 0 : nj) + ((size_t)((side & 1) * nc + k) * 4 + q) * ld;
        for (int a = 0; a < len; a++) dst[a] = src[(size_t)k * ng + g0 + a];
      }
    }
  }
  double *dev = NULL;
  if (hipMalloc((void **)&dev, h.size() * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return fail(c, POMGPU_ENOMEM, "set_tides: no memory for the coefficient lines"); }
  if (hipMemcpyAsync(dev, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
    (void)hipFree(dev);
    return fail(c, POMGPU_EHIP, "set_tides: the coefficient lines could not be copied");
  }
  (void)hipFree(t->tide_dev);
  t->tide_dev = dev;
  P.ntide = nc; P.tide_sides = sides; P.tide_ldj = ldj; P.tide_ldi = ldi;
  P.tide_j = dev; P.tide_i = dev + nj;
  P.tide_ph = c->tide_tab;
  return POMGPU_OK;
}
static void tide_off(pomgpu_ctx *t) {
  KP &P = t->P;
  P.ntide = P.tide_sides = P.tide_ldj = P.tide_ldi = 0;
  P.tide_ph = P.tide_j = P.tide_i = NULL;
  (void)hipFree(t->tide_dev);
  t->tide_dev = NULL;
}
static void harm_free(pomgpu_ctx *c) {
  if (c->harm_acc) (void)hipStreamSynchronize(c->stream);
  (void)hipFree(c->harm_acc); (void)hipFree(c->harm_coef); (void)hipFree(c->harm_file);
  c->harm_acc = c->harm_coef = c->harm_file = NULL;
  c->harm_on = c->harm_count = 0; c->harm_every = 1;
}
static void tides_free(pomgpu_ctx *c) {
  harm_free(c);
  tide_off(c);
  if (c->wide.x) tide_off(c->wide.x);
  for (int s = 0; s < 4; s++) for (int q = 0; q < 4; q++) { free(c->tide_host[s][q]); c->tide_host[s][q] = NULL; }
  (void)hipFree(c->tide_tab);
  c->tide_tab = NULL; c->tide_tab_cap = 0; c->tide_key_ok = 0;
  c->ntide = 0;
}
// is the stretch of a context of n points that begins `off` points before the tile's inside the global line of ng points?
static bool tide_inside(int g1, int off, int n, int ng) { return g1 - off >= 1 && g1 - off - 1 + n <= ng; }
// the extended tile of the wide-halo mode takes the table of its tile (pomgpu_set_wide_external, behind ctx_create)
static int tide_widen(pomgpu_ctx *c) {
  if (!c->ntide || !c->wide.x) return POMGPU_OK;
  const pomgpu_wide &Wd = c->wide;
  if (!tide_inside(c->tide_g[2], Wd.ox, Wd.x->P.im, c->tide_g[0]) || !tide_inside(c->tide_g[3], Wd.oy, Wd.x->P.jm, c->tide_g[1]))
    return fail(c, POMGPU_EINVAL, "tides: the extended tile's stretch lies outside the global line (%d x %d from %d, %d of %d x %d)", Wd.x->P.im, Wd.x->P.jm,
                c->tide_g[2] - Wd.ox, c->tide_g[3] - Wd.oy, c->tide_g[0], c->tide_g[1]);
  return tide_cut(c, Wd.x, Wd.ox, Wd.oy, c->P.tide_sides);
}
extern "C" int pomgpu_set_tides(pomgpu_ctx *c, int nc, const double *omega, int sides, const double *const *lines, const pomgpu_file_meta *meta) {
  if (c) { F32_REFUSE(c, "set_tides"); }
  NEED_HOT(c);
  if (c->flags & POMGPU_CTX_2D) return fail(c, POMGPU_EINVAL, "set_tides: the table belongs to the tile's context, not to its extended tile");   // (no public way makes such a context: no test)
  if (nc < 0 || nc > POMGPU_MAXTIDES) return fail(c, POMGPU_EINVAL, "set_tides: %d constituents asked for, 0..%d are possible", nc, POMGPU_MAXTIDES);
  if (!nc) { HIPCHK(c, hipStreamSynchronize(c->stream)); tides_free(c); return POMGPU_OK; }
  if (!omega || !meta) return fail(c, POMGPU_EINVAL, "set_tides: no omega or no meta");
  if (sides & ~15) return fail(c, POMGPU_EINVAL, "set_tides: sides = %d is not a set of POMGPU_SIDE_* bits", sides);
  if (sides && !lines) return fail(c, POMGPU_EINVAL, "set_tides: no lines");
  for (int q = 0; q < nc; q++) if (!isfinite(omega[q])) return fail(c, POMGPU_EINVAL, "set_tides: omega[%d] is not finite", q);
  const KP &P = c->P;
  const int ig = meta->im_global, jg = meta->jm_global;
  if (!tide_inside(meta->i0, 0, P.im, ig) || !tide_inside(meta->j0, 0, P.jm, jg))
    return fail(c, POMGPU_EINVAL, "set_tides: the tile's stretch (%d x %d from %d, %d) lies outside the global line (%d x %d)", P.im, P.jm, meta->i0, meta->j0, ig, jg);
  if (c->wide.x && (!tide_inside(meta->i0, c->wide.ox, c->wide.x->P.im, ig) || !tide_inside(meta->j0, c->wide.oy, c->wide.x->P.jm, jg)))
    return fail(c, POMGPU_EINVAL, "set_tides: the extended tile's stretch lies outside the global line (%d x %d)", ig, jg);
  static const int bit_of[4] = {POMGPU_SIDE_WEST, POMGPU_SIDE_EAST, POMGPU_SIDE_SOUTH, POMGPU_SIDE_NORTH}, arg_of[4] = {2, 0, 1, 3};   // W E S N -> the caller's order
  for (int s = 0; s < 4; s++) {
    if (!(sides & bit_of[s])) continue;
    const size_t n = (size_t)nc * (s < 2 ? jg : ig);
    const char *nm = s == 0 ? "west" : (s == 1 ? "east" : (s == 2 ? "south" : "north"));
    if (!lines[4 * arg_of[s]] || !lines[4 * arg_of[s] + 1]) return fail(c, POMGPU_EINVAL, "set_tides: the %s side is on and has no elevation line", nm);
    for (int q = 0; q < 4; q++) {
      const double *src = lines[4 * arg_of[s] + q];
      for (size_t e = 0; src && e < n; e++)
        if (!isfinite(src[e])) return fail(c, POMGPU_EINVAL, "set_tides: a coefficient of the %s side is not finite (line %d, element %zu)", nm, q, e);
    }
  }
  // every refusal is behind us but those of the allocator: the new table is built beside the old one
  double *nh[4][4] = {};
  bool ok = true;
  for (int s = 0; s < 4 && ok; s++) {
    if (!(sides & bit_of[s])) continue;
    const size_t n = (size_t)nc * (s < 2 ? jg : ig);
    for (int q = 0; q < 4 && ok; q++) {
      nh[s][q] = (double *)calloc(n, sizeof(double));
      if (!nh[s][q]) { ok = false; break; }
      const double *src = lines[4 * arg_of[s] + q];
      if (src) memcpy(nh[s][q], src, n * sizeof(double));
    }
  }
  if (!ok) {
    for (int s = 0; s < 4; s++) for (int q = 0; q < 4; q++) free(nh[s][q]);
    return fail(c, POMGPU_ENOMEM, "set_tides: no memory for the lines");
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));                  // the steps that still read the old lines
  tides_free(c);                                              // from here on the table changes (the analysis goes with the old table)
  c->ntide = nc;
  for (int q = 0; q < nc; q++) c->tide_omega[q] = omega[q];
  for (int s = 0; s < 4; s++) for (int q = 0; q < 4; q++) c->tide_host[s][q] = nh[s][q];
  c->tide_g[0] = ig; c->tide_g[1] = jg; c->tide_g[2] = meta->i0; c->tide_g[3] = meta->j0;
  int rc = tide_cut(c, c, 0, 0, sides);
  if (!rc && c->wide.x) rc = tide_cut(c, c->wide.x, c->wide.ox, c->wide.oy, sides);
  if (rc) { tides_free(c); return rc; }
  return POMGPU_OK;
}
extern "C" int pomgpu_tide_count(pomgpu_ctx *c) { return c ? c->ntide : 0; }
extern "C" int pomgpu_tide_phasors(pomgpu_ctx *c, int iint, int iext, double *out) {
  if (!c || !out) return POMGPU_EINVAL;
  tide_phasors(c, tide_time(c->con, iint, iext), out);
  return POMGPU_OK;
}
// The phasors of the internal step c->con.iint, every substep's, on the device: ONE launch per step while the table fits a launch's arguments
// (k_tide.hpp).  Called where a step's external mode begins; a table made for the same iint isplit dti dte time0 is kept
static int tide_table(pomgpu_ctx *c) {
  if (!c->ntide || !c->P.tide_sides) return POMGPU_OK;        // no side carries a tide (a table for the analysis alone): nobody reads the phasors
  const pom_blkcon &k = c->con;
  const double key[5] = {(double)k.iint, (double)k.isplit, k.dti, k.dte, k.time0};
  if (c->tide_key_ok && memcmp(key, c->tide_key, sizeof key) == 0) return POMGPU_OK;
  if (k.isplit < 1) return fail(c, POMGPU_EINVAL, "tides: isplit = %d", k.isplit);
  const size_t n = (size_t)k.isplit * 2 * c->ntide;
  if (n > c->tide_tab_cap) {                                  // the first step, or isplit has grown: not on the path of a run
    double *tab = NULL;
    if (hipMalloc((void **)&tab, n * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return fail(c, POMGPU_ENOMEM, "tides: no memory for the phasor table"); }
    if (c->tide_tab) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->tide_tab); }
    c->tide_tab = tab; c->tide_tab_cap = n;
    c->P.tide_ph = tab;
    if (c->wide.x) c->wide.x->P.tide_ph = tab;
  }
  std::vector<double> h(n);
  for (int iext = 1; iext <= k.isplit; iext++) tide_phasors(c, tide_time(k, k.iint, iext), h.data() + (size_t)(iext - 1) * 2 * c->ntide);
  launch_tide_table(c, c->tide_tab, h.data(), n);
  memcpy(c->tide_key, key, sizeof key);
  c->tide_key_ok = 1;
  return POMGPU_OK;
}
// ---- the harmonic analysis ---------------------------------------------------------------------------------------------------------------
static int harm_zero(pomgpu_ctx *c) {
  const size_t np = 1 + 2 * (size_t)c->ntide;
  HIPCHK(c, hipMemsetAsync(c->harm_acc, 0, 3 * np * c->P.n2 * sizeof(double), c->stream));   // +0.0 everywhere, behind whatever still accumulates
  memset(c->harm_M, 0, sizeof c->harm_M);
  c->harm_count = 0; c->harm_t[0] = c->harm_t[1] = 0.;
  return POMGPU_OK;
}
extern "C" int pomgpu_set_harmonic_analysis(pomgpu_ctx *c, int on, int every) {
  if (c) { F32_REFUSE(c, "set_harmonic_analysis"); }
  NEED_RAW(c);
  if (!on) { harm_free(c); return POMGPU_OK; }
  if (!c->ntide) return fail(c, POMGPU_EINVAL, "set_harmonic_analysis: no constituent table (pomgpu_set_tides)");
  if (every < 1) return fail(c, POMGPU_EINVAL, "set_harmonic_analysis: every = %d", every);
  const size_t np = 1 + 2 * (size_t)c->ntide, total = 3 * np * c->P.n2;
  if (total >= ((size_t)1 << 32)) return fail(c, POMGPU_EINVAL, "set_harmonic_analysis: %zu accumulator cells are beyond 32-bit offsets", total);
  if (!c->harm_acc) {
    double *acc = NULL, *coef = NULL;
    if (hipMalloc((void **)&acc, total * sizeof(double)) != hipSuccess || hipMalloc((void **)&coef, np * c->P.n2 * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError(); (void)hipFree(acc);
      return fail(c, POMGPU_ENOMEM, "set_harmonic_analysis: no memory for the accumulators (%zu MB)", total * sizeof(double) >> 20);
    }
    c->harm_acc = acc; c->harm_coef = coef;
  }
  c->harm_on = 1; c->harm_every = every;
  return harm_zero(c);
}
// the stage: what mean_accumulate completes first is what this one needs complete (elb uab vab of the current generation)
static int harm_accumulate(pomgpu_ctx *c) {
  ext_flush_deferred(c);
  wide_flush(c);
  const pom_blkcon &k = c->con;
  const double t = k.time0 * 86400. + k.dti * (double)k.iint;
  double ph[2 * POMGPU_TIDEMAX];
  tide_phasors(c, t, ph);
  HarmB b;
  const int np = 1 + 2 * c->ntide;
  double basis[HARM_MAXB];
  basis[0] = 1.;
  for (int q = 0; q < POMGPU_TIDEMAX; q++) { b.cn[q] = q < c->ntide ? ph[2 * q] : 0.; b.sn[q] = q < c->ntide ? ph[2 * q + 1] : 0.; }
  for (int q = 0; q < c->ntide; q++) { basis[1 + 2 * q] = b.cn[q]; basis[2 + 2 * q] = b.sn[q]; }
  launch_harm_accum(c, b);
  for (int p = 0; p < np; p++) for (int q = 0; q < np; q++) c->harm_M[p * np + q] = c->harm_M[p * np + q] + basis[p] * basis[q];
  if (!c->harm_count) c->harm_t[0] = t;
  c->harm_t[1] = t;
  c->harm_count += 1;
  return POMGPU_OK;
}
#define HARM_NEED(c, what)                                                                 \
  if (c) { F32_REFUSE(c, what); }                                                          \
  NEED_RAW(c);                                                                             \
  if (!c->harm_on) return fail(c, POMGPU_EINVAL, what ": the harmonic analysis is off (pomgpu_set_harmonic_analysis)")
extern "C" int pomgpu_harmonic_accumulate(pomgpu_ctx *c) {
  HARM_NEED(c, "harmonic_accumulate");
  return harm_accumulate(c);
}
extern "C" int pomgpu_harmonic_count(pomgpu_ctx *c) { return c && c->harm_on ? c->harm_count : -1; }
extern "C" int pomgpu_harmonic_reset(pomgpu_ctx *c) {
  HARM_NEED(c, "harmonic_reset");
  return harm_zero(c);
}
extern "C" int pomgpu_harmonic_sums(pomgpu_ctx *c, int field, double *out) {
  HARM_NEED(c, "harmonic_sums");
  if (field < 0 || field > 2 || !out) return fail(c, POMGPU_EINVAL, "harmonic_sums: field %d (0 elb, 1 uab, 2 vab) or no host array", field);
  const size_t np = 1 + 2 * (size_t)c->ntide, n = np * c->P.n2;
  HIPCHK(c, hipMemcpyAsync(out, c->harm_acc + (size_t)field * n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return POMGPU_OK;
}
extern "C" int pomgpu_harmonic_matrix(pomgpu_ctx *c, double *out, double *t2) {
  HARM_NEED(c, "harmonic_matrix");
  if (!out) return fail(c, POMGPU_EINVAL, "harmonic_matrix: no host array");
  const int np = 1 + 2 * c->ntide;
  memcpy(out, c->harm_M, (size_t)np * np * sizeof(double));
  if (t2) { t2[0] = c->harm_t[0]; t2[1] = c->harm_t[1]; }
  return POMGPU_OK;
}
// the inverse of the n x n matrix a (row-major) into inv by Gauss-Jordan elimination with partial pivoting; false: singular
static bool harm_invert(const double *a, int n, double *inv) {
  double w[HARM_MAXB][2 * HARM_MAXB];
  for (int p = 0; p < n; p++) for (int q = 0; q < n; q++) { w[p][q] = a[p * n + q]; w[p][n + q] = p == q ? 1. : 0.; }
  for (int col = 0; col < n; col++) {
    int piv = col;
    for (int p = col + 1; p < n; p++) if (fabs(w[p][col]) > fabs(w[piv][col])) piv = p;
    if (!(fabs(w[piv][col]) > 0.) || !isfinite(w[piv][col])) return false;
    if (piv != col) for (int q = 0; q < 2 * n; q++) { const double x = w[col][q]; w[col][q] = w[piv][q]; w[piv][q] = x; }
    const double d = w[col][col];
    for (int q = 0; q < 2 * n; q++) w[col][q] = w[col][q] / d;
    for (int p = 0; p < n; p++) {
      if (p == col) continue;
      const double f = w[p][col];
      for (int q = 0; q < 2 * n; q++) w[p][q] = w[p][q] - f * w[col][q];
    }
  }
  for (int p = 0; p < n; p++) for (int q = 0; q < n; q++) { inv[p * n + q] = w[p][n + q]; if (!isfinite(inv[p * n + q])) return false; }
  return true;
}
extern "C" int pomgpu_harmonic_solve(pomgpu_ctx *c, int field, double *coef) {
  HARM_NEED(c, "harmonic_solve");
  if (field < 0 || field > 2 || !coef) return fail(c, POMGPU_EINVAL, "harmonic_solve: field %d (0 elb, 1 uab, 2 vab) or no host array", field);
  const int np = 1 + 2 * c->ntide;
  HarmInv inv;
  memset(&inv, 0, sizeof inv);
  if (c->harm_count < np || !harm_invert(c->harm_M, np, inv.a))
    return fail(c, POMGPU_EINVAL, "harmonic_solve: the normal matrix of %d samples is singular (%d unknowns)", c->harm_count, np);
  const size_t n = (size_t)np * c->P.n2;
  launch_harm_solve(c, inv, c->harm_acc + (size_t)field * n, c->harm_coef);
  HIPCHK(c, hipMemcpyAsync(coef, c->harm_coef, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return POMGPU_OK;
}
int pomgpu_harmonic_planes(pomgpu_ctx *c, const double **planes) {
  HARM_NEED(c, "write_harmonics");
  const int np = 1 + 2 * c->ntide;
  HarmInv inv;
  memset(&inv, 0, sizeof inv);
  if (c->harm_count < np || !harm_invert(c->harm_M, np, inv.a))
    return fail(c, POMGPU_EINVAL, "write_harmonics: the normal matrix of %d samples is singular (%d unknowns)", c->harm_count, np);
  const size_t n = (size_t)np * c->P.n2;
  if (!c->harm_file && hipMalloc((void **)&c->harm_file, 3 * n * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError(); c->harm_file = NULL;
    return fail(c, POMGPU_ENOMEM, "write_harmonics: no memory for the file's planes (%zu MB)", 3 * n * sizeof(double) >> 20);
  }
  for (int f = 0; f < 3; f++) {                               // harm_coef is reused field after field: the stream orders the launches
    launch_harm_solve(c, inv, c->harm_acc + (size_t)f * n, c->harm_coef);
    launch_harm_constants(c, c->harm_coef, c->harm_file + (size_t)f * n);
  }
  *planes = c->harm_file;
  return POMGPU_OK;
}
static int advance(pomgpu_ctx *c, int more_steps_follow);
extern "C" int pomgpu_advance(pomgpu_ctx *c) { return advance(c, 0); }
static int advance(pomgpu_ctx *c, int more_steps_follow) {    // advance.f:6-59
  NEED_HOT(c);
  int rc;
  if ((rc = pomgpu_get_time(c))) return rc;
  { KP g = c->P; set_band_geometry(g, c->sw); c->P.g_strip = g.g_strip; c->P.g_lin = g.g_lin; c->P.g_rb = g.g_rb; c->P.g_nbx = g.g_nbx; c->P.g_bpl = g.g_bpl; }   // developer switches POMGPU_COL_STRIP, POMGPU_BAND_BYTES, follow pomgpu_debug_switch from step to step (tools/kbench.py)
  // advance.f:14-18: file-driven in the reference; here they run once the host has supplied records
  if (c->frc_on && (rc = pomgpu_surface_forcing(c))) return rc;
  if (!c->frc_on && c->wat_on && (rc = pomgpu_water(c))) return rc;   // water alone
  if (c->lat_on && (rc = pomgpu_lateral_bc(c))) return rc;
  // the vertical integrals of advx, advy, drhox, drhoy come out of advct / baropg themselves: on one tile, and on
  // tiles with the wide-halo external mode (there only the owned cells of adx2d ... are used)
  const bool tiles_fused = c->wide.on && c->tp.on && !SW(c, ADVCT_SPLIT);
  // (POMGPU_SUM2D_OFF: k_vint forms the integrals from the stored arrays as the reference does, advance.f:152-168 -- the same bits in fp64; in the
  // fp32-storage study variant it is what makes one tile and several tiles round alike, tests/gpu_tiles_threads.py)
  const int sum2d = ((!c->exch || tiles_fused) && c->P.mode != 2 && (c->P.npg == 1 || c->P.npg == 2)) && !SW(c, SUM2D_OFF);
  const int ph_step = prof_phase_open(c);                     // "phase_step": this whole step on the kernels' stream
  if ((rc = wide_early_start(c))) return rc;                  // most of the wide exchange, beside lateral_viscosity
  // rho's round trip is left to k_profq when this step will rewrite rho (mode 3: dens at the end of mode_internal)
  const pom_blkcon &k0 = c->con;
  const int defer_rt = k0.mode == 3 && (k0.iint != 1 || k0.time0 != 0.) && !SW(c, RHO_ROUNDTRIP);   // rho's readers before dens: k_profq, k_profq_prod(_lines)
  if ((rc = lateral_viscosity(c, sum2d, defer_rt))) return rc;
  if ((rc = mode_interaction(c, sum2d))) return rc;           // with the wide-halo mode: on the extended tile from here ...
  if (c->wr_deferred) {                                       // the previous step's realvertvl + wr exchange, beside this step's external substeps
    c->wr_deferred = 0;
    if ((rc = wr_on_side(c, 1))) return rc;
  }
  if ((rc = tide_table(c))) return rc;                        // the tide's phasors of this step's substeps: ONE launch, none without a tide
  const int ph_ext = prof_phase_open(c);                      // "phase_external": the isplit substeps of mode_external (advance.f:27-29)
  if (!ext_loop_all(c))
  for (int iext = 1; iext <= c->con.isplit; iext++) {
    if (ext_pair(c, iext)) { iext++; continue; }              // two substeps per pass over memory (large tiles)
    c->con.iext = iext;
    if ((rc = mode_external(c, 0))) return rc;                // ... to the last substep
  }
  prof_phase_close(c, ph_ext, "phase_external");
  c->con.iext = c->con.isplit + 1;
  const bool body = (c->con.iint != 1 || c->con.time0 != 0.) && c->con.mode != 2;   // mode_internal runs its 3-D part (advance.f:362)
  if ((rc = mode_internal(c, more_steps_follow))) return rc;
  if (c->mean_acc && (rc = mean_accumulate(c))) return rc;    // the time-mean output, where advance.f:38 writes
  if (c->nflt && body) float_stage(c);                        // the floats move with the u, v, w this step has left: ONE launch
  if (c->harm_on && c->con.iint % c->harm_every == 0 && (rc = harm_accumulate(c))) return rc;   // the harmonic analysis: ONE launch per sampled step
  launch_check_velocity(c);   // result stays on the device; error flag is merged at the next get_con
  prof_phase_close(c, ph_step, "phase_step");
  return POMGPU_OK;
}
extern "C" int pomgpu_run(pomgpu_ctx *c, int nsteps) {        // pom.f:17-19
  NEED_HOT(c);
  c->wr_deferred = 0;                                         // (a step that failed half way may have left it)
  for (int n = 0; n < nsteps; n++) {
    c->con.iint += 1;
    int rc = advance(c, n + 1 < nsteps);                      // the last step of the call leaves nothing to a next one
    if (rc) return rc;
  }
  return POMGPU_OK;
}

// ---- where in memory the 3-D arrays live ------------------------------------------------------------------------------------------
// The same kernels on the same bytes run up to 6 % faster or slower with WHERE in the 288 GB their arrays lie (round 4,
// profiles/round4_placement_probe.txt: blk3d starting 7200 MiB into its allocation instead of 0: the step 37.7 -> 36.3 ms in four
// processes out of four on one box, k_profq 7.55 -> 7.2, k_advuv_col 2.99 -> 2.67; 8400-19200 MiB into it on another box: 39.0).
// Which offsets are good differs from box to box and from process to process -- physical addresses and the memory system's
// interleave are not visible to a user process -- but inside one process it is reproducible to 0.1 %.  So the placement is
// MEASURED: blk3d and the 3-D scratch arrays move into ONE allocation with room in front, and a few start offsets (multiples
// of two arrays), each with the arrays at their own distance or 256 MiB further apart, are tried with `steps` internal steps each -- real steps
// of the model, timed with events on the kernels' stream; results do not depend on where an array lives -- and the fastest
// is kept.  Costs one extra allocation of the arrays' size plus the room while it moves in, ~25 ms per move at 2048x1536x50,
// and advances the model by ntried x (steps + 1) internal steps (one untimed step after every move).  Tiles below 64 MiB per array
// are left alone (ntried = 0).
// one array of n doubles from src to dst inside one allocation; the ranges may overlap (chunks no longer than the shift, in the safe order)
static int piece_move(pomgpu_ctx *c, double *dst, const double *src, size_t n) {
  if (dst == src || !n) return POMGPU_OK;
  const size_t shift = dst > src ? (size_t)(dst - src) : (size_t)(src - dst), chunk = shift < n ? shift : n;
  const size_t nch = (n + chunk - 1) / chunk;
  for (size_t q = 0; q < nch; q++) {
    const size_t m = dst > src ? nch - 1 - q : q;             // moving up: from the end
    const size_t o = m * chunk, len = (o + chunk <= n ? chunk : n - o);
    HIPCHK(c, hipMemcpyAsync(dst + o, src + o, len * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  return POMGPU_OK;
}
// a layout of the tuner's allocation: blk3d starts `f` doubles into it, its arrays are `a` doubles apart, the scratch arrays follow
struct TuneLay { size_t f, a; };
static double *tune_piece(const pomgpu_ctx *c, const TuneLay &L, int i) {   // piece i: the blk3d arrays, then the 3-D scratch arrays
  return c->tune_block + L.f + (i < POM_NBLK3D ? (size_t)i * L.a : (size_t)POM_NBLK3D * L.a + (size_t)(i - POM_NBLK3D) * c->P.n3);
}
static int tune_relayout(pomgpu_ctx *c, TuneLay to) {
  const int np = POM_NBLK3D + POMGPU_NSCR3;
  auto one_way = [&](const TuneLay &from, const TuneLay &dst_) -> int {   // every piece moves up, or every piece moves down
    const bool up = dst_.f >= from.f && dst_.a >= from.a;
    for (int q = 0; q < np; q++) {
      const int i = up ? np - 1 - q : q;                      // moving up: the last piece first
      const int rc = piece_move(c, tune_piece(c, dst_, i), tune_piece(c, from, i), c->P.n3);
      if (rc) return rc;
    }
    return POMGPU_OK;
  };
  aam_canonical(c);                                           // the trial steps between two moves may have left aam in its spare array
  const TuneLay cur = {c->tune_front, c->P.a3};
  int rc = POMGPU_OK;
  if ((to.f >= cur.f && to.a >= cur.a) || (to.f <= cur.f && to.a <= cur.a)) rc = one_way(cur, to);
  else {                                                      // one grows, the other shrinks: by way of the layout that is at least both
    const TuneLay mid = {to.f > cur.f ? to.f : cur.f, to.a > cur.a ? to.a : cur.a};
    rc = one_way(cur, mid);
    if (!rc) rc = one_way(mid, to);
  }
  if (rc) return rc;
  KP &P = c->P;
  c->tune_front = to.f;
  P.a3 = to.a;
  P.b3 = c->tune_block + to.f;
  for (int n = 0; n < POMGPU_NSCR3; n++) P.s3[n] = P.b3 + (size_t)POM_NBLK3D * P.a3 + (size_t)n * P.n3;
  aam_buffers(c);
  return POMGPU_OK;
}
extern "C" int pomgpu_tune_placement(pomgpu_ctx *c, int steps, int max_try, double *ms_out, long *front_mib_out, long *pad_mib_out, int *ntried, int *kept) {
  NEED(c);
  if (ntried) *ntried = 0;
  if (kept) *kept = 0;
  if (c->mean_acc)                                            // the trial steps are real steps: they would be accumulated
    return fail(c, POMGPU_EINVAL, "tune_placement: the time-mean output is on and the trial steps would count -- tune first, switch the mean on afterwards");
  if (c->ntr)                                                 // ... and would move the tracers
    return fail(c, POMGPU_EINVAL, "tune_placement: passive tracers are registered and the trial steps would move them -- tune first, register tracers afterwards");
  if (c->nflt)                                                // ... and the floats
    return fail(c, POMGPU_EINVAL, "tune_placement: floats are registered and the trial steps would move them -- tune first, upload floats afterwards");
  if (c->ntide || c->harm_on)                                 // ... and the tide and its analysis: the trial steps are real steps
    return fail(c, POMGPU_EINVAL, "tune_placement: a tide table or the harmonic analysis is on -- tune first, register tides afterwards");
#ifdef POMGPU_EMU
  (void)steps; (void)max_try; (void)ms_out; (void)front_mib_out; (void)pad_mib_out;
  return POMGPU_OK;
#else
  KP &P = c->P;
  if ((c->flags & POMGPU_CTX_2D) || !P.b3 || steps < 1 || max_try < 1) return fail(c, POMGPU_EINVAL, "tune_placement: a context with 3-D arrays, steps >= 1, max_try >= 1");
  if (c->dev3_handed)                                         // the arrays are about to move (and the allocations they lived in to be freed)
    return fail(c, POMGPU_EINVAL, "tune_placement: pomgpu_device_3d has handed out addresses of the 3-D arrays, which this call would leave dangling -- tune first, take addresses afterwards");
  // several tiles: the trial steps post message rounds -- every rank calls this alike (same steps, same max_try), each keeps its own best
  if (P.n3 * sizeof(double) < ((size_t)64 << 20) && !SW(c, TUNE_FORCE)) return POMGPU_OK;
  const size_t unit = 2 * P.n3;                               // start offsets: multiples of two arrays
  // a second distance between the arrays: 256 MiB more (2048x1536x50: 1200 -> 1456 MiB; round 4: 37.4 -> 36.6 ms per step on one box),
  // a quarter of an array on smaller tiles; always a multiple of 64 KiB (odd distances cost k_profq 4 %)
  size_t pad1 = P.n3 * sizeof(double) >= ((size_t)512 << 20) ? ((size_t)256 << 20) / sizeof(double) : (P.n3 / 4 + 8191) / 8192 * 8192;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->side) HIPCHK(c, hipStreamSynchronize(c->side));
  if (!c->tune_block) {
    size_t fre = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fre, &tot));
    const size_t a0 = P.a3;
    size_t amax = a0 + pad1;
    auto need = [&](int kmax, size_t am) { return ((size_t)kmax * unit + (size_t)POM_NBLK3D * am + (size_t)POMGPU_NSCR3 * P.n3) * sizeof(double) + ((size_t)2 << 30); };
    int kmax = max_try > 12 ? 30 : 10;                        // the room in front: 10 units (24 GB at 2048x1536x50) unless many trials are asked for
    while (kmax > 0 && need(kmax, amax) > fre) kmax--;
    if (kmax < 1) { amax = a0; kmax = 10; while (kmax > 0 && need(kmax, amax) > fre) kmax--; }   // no room for the wider distance: start offsets only
    if (kmax < 1) return POMGPU_OK;                           // no room to move: the placement stays what it is
    double *blk = NULL;
    if (hipMalloc((void **)&blk, need(kmax, amax) - ((size_t)2 << 30)) != hipSuccess) { (void)hipGetLastError(); return POMGPU_OK; }
    for (int n = 0; n < POM_NBLK3D; n++)
      HIPCHK(c, hipMemcpyAsync(blk + (size_t)n * a0, P.b3 + (size_t)n * a0, P.n3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    for (int n = 0; n < POMGPU_NSCR3; n++)
      HIPCHK(c, hipMemcpyAsync(blk + (size_t)POM_NBLK3D * a0 + (size_t)n * P.n3, P.s3[n], P.n3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(P.b3);
    for (int n = 0; n < POMGPU_NSCR3; n++) (void)hipFree(P.s3[n]);
    c->tune_block = blk;
    c->tune_front = 0;
    c->tune_kmax = kmax;
    c->tune_a0 = a0;
    c->tune_amax = amax;
    P.b3 = blk;
    for (int n = 0; n < POMGPU_NSCR3; n++) P.s3[n] = blk + (size_t)POM_NBLK3D * a0 + (size_t)n * P.n3;
    aam_buffers(c);
  }
  // (start offset in units of two arrays, wider distance?) in the order they are tried
  static const int KS[20][2] = {{0, 0}, {3, 0}, {10, 0}, {0, 1}, {3, 1}, {10, 1}, {5, 0}, {5, 1}, {2, 0}, {1, 0}, {7, 0}, {4, 0}, {7, 1}, {2, 1}, {15, 0}, {20, 0}, {25, 0}, {30, 0}, {15, 1}, {20, 1}};
  hipEvent_t e0 = NULL, e1 = NULL;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    if (e0) (void)hipEventDestroy(e0);
    return fail(c, POMGPU_EHIP, "tune_placement: hipEventCreate failed");   // nothing has moved yet
  }
  int n = 0, best = 0, rc = POMGPU_OK;
  TuneLay lay[20];
  double ms[20];
  for (int q = 0; q < 20 && n < max_try && !rc; q++) {
    if (KS[q][0] > c->tune_kmax || (KS[q][1] && c->tune_amax == c->tune_a0)) continue;
    lay[n].f = (size_t)KS[q][0] * unit;
    lay[n].a = KS[q][1] ? c->tune_amax : c->tune_a0;
    if ((rc = tune_relayout(c, lay[n]))) break;
    if ((rc = pomgpu_run(c, 1))) break;                       // untimed: the first step after a move (and the model's very first step, which skips its 3-D part)
    (void)hipEventRecord(e0, c->stream);
    if ((rc = pomgpu_run(c, steps))) break;
    side_join(c);
    (void)hipEventRecord(e1, c->stream);
    (void)hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    ms[n] = (double)t / steps;
    if (ms[n] < ms[best]) best = n;
    n++;
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (!rc && n) rc = tune_relayout(c, lay[best]);
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POMGPU_EHIP, "tune_placement: hipStreamSynchronize failed");
  if (rc) {
    // a move that stopped half way leaves some arrays in the old layout and some in the new one while P.b3 / P.a3 describe one of them:
    // the device mirrors no longer hold the state.  Say so once and for all -- error_status = 1 (the reference's convention), and every
    // hot-path entry point of this context refuses from here on; the host uploads its state into a fresh context.
    c->broken = 1;
    c->con.error_status = 1;
    return rc;
  }
  for (int q = 0; q < n; q++) {
    if (ms_out) ms_out[q] = ms[q];
    if (front_mib_out) front_mib_out[q] = (long)(lay[q].f * sizeof(double) >> 20);
    if (pad_mib_out) pad_mib_out[q] = (long)((lay[q].a - P.n3) * sizeof(double) >> 20);
  }
  if (ntried) *ntried = n;
  if (kept) *kept = best;
  return POMGPU_OK;
#endif
}

// ---- stand-alone kernels (device-resident), reference names ------------------------------------
extern "C" int pomgpu_advave(pomgpu_ctx *c) { NEED(c); seq_advave(c); return POMGPU_OK; }
extern "C" int pomgpu_advct(pomgpu_ctx *c) { NEED(c); seq_advct(c); return POMGPU_OK; }
extern "C" int pomgpu_baropg(pomgpu_ctx *c) { NEED(c); seq_baropg(c); return POMGPU_OK; }
extern "C" int pomgpu_baropg_mcc(pomgpu_ctx *c) { NEED(c); seq_baropg_mcc(c); return POMGPU_OK; }
extern "C" int pomgpu_advq(pomgpu_ctx *c, const double *qb, const double *q, const double *qf) {
  NEED(c);
  double *a = dev3(c, qb), *b = dev3(c, q), *d = dev3(c, qf);
  if (!a || !b || !d) return fail(c, POMGPU_EINVAL, "advq: arguments must be blk3d arrays of the bound host block");
  seq_advq(c, a, b, d, 0, 0);
  return POMGPU_OK;
}
static int advt_args(pomgpu_ctx *c, const double *fb, const double *f, const double *fclim, const double *ff, double **o) {
  o[0] = dev3(c, fb); o[1] = dev3(c, f); o[2] = dev3(c, fclim); o[3] = dev3(c, ff);
  if (!o[0] || !o[1] || !o[2] || !o[3]) return fail(c, POMGPU_EINVAL, "advt: arguments must be blk3d arrays of the bound host block");
  return POMGPU_OK;
}
extern "C" int pomgpu_advt1(pomgpu_ctx *c, const double *fb, const double *f, const double *fclim, const double *ff) {
  NEED(c);
  double *o[4];
  int rc = advt_args(c, fb, f, fclim, ff, o);
  if (rc) return rc;
  seq_advt1(c, o[0], o[1], o[2], o[3]);
  return POMGPU_OK;
}
extern "C" int pomgpu_advt2(pomgpu_ctx *c, const double *fb, const double *f, const double *fclim, const double *ff) {
  NEED(c);
  double *o[4];
  int rc = advt_args(c, fb, f, fclim, ff, o);
  if (rc) return rc;
  seq_advt2(c, o[0], o[1], o[2], o[3]);
  return POMGPU_OK;
}
extern "C" int pomgpu_advu(pomgpu_ctx *c) { NEED(c); launch_advu_profu(c, 1, 0); return POMGPU_OK; }
extern "C" int pomgpu_advv(pomgpu_ctx *c) { NEED(c); launch_advv_profv(c, 1, 0); return POMGPU_OK; }
extern "C" int pomgpu_profu(pomgpu_ctx *c) {
  NEED(c);
  launch_advu_profu(c, 0, 1);
  xch(c, 1, D2(c, wubot), 1);
  return POMGPU_OK;
}
extern "C" int pomgpu_profv(pomgpu_ctx *c) {
  NEED(c);
  launch_advv_profv(c, 0, 1);
  xch(c, 1, D2(c, wvbot), 1);
  return POMGPU_OK;
}
extern "C" int pomgpu_dens(pomgpu_ctx *c, const double *si, const double *ti, const double *rhoo) {
  NEED(c);
  double *a = dev3(c, si), *b = dev3(c, ti), *d = dev3(c, rhoo);
  if (!a || !b || !d) return fail(c, POMGPU_EINVAL, "dens: arguments must be blk3d arrays of the bound host block");
  launch_dens(c, a, b, d);
  return POMGPU_OK;
}
// ztosig(zs,tb,zz,h,t,...) (initialize.f:547-595): zs and the z-level source are the caller's own arrays and come from the host; h, zz
// are the mirrors', the neighbours the context's; t is a COMMON array like every array argument
extern "C" int pomgpu_ztosig(pomgpu_ctx *c, const double *zs, int ks, const double *src, const double *t) {
  NEED(c);
  if (!zs || !src) return fail(c, POMGPU_EINVAL, "ztosig: zs and src must be given");
  if (ks < 2 || ks > 300) return fail(c, POMGPU_EINVAL, "ztosig: ks = %d is outside 2..300 (splinc's nmax)", ks);
  for (int k = 0; k < ks; k++)
    if (!__builtin_isfinite(zs[k]) || (k && !(zs[k] > zs[k - 1])))
      return fail(c, POMGPU_EINVAL, "ztosig: zs(%d) = %g is not finite or not above zs(%d): the levels must increase strictly", k + 1, zs[k], k);
  if (c->P.im < 3 || c->P.jm < 3) return fail(c, POMGPU_EINVAL, "ztosig: the tile has no interior column");
  double *d = dev3(c, t);
  if (!d) return fail(c, POMGPU_EINVAL, "ztosig: t must be a blk3d array of the bound host block");
  const int rc = launch_ztosig(c, d, zs, ks, src);
  if (rc) return fail(c, rc, "ztosig: %s", rc == POMGPU_ENOMEM ? "no device memory for the source and the work arrays" : "a HIP call failed");
  xch(c, 1, d, c->P.kb);                                      // :586
  launch_ztosig_edges(c, d);                                  // :589-592
  return POMGPU_OK;
}
// the line form of ztosig (bounds_forcing.f:636-716): one lateral line of T or S on the z levels zs onto the sigma levels, with the depth the
// reference's block names for that edge; zs, src and out are the caller's own host arrays, no mirror changes
extern "C" int pomgpu_ztosig_line(pomgpu_ctx *c, int edge, const double *zs, int ks, const double *src, double *out) {
  NEED(c);
  if (edge < 0 || edge > 3) return fail(c, POMGPU_EINVAL, "ztosig_line: edge = %d is none of 0 east, 1 south, 2 west, 3 north", edge);
  if (!zs || !src || !out) return fail(c, POMGPU_EINVAL, "ztosig_line: zs, src and out must be given");
  if (ks < 2 || ks > 300) return fail(c, POMGPU_EINVAL, "ztosig_line: ks = %d is outside 2..300 (splinc's nmax)", ks);
  for (int k = 0; k < ks; k++)
    if (!__builtin_isfinite(zs[k]) || (k && !(zs[k] > zs[k - 1])))
      return fail(c, POMGPU_EINVAL, "ztosig_line: zs(%d) = %g is not finite or not above zs(%d): the levels must increase strictly", k + 1, zs[k], k);
  if (c->P.im < 4 || c->P.jm < 4) return fail(c, POMGPU_EINVAL, "ztosig_line: the tile has fewer than 4 x 4 cells");
  const int rc = launch_ztosig_line(c, edge, zs, ks, src, out);
  if (rc) return fail(c, rc, "ztosig_line: %s", rc == POMGPU_ENOMEM ? "no device memory for the source and the work arrays" : "a HIP call failed");
  return POMGPU_OK;
}
// the scalar device functions on the caller's own host arrays (tests): refused before anything is allocated or launched
extern "C" int pomgpu_math_probe(pomgpu_ctx *c, int op, long n, const double *const *in, int nin, double *out) {
  NEED(c);
  static const int NIN[4] = {2, 2, 1, 5};
  if (op < 0 || op > 3) return fail(c, POMGPU_EINVAL, "math_probe: op = %d is none of 0 DIVI, 1 DIVI_F32, 2 GPOW15, 3 RAD_Q", op);
  if (nin != NIN[op]) return fail(c, POMGPU_EINVAL, "math_probe: op %d takes %d input arrays, not %d", op, NIN[op], nin);
  if (n < 1 || n > (1L << 22)) return fail(c, POMGPU_EINVAL, "math_probe: n = %ld is outside 1..2^22", n);
  if (!in || !out) return fail(c, POMGPU_EINVAL, "math_probe: in and out must be given");
  for (int q = 0; q < nin; q++)
    if (!in[q]) return fail(c, POMGPU_EINVAL, "math_probe: input array %d is NULL", q);
  double *dev = NULL;                                            // the inputs one after the other, then the result
  if (hipMalloc((void **)&dev, (size_t)(nin + 1) * n * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return fail(c, POMGPU_ENOMEM, "math_probe: no device memory for %d arrays of %ld", nin + 1, n); }
  const double *din[5];
  int rc = POMGPU_OK;
  for (int q = 0; q < nin; q++) {
    din[q] = dev + (size_t)q * n;
    if (hipMemcpyAsync(dev + (size_t)q * n, in[q], n * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = POMGPU_EHIP;
  }
  double *dout = dev + (size_t)nin * n;
  if (!rc) {
    if (op == POMGPU_PROBE_GPOW15) launch_probe_gpow15(c, n, din[0], dout);
    else if (op == POMGPU_PROBE_RAD_Q) launch_probe_rad_q(c, n, din, dout);
    else launch_probe_divi(c, n, din[0], din[1], dout, op == POMGPU_PROBE_DIVI_F32);
    if (hipMemcpyAsync(out, dout, n * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = POMGPU_EHIP;
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess) rc = POMGPU_EHIP;
  (void)hipFree(dev);
  if (rc) return fail(c, rc, "math_probe: a HIP call failed");
  return POMGPU_OK;
}
extern "C" int pomgpu_profq(pomgpu_ctx *c) { NEED(c); seq_profq(c); return POMGPU_OK; }
extern "C" int pomgpu_proft(pomgpu_ctx *c, const double *f, const double *wfsurf, const double *fsurf, int nbc) {
  NEED(c);
  double *a = dev3(c, f), *b = dev2(c, wfsurf), *d = dev2(c, fsurf);
  if (!a || !b || !d) return fail(c, POMGPU_EINVAL, "proft: arguments must be arrays of the bound host blocks");
  if (nbc < 1 || nbc > 4) return fail(c, POMGPU_EINVAL, "proft: nbc must be 1..4");
  launch_proft(c, a, b, d, nbc);
  return POMGPU_OK;
}
extern "C" int pomgpu_vertvl(pomgpu_ctx *c) { NEED(c); launch_vertvl(c, 0); return POMGPU_OK; }
extern "C" int pomgpu_realvertvl(pomgpu_ctx *c) {
  if (c) c->wr_pending = 0;                                   // this call overwrites wr, from etf as the reference does
  NEED(c);
  launch_realvertvl(c);
  xch(c, 1, D3(c, wr), c->P.kbm1);
  return POMGPU_OK;
}
extern "C" int pomgpu_bcond(pomgpu_ctx *c, int idx) {
  NEED(c);
  switch (idx) {
    case 1: launch_bcond1(c); break;
    case 2: {
      if (c->ntide) {                                         // the tide's phasors are those of substep iext of step iint
        if (c->con.iext < 1 || c->con.iext > c->con.isplit) return fail(c, POMGPU_EINVAL, "bcond(2) with a tide: iext = %d is not a substep of 1..%d", c->con.iext, c->con.isplit);
        c->P.iext = c->con.iext;
        const int rct = tide_table(c);
        if (rct) return rct;
      }
      launch_ext_uvaf(c, 0);
      break;
    }
    case 4: launch_bcond4_edges(c); launch_mask_ts(c); break;
    case 5: launch_mask_w(c); break;
    case 6: launch_bcond6_edges(c); launch_mask_q(c); break;
    default: return fail(c, POMGPU_EINVAL, "bcond(%d) is not on the hot path", idx);
  }
  return POMGPU_OK;
}
extern "C" int pomgpu_bcondorl(pomgpu_ctx *c, int idx) {
  NEED(c);
  switch (idx) {
    case 3: launch_bcondorl3(c); launch_mask_uv(c); break;
    case 5: launch_mask_w(c); break;
    default: return fail(c, POMGPU_EINVAL, "bcondorl(%d) is not on the hot path", idx);
  }
  return POMGPU_OK;
}
extern "C" int pomgpu_restore_interior(pomgpu_ctx *c) { NEED(c); return seq_restore_interior(c); }
