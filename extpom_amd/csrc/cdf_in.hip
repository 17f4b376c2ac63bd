// cdf_in.hip -- a whole state from files WITHOUT PnetCDF: pomgpu_read_restart (the restart file back), pomgpu_read_tracers (the passive
// tracers' own file) and pomgpu_cold_start (the reference's grid, init and clim files), with pomgpu_set_z_inputs / pomgpu_set_z_lateral,
// which say what is on z levels.  The readers parse the
// headers and check every variable before the first mirror changes, then send raw big-endian bands through the pinned buffers of
// cdf_io.hpp to the device on a copy stream of their own, a kernel behind each copy; the forcing records are frc_files.hip's.
#include <fcntl.h>
#include <sys/stat.h>

#include <cmath>
#include <cstdio>

#include "cdf_io.hpp"
#define fail pomgpu_fail

// ---- reading the restart file back (read_restart_pnetcdf, io_pnetcdf.F:2420-2768) -----------------------------------------------
struct RItem { const RVar *v; int slot; int nlev; };            // nlev = kb: blk3d slot; 1: blk2d slot
// d = h + el, dt = h + et over the active cells (io_pnetcdf.F:2757-2762)
__global__ void k_restart_depths(KP P) {
  const int i = TID_I, j = TID_J;
  if (i > P.im || j > P.jm) return;
  F2(d, i, j) = F2(h, i, j) + F2(el, i, j);
  F2(dt, i, j) = F2(h, i, j) + F2(et, i, j);
}

extern "C" int pomgpu_read_restart(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m, double *time0_out, double *iint_out) {
  if (!c || !path || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  { const int rcw = pomgpu_io_wait(c); if (rcw) return rcw; }  // the file may be the one this context is still writing
  const KP &P = c->P;
  if (!tile_fits(m, P, 0, 0, 0, 0))
    return fail(c, POMGPU_EINVAL, "read_restart: %s: the tile (%d..%d, %d..%d) does not fit the global grid %d x %d", path, m->i0, m->i0 + P.im - 1,
                m->j0, m->j0 + P.jm - 1, m->im_global, m->jm_global);
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(c, POMGPU_EINVAL, "read_restart: cannot open %s", path);
  struct stat sb;
  if (fstat(fd, &sb)) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_restart: cannot stat %s", path); }
  const uint64_t fsize = (uint64_t)sb.st_size;
  // ---- the header, whole, before anything is written ----
  RHeader H;
  {
    std::string what;
    const int rc = read_header(fd, fsize, H, what);
    if (rc == -2) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_restart: I/O error on %s (header)", path); }
    if (rc < 0) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_restart: %s is not a restart file this library reads: %s", path, what.c_str()); }
  }
  auto refuse = [&](const std::string &why) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_restart: %s: %s", path, why.c_str()); };
  static const struct { const char *n; int slot; } r2[] = {
      {"wubot", P2_wubot}, {"wvbot", P2_wvbot}, {"aam2d", P2_aam2d}, {"ua", P2_ua}, {"uab", P2_uab}, {"va", P2_va}, {"vab", P2_vab}, {"el", P2_el},
      {"elb", P2_elb}, {"et", P2_et}, {"etb", P2_etb}, {"egb", P2_egb}, {"utb", P2_utb}, {"vtb", P2_vtb}, {"adx2d", P2_adx2d}, {"ady2d", P2_ady2d},
      {"advua", P2_advua}, {"advva", P2_advva}};
  static const struct { const char *n; int slot; } r3[] = {
      {"u", P3_u}, {"ub", P3_ub}, {"v", P3_v}, {"vb", P3_vb}, {"w", P3_w}, {"t", P3_t}, {"tb", P3_tb}, {"s", P3_s}, {"sb", P3_sb}, {"rho", P3_rho},
      {"km", P3_km}, {"kh", P3_kh}, {"kq", P3_kq}, {"l", P3_l}, {"q2", P3_q2}, {"q2b", P3_q2b}, {"aam", P3_aam}, {"q2l", P3_q2l}, {"q2lb", P3_q2lb}};
  const uint64_t img = (uint64_t)m->im_global, jmg = (uint64_t)m->jm_global;
  const RVar *v_iint = NULL, *v_time = NULL;
  std::vector<RItem> items;
  {                                                              // doubles of these lengths, no record variables, inside the file
    std::string why = check_var(H, fsize, "iint", VarWant::fixed(NC_ONLY_DOUBLE, {}, VarWant::ONE_VALUE), &v_iint);
    if (why.empty()) why = check_var(H, fsize, "time", VarWant::fixed(NC_ONLY_DOUBLE, {}, VarWant::ONE_VALUE), &v_time);
    for (auto &q : r2) { if (!why.empty()) break; const RVar *v = NULL; why = check_var(H, fsize, q.n, VarWant::fixed(NC_ONLY_DOUBLE, {jmg, img}), &v); items.push_back({v, q.slot, 1}); }
    for (auto &q : r3) { if (!why.empty()) break; const RVar *v = NULL; why = check_var(H, fsize, q.n, VarWant::fixed(NC_ONLY_DOUBLE, {(uint64_t)P.kb, jmg, img}), &v); items.push_back({v, q.slot, P.kb}); }
    if (!why.empty()) return refuse(why);
  }
  // ---- from here on the state changes ----
  { const int rcm = pomgpu_materialize(c); if (rcm) { (void)close(fd); return rcm; } }
  int bad = 0;
  double sc[2] = {0., 0.};                                       // iint, time
  for (int q = 0; q < 2 && !bad; q++) {
    uint64_t u;
    if (pread_all(fd, &u, 8, (q ? v_time : v_iint)->begin)) { bad = 1; break; }
    u = __builtin_bswap64(u);
    memcpy(&sc[q], &u, 8);
  }
  // runs: whole levels of the band of rows j0 .. j0+jm-1 at the file's full width, as many as a buffer holds.  The buffers, the stream and
  // the events live for this call only: the reader is initialisation, called once per run, and their creation is a few milliseconds of
  // the time the call takes
  const size_t band = (size_t)P.jm * (size_t)img * 8;           // bytes of one level's band
  BandReader R;
  if (!bad && (R.open(c, io_run_bytes(c, band, band * (size_t)P.kb)) || hipStreamSynchronize(c->stream) != hipSuccess)) bad = 2;   // what pomgpu_materialize enqueued precedes the first store below
  const hipStream_t cur0 = c->cur;
  c->cur = R.own;                                                // LAUNCH goes to the copy stream: each kernel behind the copy that feeds it
  for (const RItem &it : items) {
    if (bad) break;
    bad = read_levels(c, R, fd, it.v->begin + (uint64_t)(m->j0 - 1) * img * 8, band, jmg * img * 8, it.nlev, [&](int k0, int nl) {
      if (it.nlev == 1) launch_cdf_unpack(c, "k_cdf_unpack", 6, P.b2 + (size_t)it.slot * P.n2, R.stage, P.im, P.jm, nl, P.n2, P.iml, P.jm, (int)img, m->i0 - 1);
      else launch_cdf_unpack(c, "k_cdf_unpack", 6, (pomgpu_st *)(P.b3 + (size_t)it.slot * P.a3) + (size_t)k0 * P.n2, R.stage, P.im, P.jm, nl, P.n2, P.iml, P.jm, (int)img, m->i0 - 1);
    });
  }
  if (!bad) LAUNCH(c, k_restart_depths, grid2(P), blk2(), P);
  c->cur = cur0;
  if (hipStreamSynchronize(R.own) != hipSuccess && !bad) bad = 2;
  R.release();
  (void)close(fd);
  if (bad || c->launch_err) {
    if (bad == 2) (void)hipGetLastError();
    return fail(c, bad == 1 ? POMGPU_EINVAL : POMGPU_EHIP, bad == 1 ? "read_restart: I/O error on %s (the state is unspecified)" : "read_restart: a HIP call failed while reading %s (the state is unspecified)", path);
  }
  pomgpu_mirrors_written(c);
  pom_blkcon con = c->con;
  con.time0 = con.time = sc[1];
  if (con.cont_bry != 0) con.cont_bry = (int)sc[0];
  (void)pomgpu_set_con(c, &con, c->lramp);
  if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, POMGPU_EHIP, "read_restart: %s: synchronise failed", path);
  if (time0_out) *time0_out = sc[1];
  if (iint_out) *iint_out = sc[0];
  return POMGPU_OK;
}

// ---- the tracers' file back (pomgpu_read_tracers, include/pomgpu.h; the writer: cdf_out.hip) ------------------------------------------
// k_cdf_unpack's lane mapping with up to three destinations: the staged value's bytes are reversed once and stored to d0 and, where they
// are given, d1 and d2 -- trNN into tr, and into trb / trf of a file that has no trbNN / trfNN: no second read, no device-to-device copy.
// The two pointers are kernel arguments: the branches around their stores are uniform
__global__ void k_tr_unpack(double *d0, double *d1, double *d2, const void *src, int im, int jm, size_t dl, int dp, int rows, int pitch, int c0) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x), j = (int)(blockIdx.y * blockDim.y + threadIdx.y), k = (int)blockIdx.z;
  if (i >= im || j >= jm) return;
  const double x = CdfRaw<double>::get(src, ((size_t)k * rows + j) * (size_t)pitch + (size_t)(c0 + i));
  const size_t e = (size_t)k * dl + (size_t)j * dp + i;
  d0[e] = x;
  if (d1) d1[e] = x;
  if (d2) d2[e] = x;
}

extern "C" int pomgpu_read_tracers(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m, double *time_out, double *iint_out) {
#ifdef POMGPU_STORE_F32
  if (c) return fail(c, POMGPU_EINVAL, "read_tracers: not in the fp32-storage variant (3-D arrays are not doubles there)");
#endif
  if (!c || !path || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  if (c->flags & POMGPU_CTX_2D) return fail(c, POMGPU_EINVAL, "read_tracers: a context with 3-D arrays");
  if (!c->ntr) return fail(c, POMGPU_EINVAL, "read_tracers: no tracers are registered (pomgpu_set_tracers)");
  { const int rcw = pomgpu_io_wait(c); if (rcw) return rcw; }  // the file may be the one this context is still writing
  const KP &P = c->P;
  if (!tile_fits(m, P, 0, 0, 0, 0))
    return fail(c, POMGPU_EINVAL, "read_tracers: %s: the tile (%d..%d, %d..%d) does not fit the global grid %d x %d", path, m->i0, m->i0 + P.im - 1,
                m->j0, m->j0 + P.jm - 1, m->im_global, m->jm_global);
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(c, POMGPU_EINVAL, "read_tracers: cannot open %s", path);
  struct stat sb;
  if (fstat(fd, &sb)) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_tracers: cannot stat %s", path); }
  const uint64_t fsize = (uint64_t)sb.st_size;
  RHeader H;
  {
    std::string what;
    const int rc = read_header(fd, fsize, H, what);
    if (rc == -2) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_tracers: I/O error on %s (header)", path); }
    if (rc < 0) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_tracers: %s is not a tracer file this library reads: %s", path, what.c_str()); }
  }
  auto refuse = [&](const std::string &why) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_tracers: %s: %s", path, why.c_str()); };
  const uint64_t img = (uint64_t)m->im_global, jmg = (uint64_t)m->jm_global;
  const int ntr = c->ntr;
  auto nn = [](const char *stem, int n) { char b[32]; snprintf(b, sizeof b, "%s%02d", stem, n); return std::string(b); };
  // one value of an optional scalar variable: 0 = absent, 1 = read into *x, -1 = refused (why)
  auto scalar = [&](const std::string &name, double *x, std::string &why) {
    if (!find_var(H, name.c_str())) return 0;
    const RVar *v = NULL;
    why = check_var(H, fsize, name.c_str(), VarWant::fixed(NC_ONLY_DOUBLE, {}, VarWant::ONE_VALUE), &v);
    if (!why.empty()) return -1;
    uint64_t u;
    if (pread_all(fd, &u, 8, v->begin)) { why = "I/O error (" + name + ")"; return -1; }
    u = __builtin_bswap64(u);
    memcpy(x, &u, 8);
    return 1;
  };
  // ---- every variable, and every scalar's value, before anything changes ----
  struct TItem { const RVar *v; double *d[3]; };
  std::vector<TItem> items;
  int nbc[POMGPU_TRMAX], has_set[POMGPU_TRMAX];
  double lam[POMGPU_TRMAX], sc[2] = {0., 0.};                    // time, iint
  {
    std::string why;
    if (scalar("time", &sc[0], why) < 0 || scalar("iint", &sc[1], why) < 0) return refuse(why);
    const std::vector<uint64_t> want = {(uint64_t)P.kb, jmg, img};
    for (int n = 1; n <= ntr; n++) {
      pomgpu_ctx::pomgpu_tracer &t = c->trc[n - 1];
      const RVar *v = NULL, *vb = NULL, *vf = NULL;
      why = check_var(H, fsize, nn("tr", n).c_str(), VarWant::fixed(NC_ONLY_DOUBLE, want), &v);
      if (why.empty() && find_var(H, nn("trb", n).c_str())) why = check_var(H, fsize, nn("trb", n).c_str(), VarWant::fixed(NC_ONLY_DOUBLE, want), &vb);
      if (why.empty() && find_var(H, nn("trf", n).c_str())) why = check_var(H, fsize, nn("trf", n).c_str(), VarWant::fixed(NC_ONLY_DOUBLE, want), &vf);
      if (!why.empty()) return refuse(why);
      items.push_back({v, {t.tr, vb ? NULL : t.trb, vf ? NULL : t.trf}});
      if (vb) items.push_back({vb, {t.trb, NULL, NULL}});
      if (vf) items.push_back({vf, {t.trf, NULL, NULL}});
      double xn = (double)t.nbc;
      lam[n - 1] = t.lam;
      const int hn = scalar(nn("nbc", n), &xn, why), hl = hn < 0 ? -1 : scalar(nn("lam", n), &lam[n - 1], why);
      if (hn < 0 || hl < 0) return refuse(why);
      if (xn != 1. && xn != 3.)
        return refuse("variable " + nn("nbc", n) + " holds " + std::to_string(xn) + "; a tracer takes 1 (the flux wtrsurf) or 3 (the value trsurf)");
      nbc[n - 1] = (int)xn;
      has_set[n - 1] = hn > 0 || hl > 0;
    }
  }
  // ---- from here on the tracers change ----
  for (int n = 1; n <= ntr; n++) if (has_set[n - 1]) { c->trc[n - 1].nbc = nbc[n - 1]; c->trc[n - 1].lam = lam[n - 1]; }
  int bad = 0;
  const size_t band = (size_t)P.jm * (size_t)img * 8;           // bytes of one level's band
  BandReader R;
  if (R.open(c, io_run_bytes(c, band, band * (size_t)P.kb)) || hipStreamSynchronize(c->stream) != hipSuccess) bad = 2;   // the steps that still use the tracers precede the first store below
  const hipStream_t cur0 = c->cur;
  c->cur = R.own;                                                // LAUNCH goes to the copy stream: each kernel behind the copy that feeds it
  const dim3 grid((unsigned)((P.im + 63) / 64), (unsigned)((P.jm + 3) / 4), 1);
  for (const TItem &it : items) {
    if (bad) break;
    bad = read_levels(c, R, fd, it.v->begin + (uint64_t)(m->j0 - 1) * img * 8, band, jmg * img * 8, P.kb, [&](int k0, int nl) {
      const size_t o = (size_t)k0 * P.n2;
      LAUNCH(c, k_tr_unpack, dim3(grid.x, grid.y, (unsigned)nl), blk2(), it.d[0] + o, it.d[1] ? it.d[1] + o : (double *)NULL, it.d[2] ? it.d[2] + o : (double *)NULL,
             (const void *)R.stage, P.im, P.jm, P.n2, P.iml, P.jm, (int)img, m->i0 - 1);
    });
  }
  c->cur = cur0;
  if (hipStreamSynchronize(R.own) != hipSuccess && !bad) bad = 2;
  R.release();
  (void)close(fd);
  if (bad || c->launch_err) {
    if (bad == 2) (void)hipGetLastError();
    return fail(c, bad == 1 ? POMGPU_EINVAL : POMGPU_EHIP, bad == 1 ? "read_tracers: I/O error on %s (the tracers are unspecified)" : "read_tracers: a HIP call failed while reading %s (the tracers are unspecified)", path);
  }
  if (time_out) *time_out = sc[0];
  if (iint_out) *iint_out = sc[1];
  return POMGPU_OK;
}

// ---- the float file back (pomgpu_read_floats, include/pomgpu.h; the writer: cdf_out.hip) -------------------------------------------------
// 1-D arrays of a few bytes a float: read and byte-swapped on the host, then registered as pomgpu_float_upload registers host arrays
extern "C" int pomgpu_read_floats(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m, double *time_out, double *iint_out) {
#ifdef POMGPU_STORE_F32
  if (c) return fail(c, POMGPU_EINVAL, "read_floats: not in the fp32-storage variant (3-D arrays are not doubles there)");
#endif
  if (!c || !path || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  if (c->flags & POMGPU_CTX_2D) return fail(c, POMGPU_EINVAL, "read_floats: a context with 3-D arrays");
  { const int rcw = pomgpu_io_wait(c); if (rcw) return rcw; }
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(c, POMGPU_EINVAL, "read_floats: cannot open %s", path);
  struct stat sb;
  if (fstat(fd, &sb)) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_floats: cannot stat %s", path); }
  const uint64_t fsize = (uint64_t)sb.st_size;
  RHeader H;
  {
    std::string what;
    const int rc = read_header(fd, fsize, H, what);
    if (rc == -2) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_floats: I/O error on %s (header)", path); }
    if (rc < 0) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_floats: %s is not a float file this library reads: %s", path, what.c_str()); }
  }
  auto refuse = [&](const std::string &why) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_floats: %s: %s", path, why.c_str()); };
  // ---- every variable and every value before anything changes ----
  const RVar *vx = find_var(H, "x");
  if (!vx) return refuse("variable x is absent");
  if (vx->dimids.size() != 1) return refuse("variable x has the dimension lengths " + lengths_of(H, *vx) + ", wanted one dimension");
  const uint64_t N = H.dimlen[vx->dimids[0]];
  if (N == 0) return refuse("variable x is a record variable (unlimited dimension)");
  if (N > (uint64_t)POMGPU_MAXFLOATS) return refuse("the file holds " + std::to_string(N) + " floats, 0.." + std::to_string(POMGPU_MAXFLOATS) + " are possible");
  static const char *const DN[3] = {"x", "y", "sig"}, *const INAMES[3] = {"status", "kind", "id"};
  const RVar *dv[3] = {NULL, NULL, NULL}, *iv[3] = {NULL, NULL, NULL}, *v_time = NULL, *v_iint = NULL;
  std::string why;
  for (int q = 0; q < 3 && why.empty(); q++) why = check_var(H, fsize, DN[q], VarWant::fixed(NC_ONLY_DOUBLE, {N}), &dv[q]);
  for (int q = 0; q < 3 && why.empty(); q++) if (find_var(H, INAMES[q])) why = check_var(H, fsize, INAMES[q], VarWant::fixed(1u << 4, {N}), &iv[q]);
  if (why.empty() && find_var(H, "time")) why = check_var(H, fsize, "time", VarWant::fixed(NC_ONLY_DOUBLE, {}, VarWant::ONE_VALUE), &v_time);
  if (why.empty() && find_var(H, "iint")) why = check_var(H, fsize, "iint", VarWant::fixed(NC_ONLY_DOUBLE, {}, VarWant::ONE_VALUE), &v_iint);
  if (!why.empty()) return refuse(why);
  std::vector<double> dbl(3 * (size_t)N);
  std::vector<int> itg(3 * (size_t)N);
  double sc[2] = {0., 0.};                                       // time, iint
  for (int q = 0; q < 3; q++) {
    if (pread_all(fd, dbl.data() + (size_t)q * N, 8 * (size_t)N, dv[q]->begin)) return refuse(std::string("I/O error (") + DN[q] + ")");
    if (iv[q] && pread_all(fd, itg.data() + (size_t)q * N, 4 * (size_t)N, iv[q]->begin)) return refuse(std::string("I/O error (") + INAMES[q] + ")");
  }
  for (int q = 0; q < 2; q++) {
    const RVar *v = q ? v_iint : v_time;
    if (v && pread_all(fd, &sc[q], 8, v->begin)) return refuse("I/O error (time, iint)");
  }
  (void)close(fd);
  auto swap8 = [](double *p, size_t n) { for (size_t e = 0; e < n; e++) { uint64_t u; memcpy(&u, p + e, 8); u = __builtin_bswap64(u); memcpy(p + e, &u, 8); } };
  swap8(dbl.data(), dbl.size());
  swap8(sc, 2);
  for (size_t e = 0; e < itg.size(); e++) itg[e] = (int)__builtin_bswap32((uint32_t)itg[e]);
  // ---- from here on the float set changes (pomgpu_float_register makes the context's own refusals first) ----
  const int rc = pomgpu_float_register(c, "read_floats", (int)N, dbl.data(), dbl.data() + N, dbl.data() + 2 * N, iv[1] ? itg.data() + N : NULL,
                                       iv[2] ? itg.data() + 2 * N : NULL, iv[0] ? itg.data() : NULL);
  if (rc) return rc;
  if (time_out) *time_out = sc[0];
  if (iint_out) *iint_out = sc[1];
  return POMGPU_OK;
}

// ---- the tide file (pomgpu_set_tide_file, include/pomgpu.h) ---------------------------------------------------------------------------------
// omega(ncon) and, per side that has them, el_amp.<side> el_pha.<side> [un_amp.<side> un_pha.<side>], (ncon, jm_global | im_global), NC_DOUBLE,
// found by name; every variable is checked before anything changes.  A few lines: read and byte-swapped on the host, converted as the
// Python layer converts (C = A cos g, S = A sin g, g in degrees) and registered through pomgpu_set_tides, which makes its own refusals
extern "C" int pomgpu_set_tide_file(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m) {
#ifdef POMGPU_STORE_F32
  if (c) return fail(c, POMGPU_EINVAL, "set_tide_file: not in the fp32-storage variant (3-D arrays are not doubles there)");
#endif
  if (!c || !path || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(c, POMGPU_EINVAL, "set_tide_file: cannot open %s", path);
  struct stat sb;
  if (fstat(fd, &sb)) { (void)close(fd); return fail(c, POMGPU_EINVAL, "set_tide_file: cannot stat %s", path); }
  const uint64_t fsize = (uint64_t)sb.st_size;
  RHeader H;
  {
    std::string what;
    const int rc = read_header(fd, fsize, H, what);
    if (rc == -2) { (void)close(fd); return fail(c, POMGPU_EINVAL, "set_tide_file: I/O error on %s (header)", path); }
    if (rc < 0) { (void)close(fd); return fail(c, POMGPU_EINVAL, "set_tide_file: %s is not a tide file this library reads: %s", path, what.c_str()); }
  }
  auto refuse = [&](const std::string &why) { (void)close(fd); return fail(c, POMGPU_EINVAL, "set_tide_file: %s: %s", path, why.c_str()); };
  const RVar *vo = find_var(H, "omega");
  if (!vo) return refuse("variable omega is absent");
  if (vo->dimids.size() != 1) return refuse("variable omega has the dimension lengths " + lengths_of(H, *vo) + ", wanted one dimension");
  const uint64_t NC = H.dimlen[vo->dimids[0]];
  if (NC < 1 || NC > (uint64_t)POMGPU_MAXTIDES) return refuse("the file holds " + std::to_string(NC) + " constituents, 1.." + std::to_string(POMGPU_MAXTIDES) + " are possible");
  std::string why = check_var(H, fsize, "omega", VarWant::fixed(NC_ONLY_DOUBLE, {NC}), &vo);
  static const char *const SIDE[4] = {"east", "south", "west", "north"}, *const STEM[4] = {"el_amp", "el_pha", "un_amp", "un_pha"};
  const RVar *lv[4][4] = {};
  int sides = 0;
  for (int s = 0; s < 4 && why.empty(); s++) {
    const uint64_t n = (uint64_t)((s == 0 || s == 2) ? m->jm_global : m->im_global);
    bool have[4];
    for (int q = 0; q < 4; q++) have[q] = find_var(H, (std::string(STEM[q]) + "." + SIDE[s]).c_str()) != NULL;
    if (have[0] != have[1] || have[2] != have[3]) { why = std::string("the ") + SIDE[s] + " side has an amplitude without its phase, or a phase without its amplitude"; break; }
    if (have[2] && !have[0]) { why = std::string("the ") + SIDE[s] + " side has un lines and no el lines"; break; }
    for (int q = 0; q < 4 && why.empty(); q++)
      if (have[q]) why = check_var(H, fsize, (std::string(STEM[q]) + "." + SIDE[s]).c_str(), VarWant::fixed(NC_ONLY_DOUBLE, {NC, n}), &lv[s][q]);
    if (have[0]) sides |= 1 << s;
  }
  if (!why.empty()) return refuse(why);
  auto swap8 = [](double *p, size_t n) { for (size_t e = 0; e < n; e++) { uint64_t u; memcpy(&u, p + e, 8); u = __builtin_bswap64(u); memcpy(p + e, &u, 8); } };
  std::vector<double> omega((size_t)NC);
  if (pread_all(fd, omega.data(), 8 * (size_t)NC, vo->begin)) return refuse("I/O error (omega)");
  swap8(omega.data(), omega.size());
  std::vector<double> buf[4][4];
  const double *lines[16] = {};
  for (int s = 0; s < 4; s++) {
    const size_t n = (size_t)NC * (size_t)((s == 0 || s == 2) ? m->jm_global : m->im_global);
    for (int q0 = 0; q0 < 4; q0 += 2) {
      if (!lv[s][q0]) continue;
      std::vector<double> amp(n), pha(n);
      if (pread_all(fd, amp.data(), 8 * n, lv[s][q0]->begin) || pread_all(fd, pha.data(), 8 * n, lv[s][q0 + 1]->begin)) return refuse(std::string("I/O error (") + SIDE[s] + ")");
      swap8(amp.data(), n); swap8(pha.data(), n);
      buf[s][q0].resize(n); buf[s][q0 + 1].resize(n);
      for (size_t e = 0; e < n; e++) {
        const double g = pha[e] * (3.14159265358979323846 / 180.);
        buf[s][q0][e] = amp[e] * cos(g);
        buf[s][q0 + 1][e] = amp[e] * sin(g);
      }
      lines[4 * s + q0] = buf[s][q0].data(); lines[4 * s + q0 + 1] = buf[s][q0 + 1].data();
    }
  }
  (void)close(fd);
  return pomgpu_set_tides(c, (int)NC, omega.data(), sides, lines, m);   // from here on the table changes; its own refusals come first
}

// ---- a cold start from the reference's input files (pomgpu_cold_start) ---------------------------------------------------------------
// initialize.f:24-36 after read_input: initialize_arrays, read_grid (read_grid_pnetcdf io_pnetcdf.F:2085-2263, initialize.f:317-389),
// initial_conditions (read_initial_ts_pnetcdf :2771-2842, read_clim_ts_pnetcdf :2845-2909, initialize.f:392-463), update_initial
// (:466-521) and bottom_friction (:524-544) without PnetCDF.  The headers go through read_header, check_var and ff_check; the data path is
// the restart reader's.  What needs sin or log (cor, cbc) is formed on the host with libm from the band while it sits in the pinned buffer;
// dz, dzz likewise.
namespace {
struct CVar { uint32_t type; uint64_t begin; unsigned es; };   // a fixed-size variable of the grid file
struct CPlane { const char *name; int slot; };
const CPlane CS_PLANES[13] = {{"dx", P2_dx}, {"dy", P2_dy}, {"lon_rho", P2_east_e}, {"lat_rho", P2_north_e}, {"lon_u", P2_east_u}, {"lat_u", P2_north_u},
                              {"lon_v", P2_east_v}, {"lat_v", P2_north_v}, {"lon_psi", P2_east_c}, {"lat_psi", P2_north_c}, {"angle", P2_rot}, {"h", P2_h},
                              {"fsm", P2_fsm}};
const char *const CS_INIT[2] = {"T", "S"};
// `name` as one block of the lengths `want` (at_least: one dimension of at least want[0]), of a type in `types`
std::string cold_fixed(const RHeader &H, uint64_t fsize, const char *name, const std::vector<uint64_t> &want, bool at_least, unsigned types, CVar &out) {
  const RVar *v = NULL;
  const std::string why = check_var(H, fsize, name, VarWant::fixed(types, want, at_least ? VarWant::AT_LEAST : VarWant::EXACT), &v);
  if (v) out = {v->type, v->begin, NC_TYPE_BYTES[v->type]};
  return why;
}
}  // namespace
// the readers' defaults over the whole padded arrays (io_pnetcdf.F:2159-2171; the others and fsm are zero already)
__global__ void k_cold_defaults(KP P) {
  const int i = TID_I, j = TID_J;
  if (i > P.iml || j > P.jml) return;
  F2(dx, i, j) = 1.;
  F2(dy, i, j) = 1.;
  F2(h, i, j) = 1.;
}
// One plane of the grid file.  Thread mapping of k_cdf_unpack over the tile's WINDOW: the band holds wj more rows below the tile's first
// and the lanes reach wi more columns to its west (a tile with a south / west neighbour; 0 or 1).  The tile's part lands in
// X(1:im, 1:jm); `win` (dx, dy, fsm; else NULL) keeps window and tile as (0:im, 0:jm) for k_cold_grid2d, line 0 being the window's.
__global__ void k_cold_plane(double *dst, double *win, const void *src, unsigned type, int im, int jm, int iml, int wi, int wj, int pitch, int c0) {
  const int a = (int)(blockIdx.x * blockDim.x + threadIdx.x), b = (int)(blockIdx.y * blockDim.y + threadIdx.y);
  if (a >= im + wi || b >= jm + wj) return;
  const double x = cdf_raw(type, src, (size_t)b * (size_t)pitch + (size_t)(c0 + a));
  const int i = a - wi + 1, j = b - wj + 1;                       // 1-based in the tile; 0: the window line
  if (i >= 1 && j >= 1) dst[(size_t)(j - 1) * iml + (i - 1)] = x;
  if (win) win[(size_t)j * (im + 1) + i] = x;
}
// read_grid's 2-D fields (initialize.f:361-384, io_pnetcdf.F:2243-2254, parallel_mpi.f:496), one lane per cell.  art, d, dt are
// whole-array statements and cover the padding; the rest covers (1:im, 1:jm).  aru, arv: the loop's formula wherever its operands
// exist -- the window supplies column 0 / row 0 of a tile with a neighbour there, which is what exchange2d_mpi brings from the owner --
// and on global column 1, then global row 1, the copy of the line next to it (:373-381), i.e. the formula of that line.
#define WN(p, ii, jj) (p)[(size_t)(jj) * (size_t)(P.im + 1) + (size_t)(ii)]
__global__ void k_cold_grid2d(KP P, const double *wdx, const double *wdy, const double *wfsm, int wi, int wj, double *cfl) {
  const int i = TID_I, j = TID_J;
  if (i > P.iml || j > P.jml) return;
  const double dxc = F2(dx, i, j), dyc = F2(dy, i, j), hc = F2(h, i, j);
  F2(art, i, j) = dxc * dyc;
  F2(d, i, j) = hc + F2(el, i, j);
  F2(dt, i, j) = hc + F2(et, i, j);
  if (i > P.im || j > P.jm) return;
  const int ie = (i == 1 && !wi) ? 2 : i, je = (j == 1 && !wj) ? 2 : j;
  F2(aru, i, j) = .25 * (WN(wdx, ie, je) + WN(wdx, ie - 1, je)) * (WN(wdy, ie, je) + WN(wdy, ie - 1, je));
  F2(arv, i, j) = .25 * (WN(wdx, ie, je) + WN(wdx, ie, je - 1)) * (WN(wdy, ie, je) + WN(wdy, ie, je - 1));
  const double fs = WN(wfsm, i, j);
  const bool west = i > 1 || wi, south = j > 1 || wj;            // is there a cell behind this one?
  F2(dum, i, j) = (west && WN(wfsm, i - 1, j) == 0. && fs != 0.) ? 0. : fs;
  F2(dvm, i, j) = (south && WN(wfsm, i, j - 1) == 0. && fs != 0.) ? 0. : fs;
  cfl[IX2(i, j)] = .5 / sqrt(1. / (dxc * dxc) + 1. / (dyc * dyc)) / sqrt(P.grav * (hc + P.small_)) * fs;
}
#undef WN
// minval(cfl, cfl > 0) (parallel_mpi.f:499) over (1:im, 1:jm): one workgroup, k_reduce.hip's tree (a strided share per lane, the
// wavefront shuffle tree, four partials through LDS), no atomics.  min is exact, so the shape does not show in the result.  The host
// emulation, which has no lanes to shuffle between, scans the plane in the launcher instead
#ifndef POMGPU_EMU
__global__ void __launch_bounds__(256) k_cold_cflmin(KP P, const double *cfl, double *out) {
  __shared__ double part[4];
  double m = __DBL_MAX__;                                        // minval of nothing: huge()
  const long long total = (long long)P.im * P.jm;
  for (long long n = threadIdx.x; n < total; n += blockDim.x) {
    const double x = cfl[IX2((int)(n % P.im) + 1, (int)(n / P.im) + 1)];
    if (x > 0. && x < m) m = x;
  }
  for (int off = 32; off > 0; off >>= 1) { const double y = __shfl_down(m, off, 64); if (y < m) m = y; }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) { for (int w = 1; w < 4; w++) if (part[w] < m) m = part[w]; out[0] = m; }
}
#endif
// Levels k0+1 .. k0+gridDim.z (all <= kbm1) of T (which = 0) or S (1), read from the staging buffer once: tb and t (sb and s) get the
// same bits -- rounded to the storage type as an upload rounds -- tsurf (ssurf) level 1, and the boundary arrays their lines
// (initialize.f:437-438, :447-460, :497-498)
template <class T>
__global__ void k_cold_ts(KP P, int which, const void *src, int rows, int pitch, int c0, int k0) {
  const int i = TID_I, j = TID_J, k = k0 + (int)blockIdx.z + 1;
  if (i > P.im || j > P.jm) return;
  const double x = (double)(pomgpu_st)CdfRaw<T>::get(src, ((size_t)blockIdx.z * rows + (size_t)(j - 1)) * (size_t)pitch + (size_t)(c0 + i - 1));
  if (which == 0) {
    F3(tb, i, j, k) = x; F3(t, i, j, k) = x;
    if (k == 1) F2(tsurf, i, j) = x;
    if (i == P.im) BDJ(tbe, j, k) = x;
    if (i == 1) BDJ(tbw, j, k) = x;
    if (j == P.jm) BDI(tbn, i, k) = x;
    if (j == 1) BDI(tbs, i, k) = x;
  } else {
    F3(sb, i, j, k) = x; F3(s, i, j, k) = x;
    if (k == 1) F2(ssurf, i, j) = x;
    if (i == P.im) BDJ(sbe, j, k) = x;
    if (i == 1) BDJ(sbw, j, k) = x;
    if (j == P.jm) BDI(sbn, i, k) = x;
    if (j == 1) BDI(sbs, i, k) = x;
  }
}
// update_initial (initialize.f:472-500) on a state whose uab, vab, elb, etb, vfluxf, ub, vb are zero: store only, the column's levels
// in the thread.  ua va el et etf, w(:,:,1), u v are whole-array copies of those zeros; l .. aam cover (1:im, 1:jm) and all kb levels,
// each value formed in fp64 from dt(i,j) and rounded by the store alone; a lane outside aims its stores outside the descriptor.
// d = h+el, dt = h+et (:477-478) repeat what k_cold_grid2d has stored.  0.1 is a REAL(4) literal (:484); q2 = q2b, q2l = q2lb (:495-496)
__global__ void k_cold_update(KP P, double aam_init, double sqrt_small) {
  const int i = TID_I, j = TID_J;
  if (i > P.iml || j > P.jml) return;
  const unsigned o = BOFF2(i, j), oa = (i <= P.im && j <= P.jm) ? o : BOFF_NONE;
  const double lc = (double)0.1f * F2(dt, i, j), q2bc = P.small_, q2lbc = lc * q2bc, khc = lc * sqrt_small;
  F2(ua, i, j) = 0.; F2(va, i, j) = 0.; F2(el, i, j) = 0.; F2(et, i, j) = 0.; F2(etf, i, j) = 0.;
  const BufA bl = BUF3(A3(l)), bq2b = BUF3(A3(q2b)), bq2lb = BUF3(A3(q2lb)), bkh = BUF3(A3(kh)), bkm = BUF3(A3(km)), bkq = BUF3(A3(kq)),
             baam = BUF3(A3(aam)), bq2 = BUF3(A3(q2)), bq2l = BUF3(A3(q2l)), bu = BUF3(A3(u)), bv = BUF3(A3(v)), bw = BUF3(A3(w));
  bst(bw, o, 0u, 0.);
  unsigned so = 0u;
  for (int k = 1; k <= P.kb; k++) {
    bst(bl, oa, so, lc); bst(bq2b, oa, so, q2bc); bst(bq2lb, oa, so, q2lbc);
    bst(bkh, oa, so, khc); bst(bkm, oa, so, khc); bst(bkq, oa, so, khc); bst(baam, oa, so, aam_init);
    bst(bq2, oa, so, q2bc); bst(bq2l, oa, so, q2lbc);
    bst(bu, o, so, 0.); bst(bv, o, so, 0.);
    so += LVB;
  }
}
// drx2d, dry2d (initialize.f:511-518): running sums, from zero, of drhox, drhoy AS STORED (baropg has rounded them to the storage type)
// times dz(k), k ascending
__global__ void k_cold_drsum(KP P) {
  const int i = TID_I, j = TID_J;
  const bool act = i <= P.im && j <= P.jm;
  const unsigned o = act ? BOFF2(i, j) : BOFF_NONE;
  const BufA bx = BUF3(A3(drhox)), by = BUF3(A3(drhoy));
  double sx = 0., sy = 0.;
  unsigned so = 0u;
  for (int k = 1; k <= P.kbm1; k++) {
    const double dzk = F1(dz, k);
    sx = sx + bld(bx, o, so) * dzk;
    sy = sy + bld(by, o, so) * dzk;
    so += LVB;
  }
  if (act) { F2(drx2d, i, j) = sx; F2(dry2d, i, j) = sy; }
}
static void cold_update_initial(pomgpu_ctx *c) { LAUNCH(c, k_cold_update, grid2(c->P), blk2(), c->P, c->con.aam_init, sqrt(c->con.small)); }
static void cold_sums(pomgpu_ctx *c) { LAUNCH(c, k_cold_drsum, grid2(c->P), blk2(), c->P); }

// tb (which = 0) or sb (1) as ztosig has stored it, all kb levels, into what initialize.f:437-460 and update_initial's `t = tb` derive from
// it: the bits k_cold_ts hands out, read back from the mirror (the fp32-storage variants: the rounded value)
__global__ void k_cold_zts(KP P, int which) {
  const int i = TID_I, j = TID_J, k = (int)blockIdx.z + 1;
  if (i > P.im || j > P.jm) return;
  if (which == 0) {
    const double x = F3(tb, i, j, k);
    F3(t, i, j, k) = x;
    if (k == 1) F2(tsurf, i, j) = x;
    if (k <= P.kbm1) {
      if (i == P.im) BDJ(tbe, j, k) = x;
      if (i == 1) BDJ(tbw, j, k) = x;
      if (j == P.jm) BDI(tbn, i, k) = x;
      if (j == 1) BDI(tbs, i, k) = x;
    }
  } else {
    const double x = F3(sb, i, j, k);
    F3(s, i, j, k) = x;
    if (k == 1) F2(ssurf, i, j) = x;
    if (k <= P.kbm1) {
      if (i == P.im) BDJ(sbe, j, k) = x;
      if (i == 1) BDJ(sbw, j, k) = x;
      if (j == P.jm) BDI(sbn, i, k) = x;
      if (j == 1) BDI(sbs, i, k) = x;
    }
  }
}

extern "C" int pomgpu_set_z_inputs(pomgpu_ctx *c, int init_on_z, int clim_on_z) {
  if (!c) return POMGPU_EINVAL;
  if (pomgpu_ff_has(c, 2) && (clim_on_z != 0) != (c->z_clim != 0))
    return fail(c, POMGPU_EINVAL, "set_z_inputs: a clim file is registered (pomgpu_set_forcing_files) as a %s file", c->z_clim ? "z-level" : "sigma-level");
  c->z_init = init_on_z != 0;
  c->z_clim = clim_on_z != 0;
  return POMGPU_OK;
}

extern "C" int pomgpu_set_z_lateral(pomgpu_ctx *c, int lbry_on_z) {
  if (!c) return POMGPU_EINVAL;
  if (pomgpu_ff_has(c, 1) && (lbry_on_z != 0) != (c->z_lbry != 0))
    return fail(c, POMGPU_EINVAL, "set_z_lateral: an lbry file is registered (pomgpu_set_forcing_files) as a %s file", c->z_lbry ? "z-level" : "sigma-level");
  c->z_lbry = lbry_on_z != 0;
  return POMGPU_OK;
}

extern "C" int pomgpu_set_lateral_sides(pomgpu_ctx *c, int sides) {
  if (!c) return POMGPU_EINVAL;
  if (sides < 1 || sides > 15) return fail(c, POMGPU_EINVAL, "set_lateral_sides: the mask %d is outside 1..15 (east 1, south 2, west 4, north 8)", sides);
  if (pomgpu_ff_has(c, 1) && sides != c->lbry_sides)
    return fail(c, POMGPU_EINVAL, "set_lateral_sides: an lbry file is registered (pomgpu_set_forcing_files) under the mask %d, not %d", c->lbry_sides, sides);
  c->lbry_sides = sides;
  return POMGPU_OK;
}

extern "C" int pomgpu_cold_start(pomgpu_ctx *c, const char *grid, const char *init, const char *clim, const pomgpu_file_meta *m, pomgpu_cold_info *info) {
  if (!c || !grid || !init || !clim || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  { const int rcw = pomgpu_io_wait(c); if (rcw) return rcw; }  // a file this context is still writing
  const KP &P = c->P;
  if (c->flags & POMGPU_CTX_2D) return fail(c, POMGPU_EINVAL, "cold_start: not on a 2-D context");
  const int wi = P.W ? 0 : 1, wj = P.S ? 0 : 1;                // one more column / row on the low side of a tile with a neighbour there
  const int zin[2] = {c->z_init, c->z_clim};                   // pomgpu_set_z_inputs: T, S / Tclim, Sclim are on z levels and go through ztosig,
  const int we = (zin[0] || zin[1]) && !P.E ? 1 : 0, wn = (zin[0] || zin[1]) && !P.N ? 1 : 0;   // whose fill-in looks at the neighbour on the high side too
  if (!tile_fits(m, P, wi, we, wj, wn))
    return fail(c, POMGPU_EINVAL, "cold_start: %s: the tile (%d..%d, %d..%d)%s does not fit the global grid %d x %d", grid, m->i0, m->i0 + P.im - 1, m->j0,
                m->j0 + P.jm - 1, we || wn ? " with its window lines towards every neighbour" : (wi || wj ? " with its window line towards the west / south neighbour" : ""),
                m->im_global, m->jm_global);
  if ((zin[0] || zin[1]) && (P.im < 3 || P.jm < 3)) return fail(c, POMGPU_EINVAL, "cold_start: z-level input needs a tile of at least 3 x 3 cells");
  if (c->con.npg != 1 && c->con.npg != 2) return fail(c, POMGPU_EINVAL, "cold_start: invalid value for npg (%d)", c->con.npg);
  const uint64_t img = (uint64_t)m->im_global, jmg = (uint64_t)m->jm_global, kb = (uint64_t)P.kb;
  const char *paths[3] = {grid, init, clim};
  static const char *const kind[3] = {"grid", "init", "clim"};
  FSource F[3];
  RHeader H[3];
  auto drop = [&]() { for (FSource &s : F) if (s.fd >= 0) (void)close(s.fd); };
  for (int q = 0; q < 3; q++) {
    F[q].path = paths[q];
    F[q].fd = open(paths[q], O_RDONLY);
    if (F[q].fd < 0) { drop(); return fail(c, POMGPU_EINVAL, "cold_start: cannot open %s", paths[q]); }
    struct stat sb;
    if (fstat(F[q].fd, &sb)) { drop(); return fail(c, POMGPU_EINVAL, "cold_start: cannot stat %s", paths[q]); }
    F[q].fsize = (uint64_t)sb.st_size;
    std::string what;
    if (read_header(F[q].fd, F[q].fsize, H[q], what) < 0) { drop(); return fail(c, POMGPU_EINVAL, "cold_start: %s is not a %s file this library reads: %s", paths[q], kind[q], what.c_str()); }
  }
  auto refuse = [&](int q, const std::string &why) { drop(); return fail(c, POMGPU_EINVAL, "cold_start: %s: %s", paths[q], why.c_str()); };
  // grid
  CVar vz, vzz, vp[13];
  {
    std::string why = cold_fixed(H[0], F[0].fsize, "z", {kb}, true, NC_REAL, vz);
    if (why.empty()) why = cold_fixed(H[0], F[0].fsize, "zz", {kb}, true, NC_REAL, vzz);
    for (int q = 0; q < 13 && why.empty(); q++) why = cold_fixed(H[0], F[0].fsize, CS_PLANES[q].name, {jmg, img}, false, q == 12 ? NC_NUMBER : NC_REAL, vp[q]);
    if (!why.empty()) return refuse(0, why);
  }
  // init: record 1, levels 1..kb-1 of T, S
  uint64_t nlev[2] = {kb - 1, kb - 1};
  std::vector<double> zlev[2];                                  // the z levels of the init / clim file (pomgpu_set_z_inputs)
  {
    bool unlimited = false, level = false;
    for (uint64_t len : H[1].dimlen) if (len == 0) unlimited = true;
    for (const RVar &v : H[1].vars) {
      if (v.name == "Level") level = true;
      for (int q = 0; q < 2; q++) if (v.name == CS_INIT[q] && v.dimids.size() == 4) nlev[q] = H[1].dimlen[v.dimids[1]];
    }
    if (!unlimited) return refuse(1, "the file has no unlimited dimension");
    if (!level) return refuse(1, "variable Level is absent");
    std::string why = zin[0] ? z_levels(H[1], F[1], "Level", zlev[0]) : std::string();
    if (zin[0] && why.empty()) nlev[0] = nlev[1] = (uint64_t)zlev[0].size();   // T, S must have Level's length, wherever they stand in the header
    if (why.empty()) why = ff_check(H[1], F[1], CS_INIT, {{nlev[0], jmg, img}, {nlev[1], jmg, img}}, 1);
    for (int q = 0; q < 2 && why.empty(); q++) {
      if (!zin[0] && nlev[q] < kb - 1) why = std::string("variable ") + CS_INIT[q] + " has " + std::to_string(nlev[q]) + " levels, wanted >= " + std::to_string(kb - 1);
      else if (!F[1].v[q].rec) why = std::string("variable ") + CS_INIT[q] + " is not a record variable";
    }
    if (why.empty() && (F[1].numrecs < 1 || F[1].numrecs == 0xffffffffu)) why = "the file holds no complete record (numrecs " + std::to_string(F[1].numrecs) + ")";
    if (!why.empty()) return refuse(1, why);
  }
  // clim: record 10 (initialize.f:407), the forcing reader's layout check
  {
    std::string why = zin[1] ? z_levels(H[2], F[2], "z", zlev[1]) : std::string();
    const uint64_t kc = zin[1] && why.empty() ? (uint64_t)zlev[1].size() : kb;
    if (why.empty()) why = ff_check(H[2], F[2], FF_CLIM, {{kc, jmg, img}, {kc, jmg, img}}, 10);
    if (why.empty() && F[2].v[0].rec && F[2].numrecs == 0xffffffffu) why = "the record count is unknown (a file still being written)";
    if (!why.empty()) return refuse(2, why);
  }
  // the reference stops where cor(im/2, jm/2) is zero (initialize.f:354-355): looked at before anything changes
  const double deg2rad = c->con.pi / 180.;
  auto cor_of = [&](double lat) { return 2. * 7.29e-5 * sin(lat * deg2rad); };
  const CVar &vlat = vp[3], &vh = vp[11];
  double cor_mid = 0.;
  {
    unsigned char raw[8];
    const uint64_t cell = (uint64_t)(m->j0 - 1 + P.jm / 2 - 1) * img + (uint64_t)(m->i0 - 1 + P.im / 2 - 1);
    if (pread_all(F[0].fd, raw, vlat.es, vlat.begin + cell * vlat.es)) return refuse(0, "I/O error (lat_rho)");
    cor_mid = cor_of(cdf_raw(vlat.type, raw, 0));
    if (cor_mid == 0.) return refuse(0, "Coriolis problem: cor(im/2, jm/2) of this tile is zero (lat_rho = " + std::to_string(cdf_raw(vlat.type, raw, 0)) + ")");
  }
  // masks are 0 or 1 (the kernels fold repeated mask multiplies; pomgpu_upload checks the same): the tile's window of fsm, read ahead
  {
    const CVar &vf = vp[12];
    std::vector<unsigned char> row((size_t)(P.im + wi) * vf.es);
    for (int j = 0; j < P.jm + wj; j++) {
      const uint64_t cell = (uint64_t)(m->j0 - 1 - wj + j) * img + (uint64_t)(m->i0 - 1 - wi);
      if (pread_all(F[0].fd, row.data(), row.size(), vf.begin + cell * vf.es)) return refuse(0, "I/O error (fsm)");
      for (int i = 0; i < P.im + wi; i++) {
        const double x = cdf_raw(vf.type, row.data(), (size_t)i);
        if (x != 0. && x != 1.)
          return refuse(0, "variable fsm holds " + std::to_string(x) + " at global (" + std::to_string(m->i0 - wi + i) + ", " + std::to_string(m->j0 - wj + j) + "), neither 0 nor 1");
      }
    }
  }
  // ---- from here on the state changes ----
  { const int rcm = pomgpu_materialize(c); if (rcm) { drop(); return rcm; } }
  int bad = 0;
  const size_t nbd = P.bdoff[PB__count - 1] + (size_t)P.iml * P.kb;
  std::vector<double> b1((size_t)POM_NBLK1D * P.kb, 0.), hcor(P.n2, 0.), hcbc(P.n2, 0.);
  {                                                            // z, zz; dz, dzz (initialize.f:331-336)
    std::vector<unsigned char> raw((size_t)P.kb * 8);
    for (int q = 0; q < 2 && !bad; q++) {
      const CVar &v = q ? vzz : vz;
      if (pread_all(F[0].fd, raw.data(), (size_t)P.kb * v.es, v.begin)) { bad = 1; break; }
      double *x = b1.data() + (size_t)(q ? P1_zz : P1_z) * P.kb, *dx = b1.data() + (size_t)(q ? P1_dzz : P1_dz) * P.kb;
      for (int k = 0; k < P.kb; k++) x[k] = cdf_raw(v.type, raw.data(), (size_t)k);
      for (int k = 0; k < P.kb - 1; k++) dx[k] = x[k] - x[k + 1];
      dx[P.kb - 1] = 0.;
    }
  }
  // the COMMON blocks as they are at program start and as initialize_arrays leaves them, then the readers' defaults
  if (!bad && (hipMemsetAsync(P.b2, 0, sizeof(double) * POM_NBLK2D * P.n2, c->stream) != hipSuccess || hipMemsetAsync(P.bd, 0, sizeof(double) * nbd, c->stream) != hipSuccess ||
               hipMemcpyAsync(P.b1, b1.data(), sizeof(double) * b1.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess)) bad = 2;
  for (int n = 0; n < POM_NBLK3D && !bad; n++) if (hipMemsetAsync(P.b3 + (size_t)n * P.a3, 0, sizeof(double) * P.n3, c->stream) != hipSuccess) bad = 2;
  if (!bad) LAUNCH(c, k_cold_defaults, grid2(P), blk2(), P);
  // the buffers of the restart reader's loop, for this call only; a run is whole levels of the tile's band of rows at the file's full width
  const size_t band2 = (size_t)(P.jm + wj + wn) * (size_t)img * 8, band3 = (size_t)P.jm * (size_t)img * 8;
  const size_t nwin = (size_t)(P.im + 1) * (size_t)(P.jm + 1);
  double *win = NULL;                                            // dx, dy, fsm over the window
  if (!bad && hipMalloc((void **)&win, 3 * nwin * sizeof(double)) != hipSuccess) bad = 2;
  ZWindow Z;                                                     // z-level input: one window, the table of either file
  if (!bad && (zin[0] || zin[1]) && Z.alloc(c, wi, we, wj, wn, zlev[0], zlev[1])) bad = 2;
  BandReader R;
  if (!bad && R.open(c, io_run_bytes(c, band2, band3 * (size_t)P.kb))) bad = 2;
  if (hipStreamSynchronize(c->stream) != hipSuccess && !bad) bad = 2;   // the zeroes precede the first store of the copy stream
  const hipStream_t cur0 = c->cur;
  c->cur = R.own;
  const int c0 = m->i0 - 1 - wi;                                 // the file column (0-based) of the window's first
  for (int q = 0; q < 13 && !bad; q++) {                         // the planes of the grid file, rows j0-wj .. j0+jm-1
    const CVar &v = vp[q];
    const size_t bytes = (size_t)(P.jm + wj) * (size_t)img * v.es;
    unsigned char *pin = R.acquire();
    if (!pin) { bad = 2; break; }
    if (read_bands(F[0].fd, pin, v.begin + (uint64_t)(m->j0 - 1 - wj) * img * v.es, bytes, bytes, 1)) { bad = 1; break; }
    if (R.send(c, bytes)) { bad = 2; break; }
    if (&v == &vlat || &v == &vh) {                              // cor (initialize.f:349) and cbc (:536-540) on the host, from the band still in the pinned buffer
      const double zk = 1. + b1[(size_t)P1_zz * P.kb + (P.kbm1 - 1)];
      for (int j = 0; j < P.jm; j++)
        for (int i = 0; i < P.im; i++) {
          const double x = cdf_raw(v.type, pin, (size_t)(j + wj) * (size_t)img + (size_t)(m->i0 - 1 + i));
          if (&v == &vlat) hcor[(size_t)j * P.iml + i] = cor_of(x);
          else {
            const double t = c->con.kappa / log(zk * x / c->con.z0b), cb = t * t;
            hcbc[(size_t)j * P.iml + i] = fmin(c->con.cbcmax, fmax(c->con.cbcmin, cb));
          }
        }
    }
    double *w = q == 0 ? win : (q == 1 ? win + nwin : (q == 12 ? win + 2 * nwin : NULL));
    LAUNCH(c, k_cold_plane, dim3((unsigned)((P.im + wi + 63) / 64), (unsigned)((P.jm + wj + 3) / 4), 1), blk2(), P.b2 + (size_t)CS_PLANES[q].slot * P.n2, w, (const void *)R.stage,
           (unsigned)v.type, P.im, P.jm, P.iml, wi, wj, (int)img, c0);
  }
  for (int q = 0; q < 4 && !bad; q++) {                          // T, S (record 1, levels 1..kbm1), Tclim, Sclim (record 10, kb levels)
    const bool ini = q < 2;
    const FVar &f = ini ? F[1].v[q] : F[2].v[q - 2];
    const int zq = ini ? 0 : 1, onz = zin[zq];                   // all ks levels over the window, then ztosig; else the sigma levels over the tile
    const int nlv = onz ? Z.ks[zq] : (ini ? P.kbm1 : P.kb), rows = onz ? Z.rows(P) : P.jm, cols = Z.cols(P);
    const uint64_t base = f.begin + (ini ? 0 : 9 * f.stride) + (uint64_t)(m->j0 - 1 - (onz ? wj : 0)) * img * f.esize();
    double *t = P.b3 + (size_t)(q == 0 ? P3_tb : (q == 1 ? P3_sb : (q == 2 ? P3_tclim : P3_sclim))) * P.a3;
    bad = read_levels(c, R, ini ? F[1].fd : F[2].fd, base, (size_t)rows * (size_t)img * f.esize(), jmg * img * f.esize(), nlv, [&](int k0, int nl) {
      if (onz) launch_cdf_unpack(c, "k_rst_unpack", f.type, Z.win() + (size_t)k0 * rows * cols, R.stage, cols, rows, nl, (size_t)rows * cols, cols, rows, (int)img, c0);
      else if (ini) {
        const dim3 g((unsigned)((P.im + 63) / 64), (unsigned)((P.jm + 3) / 4), (unsigned)nl);
        if (f.type == 5) LAUNCHN(c, "k_cold_ts", k_cold_ts<float>, g, blk2(), P, q, (const void *)R.stage, P.jm, (int)img, m->i0 - 1, k0);
        else LAUNCHN(c, "k_cold_ts", k_cold_ts<double>, g, blk2(), P, q, (const void *)R.stage, P.jm, (int)img, m->i0 - 1, k0);
      } else launch_cdf_unpack(c, "k_cold_vol", f.type, (pomgpu_st *)t + (size_t)k0 * P.n2, R.stage, P.im, P.jm, nl, P.n2, P.iml, P.jm, (int)img, m->i0 - 1);
    });
    if (onz && !bad) {
      launch_ztosig_window(c, t, 0, Z, zq);
      if (ini) LAUNCH(c, k_cold_zts, grid3(P, P.kb), blk2(), P, q);
    }
  }
  c->cur = cur0;
  if (hipStreamSynchronize(R.own) != hipSuccess && !bad) bad = 2;
  R.release();
  drop();
  // ---- the files are on the device: what read_grid, initial_conditions, update_initial and bottom_friction derive ----
  double cflmin = __DBL_MAX__;
  if (!bad && !c->launch_err) {
    pom_blkcon con = c->con;
    con.period = (2. * con.pi) / fabs(cor_mid) / 86400.;         // initialize.f:357, from THIS tile's midpoint
    con.rfe = con.rfw = con.rfn = con.rfs = 1.;                  // :442-445
    (void)pomgpu_set_con(c, &con, c->lramp);
    if (hipMemcpyAsync(P.b2 + (size_t)P2_cor * P.n2, hcor.data(), sizeof(double) * P.n2, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(P.b2 + (size_t)P2_cbc * P.n2, hcbc.data(), sizeof(double) * P.n2, hipMemcpyHostToDevice, c->stream) != hipSuccess) bad = 2;
    double *cfl = P.s2[7];
    LAUNCH(c, k_cold_grid2d, grid2(P), blk2(), P, (const double *)win, (const double *)(win + nwin), (const double *)(win + 2 * nwin), wi, wj, cfl);
#ifndef POMGPU_EMU
    LAUNCH(c, k_cold_cflmin, dim3(1), dim3(256), P, (const double *)cfl, c->d_stats);
    if (hipMemcpyAsync(&cflmin, c->d_stats, sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) bad = 2;
#else
    for (int j = 1; j <= P.jm; j++) for (int i = 1; i <= P.im; i++) { const double x = cfl[IX2(i, j)]; if (x > 0. && x < cflmin) cflmin = x; }
#endif
    pomgpu_cold_tail(c, cold_update_initial, cold_sums);
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess && !bad) bad = 2;
  if (win) (void)hipFree(win);
  Z.free();
  if (bad || c->launch_err) {
    if (bad == 2) (void)hipGetLastError();
    return fail(c, bad == 1 ? POMGPU_EINVAL : POMGPU_EHIP, bad == 1 ? "cold_start: I/O error on %s, %s or %s (the state is unspecified)" : "cold_start: a HIP call failed while reading %s, %s or %s (the state is unspecified)", grid, init, clim);
  }
  if (info) { info->cflmin = cflmin; info->period = c->con.period; }
  return POMGPU_OK;
}
