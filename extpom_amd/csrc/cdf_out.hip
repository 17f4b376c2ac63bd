// cdf_out.hip -- the writer: the output and restart files of the reference WITHOUT PnetCDF.  Host code plus device-to-host copies; the
// only kernels are the two of the time-mean output (k_mean_accum, k_mean_snapshot); the passive tracers' files and means (pomgpu_write_tracers)
// are at the end of the file.  The readers are cdf_in.hip
// (restart, cold start) and frc_files.hip (forcing records).
// io_pnetcdf.F writes NetCDF "64-bit offset" files
// (nf_64bit_offset = CDF-2) through the parallel library: write_output_pnetcdf (:57-410) and
// write_restart_pnetcdf (:1661-2083).  The classic format is simple enough to emit directly: a header (dimensions,
// global attributes, variables with their attributes and byte offsets) followed by every variable's values as
// big-endian doubles in definition order.  Same dimension names and lengths, same variable names, order,
// dimensions (Fortran's (x,y,zz,time) is (time,zz,y,x) in the file), types (all nf_double, def_var_pnetcdf :6-40)
// and attribute texts, so existing post-processing keeps working.  Every rank writes its own (im,jm) patch at
// (i_global(1), j_global(1)) with pwrite into the one file, as the collective put_vara calls do; rank 0 creates
// it (create = 1), the others open it afterwards (create = 0; the caller orders the two with a barrier).
// One deliberate difference: the reference passes length 26 for the 10-character text of vtot's
// formula_terms attribute (:133-135, reading past the literal); here the attribute is the 10 characters.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#ifndef POMGPU_EMU
#include <thread>
#endif

#include "cdf_io.hpp"
#define fail pomgpu_fail

namespace {
struct Att { std::string name, text; };
enum Src { SCALAR, LEVELS1D, PLANE2D, VOLUME3D, VALUES1D };
struct Var {
  std::string name;
  std::vector<int> dims;          // dimension ids, slowest first (file order)
  std::vector<Att> atts;
  Src src; int slot; int nlev;    // slot: blk1d / blk2d / blk3d member; nlev: levels written (3-D), values (1-D)
  double value;                   // SCALAR
  uint64_t begin;
  const double *dev;              // VOLUME3D outside blk3d (a tracer's array): the device address; NULL = the slot's mirror
  int tmean;                      // the tracer (0-based) whose mean accumulator supplies the values in a tracer mean file, -1 = none
  std::vector<double> vals;       // VALUES1D: the values of a 1-D variable the caller holds on the host (the harmonics file's omega)
};
struct Spec { std::vector<std::pair<std::string, int>> dims; std::vector<Att> gatts; std::vector<Var> vars; };

void put32(std::string &h, uint32_t v) { for (int s = 24; s >= 0; s -= 8) h.push_back((char)((v >> s) & 0xff)); }
void put64(std::string &h, uint64_t v) { for (int s = 56; s >= 0; s -= 8) h.push_back((char)((v >> s) & 0xff)); }
void putname(std::string &h, const std::string &s) { put32(h, (uint32_t)s.size()); h += s; while (h.size() % 4) h.push_back('\0'); }
void putatts(std::string &h, const std::vector<Att> &a) {
  if (a.empty()) { put32(h, 0); put32(h, 0); return; }          // ABSENT
  put32(h, 0x0C); put32(h, (uint32_t)a.size());                  // NC_ATTRIBUTE
  for (const Att &t : a) { putname(h, t.name); put32(h, 2); put32(h, (uint32_t)t.text.size()); h += t.text; while (h.size() % 4) h.push_back('\0'); }
}
uint64_t var_bytes(const Spec &S, const Var &v) { uint64_t n = 8; for (int d : v.dims) n *= (uint64_t)S.dims[d].second; return n; }
std::string header(Spec &S) {
  for (int pass = 0; pass < 2; pass++) {                         // pass 0 measures, pass 1 has the offsets
    std::string h("CDF\002", 4);
    put32(h, 0);                                                 // numrecs: no record dimension
    put32(h, 0x0A); put32(h, (uint32_t)S.dims.size());           // NC_DIMENSION
    for (auto &d : S.dims) { putname(h, d.first); put32(h, (uint32_t)d.second); }
    putatts(h, S.gatts);
    put32(h, 0x0B); put32(h, (uint32_t)S.vars.size());           // NC_VARIABLE
    for (Var &v : S.vars) {
      putname(h, v.name); put32(h, (uint32_t)v.dims.size());
      for (int d : v.dims) put32(h, (uint32_t)d);
      putatts(h, v.atts);
      put32(h, 6);                                               // NC_DOUBLE
      const uint64_t nb = var_bytes(S, v);
      put32(h, nb > 0xffffffffULL ? 0xffffffffu : (uint32_t)nb); // vsize (saturates, as the format prescribes)
      put64(h, v.begin);
    }
    if (pass == 1) return h;
    uint64_t off = h.size();
    for (Var &v : S.vars) { v.begin = off; off += var_bytes(S, v); }
  }
  return std::string();
}
Var mk(const char *name, std::vector<int> dims, const char *long_name, const char *units, const char *coords, Src src, int slot, int nlev,
       double value = 0.) {
  Var v; v.name = name; v.dims = dims; v.src = src; v.slot = slot; v.nlev = nlev; v.value = value; v.begin = 0; v.dev = NULL; v.tmean = -1;
  v.atts.push_back({"long_name", long_name}); v.atts.push_back({"units", units});
  if (coords) v.atts.push_back({"coordinates", coords});
  return v;
}
int write_be(int fd, const double *x, size_t n, uint64_t off, std::vector<uint64_t> &tmp) {
  tmp.resize(n);
  for (size_t q = 0; q < n; q++) { uint64_t u; memcpy(&u, &x[q], 8); tmp[q] = __builtin_bswap64(u); }
  const char *p = (const char *)tmp.data();
  size_t left = n * 8;
  while (left) { const ssize_t w = pwrite(fd, p, left, (off_t)off); if (w <= 0) return -1; p += w; off += (uint64_t)w; left -= (size_t)w; }
  return 0;
}
}  // namespace

// Writing a file does not hold the model up ("async D2H on a copy stream").  The call (i) lays the file out
// (header, full length) at once, so that other ranks may open it after the caller's barrier, (ii) takes a SNAPSHOT of
// every array the file holds with device-to-device copies on the kernels' stream (a few ms at HBM speed; the model may
// overwrite the arrays right after), records an event and returns; (iii) a host thread waits for that event on a copy
// stream of its own, brings the snapshot over through a pinned buffer, swaps bytes and pwrites.  pomgpu_io_wait() joins
// it (also called by pomgpu_sync, the next write and pomgpu_destroy) and reports its I/O status.  POMGPU_IO_SYNC=1, a
// snapshot that does not fit, and the host emulation keep the old synchronous path.
struct IoJob {
  Spec S;
  std::string path;
  int fd = -1, im = 0, jm = 0, iml = 0, jml = 0, kb = 0, i0 = 1, j0 = 1, im_global = 0, jm_global = 0, create = 0, device = 0;
  size_t n2 = 0;
  double *snap = NULL;                 // device: the snapshot, variables back to back in the order of S.vars
  std::vector<double> b1;              // blk1d (host copy taken at the call)
#ifndef POMGPU_EMU
  std::thread th;
  hipEvent_t ev = NULL;
  hipStream_t st = NULL;
#endif
  int rc = 0, active = 0;
};
static size_t var_doubles(const IoJob &J, const Var &v) { return v.src == PLANE2D ? J.n2 : (v.src == VOLUME3D ? (size_t)v.nlev * J.n2 : 0); }
// rows of one variable (host copy `host`, leading dimensions iml x jml) into the file
static int put_var(const IoJob &J, const Var &v, const double *host, std::vector<uint64_t> &tmp) {
  const int nlev = v.src == PLANE2D ? 1 : v.nlev;
  int bad = 0;
  for (int k = 0; k < nlev && !bad; k++)
    for (int j = 0; j < J.jm && !bad; j++) {
      const uint64_t cell = ((uint64_t)k * J.jm_global + (uint64_t)(J.j0 - 1 + j)) * J.im_global + (uint64_t)(J.i0 - 1);
      bad |= write_be(J.fd, host + ((size_t)k * J.jml + j) * J.iml, (size_t)J.im, v.begin + cell * 8, tmp);
    }
  return bad;
}
#ifndef POMGPU_EMU
static void io_worker(IoJob *J) {
  (void)hipSetDevice(J->device);
  int bad = 0;
  size_t big = 0;
  for (const Var &v : J->S.vars) { const size_t n = var_doubles(*J, v); if (n > big) big = n; }
  double *pin = NULL;
  if (big && hipHostMalloc((void **)&pin, big * sizeof(double), hipHostMallocDefault) != hipSuccess) bad = 1;
  if (!bad && hipStreamWaitEvent(J->st, J->ev, 0) != hipSuccess) bad = 1;
  std::vector<uint64_t> tmp;
  size_t off = 0;
  for (const Var &v : J->S.vars) {
    const size_t n = var_doubles(*J, v);
    if (!n) continue;
    if (!bad && (hipMemcpyAsync(pin, J->snap + off, n * sizeof(double), hipMemcpyDeviceToHost, J->st) != hipSuccess ||
                 hipStreamSynchronize(J->st) != hipSuccess)) bad = 1;
    if (!bad) bad |= put_var(*J, v, pin, tmp);
    off += n;
  }
  if (pin) (void)hipHostFree(pin);
  if (close(J->fd)) bad = 1;
  J->fd = -1;
  J->rc = bad;
}
#endif
extern "C" int pomgpu_io_wait(pomgpu_ctx *c) {
  if (!c) return POMGPU_EINVAL;
  IoJob *J = (IoJob *)c->io_job;
  if (!J) return POMGPU_OK;
  int rc = POMGPU_OK;
#ifndef POMGPU_EMU
  if (J->active) {
    J->th.join();
    if (J->rc) rc = fail(c, POMGPU_EINVAL, "write: I/O error on %s", J->path.c_str());
  }
  (void)hipFree(J->snap);
  if (J->ev) (void)hipEventDestroy(J->ev);
  if (J->st) (void)hipStreamDestroy(J->st);
#endif
  delete J;
  c->io_job = NULL;
  return rc;
}

// the nine time-dependent fields of the output file, in the order of pomgpu_ctx::mean_off
#define MEAN_NF 9
static const int MEAN_3D[MEAN_NF] = {0, 0, 0, 1, 1, 1, 1, 1, 1};
static const int MEAN_SLOT[MEAN_NF] = {P2_uab, P2_vab, P2_elb, P3_u, P3_v, P3_t, P3_s, P3_rho, P3_w};
static int mean_field(const Var &v) {                                 // which of them a variable of the file is, -1 = none
  for (int q = 0; q < MEAN_NF; q++)
    if ((v.src == VOLUME3D) == (MEAN_3D[q] != 0) && (v.src == VOLUME3D || v.src == PLANE2D) && v.slot == MEAN_SLOT[q]) return q;
  return -1;
}
static void launch_mean_snapshot(pomgpu_ctx *c, double *const *dst, const size_t *nout);
static void launch_tracer_mean_snapshot(pomgpu_ctx *c, double *const *dst, const size_t *nout);
// mean == 1 (pomgpu_write_output_mean): the nine fields come from the accumulators -- k_mean_snapshot stores acc / count into the snapshot
// and +0.0 into acc in one pass, on the kernels' stream -- and the count returns to 0.  mean == 2 (pomgpu_write_tracers, the mean kind):
// the same for the variables that name a tracer (Var::tmean), from the tracers' accumulators and with the tracers' count
static int write_file(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m, Spec &S, int mean = 0) {
  const KP &P = c->P;
  auto mean_of = [&](const Var &v) { return mean == 2 ? v.tmean : (mean ? mean_field(v) : -1); };   // which accumulator supplies v, -1 = none
  if (!tile_fits(m, P, 0, 0, 0, 0))
    return fail(c, POMGPU_EINVAL, "write: the tile (%d..%d, %d..%d) does not fit the global grid %d x %d", m->i0, m->i0 + P.im - 1, m->j0,
                m->j0 + P.jm - 1, m->im_global, m->jm_global);
  { const int rcw = pomgpu_io_wait(c); if (rcw) return rcw; }  // one file in flight at a time
  // the snapshot below reads the mirrors directly: whatever the library keeps lazily is brought up to date first, whether or not
  // the caller supplied the statistics (pomgpu_domain_stats would have done it as a side effect)
  { const int rcm = pomgpu_materialize(c); if (rcm) return rcm; }
  const std::string h = header(S);
  const int fd = open(path, m->create ? (O_WRONLY | O_CREAT | O_TRUNC) : O_WRONLY, 0644);
  if (fd < 0) return fail(c, POMGPU_EINVAL, "write: cannot open %s", path);
  std::vector<uint64_t> tmp;
  std::vector<double> host;
  int bad = 0;
  if (m->create) {
    size_t left = h.size(); const char *p = h.data(); off_t off = 0;
    while (left && !bad) { const ssize_t w = pwrite(fd, p, left, off); if (w <= 0) bad = 1; else { p += w; off += w; left -= (size_t)w; } }
    const Var &last = S.vars.back();                                   // full length even where no tile has written yet
    if (!bad && ftruncate(fd, (off_t)(last.begin + var_bytes(S, last)))) bad = 1;
  }
  IoJob *J = new IoJob();
  J->path = path; J->fd = fd; J->im = P.im; J->jm = P.jm; J->iml = P.iml; J->jml = P.jml; J->kb = P.kb; J->n2 = P.n2;
  J->i0 = m->i0; J->j0 = m->j0; J->im_global = m->im_global; J->jm_global = m->jm_global; J->create = m->create; J->device = c->device;
  // scalars and the vertical grid: small, written here
  J->b1.resize((size_t)POM_NBLK1D * P.kb);
  if (hipMemcpyAsync(J->b1.data(), P.b1, sizeof(double) * J->b1.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) bad = 1;
  for (const Var &v : S.vars) {
    if (bad) break;
    if (v.src == SCALAR) { if (m->create) bad |= write_be(fd, &v.value, 1, v.begin, tmp); continue; }
    if (v.src == LEVELS1D && m->create) bad |= write_be(fd, J->b1.data() + (size_t)v.slot * P.kb, (size_t)v.nlev, v.begin, tmp);
    if (v.src == VALUES1D && m->create) bad |= write_be(fd, v.vals.data(), v.vals.size(), v.begin, tmp);
  }
  size_t total = 0;
  for (const Var &v : S.vars) total += var_doubles(*J, v);
  bool async = !bad && total > 0 && !SW(c, IO_SYNC);
#ifdef POMGPU_EMU
  async = false;
#else
  if (async && hipMalloc((void **)&J->snap, total * sizeof(double)) != hipSuccess) { J->snap = NULL; (void)hipGetLastError(); async = false; }
#endif
  auto dev_of = [&](const Var &v) { return v.dev ? v.dev : (v.src == PLANE2D ? P.b2 + (size_t)v.slot * P.n2 : P.b3 + (size_t)v.slot * P.a3); };
  // the means: where each of the nine lands in `base` (the snapshot, or on the synchronous path a buffer for the nine alone), one launch
  double *mdst[MEAN_NF] = {NULL};
  size_t mout[MEAN_NF] = {0};
  auto take_means = [&](double *base, bool nine_only) {
    size_t o = 0;
    for (const Var &v : S.vars) {
      const size_t n = var_doubles(*J, v);
      const int q = mean_of(v);
      if (q >= 0 && n) { mdst[q] = base + o; mout[q] = n; }
      if (q >= 0 || !nine_only) o += n;
    }
    if (mean == 2) { launch_tracer_mean_snapshot(c, mdst, mout); c->trmean_count = 0; }
    else { launch_mean_snapshot(c, mdst, mout); c->mean_count = 0; }
  };
  if (!async) {                                                        // the synchronous path: variable by variable through pageable memory
    double *nine = NULL;
    if (mean && !bad) {
      size_t tot9 = 0;
      for (const Var &v : S.vars) if (mean_of(v) >= 0) tot9 += var_doubles(*J, v);
      if (hipMalloc((void **)&nine, (tot9 ? tot9 : 1) * sizeof(double)) != hipSuccess) { nine = NULL; (void)hipGetLastError(); bad = 1; }
      else take_means(nine, true);
    }
    for (const Var &v : S.vars) {
      const size_t n = var_doubles(*J, v);
      if (bad || !n) continue;
      host.resize(n);
      const int q = mean_of(v);
      if (hipMemcpyAsync(host.data(), q >= 0 ? mdst[q] : dev_of(v), sizeof(double) * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
          hipStreamSynchronize(c->stream) != hipSuccess) { bad = 1; break; }
      bad |= put_var(*J, v, host.data(), tmp);
    }
    if (nine) { (void)hipStreamSynchronize(c->stream); (void)hipFree(nine); }
    if (close(fd)) bad = 1;
    J->fd = -1;
    c->io_job = J;
    (void)pomgpu_io_wait(c);
    return bad ? fail(c, POMGPU_EINVAL, "write: I/O error on %s", path) : POMGPU_OK;
  }
#ifndef POMGPU_EMU
  size_t off = 0;
  for (const Var &v : S.vars) {                                        // the snapshot, on the kernels' stream
    const size_t n = var_doubles(*J, v);
    if (!n) continue;
    if (mean_of(v) < 0 &&
        hipMemcpyAsync(J->snap + off, dev_of(v), n * sizeof(double), hipMemcpyDeviceToDevice, c->stream) != hipSuccess) bad = 1;
    off += n;
  }
  if (mean) take_means(J->snap, false);
  if (hipEventCreateWithFlags(&J->ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(J->ev, c->stream) != hipSuccess ||
      hipStreamCreateWithFlags(&J->st, hipStreamNonBlocking) != hipSuccess) bad = 1;
  J->S = S;
  c->io_job = J;
  if (bad) { (void)close(fd); J->fd = -1; (void)pomgpu_io_wait(c); return fail(c, POMGPU_EHIP, "write: cannot start the copy of %s", path); }
  J->active = 1;
  J->th = std::thread(io_worker, J);
#endif
  return POMGPU_OK;
}

static void stats_for_file(pomgpu_ctx *c, const pomgpu_file_meta *m, double *s8) {
  if (m->stats) { memcpy(s8, m->stats, 8 * sizeof(double)); return; }   // the caller's rank-reduced values
  (void)pomgpu_domain_stats(c, s8, 0);
}

// the output file's layout (io_pnetcdf.F:57-410) with `time` and the statistics as of now: the snapshot file's and the mean file's alike
static void output_spec(pomgpu_ctx *c, const pomgpu_file_meta *m, Spec &S) {
  const KP &P = c->P;
  double s8[8];
  stats_for_file(c, m, s8);                                   // also brings every lazily kept array up to date (NEED)
  S.dims = {{"time", 1}, {"z", P.kb}, {"zz", P.kbm1}, {"y", m->jm_global}, {"x", m->im_global}};
  S.gatts = {{"title", m->title ? m->title : ""}, {"description", "output file"}};
  const std::string since = std::string("days since ") + (m->time_start ? m->time_start : "");
  const int T = 0, Z = 1, ZZ = 2, Y = 3, X = 4;
  S.vars.push_back(mk("time", {T}, "time", since.c_str(), NULL, SCALAR, 0, 0, c->con.time));
  S.vars.push_back(mk("vtot", {T}, "domain total volume", "metre^3", NULL, SCALAR, 0, 0, s8[0]));
  S.vars.back().atts.push_back({"standard_name", "basin total volume"});
  S.vars.back().atts.push_back({"formula_terms", "time: time"});
  S.vars.push_back(mk("mtot", {T}, "domain total mass", "kg^3", NULL, SCALAR, 0, 0, s8[2]));
  S.vars.push_back(mk("tavg", {T}, "domain average temperature", "degrees Celsius", NULL, SCALAR, 0, 0, s8[4]));
  S.vars.push_back(mk("savg", {T}, "domain average salinity", "psu", NULL, SCALAR, 0, 0, s8[5]));
  S.vars.push_back(mk("eavg", {T}, "domain potential energy (anomaly)", "metre", NULL, SCALAR, 0, 0, s8[6]));
  S.vars.push_back(mk("ekin", {T}, "domain kinetic energy", "J", NULL, SCALAR, 0, 0, s8[7]));
  S.vars.push_back(mk("z", {Z}, "sigma of cell face", "sigma_level", NULL, LEVELS1D, P1_z, P.kb));
  S.vars.back().atts.push_back({"standard_name", "ocean_sigma_coordinate"});
  S.vars.back().atts.push_back({"formula_terms", "sigma: z eta: elb depth: h"});
  S.vars.push_back(mk("zz", {ZZ}, "sigma of cell centre", "sigma_level", NULL, LEVELS1D, P1_zz, P.kbm1));
  S.vars.back().atts.push_back({"standard_name", "ocean_sigma_coordinate"});
  S.vars.back().atts.push_back({"formula_terms", "sigma: zz eta: elb depth: h"});
  struct { const char *n, *ln, *u, *co; int slot; } p2[] = {
      {"dx", "grid increment in x", "metre", "east_e north_e", P2_dx}, {"dy", "grid increment in y", "metre", "east_e north_e", P2_dy},
      {"east_u", "easting of u-points", "metre", "east_u north_u", P2_east_u}, {"east_v", "easting of v-points", "metre", "east_v north_v", P2_east_v},
      {"east_e", "easting of elevation points", "metre", "east_e north_e", P2_east_e}, {"east_c", "easting of cell corners", "metre", "east_c north_c", P2_east_c},
      {"north_u", "northing of u-points", "metre", "east_u north_u", P2_north_u}, {"north_v", "northing of v-points", "metre", "east_v north_v", P2_north_v},
      {"north_e", "northing of elevation points", "metre", "east_e north_e", P2_north_e}, {"north_c", "northing of cell corners", "metre", "east_c north_c", P2_north_c},
      {"rot", "Rotation angle of x-axis wrt. east", "degree", "east_e north_e", P2_rot}, {"h", "undisturbed water depth", "metre", "east_e north_e", P2_h},
      {"fsm", "free surface mask", "dimensionless", "east_e north_e", P2_fsm}, {"dum", "u-velocity mask", "dimensionless", "east_u north_u", P2_dum},
      {"dvm", "v-velocity mask", "dimensionless", "east_v north_v", P2_dvm}};
  for (auto &q : p2) S.vars.push_back(mk(q.n, {Y, X}, q.ln, q.u, q.co, PLANE2D, q.slot, 1));
  S.vars.push_back(mk("uab", {T, Y, X}, "depth-averaged u", "metre/sec", "east_u north_u", PLANE2D, P2_uab, 1));
  S.vars.push_back(mk("vab", {T, Y, X}, "depth-averaged v", "metre/sec", "east_v north_v", PLANE2D, P2_vab, 1));
  S.vars.push_back(mk("elb", {T, Y, X}, "surface elevation", "metre", "east_e north_e", PLANE2D, P2_elb, 1));
  S.vars.push_back(mk("u", {T, ZZ, Y, X}, "x-velocity", "metre/sec", "east_u north_u zz", VOLUME3D, P3_u, P.kbm1));
  S.vars.push_back(mk("v", {T, ZZ, Y, X}, "y-velocity", "metre/sec", "east_v north_v zz", VOLUME3D, P3_v, P.kbm1));
  S.vars.push_back(mk("t", {T, ZZ, Y, X}, "potential temperature", "K", "east_e north_e zz", VOLUME3D, P3_t, P.kbm1));
  S.vars.push_back(mk("s", {T, ZZ, Y, X}, "salinity x rho / rhoref", "PSS", "east_e north_e zz", VOLUME3D, P3_s, P.kbm1));
  S.vars.push_back(mk("rho", {T, ZZ, Y, X}, "(density-1000)/rhoref", "dimensionless", "east_e north_e zz", VOLUME3D, P3_rho, P.kbm1));
  S.vars.push_back(mk("w", {T, Z, Y, X}, "z-velocity", "metre/sec", "east_e north_e z", VOLUME3D, P3_w, P.kb));
}
extern "C" int pomgpu_write_output(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m) {   // io_pnetcdf.F:57-410
#ifdef POMGPU_STORE_F32
  if (c) return pomgpu_fail(c, POMGPU_EINVAL, "write_output: not in the fp32-storage variant (download and write from the host)");
#endif
  if (!c || !path || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  Spec S;
  output_spec(c, m, S);
  return write_file(c, path, m, S);
}

extern "C" int pomgpu_write_restart(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m) {   // io_pnetcdf.F:1661-2083
#ifdef POMGPU_STORE_F32
  if (c) return pomgpu_fail(c, POMGPU_EINVAL, "write_restart: not in the fp32-storage variant (download and write from the host)");
#endif
  if (!c || !path || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  const KP &P = c->P;
  double s8[8];
  stats_for_file(c, m, s8);                                   // (values unused: the call brings the state up to date)
  Spec S;
  S.dims = {{"time", 1}, {"z", P.kb}, {"y", m->jm_global}, {"x", m->im_global}};
  S.gatts = {{"title", m->title ? m->title : ""}, {"description", "restart file"}};
  const std::string since = std::string("days since ") + (m->time_start ? m->time_start : "");
  const int T = 0, Z = 1, Y = 2, X = 3;
  S.vars.push_back(mk("iint", {}, "i_internal", "model internal step number", NULL, SCALAR, 0, 0, (double)c->con.iint));
  S.vars.push_back(mk("time", {T}, "time", since.c_str(), NULL, SCALAR, 0, 0, c->con.time));
  struct { const char *n, *ln, *u, *co; int slot; } p2[] = {
      {"wubot", "x-momentum flux at the bottom", "metre^2/sec^2", "east_u north_u", P2_wubot},
      {"wvbot", "y-momentum flux at the bottom", "metre^2/sec^2", "east_v north_v", P2_wvbot},
      {"aam2d", "vertical average of aam", "metre^2/sec", "east_e north_e", P2_aam2d},
      {"ua", "vertical mean of u", "metre/sec", "east_u north_u", P2_ua}, {"uab", "vertical mean of u at time -dt", "metre/sec", "east_u north_u", P2_uab},
      {"va", "vertical mean of v", "metre/sec", "east_v north_v", P2_va}, {"vab", "vertical mean of v at time -dt", "metre/sec", "east_v north_v", P2_vab},
      {"el", "surface elevation in external mode", "metre", "east_e north_e", P2_el},
      {"elb", "surface elevation in external mode at -dt", "metre", "east_e north_e", P2_elb},
      {"et", "surface elevation in internal mode", "metre", "east_e north_e", P2_et},
      {"etb", "surface elevation in internal mode at -dt", "metre", "east_e north_e", P2_etb},
      {"egb", "surface elevation for pres. grad. at -dt", "metre", "east_e north_e", P2_egb},
      {"utb", "ua time averaged over dti", "metre/sec", "east_u north_u", P2_utb}, {"vtb", "va time averaged over dti", "metre/sec", "east_v north_v", P2_vtb},
      {"adx2d", "vertical integral of advx", "-", "east_u north_u", P2_adx2d}, {"ady2d", "vertical integral of advy", "-", "east_v north_v", P2_ady2d},
      {"advua", "sum of 2nd, 3rd and 4th terms in eq (18)", "-", "east_u north_u", P2_advua},
      {"advva", "sum of 2nd, 3rd and 4th terms in eq (19)", "-", "east_v north_v", P2_advva}};
  for (auto &q : p2) S.vars.push_back(mk(q.n, {Y, X}, q.ln, q.u, q.co, PLANE2D, q.slot, 1));
  struct { const char *n, *ln, *u, *co; int slot; } p3[] = {
      {"u", "x-velocity", "metre/sec", "east_u north_u zz", P3_u}, {"ub", "x-velocity at time -dt", "metre/sec", "east_u north_u zz", P3_ub},
      {"v", "y-velocity", "metre/sec", "east_v north_v zz", P3_v}, {"vb", "y-velocity at time -dt", "metre/sec", "east_v north_v zz", P3_vb},
      {"w", "sigma-velocity", "metre/sec", "east_e north_e zz", P3_w}, {"t", "potential temperature", "K", "east_e north_e zz", P3_t},
      {"tb", "potential temperature at time -dt", "K", "east_e north_e zz", P3_tb}, {"s", "salinity x rho / rhoref", "PSS", "east_e north_e zz", P3_s},
      {"sb", "salinity x rho / rhoref at time -dt", "PSS", "east_e north_e zz", P3_sb},
      {"rho", "(density-1000)/rhoref", "dimensionless", "east_e north_e zz", P3_rho},
      {"km", "vertical kinematic viscosity", "metre^2/sec", "east_e north_e zz", P3_km}, {"kh", "vertical diffusivity", "metre^2/sec", "east_e north_e zz", P3_kh},
      {"kq", "kq", "metre^2/sec", "east_e north_e zz", P3_kq}, {"l", "turbulence length scale", "-", "east_e north_e zz", P3_l},
      {"q2", "twice the turbulent kinetic energy", "metre^2/sec^2", "east_e north_e zz", P3_q2},
      {"q2b", "twice the turbulent kinetic energy at -dt", "metre^2/sec^2", "east_e north_e zz", P3_q2b},
      {"aam", "horizontal kinematic viscosity", "metre^2/sec", "east_e north_e zz", P3_aam}, {"q2l", "q2 x l", "metre^3/sec^2", "east_e north_e zz", P3_q2l},
      {"q2lb", "q2 x l at time -dt", "metre^3/sec^2", "east_e north_e zz", P3_q2lb}};
  for (auto &q : p3) S.vars.push_back(mk(q.n, {Z, Y, X}, q.ln, q.u, q.co, VOLUME3D, q.slot, P.kb));
  return write_file(c, path, m, S);
}

// ---- the time-mean output (include/pomgpu.h: pomgpu_set_mean_output; no counterpart in the reference) -------------------------------
// One fp64 accumulator per time-dependent field of the output file.  k_mean_accum, once per internal step behind mode_internal: acc =
// acc + x, one add per cell in step order, for all nine fields in ONE launch -- blockIdx.y picks the field from a table passed by value.
// A pure stream: x read, acc read, acc written.  A workgroup moves 1024 consecutive doubles of its field, 16 bytes per lane and access
// where x and acc are 16-byte aligned alike (pomgpu_set_mean_output places every accumulator that way for the mirror as it lies then).
// Array n of blk3d starts n * a3 doubles into the block: with an odd a3 (65x49x21: 66885) every other one is 8-byte aligned only and the
// length is odd, so a field is [one head element] + pairs + [one tail element].  Head and tail are lanes 0 and 1 of the field's first
// workgroup with an 8-byte access of their own; everywhere a lane without work carries the offset BOFF_NONE, which the descriptor's range
// check drops (pomgpu_internal.hpp), so no load or store stands in a divergent branch: the only branches are uniform per workgroup.
// A field whose x and acc differ in alignment (uab, vab, elb while the external mode's result lives in the other generation of its
// arrays and n2 is odd) takes the 8-byte form throughout.
struct MeanJob { const double *x; double *acc; double *dst; unsigned n, nout; };
struct MeanTab { MeanJob j[MEAN_NF]; double cnt; };
struct Pair2 { double a, b; };
#ifndef POMGPU_EMU
typedef unsigned int pomgpu_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ Pair2 bld2x2(const BufA &b, unsigned voff) {
  const pomgpu_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(b.r, (int)voff, 0, 0);
  Pair2 r;
  r.a = __hiloint2double((int)v.y, (int)v.x); r.b = __hiloint2double((int)v.w, (int)v.z);
  return r;
}
__device__ __forceinline__ void bst2x2(const BufA &b, unsigned voff, Pair2 x) {
  pomgpu_u32x4 v;
  v.x = (unsigned)__double2loint(x.a); v.y = (unsigned)__double2hiint(x.a); v.z = (unsigned)__double2loint(x.b); v.w = (unsigned)__double2hiint(x.b);
  __builtin_amdgcn_raw_buffer_store_b128(v, b.r, (int)voff, 0, 0);
}
#else
static inline Pair2 bld2x2(const BufA &b, unsigned voff) { Pair2 r = {0., 0.}; if (voff < BOFF_NONE) { r.a = b.p[voff >> 3]; r.b = b.p[(voff >> 3) + 1]; } return r; }
static inline void bst2x2(const BufA &b, unsigned voff, Pair2 x) { if (voff < BOFF_NONE) { b.p[voff >> 3] = x.a; b.p[(voff >> 3) + 1] = x.b; } }
#endif
#define MEAN_WG 1024u                                                  /* doubles of a field per workgroup of 256 lanes */
// workgroup and lane: the launch's own (the workgroup number is a scalar, so every branch on it is one the compiler knows to be uniform);
// the host emulation runs workgroups of width 1 and takes both from the global lane number
#ifndef POMGPU_EMU
#define MEAN_WG_ID blockIdx.x
#define MEAN_LANE_ID threadIdx.x
#else
#define MEAN_WG_ID ((blockIdx.x * blockDim.x + threadIdx.x) >> 8)
#define MEAN_LANE_ID ((blockIdx.x * blockDim.x + threadIdx.x) & 255u)
#endif
__global__ void __launch_bounds__(256) k_mean_accum(MeanTab T) {
  const MeanJob J = T.j[blockIdx.y];
  const unsigned wg = MEAN_WG_ID, lane = MEAN_LANE_ID, n = J.n;
  if ((size_t)wg * MEAN_WG >= n) return;
  if (((((size_t)J.x ^ (size_t)J.acc) >> 3) & 1) == 0) {
    const unsigned head = (unsigned)(((size_t)J.x >> 3) & 1), np = (n - head) >> 1, tail = (n - head) & 1u;
    const BufA bx = buf2_of(J.x + head, 2 * (size_t)np), ba = buf2_of(J.acc + head, 2 * (size_t)np);
    unsigned off[2];
    Pair2 x[2], a[2];
#pragma unroll
    for (int u = 0; u < 2; u++) { const unsigned p = wg * (MEAN_WG / 2) + (unsigned)u * 256u + lane; off[u] = p < np ? p * 16u : BOFF_NONE; }
#pragma unroll
    for (int u = 0; u < 2; u++) { x[u] = bld2x2(bx, off[u]); a[u] = bld2x2(ba, off[u]); }
#pragma unroll
    for (int u = 0; u < 2; u++) { a[u].a = a[u].a + x[u].a; a[u].b = a[u].b + x[u].b; bst2x2(ba, off[u], a[u]); }
    if (wg == 0) {                                                     // the element in front of the pairs and the one behind them
      const BufA b1 = buf2_of(J.x, n), b2 = buf2_of(J.acc, n);
      const unsigned o = (lane == 0 && head) ? 0u : ((lane == 1 && tail) ? (n - 1) * 8u : BOFF_NONE);
      bst2(b2, o, 0, bld2(b2, o, 0) + bld2(b1, o, 0));
    }
  } else {
    const BufA bx = buf2_of(J.x, n), ba = buf2_of(J.acc, n);
    unsigned off[4];
    double x[4], a[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { const unsigned e = wg * MEAN_WG + (unsigned)u * 256u + lane; off[u] = e < n ? e * 8u : BOFF_NONE; }
#pragma unroll
    for (int u = 0; u < 4; u++) { x[u] = bld2(bx, off[u], 0); a[u] = bld2(ba, off[u], 0); }
#pragma unroll
    for (int u = 0; u < 4; u++) bst2(ba, off[u], 0, a[u] + x[u]);
  }
}
// The mean file's snapshot: dst = acc / count -- one IEEE division per cell, no reciprocal -- over the `nout` doubles the file holds of a
// field (kbm1 levels of u v t s rho) and acc = +0.0 over all n of them, in one pass: a pomgpu_run issued right after the call accumulates
// into clean sums behind this kernel while the writer's thread is still copying the snapshot.  Once per output interval: 8 bytes per lane
__global__ void __launch_bounds__(256) k_mean_snapshot(MeanTab T) {
  const MeanJob J = T.j[blockIdx.y];
  const unsigned wg = MEAN_WG_ID, lane = MEAN_LANE_ID, n = J.n;
  if ((size_t)wg * MEAN_WG >= n) return;
  const BufA ba = buf2_of(J.acc, n), bd = buf2_of(J.dst, J.nout);
  unsigned off[4];
  double a[4];
#pragma unroll
  for (int u = 0; u < 4; u++) { const unsigned e = wg * MEAN_WG + (unsigned)u * 256u + lane; off[u] = e < n ? e * 8u : BOFF_NONE; }
#pragma unroll
  for (int u = 0; u < 4; u++) a[u] = bld2(ba, off[u], 0);
#pragma unroll
  for (int u = 0; u < 4; u++) {
    bst2(bd, off[u] < J.nout * 8u ? off[u] : BOFF_NONE, 0, a[u] / T.cnt);
    bst2(ba, off[u], 0, 0.);
  }
}
static size_t mean_len(const pomgpu_ctx *c, int q) { return MEAN_3D[q] ? c->P.n3 : c->P.n2; }
static dim3 mean_grid(const pomgpu_ctx *c) { return dim3((unsigned)((c->P.n3 + MEAN_WG - 1) / MEAN_WG), MEAN_NF, 1); }
void launch_mean_accum(pomgpu_ctx *c, const double *const *x) {
  MeanTab T;
  for (int q = 0; q < MEAN_NF; q++) { T.j[q].x = x[q]; T.j[q].acc = c->mean_acc + c->mean_off[q]; T.j[q].dst = NULL; T.j[q].n = (unsigned)mean_len(c, q); T.j[q].nout = 0; }
  T.cnt = 0.;
  LAUNCH(c, k_mean_accum, mean_grid(c), dim3(256), T);
}
static void launch_mean_snapshot(pomgpu_ctx *c, double *const *dst, const size_t *nout) {
  MeanTab T;
  for (int q = 0; q < MEAN_NF; q++) {
    T.j[q].x = NULL; T.j[q].acc = c->mean_acc + c->mean_off[q]; T.j[q].dst = dst[q] ? dst[q] : T.j[q].acc; T.j[q].n = (unsigned)mean_len(c, q);
    T.j[q].nout = dst[q] ? (unsigned)nout[q] : 0;
  }
  T.cnt = (double)c->mean_count;
  LAUNCH(c, k_mean_snapshot, mean_grid(c), dim3(256), T);
}
static int mean_which(int is3d, int slot) {
  for (int q = 0; q < MEAN_NF; q++)
    if ((is3d != 0) == (MEAN_3D[q] != 0) && slot == MEAN_SLOT[q]) return q;
  return -1;
}
extern "C" int pomgpu_mean_download(pomgpu_ctx *c, int is3d, int slot, double *host) {
  if (!c || !host) return POMGPU_EINVAL;
  if (!c->mean_acc) return pomgpu_fail(c, POMGPU_EINVAL, "mean_download: the time-mean output is off (pomgpu_set_mean_output)");
  const int q = mean_which(is3d, slot);
  if (q < 0) return pomgpu_fail(c, POMGPU_EINVAL, "mean_download: %s slot %d is not accumulated (uab vab elb; u v t s rho w)", is3d ? "blk3d" : "blk2d", slot);
  if (c->mean_count < 1) return pomgpu_fail(c, POMGPU_EINVAL, "mean_download: no step has been accumulated since the switch or the last mean file");
  (void)hipSetDevice(c->device);
  const size_t n = mean_len(c, q);
  if (hipMemcpyAsync(host, c->mean_acc + c->mean_off[q], n * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) return pomgpu_fail(c, POMGPU_EHIP, "mean_download: the copy failed");
  const double cnt = (double)c->mean_count;
  for (size_t e = 0; e < n; e++) host[e] = host[e] / cnt;            // the division k_mean_snapshot makes
  return POMGPU_OK;
}
extern "C" int pomgpu_write_output_mean(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m) {
#ifdef POMGPU_STORE_F32
  if (c) return pomgpu_fail(c, POMGPU_EINVAL, "write_output_mean: not in the fp32-storage variant (download and write from the host)");
#endif
  if (!c || !path || !m) return POMGPU_EINVAL;
  if (!c->mean_acc) return pomgpu_fail(c, POMGPU_EINVAL, "write_output_mean: the time-mean output is off (pomgpu_set_mean_output)");
  if (c->mean_count < 1) return pomgpu_fail(c, POMGPU_EINVAL, "write_output_mean: no step has been accumulated since the switch or the last mean file -- %s is not written", path);
  (void)hipSetDevice(c->device);
  Spec S;
  output_spec(c, m, S);
  return write_file(c, path, m, S, 1);
}

// ---- the tracers' files (include/pomgpu.h: pomgpu_write_tracers; no counterpart in the reference) -----------------------------------
// The tracers' time mean is the nine fields' machinery with a table of its own: k_mean_accum once more per step, blockIdx.y the tracer
// (ONE added launch per step while the mean is on and tracers are registered, whatever their number), and k_mean_snapshot for the mean
// file.  A tracer's arrays and its accumulator are allocations of their own and 16-byte aligned alike (pomgpu_ctx::trmean_stride is
// even), so the accumulation takes the 16-byte form; an odd n3 leaves the one tail element.
static_assert(POMGPU_TRMAX <= MEAN_NF, "the tracers' table is a MeanTab");
static dim3 tracer_mean_grid(const pomgpu_ctx *c) { return dim3((unsigned)((c->P.n3 + MEAN_WG - 1) / MEAN_WG), (unsigned)c->ntr, 1); }
static void tracer_mean_tab(const pomgpu_ctx *c, MeanTab &T) {
  for (int q = 0; q < MEAN_NF; q++) {
    const bool on = q < c->ntr;
    T.j[q].x = on ? c->trc[q].tr : NULL; T.j[q].acc = on ? c->trmean_acc + (size_t)q * c->trmean_stride : NULL; T.j[q].dst = T.j[q].acc;
    T.j[q].n = on ? (unsigned)c->P.n3 : 0u; T.j[q].nout = 0;
  }
  T.cnt = 0.;
}
void launch_tracer_mean_accum(pomgpu_ctx *c) {
  MeanTab T;
  tracer_mean_tab(c, T);
  LAUNCH(c, k_mean_accum, tracer_mean_grid(c), dim3(256), T);
}
static void launch_tracer_mean_snapshot(pomgpu_ctx *c, double *const *dst, const size_t *nout) {
  MeanTab T;
  tracer_mean_tab(c, T);
  for (int q = 0; q < c->ntr; q++) if (dst[q]) { T.j[q].dst = dst[q]; T.j[q].nout = (unsigned)nout[q]; }
  T.cnt = (double)c->trmean_count;
  LAUNCH(c, k_mean_snapshot, tracer_mean_grid(c), dim3(256), T);
}
extern "C" int pomgpu_write_tracers(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m, int kind, const double *trstats) {
#ifdef POMGPU_STORE_F32
  if (c) return pomgpu_fail(c, POMGPU_EINVAL, "write_tracers: not in the fp32-storage variant (3-D arrays are not doubles there)");
#endif
  if (!c || !path || !m) return POMGPU_EINVAL;
  if (!c->ntr) return fail(c, POMGPU_EINVAL, "write_tracers: no tracers are registered (pomgpu_set_tracers)");
  if (kind != POMGPU_TRFILE_RESTART && kind != POMGPU_TRFILE_OUTPUT && kind != POMGPU_TRFILE_OUTPUT_MEAN)
    return fail(c, POMGPU_EINVAL, "write_tracers: kind = %d; POMGPU_TRFILE_RESTART (0), _OUTPUT (1) or _OUTPUT_MEAN (2)", kind);
  const bool mean = kind == POMGPU_TRFILE_OUTPUT_MEAN;
  if (mean && !c->trmean_acc) return fail(c, POMGPU_EINVAL, "write_tracers: the time-mean output is off (pomgpu_set_mean_output)");
  if (mean && c->trmean_count < 1)
    return fail(c, POMGPU_EINVAL, "write_tracers: no step has been accumulated since the switch, pomgpu_set_tracers or the last mean file -- %s is not written", path);
  (void)hipSetDevice(c->device);
  const KP &P = c->P;
  const int ntr = c->ntr;
  const std::string since = std::string("days since ") + (m->time_start ? m->time_start : "");
  auto nn = [](const char *stem, int n) { char b[32]; snprintf(b, sizeof b, "%s%02d", stem, n); return std::string(b); };
  auto volume = [&](const std::string &name, std::vector<int> dims, const std::string &ln, const char *co, const double *dev, int nlev, int tmean) {
    Var v = mk(name.c_str(), dims, ln.c_str(), "tracer units", co, VOLUME3D, -1, nlev);
    v.dev = dev; v.tmean = tmean;
    return v;
  };
  Spec S;
  if (kind == POMGPU_TRFILE_RESTART) {
    S.dims = {{"time", 1}, {"z", P.kb}, {"y", m->jm_global}, {"x", m->im_global}};
    S.gatts = {{"title", m->title ? m->title : ""}, {"description", "tracer restart file"}};
    const int T = 0, Z = 1, Y = 2, X = 3;
    S.vars.push_back(mk("iint", {}, "i_internal", "model internal step number", NULL, SCALAR, 0, 0, (double)c->con.iint));
    S.vars.push_back(mk("time", {T}, "time", since.c_str(), NULL, SCALAR, 0, 0, c->con.time));
    S.vars.push_back(mk("ntr", {}, "number of passive tracers", "dimensionless", NULL, SCALAR, 0, 0, (double)ntr));
    for (int n = 1; n <= ntr; n++) {
      S.vars.push_back(mk(nn("nbc", n).c_str(), {}, ("surface condition of tracer " + nn("", n)).c_str(), "1: flux, 3: value", NULL, SCALAR, 0, 0, (double)c->trc[n - 1].nbc));
      S.vars.push_back(mk(nn("lam", n).c_str(), {}, ("decay rate of tracer " + nn("", n)).c_str(), "1/sec", NULL, SCALAR, 0, 0, c->trc[n - 1].lam));
    }
    for (int n = 1; n <= ntr; n++) {
      const pomgpu_ctx::pomgpu_tracer &t = c->trc[n - 1];
      S.vars.push_back(volume(nn("tr", n), {Z, Y, X}, "passive tracer " + nn("", n), "east_e north_e zz", t.tr, P.kb, -1));
      S.vars.push_back(volume(nn("trb", n), {Z, Y, X}, "passive tracer " + nn("", n) + " at time -dt", "east_e north_e zz", t.trb, P.kb, -1));
      S.vars.push_back(volume(nn("trf", n), {Z, Y, X}, "work array of passive tracer " + nn("", n), "east_e north_e zz", t.trf, P.kb, -1));
    }
    return write_file(c, path, m, S);
  }
  double st[4 * POMGPU_TRMAX];
  if (trstats) memcpy(st, trstats, 4 * (size_t)ntr * sizeof(double));   // the caller's rank-reduced values
  else { const int rcs = pomgpu_tracer_stats(c, st); if (rcs) return rcs; }
  S.dims = {{"time", 1}, {"z", P.kb}, {"zz", P.kbm1}, {"y", m->jm_global}, {"x", m->im_global}};
  S.gatts = {{"title", m->title ? m->title : ""}, {"description", "tracer output file"}};
  const int T = 0, Z = 1, ZZ = 2, Y = 3, X = 4;
  S.vars.push_back(mk("time", {T}, "time", since.c_str(), NULL, SCALAR, 0, 0, c->con.time));
  for (int n = 1; n <= ntr; n++) {
    static const char *const stem[4] = {"tot", "avg", "min", "max"};
    static const char *const what[4] = {"domain inventory", "domain average", "minimum", "maximum"};
    static const char *const unit[4] = {"tracer units metre^3", "tracer units", "tracer units", "tracer units"};
    for (int q = 0; q < 4; q++)
      S.vars.push_back(mk(nn(stem[q], n).c_str(), {T}, (std::string(what[q]) + " of tracer " + nn("", n)).c_str(), unit[q], NULL, SCALAR, 0, 0, st[4 * (n - 1) + q]));
  }
  S.vars.push_back(mk("z", {Z}, "sigma of cell face", "sigma_level", NULL, LEVELS1D, P1_z, P.kb));
  S.vars.back().atts.push_back({"standard_name", "ocean_sigma_coordinate"});
  S.vars.back().atts.push_back({"formula_terms", "sigma: z eta: elb depth: h"});
  S.vars.push_back(mk("zz", {ZZ}, "sigma of cell centre", "sigma_level", NULL, LEVELS1D, P1_zz, P.kbm1));
  S.vars.back().atts.push_back({"standard_name", "ocean_sigma_coordinate"});
  S.vars.back().atts.push_back({"formula_terms", "sigma: zz eta: elb depth: h"});
  for (int n = 1; n <= ntr; n++)
    S.vars.push_back(volume(nn("tr", n), {T, ZZ, Y, X}, "passive tracer " + nn("", n), "east_e north_e zz", c->trc[n - 1].tr, P.kbm1, n - 1));
  return write_file(c, path, m, S, mean ? 2 : 0);
}

// ---- the harmonics file (include/pomgpu.h: pomgpu_write_harmonics; no counterpart in the reference) -----------------------------------------
// omega(ncon), count, t_first, t_last and per field of elb uab vab <f>_mean(y,x), <f>_amp(ncon,y,x), <f>_pha(ncon,y,x): the planes
// pomgpu_harmonic_planes leaves on the device go through the patch writer like any array of a tile.  Writing resets nothing
extern "C" int pomgpu_write_harmonics(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m) {
#ifdef POMGPU_STORE_F32
  if (c) return pomgpu_fail(c, POMGPU_EINVAL, "write_harmonics: not in the fp32-storage variant (3-D arrays are not doubles there)");
#endif
  if (!c || !path || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  { const int rcw = pomgpu_io_wait(c); if (rcw) return rcw; }  // the planes are rewritten below: no file may still be reading them
  const double *planes = NULL;
  { const int rcp = pomgpu_harmonic_planes(c, &planes); if (rcp) return rcp; }
  const KP &P = c->P;
  const int nc = c->ntide;
  Spec S;
  S.dims = {{"ncon", nc}, {"y", m->jm_global}, {"x", m->im_global}};
  S.gatts = {{"title", m->title ? m->title : ""}, {"description", "harmonics file"}};
  const int N = 0, Y = 1, X = 2;
  Var om = mk("omega", {N}, "angular frequency of the constituent", "radian/sec", NULL, VALUES1D, 0, nc);
  om.vals.assign(c->tide_omega, c->tide_omega + nc);
  S.vars.push_back(om);
  S.vars.push_back(mk("count", {}, "samples in the sums", "dimensionless", NULL, SCALAR, 0, 0, (double)c->harm_count));
  S.vars.push_back(mk("t_first", {}, "time of the first sample", "sec", NULL, SCALAR, 0, 0, c->harm_t[0]));
  S.vars.push_back(mk("t_last", {}, "time of the last sample", "sec", NULL, SCALAR, 0, 0, c->harm_t[1]));
  static const struct { const char *n, *ln, *u, *co; } F[3] = {{"elb", "surface elevation", "metre", "east_e north_e"}, {"uab", "depth-averaged u", "metre/sec", "east_u north_u"},
                                                               {"vab", "depth-averaged v", "metre/sec", "east_v north_v"}};
  const size_t np = 1 + 2 * (size_t)nc;
  for (int f = 0; f < 3; f++) {
    const double *base = planes + (size_t)f * np * P.n2;
    const std::string n = F[f].n, ln = F[f].ln;
    Var a = mk((n + "_mean").c_str(), {Y, X}, ("mean of " + ln).c_str(), F[f].u, F[f].co, PLANE2D, -1, 1);
    a.dev = base;
    S.vars.push_back(a);
    Var b = mk((n + "_amp").c_str(), {N, Y, X}, ("amplitude of " + ln).c_str(), F[f].u, F[f].co, VOLUME3D, -1, nc);
    b.dev = base + P.n2;
    S.vars.push_back(b);
    Var g = mk((n + "_pha").c_str(), {N, Y, X}, ("phase g of " + ln + ", A cos(omega t - g)").c_str(), "degree", F[f].co, VOLUME3D, -1, nc);
    g.dev = base + (1 + (size_t)nc) * P.n2;
    S.vars.push_back(g);
  }
  return write_file(c, path, m, S);
}

// ---- the float file (include/pomgpu.h: pomgpu_write_floats; no counterpart in the reference) ------------------------------------------------
// Output and checkpoint of the Lagrangian floats in one: the state (x y sig status kind id) and what pomgpu_float_sample shows of it.  One
// dimension, eight NC_DOUBLE and three NC_INT variables; no tile writes a patch, the arrays are the whole file.  Written synchronously, behind
// whatever file is still in flight: 68 bytes a float, a million floats are 68 MB
extern "C" int pomgpu_write_floats(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m) {
#ifdef POMGPU_STORE_F32
  if (c) return pomgpu_fail(c, POMGPU_EINVAL, "write_floats: not in the fp32-storage variant (3-D arrays are not doubles there)");
#endif
  if (!c || !path || !m) return POMGPU_EINVAL;
  if (!c->nflt) return fail(c, POMGPU_EINVAL, "write_floats: no floats are registered (pomgpu_float_upload)");
  (void)hipSetDevice(c->device);
  { const int rcw = pomgpu_io_wait(c); if (rcw) return rcw; }
  const size_t N = (size_t)c->nflt;
  std::vector<double> dbl(8 * N);                              // x y sig, then lon lat depth t s
  std::vector<int> itg(3 * N);                                 // status kind id
  int rc = pomgpu_float_download(c, dbl.data(), dbl.data() + N, dbl.data() + 2 * N, itg.data(), itg.data() + N, itg.data() + 2 * N);
  if (!rc) rc = pomgpu_float_sample(c, dbl.data() + 3 * N);
  if (rc) return rc;
  static const struct { const char *name, *long_name, *units; } DV[8] = {
      {"x", "index coordinate along i (cell centre i at x = i)", "grid cells"}, {"y", "index coordinate along j (cell centre j at y = j)", "grid cells"},
      {"sig", "sigma", "sigma_level"}, {"lon", "longitude", "degree"}, {"lat", "latitude", "degree"}, {"depth", "height relative to the resting surface", "metre"},
      {"t", "potential temperature of the containing column", "K"}, {"s", "salinity of the containing column", "PSS"}};
  static const struct { const char *name, *long_name, *units; } IV[3] = {
      {"status", "0 active, 1 exited, 2 lost", "dimensionless"}, {"kind", "0 follows w, 1 keeps its sigma", "dimensionless"}, {"id", "the caller's number", "dimensionless"}};
  const std::string since = std::string("days since ") + (m->time_start ? m->time_start : "");
  uint64_t begin[13] = {0};
  std::string h;
  for (int pass = 0; pass < 2; pass++) {                         // pass 0 measures, pass 1 has the offsets (as header() above)
    h.assign("CDF\002", 4);
    put32(h, 0);
    put32(h, 0x0A); put32(h, 1); putname(h, "nfloat"); put32(h, (uint32_t)N);
    putatts(h, {{"title", m->title ? m->title : ""}, {"description", "float file"}});
    put32(h, 0x0B); put32(h, 13);
    auto var = [&](const char *name, bool vec, const char *ln, const std::string &un, uint32_t type, int q) {
      putname(h, name); put32(h, vec ? 1 : 0);
      if (vec) put32(h, 0);
      putatts(h, {{"long_name", ln}, {"units", un}});
      put32(h, type);
      const uint64_t nb = (vec ? N : 1) * (type == 6 ? 8 : 4);
      put32(h, (uint32_t)((nb + 3) & ~(uint64_t)3)); put64(h, begin[q]);
    };
    var("iint", false, "i_internal", "model internal step number", 6, 0);
    var("time", false, "time", since, 6, 1);
    for (int q = 0; q < 8; q++) var(DV[q].name, true, DV[q].long_name, DV[q].units, 6, 2 + q);
    for (int q = 0; q < 3; q++) var(IV[q].name, true, IV[q].long_name, IV[q].units, 4, 10 + q);
    uint64_t off = h.size();
    for (int q = 0; q < 13; q++) { begin[q] = off; off += q < 2 ? 8 : (q < 10 ? 8 * N : 4 * N); }
  }
  const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) return fail(c, POMGPU_EINVAL, "write_floats: cannot open %s", path);
  auto put_bytes = [&](const void *src, size_t bytes, uint64_t off) {
    const char *p = (const char *)src;
    while (bytes) { const ssize_t w = pwrite(fd, p, bytes, (off_t)off); if (w <= 0) return 1; p += w; off += (uint64_t)w; bytes -= (size_t)w; }
    return 0;
  };
  std::vector<uint64_t> tmp;
  int bad = put_bytes(h.data(), h.size(), 0);
  const double sc[2] = {(double)c->con.iint, c->con.time};
  for (int q = 0; q < 2 && !bad; q++) bad = write_be(fd, &sc[q], 1, begin[q], tmp);
  for (int q = 0; q < 8 && !bad; q++) bad = write_be(fd, dbl.data() + (size_t)q * N, N, begin[2 + q], tmp);
  for (size_t e = 0; e < itg.size(); e++) itg[e] = (int)__builtin_bswap32((uint32_t)itg[e]);
  for (int q = 0; q < 3 && !bad; q++) bad = put_bytes(itg.data() + (size_t)q * N, 4 * N, begin[10 + q]);
  if (close(fd)) bad = 1;
  return bad ? fail(c, POMGPU_EINVAL, "write_floats: I/O error on %s", path) : POMGPU_OK;
}

// A source list from before the readers moved out names this file for writer and readers alike.  Every list of the project names the
// four units and says so with POMGPU_FILE_UNITS (the device build needs no word: it has no such old list); a host build without it still
// gets the readers, through here.
#if defined(POMGPU_EMU) && !defined(POMGPU_FILE_UNITS)
#include "cdf_in.hip"
#include "frc_files.hip"
#include "ztosig.hip"
#endif
