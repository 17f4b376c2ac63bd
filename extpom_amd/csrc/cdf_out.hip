// cdf_out.hip -- the library's file I/O unit: the output and restart files of the reference WITHOUT PnetCDF, written and (the
// restart file) read back, and the forcing files read record by record.  Writing is host code plus device-to-host copies; reading has the
// kernels of this file: k_cdf_unpack (restart), k_frc_unpack, k_lat_unpack, k_rst_unpack (forcing).
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
// pomgpu_read_restart (the end of this file) is read_restart_pnetcdf (:2420-2768): a parser of the classic header that finds
// the variables by name, raw big-endian bytes through pinned buffers to the device, byte reversal and scatter in a kernel.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#ifndef POMGPU_EMU
#include <thread>
#endif

#include "pomgpu.h"
#include "pomgpu_internal.hpp"
#define fail pomgpu_fail

namespace {
struct Att { std::string name, text; };
enum Src { SCALAR, LEVELS1D, PLANE2D, VOLUME3D };
struct Var {
  std::string name;
  std::vector<int> dims;          // dimension ids, slowest first (file order)
  std::vector<Att> atts;
  Src src; int slot; int nlev;    // slot: blk1d / blk2d / blk3d member; nlev: levels written (3-D), values (1-D)
  double value;                   // SCALAR
  uint64_t begin;
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
  Var v; v.name = name; v.dims = dims; v.src = src; v.slot = slot; v.nlev = nlev; v.value = value; v.begin = 0;
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

static int write_file(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m, Spec &S) {
  const KP &P = c->P;
  if (m->i0 < 1 || m->j0 < 1 || m->i0 + P.im - 1 > m->im_global || m->j0 + P.jm - 1 > m->jm_global)
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
  }
  size_t total = 0;
  for (const Var &v : S.vars) total += var_doubles(*J, v);
  bool async = !bad && total > 0 && !SW(c, IO_SYNC);
#ifdef POMGPU_EMU
  async = false;
#else
  if (async && hipMalloc((void **)&J->snap, total * sizeof(double)) != hipSuccess) { J->snap = NULL; (void)hipGetLastError(); async = false; }
#endif
  auto dev_of = [&](const Var &v) { return v.src == PLANE2D ? P.b2 + (size_t)v.slot * P.n2 : P.b3 + (size_t)v.slot * P.a3; };
  if (!async) {                                                        // the synchronous path: variable by variable through pageable memory
    for (const Var &v : S.vars) {
      const size_t n = var_doubles(*J, v);
      if (bad || !n) continue;
      host.resize(n);
      if (hipMemcpyAsync(host.data(), dev_of(v), sizeof(double) * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
          hipStreamSynchronize(c->stream) != hipSuccess) { bad = 1; break; }
      bad |= put_var(*J, v, host.data(), tmp);
    }
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
    if (hipMemcpyAsync(J->snap + off, dev_of(v), n * sizeof(double), hipMemcpyDeviceToDevice, c->stream) != hipSuccess) bad = 1;
    off += n;
  }
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

extern "C" int pomgpu_write_output(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m) {   // io_pnetcdf.F:57-410
#ifdef POMGPU_STORE_F32
  if (c) return pomgpu_fail(c, POMGPU_EINVAL, "write_output: not in the fp32-storage variant (download and write from the host)");
#endif
  if (!c || !path || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  const KP &P = c->P;
  double s8[8];
  stats_for_file(c, m, s8);                                   // also brings every lazily kept array up to date (NEED)
  Spec S;
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

// ---- reading the restart file back (read_restart_pnetcdf, io_pnetcdf.F:2420-2768) -----------------------------------------------
// The header is parsed as it stands in the file (CDF-1 or CDF-2; dimension list, attributes skipped, every variable's type,
// dimension ids and `begin`), because a file written by PnetCDF itself aligns its data section differently from the writer
// above and may hold its variables in another order.  Everything is checked before the first mirror is written.
namespace {
struct RVar { std::string name; std::vector<uint32_t> dimids; uint32_t type = 0; uint64_t begin = 0; };
struct RHeader { std::vector<uint64_t> dimlen; std::vector<RVar> vars; uint32_t numrecs = 0; };   // numrecs: records written so far (the forcing files)
struct Cur {                                                    // big-endian cursor over the bytes read so far
  const unsigned char *p; size_t n, at = 0; bool shortfall = false;
  bool need(size_t k) { if (at + k > n) { shortfall = true; return false; } return true; }
  uint32_t u32() { if (!need(4)) return 0; uint32_t v = 0; for (int q = 0; q < 4; q++) v = (v << 8) | p[at + q]; at += 4; return v; }
  uint64_t u64() { if (!need(8)) return 0; uint64_t v = 0; for (int q = 0; q < 8; q++) v = (v << 8) | p[at + q]; at += 8; return v; }
  void skip(uint64_t k) { k = (k + 3) & ~(uint64_t)3; if (need(k)) at += k; }
  std::string name() { const uint32_t len = u32(); std::string s; if (need(((size_t)len + 3) & ~(size_t)3)) { s.assign((const char *)p + at, len); at += ((size_t)len + 3) & ~(size_t)3; } return s; }
};
const unsigned NC_TYPE_BYTES[7] = {0, 1, 1, 2, 4, 4, 8};      // byte, char, short, int, float, double
// 0 = parsed, 1 = more bytes needed, -1 = not a classic header (why: `what`)
int parse_atts(Cur &c, std::string &what) {
  const uint32_t tag = c.u32(), cnt = c.u32();
  if (c.shortfall) return 1;
  if (tag == 0 && cnt == 0) return 0;
  if (tag != 0x0C) { what = "attribute list expected"; return -1; }
  for (uint32_t a = 0; a < cnt; a++) {
    (void)c.name();
    const uint32_t type = c.u32(), nel = c.u32();
    if (c.shortfall) return 1;
    if (type < 1 || type > 6) { what = "unknown attribute type"; return -1; }
    c.skip((uint64_t)nel * NC_TYPE_BYTES[type]);
    if (c.shortfall) return 1;
  }
  return 0;
}
int parse_header(const unsigned char *buf, size_t n, RHeader &H, std::string &what) {
  Cur c{buf, n};
  if (n < 4) return 1;
  if (memcmp(buf, "CDF", 3) != 0 || (buf[3] != 1 && buf[3] != 2)) {
    what = buf[0] == 'C' && buf[1] == 'D' && buf[2] == 'F' ? "CDF version " + std::to_string((int)buf[3]) + " (only the classic formats CDF-1 and CDF-2 are read)"
           : (n >= 4 && memcmp(buf, "\x89HDF", 4) == 0 ? std::string("an HDF5 / NetCDF-4 file (only the classic formats CDF-1 and CDF-2 are read)") : std::string("no NetCDF magic"));
    return -1;
  }
  const bool wide = buf[3] == 2;
  c.at = 4;
  H.numrecs = c.u32();
  uint32_t tag = c.u32(), cnt = c.u32();
  if (c.shortfall) return 1;
  H.dimlen.clear(); H.vars.clear();
  if (!(tag == 0 && cnt == 0)) {
    if (tag != 0x0A) { what = "dimension list expected"; return -1; }
    for (uint32_t d = 0; d < cnt; d++) { (void)c.name(); H.dimlen.push_back(c.u32()); if (c.shortfall) return 1; }
  }
  int rc = parse_atts(c, what);
  if (rc) return rc;
  tag = c.u32(); cnt = c.u32();
  if (c.shortfall) return 1;
  if (tag == 0 && cnt == 0) return 0;
  if (tag != 0x0B) { what = "variable list expected"; return -1; }
  for (uint32_t v = 0; v < cnt; v++) {
    RVar r;
    r.name = c.name();
    const uint32_t nd = c.u32();
    if (c.shortfall) return 1;
    if (nd > 1024) { what = "variable with more than 1024 dimensions"; return -1; }
    for (uint32_t d = 0; d < nd; d++) r.dimids.push_back(c.u32());
    if (c.shortfall) return 1;
    rc = parse_atts(c, what);
    if (rc) return rc;
    r.type = c.u32();
    (void)c.u32();                                              // vsize: recomputed from the dimensions (it saturates at 4 GiB)
    r.begin = wide ? c.u64() : (uint64_t)c.u32();
    if (c.shortfall) return 1;
    for (uint32_t id : r.dimids) if (id >= H.dimlen.size()) { what = "variable " + r.name + " names a dimension the file does not define"; return -1; }
    H.vars.push_back(r);
  }
  return 0;
}
std::string lengths_of(const RHeader &H, const RVar &v) {
  std::string s = "(";
  for (size_t d = 0; d < v.dimids.size(); d++) { if (d) s += ", "; const uint64_t len = H.dimlen[v.dimids[d]]; s += len ? std::to_string(len) : std::string("unlimited"); }
  return s + ")";
}
struct RItem { const RVar *v; int slot; int nlev; };            // nlev = kb: blk3d slot; 1: blk2d slot
}  // namespace

// One lane, one value: threadIdx.x runs along i, so a wavefront loads a contiguous piece of a file row (raw big-endian bytes in
// `src`, `rows` rows per level, src_pitch values per row, the tile's first column at src_i0) and stores a contiguous piece of
// the mirror's row.  T = pomgpu_st for the arrays of blk3d (the rounding k_cvt_to_st applies on upload), double for blk2d.
template <class T>
__global__ void k_cdf_unpack(T *dst, const unsigned long long *src, int im, int jm, int iml, size_t n2, int rows, int src_pitch, int src_i0) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x), j = (int)(blockIdx.y * blockDim.y + threadIdx.y), k = (int)blockIdx.z;
  if (i >= im || j >= jm) return;
  const unsigned long long u = __builtin_bswap64(src[((size_t)k * rows + j) * (size_t)src_pitch + (size_t)(src_i0 + i)]);
  double x;
  __builtin_memcpy(&x, &u, 8);
  dst[(size_t)k * n2 + (size_t)j * iml + i] = (T)x;
}
// d = h + el, dt = h + et over the active cells (io_pnetcdf.F:2757-2762)
__global__ void k_restart_depths(KP P) {
  const int i = TID_I, j = TID_J;
  if (i > P.im || j > P.jm) return;
  F2(d, i, j) = F2(h, i, j) + F2(el, i, j);
  F2(dt, i, j) = F2(h, i, j) + F2(et, i, j);
}

static int pread_all(int fd, void *buf, size_t n, uint64_t off) {
  char *p = (char *)buf;
  while (n) { const ssize_t r = pread(fd, p, n, (off_t)off); if (r <= 0) return -1; p += r; off += (uint64_t)r; n -= (size_t)r; }
  return 0;
}

extern "C" int pomgpu_read_restart(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m, double *time0_out, double *iint_out) {
  if (!c || !path || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  { const int rcw = pomgpu_io_wait(c); if (rcw) return rcw; }  // the file may be the one this context is still writing
  const KP &P = c->P;
  if (m->i0 < 1 || m->j0 < 1 || m->i0 + P.im - 1 > m->im_global || m->j0 + P.jm - 1 > m->jm_global)
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
    std::vector<unsigned char> hb;
    std::string what;
    int rc = 1;
    for (size_t want = 1 << 16; rc == 1; want *= 4) {
      const size_t n = (size_t)(want < fsize ? want : fsize);
      hb.resize(n);
      if (n && pread_all(fd, hb.data(), n, 0)) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_restart: I/O error on %s (header)", path); }
      rc = parse_header(hb.data(), n, H, what);
      if (rc == 1 && n == fsize) { what = fsize ? "the file ends inside its header" : "the file is empty"; rc = -1; }
    }
    if (rc < 0) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_restart: %s is not a restart file this library reads: %s", path, what.c_str()); }
  }
  auto find = [&](const char *name) -> const RVar * { for (const RVar &v : H.vars) if (v.name == name) return &v; return NULL; };
  auto refuse = [&](const std::string &why) { (void)close(fd); return fail(c, POMGPU_EINVAL, "read_restart: %s: %s", path, why.c_str()); };
  // a variable of `want` = (d0, d1, ...) doubles, not a record variable, inside the file
  auto check = [&](const char *name, const std::vector<uint64_t> &want, bool one_value, const RVar **out) -> std::string {
    const RVar *v = find(name);
    if (!v) return std::string("variable ") + name + " is absent";
    if (v->type != 6) return std::string("variable ") + name + " has NetCDF type " + std::to_string(v->type) + ", not NC_DOUBLE (6)";
    uint64_t count = 1;
    bool same = v->dimids.size() == want.size();
    for (size_t d = 0; d < v->dimids.size(); d++) {
      const uint64_t len = H.dimlen[v->dimids[d]];
      if (len == 0) return std::string("variable ") + name + " is a record variable (unlimited dimension)";
      if (__builtin_mul_overflow(count, len, &count)) count = UINT64_MAX / 8;   // a hostile header: saturate, the checks below refuse it
      if (same && len != want[d]) same = false;
    }
    if (one_value ? count != 1 : !same) {
      std::string w = "(";
      for (size_t d = 0; d < want.size(); d++) w += (d ? ", " : "") + std::to_string(want[d]);
      return std::string("variable ") + name + " has the dimension lengths " + lengths_of(H, *v) + ", wanted " + (one_value ? std::string("one value") : w + ")");
    }
    if (v->begin > fsize || count * 8 > fsize - v->begin)
      return std::string("variable ") + name + " (" + std::to_string(count * 8) + " bytes at " + std::to_string(v->begin) + ") reaches beyond the file's " + std::to_string(fsize) + " bytes";
    *out = v;
    return std::string();
  };
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
  {
    std::string why = check("iint", {}, true, &v_iint);
    if (why.empty()) why = check("time", {}, true, &v_time);
    for (auto &q : r2) { if (!why.empty()) break; const RVar *v = NULL; why = check(q.n, {jmg, img}, false, &v); items.push_back({v, q.slot, 1}); }
    for (auto &q : r3) { if (!why.empty()) break; const RVar *v = NULL; why = check(q.n, {(uint64_t)P.kb, jmg, img}, false, &v); items.push_back({v, q.slot, P.kb}); }
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
  // runs: whole levels of the band of rows j0 .. j0+jm-1 at the file's full width, as many as a buffer holds
  const size_t band = (size_t)P.jm * (size_t)img;               // values of one level's band
  size_t cap = (SW(c, IO_CHUNK_KB) && SWV(c, IO_CHUNK_KB) > 0 ? (size_t)SWV(c, IO_CHUNK_KB) << 10 : (size_t)64 << 20) / 8;   // values per buffer
  if (cap < band) cap = band;
  if (cap > band * (size_t)P.kb) cap = band * (size_t)P.kb;
  const int lev_per_run = (int)(cap / band);
  const bool whole_rows = (uint64_t)P.jm == jmg;                // the bands of consecutive levels touch: one pread per run
  // the pinned buffers, the staging buffer, the stream and the events live for this call only: the reader is initialisation, called once
  // per run, and their creation is a few milliseconds of the time the call takes
  unsigned long long *pin[2] = {NULL, NULL}, *stage = NULL;
#ifdef POMGPU_EMU
  // host emulation: a plain loop, one buffer, the same kernel through the emulated launch
  if (!bad && hipMalloc((void **)&pin[0], cap * 8) != hipSuccess) bad = 1;
  stage = pin[0];
  hipStream_t rs = c->stream;
#else
  hipStream_t rs = NULL;
  hipEvent_t ev[2] = {NULL, NULL};                              // the copy out of pin[b] has completed
  if (!bad && (hipHostMalloc((void **)&pin[0], cap * 8, hipHostMallocDefault) != hipSuccess || hipHostMalloc((void **)&pin[1], cap * 8, hipHostMallocDefault) != hipSuccess ||
               hipMalloc((void **)&stage, cap * 8) != hipSuccess || hipStreamCreateWithFlags(&rs, hipStreamNonBlocking) != hipSuccess ||
               hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) != hipSuccess ||
               hipStreamSynchronize(c->stream) != hipSuccess))  // what pomgpu_materialize enqueued precedes the first store below
    bad = 2;
  int used[2] = {0, 0};
#endif
  const hipStream_t cur0 = c->cur;
  c->cur = rs;                                                   // LAUNCH goes to the copy stream: each kernel behind the copy that feeds it
  int b = 0;
  for (const RItem &it : items) {
    for (int k0 = 0; k0 < it.nlev && !bad; k0 += lev_per_run) {
      const int nl = it.nlev - k0 < lev_per_run ? it.nlev - k0 : lev_per_run;
#ifndef POMGPU_EMU
      if (used[b] && hipEventSynchronize(ev[b]) != hipSuccess) { bad = 2; break; }   // the buffer's last run has left it
#endif
      const uint64_t first = it.v->begin + (((uint64_t)k0 * jmg + (uint64_t)(m->j0 - 1)) * img) * 8;
      if (whole_rows) { if (pread_all(fd, pin[b], (size_t)nl * band * 8, first)) bad = 1; }
      else for (int k = 0; k < nl && !bad; k++) if (pread_all(fd, pin[b] + (size_t)k * band, band * 8, first + (uint64_t)k * jmg * img * 8)) bad = 1;
      if (bad) break;
#ifndef POMGPU_EMU
      if (hipMemcpyAsync(stage, pin[b], (size_t)nl * band * 8, hipMemcpyHostToDevice, rs) != hipSuccess || hipEventRecord(ev[b], rs) != hipSuccess) { bad = 2; break; }
      used[b] = 1;
#endif
      const dim3 grid((unsigned)((P.im + 63) / 64), (unsigned)((P.jm + 3) / 4), (unsigned)nl);
      if (it.nlev == 1)
        LAUNCHN(c, "k_cdf_unpack", k_cdf_unpack<double>, grid, blk2(), P.b2 + (size_t)it.slot * P.n2, (const unsigned long long *)stage, P.im, P.jm, P.iml, P.n2, P.jm, (int)img, m->i0 - 1);
      else
        LAUNCHN(c, "k_cdf_unpack", k_cdf_unpack<pomgpu_st>, grid, blk2(), (pomgpu_st *)(P.b3 + (size_t)it.slot * P.a3) + (size_t)k0 * P.n2, (const unsigned long long *)stage, P.im, P.jm,
                P.iml, P.n2, P.jm, (int)img, m->i0 - 1);
#ifndef POMGPU_EMU
      b ^= 1;
#endif
    }
    if (bad) break;
  }
  if (!bad) LAUNCH(c, k_restart_depths, grid2(P), blk2(), P);
  c->cur = cur0;
  if (hipStreamSynchronize(rs) != hipSuccess && !bad) bad = 2;
#ifndef POMGPU_EMU
  if (ev[0]) (void)hipEventDestroy(ev[0]);
  if (ev[1]) (void)hipEventDestroy(ev[1]);
  if (rs) (void)hipStreamDestroy(rs);
  if (pin[0]) (void)hipHostFree(pin[0]);
  if (pin[1]) (void)hipHostFree(pin[1]);
  if (stage) (void)hipFree(stage);
#else
  (void)hipFree(pin[0]);
#endif
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

// ---- forcing records from the files (pomgpu_set_forcing_files) ---------------------------------------------------------------------
// read_wind_pnetcdf, read_heat_pnetcdf, read_surface_pnetcdf (io_pnetcdf.F:2912-2998, :3110-3224), read_boundary_conditions_pnetcdf
// (:3393-3621) and read_restore_ts_interior_pnetcdf (:3275-3333) without PnetCDF.  The host names the files once; the schedule code of
// pomgpu_api.hip (frc_read, lat_read, restore_prepare) asks for record n when the step needs it, and the fetch below puts it where
// the setter of the same record would have put it: the tile's band of raw big-endian values with pread into a pinned buffer, one copy
// to the device on the stream the step is being enqueued on, and a kernel that swaps bytes, widens, converts units, tapers the wind
// and scatters.  Nothing here waits for the device but the reuse of a pinned buffer (an event per buffer).
namespace {
struct FVar {                                                   // one variable a reader asks for, as the header describes it
  const char *name;
  uint32_t type = 0;                                            // 5 = NC_FLOAT, 6 = NC_DOUBLE
  bool rec = false;                                             // its first dimension is the unlimited one
  uint64_t begin = 0, stride = 0, slab = 0;                     // record n at begin + (n-1) * stride; slab: bytes of one record of this variable
  uint64_t nfixed = 0;                                          // records along a fixed first dimension
  unsigned esize() const { return type == 5 ? 4u : 8u; }
};
struct FSource {
  int fd = -1;
  std::string path;
  uint64_t fsize = 0;
  uint32_t numrecs = 0;
  std::vector<FVar> v;
};
struct FFiles {
  FSource s[4];                                                 // sfrc, lbry, clim; [3]: the restore rate (pomgpu_set_restore_rate_file)
  int im_global = 0, jm_global = 0, i0 = 1, j0 = 1;
  unsigned char *pin[2] = {NULL, NULL}, *stage = NULL;          // two pinned buffers and the device buffer their copies land in
  size_t cap = 0;                                               // bytes of each
#ifndef POMGPU_EMU
  hipEvent_t ev[2] = {NULL, NULL};                              // the copy out of pin[b] has completed
  int used[2] = {0, 0};
#endif
  int b = 0;
  // a clim file on z levels (pomgpu_set_z_inputs): its level count, the window lines towards the west, east, south, north neighbour, and
  // one allocation: the window of one variable as doubles, ztosig's two work arrays, its table
  int zks = 0, wi = 0, we = 0, wj = 0, wn = 0;
  double *zdev = NULL;
  size_t zwin = 0, zwork = 0;
  // an lbry file on z levels (pomgpu_set_z_lateral): its level count, the window points of the east lines (lwj, lwn: towards the south, north
  // neighbour) and of the south lines (lwi, lwe), and one allocation: ztosig's table, then the two work arrays of the record's four lines
  int lks = 0, lwi = 0, lwe = 0, lwj = 0, lwn = 0;
  double *ldev = NULL;
  // the rate file: `tau` on the rks levels of its `z`, always through ztosig; window lines and one allocation as for the z-level clim file;
  // rsteady: it holds one record (or has no record dimension), which serves every record number
  int rks = 0, rwi = 0, rwe = 0, rwj = 0, rwn = 0, rsteady = 0;
  double *rdev = NULL;
  size_t rwin = 0, rwork = 0;
};
const char *const FF_WHAT[3] = {"sfrc", "lbry", "clim"};
const char *const FF_SFRC[6] = {"sustr", "svstr", "shflux", "swrad", "SST", "SSS"};
const char *const FF_LBRY[10] = {"zeta.east", "zeta.south", "u.east", "v.east", "temp.east", "salt.east", "u.south", "v.south", "temp.south", "salt.south"};
const char *const FF_CLIM[2] = {"Tclim", "Sclim"};
const char *const FF_RATE[1] = {"tau"};

template <class T> struct CdfRaw;
template <> struct CdfRaw<float> {
  static __device__ __forceinline__ double get(const void *p, size_t q) {
    const unsigned u = __builtin_bswap32(((const unsigned *)p)[q]);
    float x;
    __builtin_memcpy(&x, &u, 4);
    return (double)x;                                           // exact, what get_vara_double does with an NC_FLOAT variable
  }
};
template <> struct CdfRaw<double> {
  static __device__ __forceinline__ double get(const void *p, size_t q) {
    const unsigned long long u = __builtin_bswap64(((const unsigned long long *)p)[q]);
    double x;
    __builtin_memcpy(&x, &u, 8);
    return x;
  }
};
}  // namespace

// the reader's unit conversion, in its own order and with its own literals
__device__ __forceinline__ double frc_convert(int kind, double x, double rhoref) {
  if (kind == 0) return -x / 1025.;                             // io_pnetcdf.F:2963-2964
  if (kind == 1) return -x / rhoref / 3986.;                    // :3163-3164
  return x;
}
// The wind taper (:2966-2995) of the cell (i,j), whose converted value is x; m = dum for wu, dvm for wv.  The interior, the four edge
// lines and the four corners have a formula each; the corners see raw values because no statement before theirs writes them.  Row jm
// of the columns 2..imm1 is formed from ROW 1 as the statement before has left it (":2971 wu(2:imm1,jm) = wu(2:imm1,1)/3.d0*..."), so
// the caller hands that lane x1 = the converted value of (i,1) and the lane redoes row 1's statement itself.
__device__ __forceinline__ double frc_taper(const KP &P, const double *m, int i, int j, double x, double x1) {
  const int im = P.im, jm = P.jm;
  const bool iin = i >= 2 && i <= im - 1, jin = j >= 2 && j <= jm - 1;
  if (iin && jin) return .25 * x * (G2(m, i, j + 1) + G2(m, i, j - 1) + G2(m, i + 1, j) + G2(m, i - 1, j));
  if (iin && j == 1) return x / 3. * (G2(m, i, 2) + G2(m, i - 1, 1) + G2(m, i + 1, 1));
  if (iin) {                                                    // j == jm
    const double r1 = x1 / 3. * (G2(m, i, 2) + G2(m, i - 1, 1) + G2(m, i + 1, 1));
    return r1 / 3. * (G2(m, i, jm - 1) + G2(m, i - 1, jm) + G2(m, i + 1, jm));
  }
  if (jin && i == 1) return x / 3. * (G2(m, 2, j) + G2(m, 1, j - 1) + G2(m, 1, j + 1));
  if (jin) return x / 3. * (G2(m, im - 1, j) + G2(m, im, j - 1) + G2(m, im, j + 1));   // i == im
  if (i == 1 && j == 1) return .5 * x * (G2(m, 1, 2) + G2(m, 2, 1));
  if (j == 1) return .5 * x * (G2(m, im, 2) + G2(m, im - 1, 1));
  if (i == im) return .5 * x * (G2(m, im, jm - 1) + G2(m, im - 1, jm));
  return .5 * x * (G2(m, 1, jm - 1) + G2(m, 2, jm));
}
// One record of wind (kind 0), heat (1) or surface (2): the tile's band of rows of one or two variables (raw bytes at sa, sb -- sb NULL:
// the second field is not wanted -- `pitch` values per row, the tile's first column at i0) into the (im,jm) records da, db that
// pomgpu_set_forcing_record fills.  Thread mapping of k_cdf_unpack: threadIdx.x runs along i.
template <class TA, class TB>
__global__ void k_frc_unpack(KP P, int kind, double *da, double *db, const void *sa, const void *sb, int pitch, int i0) {
  const int i = TID_I, j = TID_J;
  if (i > P.im || j > P.jm) return;
  const size_t q = (size_t)(j - 1) * (size_t)pitch + (size_t)(i0 + i - 1), q1 = (size_t)(i0 + i - 1);
  const size_t r = (size_t)(j - 1) * P.im + (size_t)(i - 1);
  const bool top = kind == 0 && j == P.jm;                          // the only lanes that need their column's row-1 value
  double a = frc_convert(kind, CdfRaw<TA>::get(sa, q), P.rhoref);
  if (kind == 0) a = frc_taper(P, A2(dum), i, j, a, top ? frc_convert(0, CdfRaw<TA>::get(sa, q1), P.rhoref) : 0.);
  da[r] = a;
  if (!sb) return;
  double b = frc_convert(kind, CdfRaw<TB>::get(sb, q), P.rhoref);
  if (kind == 0) b = frc_taper(P, A2(dvm), i, j, b, top ? frc_convert(0, CdfRaw<TB>::get(sb, q1), P.rhoref) : 0.);
  db[r] = b;
}
// One record of read_boundary_conditions_pnetcdf (:3426-3614) into the 20 concatenated arrays pomgpu_set_lateral_record fills (the order
// of the reader's arguments; k_lateral's phase 0 consumes them).  One thread per edge point, as in k_lateral.  From the file, compact
// (the tile's jm or im values per level): src[0] zeta.east, [1] zeta.south, [2..5] u v temp salt .east, [6..9] u v temp salt .south;
// f32 bit q: that variable is NC_FLOAT.  t_w s_w / t_n s_n: line i = 1 / j = jm of tclim, sclim; u_w v_w u_n v_n: zero; everything
// beyond jm / im: zero, but in the elevations, which the reader leaves as they are there -- as it leaves elw, eln everywhere.
// zts (an lbry file on z levels): temp / salt .east / .south hold other levels and are left to k_ztosig_line, which fills those four arrays.
struct LatSrc { const void *p[10]; unsigned f32; int zts; };
__device__ __forceinline__ double lat_raw(const LatSrc &s, int q, size_t at) { return (s.f32 >> q) & 1u ? CdfRaw<float>::get(s.p[q], at) : CdfRaw<double>::get(s.p[q], at); }
__global__ void k_lat_unpack(KP P, double *rec, LatSrc s) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int kb = P.kb, jml = P.jml, iml = P.iml;
  if (t >= jml + iml) return;
  const size_t njk = (size_t)jml * kb, nik = (size_t)iml * kb;
  double *e = rec + 8 * njk + 8 * nik;                            // elw ele (jml each), eln els (iml each)
  if (t < jml) {
    const int a = t + 1;
    const bool in = a <= P.jm;
    for (int k = 1; k <= kb; k++) {
      const size_t o = (size_t)(k - 1) * jml + (a - 1), f = (size_t)(k - 1) * P.jm + (a - 1);
      rec[o] = in ? (double)F3(tclim, 1, a, k) : 0.;
      rec[njk + o] = in ? (double)F3(sclim, 1, a, k) : 0.;
      rec[2 * njk + o] = 0.;
      rec[3 * njk + o] = 0.;
      if (!s.zts) {
        rec[4 * njk + o] = in ? lat_raw(s, 4, f) : 0.;
        rec[5 * njk + o] = in ? lat_raw(s, 5, f) : 0.;
      }
      rec[6 * njk + o] = in ? lat_raw(s, 2, f) : 0.;
      rec[7 * njk + o] = in ? lat_raw(s, 3, f) : 0.;
    }
    e[a - 1] = BD1(elw, a);
    e[jml + a - 1] = in ? lat_raw(s, 0, (size_t)(a - 1)) : BD1(ele, a);
  } else {
    const int a = t - jml + 1;
    const bool in = a <= P.im;
    double *r = rec + 8 * njk;
    for (int k = 1; k <= kb; k++) {
      const size_t o = (size_t)(k - 1) * iml + (a - 1), f = (size_t)(k - 1) * P.im + (a - 1);
      r[o] = in ? (double)F3(tclim, a, P.jm, k) : 0.;
      r[nik + o] = in ? (double)F3(sclim, a, P.jm, k) : 0.;
      r[2 * nik + o] = 0.;
      r[3 * nik + o] = 0.;
      if (!s.zts) {
        r[4 * nik + o] = in ? lat_raw(s, 8, f) : 0.;
        r[5 * nik + o] = in ? lat_raw(s, 9, f) : 0.;
      }
      r[6 * nik + o] = in ? lat_raw(s, 7, f) : 0.;
      r[7 * nik + o] = in ? lat_raw(s, 6, f) : 0.;
    }
    e[2 * (size_t)jml + a - 1] = BD1(eln, a);
    e[2 * (size_t)jml + iml + a - 1] = in ? lat_raw(s, 1, (size_t)(a - 1)) : BD1(els, a);
  }
}
// Levels k0 .. k0+gridDim.z-1 of Tclim or Sclim (bands of `rows` rows, `pitch` values per row) into the (im,jm,kb) record
// pomgpu_set_restore_record fills; k_restore_load rounds it into the fp32-storage variants' mirrors as it does the setter's.
template <class T>
__global__ void k_rst_unpack(double *dst, const void *src, int im, int jm, int rows, int pitch, int i0, int k0) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x), j = (int)(blockIdx.y * blockDim.y + threadIdx.y), k = (int)blockIdx.z;
  if (i >= im || j >= jm) return;
  dst[((size_t)(k0 + k) * jm + j) * im + i] = CdfRaw<T>::get(src, ((size_t)k * rows + j) * (size_t)pitch + (size_t)(i0 + i));
}

static FFiles *FF(pomgpu_ctx *c) { return (FFiles *)c->frc_files; }
// ztosig for a clim file on z levels (defined with the kernel, further down)
static std::string z_levels(const RHeader &H, const FSource &S, const char *name, std::vector<double> &zs);
static void ztosig_table(const double *zs, int ks, double *tab);
static void launch_ztosig_window(pomgpu_ctx *c, double *out, int record, const double *zsrc, const double *tab, double *wa, double *wb, int ks, int wi, int we, int wj, int wn);
// ztosig for the lines of an lbry file on z levels (defined with the kernel, further down)
struct ZtlLine { double *out; const void *src; int fmt, edge, n, npad, lo, hi, sp, so, op; };
struct ZtlJob { ZtlLine l[4]; };
static ZtlLine ztosig_line_of(const KP &P, int edge, double *out, const void *src, int fmt, int sp, int so);
static void launch_ztosig_lines(pomgpu_ctx *c, const ZtlJob &job, int nlines, const double *tab, double *wa, double *wb, int ks, int pitch);
int pomgpu_ff_has(pomgpu_ctx *c, int src) { return c->frc_files && FF(c)->s[src].fd >= 0; }
void pomgpu_ff_free(pomgpu_ctx *c) {
  FFiles *F = FF(c);
  if (!F) return;
  for (FSource &s : F->s) if (s.fd >= 0) (void)close(s.fd);
#ifndef POMGPU_EMU
  for (int b = 0; b < 2; b++) { if (F->ev[b]) (void)hipEventDestroy(F->ev[b]); if (F->pin[b]) (void)hipHostFree(F->pin[b]); }
  if (F->stage) (void)hipFree(F->stage);
#else
  if (F->pin[0]) (void)hipFree(F->pin[0]);
#endif
  if (F->zdev) (void)hipFree(F->zdev);
  if (F->ldev) (void)hipFree(F->ldev);
  if (F->rdev) (void)hipFree(F->rdev);
  delete F;
  c->frc_files = NULL;
}
// the header of `fd`, whole: 0 = parsed, -1 = refused (why: `what`)
static int ff_header(int fd, uint64_t fsize, RHeader &H, std::string &what) {
  std::vector<unsigned char> hb;
  int rc = 1;
  for (size_t want = 1 << 16; rc == 1; want *= 4) {
    const size_t n = (size_t)(want < fsize ? want : fsize);
    hb.resize(n);
    if (n && pread_all(fd, hb.data(), n, 0)) { what = "I/O error (header)"; return -1; }
    rc = parse_header(hb.data(), n, H, what);
    if (rc == 1 && n == fsize) { what = fsize ? "the file ends inside its header" : "the file is empty"; rc = -1; }
  }
  return rc;
}
// One source's variables against what its reader asks for: `want[q]` = the dimension lengths after the record dimension; min_rec: records a
// fixed first dimension must at least have.  Empty string = accepted, S.v filled.
static std::string ff_check(const RHeader &H, FSource &S, const char *const *names, const std::vector<std::vector<uint64_t>> &want, uint64_t min_rec) {
  // bytes of one record of the file: the record variables' per-record sizes, each from its dimensions, padded to 4 bytes (a lone record
  // variable is not padded); vsize is not trusted (it saturates)
  uint64_t recsize = 0, lone = 0;
  int nrecvar = 0;
  for (const RVar &v : H.vars) {
    if (v.dimids.empty() || H.dimlen[v.dimids[0]] != 0) continue;
    if (v.type < 1 || v.type > 6) return "variable " + v.name + " has the unknown NetCDF type " + std::to_string(v.type);
    uint64_t n = NC_TYPE_BYTES[v.type];
    for (size_t d = 1; d < v.dimids.size(); d++) if (__builtin_mul_overflow(n, H.dimlen[v.dimids[d]], &n)) return "variable " + v.name + " is larger than 2^64 bytes";
    recsize += (n + 3) & ~(uint64_t)3;
    lone = n;
    nrecvar++;
  }
  if (nrecvar == 1) recsize = lone;
  S.v.clear();
  S.numrecs = H.numrecs;
  for (size_t q = 0; q < want.size(); q++) {
    const char *name = names[q];
    const RVar *v = NULL;
    for (const RVar &x : H.vars) if (x.name == name) { v = &x; break; }
    if (!v) return std::string("variable ") + name + " is absent";
    if (v->type != 5 && v->type != 6) return std::string("variable ") + name + " has NetCDF type " + std::to_string(v->type) + ", neither NC_FLOAT (5) nor NC_DOUBLE (6)";
    bool same = v->dimids.size() == want[q].size() + 1;
    for (size_t d = 1; same && d < v->dimids.size(); d++) if (H.dimlen[v->dimids[d]] != want[q][d - 1]) same = false;
    if (same && H.dimlen[v->dimids[0]] != 0 && H.dimlen[v->dimids[0]] < min_rec) same = false;
    if (!same) {
      std::string w = min_rec > 1 ? "(>= " + std::to_string(min_rec) : std::string("(records");
      for (uint64_t len : want[q]) w += ", " + std::to_string(len);
      return std::string("variable ") + name + " has the dimension lengths " + lengths_of(H, *v) + ", wanted " + w + ")";
    }
    FVar f;
    f.name = name; f.type = v->type; f.begin = v->begin;
    f.slab = f.esize();
    for (uint64_t len : want[q]) f.slab *= len;
    f.rec = H.dimlen[v->dimids[0]] == 0;
    f.stride = f.rec ? recsize : f.slab;
    f.nfixed = f.rec ? 0 : H.dimlen[v->dimids[0]];
    const uint64_t nrec = f.rec ? (uint64_t)H.numrecs : f.nfixed;
    if (f.rec && H.numrecs == 0xffffffffu) { S.v.push_back(f); continue; }   // "streaming": the length is known at the fetch alone
    if (f.begin > S.fsize || (nrec && ((nrec - 1) > (S.fsize - f.begin) / (f.stride ? f.stride : 1) || (nrec - 1) * f.stride + f.slab > S.fsize - f.begin)))
      return std::string("variable ") + name + " (" + std::to_string(nrec) + " records of " + std::to_string(f.slab) + " bytes from " + std::to_string(f.begin) +
             ") reaches beyond the file's " + std::to_string(S.fsize) + " bytes: a truncated file";
    S.v.push_back(f);
  }
  if (min_rec > 1 && S.v[0].rec && H.numrecs < min_rec) return std::string("variable ") + names[0] + " has " + std::to_string(H.numrecs) + " records, wanted >= " + std::to_string(min_rec);
  return std::string();
}

// the two pinned buffers and the device buffer behind them, grown to `need` bytes each (never inside a step); 1 = a HIP call failed
static int ff_reserve(pomgpu_ctx *c, FFiles *F, size_t need) {
  int bad = 0;
  if (F->cap < need) {
    if (hipStreamSynchronize(c->stream) != hipSuccess) bad = 1;   // (a second registration: earlier fetches may still be copying)
#ifndef POMGPU_EMU
    for (int b = 0; b < 2; b++) { if (F->pin[b]) (void)hipHostFree(F->pin[b]); F->pin[b] = NULL; F->used[b] = 0; }
    if (F->stage) (void)hipFree(F->stage);
    F->stage = NULL;
    if (hipHostMalloc((void **)&F->pin[0], need, hipHostMallocDefault) != hipSuccess || hipHostMalloc((void **)&F->pin[1], need, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&F->stage, need) != hipSuccess) bad = 1;
    for (int b = 0; b < 2 && !bad; b++) if (!F->ev[b] && hipEventCreateWithFlags(&F->ev[b], hipEventDisableTiming) != hipSuccess) bad = 1;
#else
    if (F->pin[0]) (void)hipFree(F->pin[0]);
    if (hipMalloc((void **)&F->pin[0], need) != hipSuccess) bad = 1;
    F->stage = F->pin[0];                                         // host emulation: one buffer, no copy
#endif
    F->cap = bad ? 0 : need;
  }
  return bad;
}

extern "C" int pomgpu_set_forcing_files(pomgpu_ctx *c, const char *sfrc, const char *lbry, const char *clim, const pomgpu_file_meta *m) {
  if (!c || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  const KP &P = c->P;
  if (m->i0 < 1 || m->j0 < 1 || m->i0 + P.im - 1 > m->im_global || m->j0 + P.jm - 1 > m->jm_global)
    return fail(c, POMGPU_EINVAL, "set_forcing_files: the tile (%d..%d, %d..%d) does not fit the global grid %d x %d", m->i0, m->i0 + P.im - 1, m->j0,
                m->j0 + P.jm - 1, m->im_global, m->jm_global);
  if (P.im < 3 || P.jm < 3) return fail(c, POMGPU_EINVAL, "set_forcing_files: the wind taper needs a tile of at least 3 x 3 cells");
  // a clim file on z levels (pomgpu_set_z_inputs): ztosig's fill-in looks at all four neighbours, so the monthly fetch reads one more column / row
  // towards every neighbour of the tile
  const int zc = clim && c->z_clim, wi = zc && !P.W, we = zc && !P.E, wj = zc && !P.S, wn = zc && !P.N;
  if (m->i0 - wi < 1 || m->j0 - wj < 1 || m->i0 + P.im - 1 + we > m->im_global || m->j0 + P.jm - 1 + wn > m->jm_global)
    return fail(c, POMGPU_EINVAL, "set_forcing_files: %s: the tile (%d..%d, %d..%d) with its window lines towards every neighbour does not fit the global grid %d x %d", clim,
                m->i0, m->i0 + P.im - 1, m->j0, m->j0 + P.jm - 1, m->im_global, m->jm_global);
  // an lbry file on z levels (pomgpu_set_z_lateral): the fill-in of a line point looks at the points before and after it, so the fetch reads one
  // more point of temp / salt towards every neighbour of the tile: .east towards the south and north one, .south towards the west and east one
  const int zl = lbry && c->z_lbry, lwi = zl && !P.W, lwe = zl && !P.E, lwj = zl && !P.S, lwn = zl && !P.N;
  if (zl && (P.im < 4 || P.jm < 4)) return fail(c, POMGPU_EINVAL, "set_forcing_files: %s: a z-level lbry file needs a tile of at least 4 x 4 cells, this one has %d x %d", lbry, P.im, P.jm);
  if (m->i0 - lwi < 1 || m->j0 - lwj < 1 || m->i0 + P.im - 1 + lwe > m->im_global || m->j0 + P.jm - 1 + lwn > m->jm_global)
    return fail(c, POMGPU_EINVAL, "set_forcing_files: %s: the tile (%d..%d, %d..%d) with its window points towards every neighbour does not fit the global grid %d x %d", lbry,
                m->i0, m->i0 + P.im - 1, m->j0, m->j0 + P.jm - 1, m->im_global, m->jm_global);
  std::vector<double> zlev, llev;
  FFiles *old = FF(c);
  if (old && (old->im_global != m->im_global || old->jm_global != m->jm_global || old->i0 != m->i0 || old->j0 != m->j0))
    return fail(c, POMGPU_EINVAL, "set_forcing_files: files are registered under another global grid or tile origin");
  const uint64_t img = (uint64_t)m->im_global, jmg = (uint64_t)m->jm_global, kb = (uint64_t)P.kb;
  const char *paths[3] = {sfrc, lbry, clim};
  FSource fresh[3];
  auto drop = [&]() { for (FSource &s : fresh) if (s.fd >= 0) (void)close(s.fd); };
  for (int q = 0; q < 3; q++) {                                 // every file is opened and checked before anything is kept
    if (!paths[q]) continue;
    FSource &S = fresh[q];
    S.path = paths[q];
    S.fd = open(paths[q], O_RDONLY);
    if (S.fd < 0) { drop(); return fail(c, POMGPU_EINVAL, "set_forcing_files: cannot open %s", paths[q]); }
    struct stat sb;
    if (fstat(S.fd, &sb)) { drop(); return fail(c, POMGPU_EINVAL, "set_forcing_files: cannot stat %s", paths[q]); }
    S.fsize = (uint64_t)sb.st_size;
    RHeader H;
    std::string what;
    if (ff_header(S.fd, S.fsize, H, what) < 0) { drop(); return fail(c, POMGPU_EINVAL, "set_forcing_files: %s is not a %s file this library reads: %s", paths[q], FF_WHAT[q], what.c_str()); }
    std::string why;
    if (q == 0) why = ff_check(H, S, FF_SFRC, std::vector<std::vector<uint64_t>>(6, {jmg, img}), 1);
    else if (q == 1) {
      if (zl) why = z_levels(H, S, "z", llev);
      const uint64_t kl = zl && why.empty() ? (uint64_t)llev.size() : kb;   // temp, salt on the levels of z; u, v stay on the sigma levels
      if (why.empty()) why = ff_check(H, S, FF_LBRY, {{jmg}, {img}, {kb, jmg}, {kb, jmg}, {kl, jmg}, {kl, jmg}, {kb, img}, {kb, img}, {kl, img}, {kl, img}}, 1);
    }
    else {
      if (zc) why = z_levels(H, S, "z", zlev);
      const uint64_t kc = zc && why.empty() ? (uint64_t)zlev.size() : kb;
      if (why.empty()) why = ff_check(H, S, FF_CLIM, {{kc, jmg, img}, {kc, jmg, img}}, 12);
    }
    if (!why.empty()) { drop(); return fail(c, POMGPU_EINVAL, "set_forcing_files: %s: %s", paths[q], why.c_str()); }
  }
  // ---- accepted: the buffers every fetch uses, sized once (no allocation inside a step) ----
  FFiles *F = old ? old : new FFiles();
  const size_t band2 = (size_t)(P.jm + wj + wn) * (size_t)img * 8;   // one level's band of rows (the window's, for a z-level clim file) at the file's full width, doubles
  const size_t zks = zlev.size(), nlevmax = zks > (size_t)P.kb ? zks : (size_t)P.kb;
  size_t run = (SW(c, IO_CHUNK_KB) && SWV(c, IO_CHUNK_KB) > 0 ? (size_t)SWV(c, IO_CHUNK_KB) << 10 : (size_t)64 << 20);
  if (run < band2) run = band2;
  if (run > band2 * nlevmax) run = band2 * nlevmax;
  size_t need = 2 * band2;                                        // sfrc: two variables' bands
  const size_t lat = 8 * ((size_t)P.jm + P.im) + 4 * 8 * (size_t)P.kb * ((size_t)P.jm + P.im);
  if (need < lat) need = lat;
  const size_t lks = llev.size();                                 // a z-level lbry record: two of the four arrays of either edge on lks levels over the window
  const size_t latz = 8 * ((size_t)P.jm + P.im) + 2 * 8 * (size_t)P.kb * ((size_t)P.jm + P.im) + 2 * 8 * lks * ((size_t)P.jm + P.im + 4);
  if (lks && need < latz) need = latz;
  if (need < run) need = run;
  int bad = ff_reserve(c, F, need);
  // the slots the setters would have allocated on their first call
  const size_t rec2 = sizeof(double) * (size_t)P.im * P.jm, rec3 = rec2 * (size_t)P.kb;
  const size_t latrec = sizeof(double) * (8 * (size_t)P.jml * P.kb + 8 * (size_t)P.iml * P.kb + 2 * (size_t)P.jml + 2 * (size_t)P.iml);
  if (!bad && paths[0])
    for (int k = 0; k < 3; k++) for (int sl = 0; sl < 4; sl++) for (int f = 0; f < 2; f++)
      if (!c->frc_dev[k][sl][f] && hipMalloc((void **)&c->frc_dev[k][sl][f], rec2) != hipSuccess) bad = 1;
  if (!bad && paths[1]) for (int sl = 0; sl < 4; sl++) if (!c->lat_dev[sl] && hipMalloc((void **)&c->lat_dev[sl], latrec) != hipSuccess) bad = 1;
  if (!bad && paths[2] && !c->rec_t[0] && (hipMalloc((void **)&c->rec_t[0], rec3) != hipSuccess || hipMalloc((void **)&c->rec_s[0], rec3) != hipSuccess)) bad = 1;
  // ztosig's buffers and table: allocated here, so that a step allocates nothing; an earlier registration keeps its own until these exist
  const size_t zwin = zks * (size_t)(P.im + wi + we) * (size_t)(P.jm + wj + wn), zwork = zks * P.n2;
  double *znew = NULL;
  if (!bad && paths[2] && zks) {
    std::vector<double> tab(4 * zks);
    ztosig_table(zlev.data(), (int)zks, tab.data());
    if (hipMalloc((void **)&znew, (zwin + 2 * zwork + 4 * zks) * sizeof(double)) != hipSuccess ||
        hipMemcpyAsync(znew + zwin + 2 * zwork, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
      bad = 1;
      if (znew) (void)hipFree(znew);
      znew = NULL;
    }
  }
  const size_t lpitch = (size_t)(P.jml > P.iml ? P.jml : P.iml);
  double *lnew = NULL;
  if (!bad && lks) {
    std::vector<double> tab(4 * lks);
    ztosig_table(llev.data(), (int)lks, tab.data());
    if (hipMalloc((void **)&lnew, (4 * lks + 8 * lks * lpitch) * sizeof(double)) != hipSuccess ||
        hipMemcpyAsync(lnew, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {           // (and an earlier fetch has stopped mapping out of the old buffers)
      bad = 1;
      if (lnew) (void)hipFree(lnew);
      if (znew) (void)hipFree(znew);
      lnew = znew = NULL;
    }
  }
  if (!bad && paths[1]) {
    if (F->ldev && !lks && hipStreamSynchronize(c->stream) != hipSuccess) { bad = 1; if (znew) (void)hipFree(znew); znew = NULL; }
    else {
      if (F->ldev) (void)hipFree(F->ldev);
      F->ldev = lnew;
      F->lks = (int)lks; F->lwi = lwi; F->lwe = lwe; F->lwj = lwj; F->lwn = lwn;
    }
  }
  if (!bad && paths[2]) {
    if (F->zdev && hipStreamSynchronize(c->stream) != hipSuccess) bad = 1;   // an earlier fetch may still be mapping out of the old buffers
    if (F->zdev) (void)hipFree(F->zdev);
    F->zdev = znew;
    F->zks = (int)zks; F->wi = wi; F->we = we; F->wj = wj; F->wn = wn;
    F->zwin = zwin; F->zwork = zwork;
  }
  c->frc_files = F;
  if (bad) {
    drop();
    (void)hipGetLastError();
    if (!old) pomgpu_ff_free(c);
    return fail(c, POMGPU_ENOMEM, "set_forcing_files: no memory for the read buffers (%zu bytes, twice pinned)", need);
  }
  F->im_global = m->im_global; F->jm_global = m->jm_global; F->i0 = m->i0; F->j0 = m->j0;
  for (int q = 0; q < 3; q++) {
    if (!paths[q]) continue;
    if (F->s[q].fd >= 0) (void)close(F->s[q].fd);
    F->s[q] = fresh[q];
    if (q == 0) { for (int k = 0; k < 3; k++) for (int sl = 0; sl < 4; sl++) c->frc_n[k][sl] = 0; c->frc_on = 1; }   // records the setters left are not the file's
    if (q == 1) { for (int sl = 0; sl < 4; sl++) c->lat_n[sl] = 0; c->lat_on = 1; }
  }
  return POMGPU_OK;
}

// Is record n (1-based) of every variable in `which` inside the file?  A record beyond numrecs or the file's end gets ONE second look
// (the file may have grown); then the step fails, before anything is written.
static int ff_have(pomgpu_ctx *c, FSource &S, const char *who, int n, std::initializer_list<int> which) {
  for (int pass = 0; pass < 2; pass++) {
    bool ok = n >= 1;
    for (int q : which) {
      const FVar &f = S.v[q];
      const uint64_t nrec = f.rec ? (uint64_t)S.numrecs : f.nfixed;
      if (!ok || (uint64_t)n > nrec) { ok = false; break; }
      if (f.begin > S.fsize || (uint64_t)(n - 1) > (S.fsize - f.begin) / (f.stride ? f.stride : 1) || (uint64_t)(n - 1) * f.stride + f.slab > S.fsize - f.begin) { ok = false; break; }
    }
    if (ok) return POMGPU_OK;
    if (pass == 1 || n < 1) break;
    unsigned char h8[8];
    struct stat sb;
    if (fstat(S.fd, &sb) || pread_all(S.fd, h8, 8, 0)) break;
    S.fsize = (uint64_t)sb.st_size;
    S.numrecs = ((uint32_t)h8[4] << 24) | ((uint32_t)h8[5] << 16) | ((uint32_t)h8[6] << 8) | (uint32_t)h8[7];
  }
  return fail(c, POMGPU_EINVAL, "%s: record %d is not in %s (%u records, %llu bytes)", who, n, S.path.c_str(), (unsigned)S.numrecs, (unsigned long long)S.fsize);
}
// a pinned buffer free for the next run's preads / its bytes on their way to the device, in stream order behind the kernels that read the last run
static unsigned char *ff_buffer(FFiles *F) {
#ifndef POMGPU_EMU
  if (F->used[F->b] && hipEventSynchronize(F->ev[F->b]) != hipSuccess) return NULL;
#endif
  return F->pin[F->b];
}
static int ff_send(pomgpu_ctx *c, FFiles *F, size_t bytes) {
#ifndef POMGPU_EMU
  if (hipMemcpyAsync(F->stage, F->pin[F->b], bytes, hipMemcpyHostToDevice, c->cur) != hipSuccess || hipEventRecord(F->ev[F->b], c->cur) != hipSuccess) return 1;
  F->used[F->b] = 1;
  F->b ^= 1;
#else
  (void)c; (void)bytes;
#endif
  return 0;
}
static int ff_io_error(pomgpu_ctx *c, const char *who, int n, const FSource &S, int hip) {
  if (hip) (void)hipGetLastError();
  return fail(c, hip ? POMGPU_EHIP : POMGPU_EINVAL, hip ? "%s: a HIP call failed while reading record %d of %s" : "%s: I/O error reading record %d of %s", who, n, S.path.c_str());
}

// record n of wind (kind 0), heat (1), surface (2) into the slot pomgpu_set_forcing_record(kind, n, ...) fills
int pomgpu_ff_fetch_surface(pomgpu_ctx *c, int kind, int n) {
  FFiles *F = FF(c);
  FSource &S = F->s[0];
  const KP &P = c->P;
  static const char *const who[3] = {"wind", "heat", "surface"};
  const int va = 2 * kind, vb = 2 * kind + 1, nvar = kind == 2 ? 1 : 2;   // SSS is read by the reference and dropped (bounds_forcing.f:978-979): not read here
  int rc = kind == 2 ? ff_have(c, S, who[kind], n, {va}) : ff_have(c, S, who[kind], n, {va, vb});
  if (rc) return rc;
  const int sl = n % 4;
  unsigned char *pin = ff_buffer(F);
  if (!pin) return ff_io_error(c, who[kind], n, S, 1);
  const size_t half = (size_t)P.jm * (size_t)F->im_global * 8;   // where the second variable's band starts (8-byte aligned whatever the types)
  for (int q = 0; q < nvar; q++) {
    const FVar &f = S.v[q ? vb : va];
    const uint64_t at = f.begin + (uint64_t)(n - 1) * f.stride + (uint64_t)(F->j0 - 1) * (uint64_t)F->im_global * f.esize();
    if (pread_all(S.fd, pin + q * half, (size_t)P.jm * (size_t)F->im_global * f.esize(), at)) return ff_io_error(c, who[kind], n, S, 0);
  }
  if (ff_send(c, F, nvar == 2 ? 2 * half : half)) return ff_io_error(c, who[kind], n, S, 1);
  double *da = c->frc_dev[kind][sl][0], *db = c->frc_dev[kind][sl][1];
  const void *sa = F->stage, *sb = nvar == 2 ? (const void *)(F->stage + half) : NULL;
  const bool fa = S.v[va].type == 5, fb = nvar == 2 && S.v[vb].type == 5;
  const int pitch = F->im_global, i0 = F->i0 - 1;
  if (fa && fb) LAUNCHN(c, "k_frc_unpack", (k_frc_unpack<float, float>), grid2(P), blk2(), P, kind, da, db, sa, sb, pitch, i0);
  else if (fa) LAUNCHN(c, "k_frc_unpack", (k_frc_unpack<float, double>), grid2(P), blk2(), P, kind, da, db, sa, sb, pitch, i0);
  else if (fb) LAUNCHN(c, "k_frc_unpack", (k_frc_unpack<double, float>), grid2(P), blk2(), P, kind, da, db, sa, sb, pitch, i0);
  else LAUNCHN(c, "k_frc_unpack", (k_frc_unpack<double, double>), grid2(P), blk2(), P, kind, da, db, sa, sb, pitch, i0);
  c->frc_n[kind][sl] = n;
  return POMGPU_OK;
}
// record n of the lateral file into the slot pomgpu_set_lateral_record(n, ...) fills
int pomgpu_ff_fetch_lateral(pomgpu_ctx *c, int n) {
  FFiles *F = FF(c);
  FSource &S = F->s[1];
  const KP &P = c->P;
  int rc = ff_have(c, S, "lateral_bc", n, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9});
  if (rc) return rc;
  const int sl = n % 4;
  unsigned char *pin = ff_buffer(F);
  if (!pin) return ff_io_error(c, "lateral_bc", n, S, 1);
  LatSrc src;
  src.f32 = 0;
  size_t at = 0, off[10];
  // a z-level lbry file: temp, salt of either edge on all lks levels over the line and its window points, mapped by k_ztosig_line behind k_lat_unpack
  const int onz = F->lks > 0;
  int cnt[10], wlo[10];
  for (int q = 0; q < 10; q++) {
    const FVar &f = S.v[q];
    const bool east = q == 0 || (q >= 2 && q <= 5);              // along j: the tile's jm values from j0; else im values from i0
    const bool zq = onz && (q == 4 || q == 5 || q == 8 || q == 9);
    const int nlev = q < 2 ? 1 : (zq ? F->lks : P.kb);
    wlo[q] = zq ? (east ? F->lwj : F->lwi) : 0;
    cnt[q] = (east ? P.jm : P.im) + wlo[q] + (zq ? (east ? F->lwn : F->lwe) : 0);
    const uint64_t glen = east ? (uint64_t)F->jm_global : (uint64_t)F->im_global, first = (uint64_t)((east ? F->j0 : F->i0) - 1 - wlo[q]);
    const size_t len = (size_t)cnt[q] * f.esize();
    const uint64_t base = f.begin + (uint64_t)(n - 1) * f.stride + first * f.esize();
    off[q] = at;
    if ((uint64_t)cnt[q] == glen) { if (pread_all(S.fd, pin + at, len * nlev, base)) return ff_io_error(c, "lateral_bc", n, S, 0); }
    else for (int k = 0; k < nlev; k++) if (pread_all(S.fd, pin + at + (size_t)k * len, len, base + (uint64_t)k * glen * f.esize())) return ff_io_error(c, "lateral_bc", n, S, 0);
    at += (len * nlev + 7) & ~(size_t)7;
    if (f.type == 5) src.f32 |= 1u << q;
  }
  if (ff_send(c, F, at)) return ff_io_error(c, "lateral_bc", n, S, 1);
  for (int q = 0; q < 10; q++) src.p[q] = F->stage + off[q];
  src.zts = onz;
  const int nt = P.jml + P.iml;
  LAUNCH(c, k_lat_unpack, dim3((unsigned)((nt + 63) / 64), 1, 1), dim3(64, 1, 1), P, c->lat_dev[sl], src);
  if (onz) {                                                     // tbe sbe / tbs sbs: the record's arrays 4, 5 of either edge
    const size_t njk = (size_t)P.jml * P.kb, nik = (size_t)P.iml * P.kb;
    const int pitch = P.jml > P.iml ? P.jml : P.iml;
    static const int zq[4] = {4, 5, 8, 9};
    ZtlJob job;
    for (int l = 0; l < 4; l++) {
      const int q = zq[l];
      double *out = c->lat_dev[sl] + (l < 2 ? (size_t)(4 + l) * njk : 8 * njk + (size_t)(2 + l) * nik);
      job.l[l] = ztosig_line_of(P, l < 2 ? 0 : 1, out, src.p[q], S.v[q].type == 5 ? 1 : 2, cnt[q], wlo[q]);
    }
    launch_ztosig_lines(c, job, 4, F->ldev, F->ldev + 4 * (size_t)F->lks, F->ldev + 4 * (size_t)F->lks + 4 * (size_t)F->lks * pitch, F->lks, pitch);
  }
  c->lat_n[sl] = n;
  return POMGPU_OK;
}
// Tclim, Sclim of month mod(n+9,12)+1 (io_pnetcdf.F:3316) into rec_t[0], rec_s[0], the (im,jm,kb) records k_restore_load reads
int pomgpu_ff_fetch_restore(pomgpu_ctx *c, int n) {
  FFiles *F = FF(c);
  FSource &S = F->s[2];
  const KP &P = c->P;
  if (n < 1) return fail(c, POMGPU_EINVAL, "restore_interior: record %d", n);
  const int month = (n + 9) % 12 + 1;
  int rc = ff_have(c, S, "restore_interior", month, {0, 1});
  if (rc) return rc;
  const uint64_t img = (uint64_t)F->im_global, jmg = (uint64_t)F->jm_global;
  // a z-level clim file: all zks levels over the tile's window into the window buffer, then ztosig into the record, in k_rst_unpack's place
  const int onz = F->zks > 0, rows = P.jm + F->wj + F->wn, cols = P.im + F->wi + F->we, nlev = onz ? F->zks : P.kb;
  const size_t band = (size_t)rows * (size_t)img;               // values of one level's band
  const bool whole_rows = (uint64_t)rows == jmg;
  for (int q = 0; q < 2; q++) {
    const FVar &f = S.v[q];
    const int lev_per_run = (int)(F->cap / (band * f.esize())) < nlev ? (int)(F->cap / (band * f.esize())) : nlev;
    double *dst = q ? c->rec_s[0] : c->rec_t[0];
    for (int k0 = 0; k0 < nlev; k0 += lev_per_run) {
      const int nl = nlev - k0 < lev_per_run ? nlev - k0 : lev_per_run;
      unsigned char *pin = ff_buffer(F);
      if (!pin) return ff_io_error(c, "restore_interior", n, S, 1);
      const uint64_t first = f.begin + (uint64_t)(month - 1) * f.stride + (((uint64_t)k0 * jmg + (uint64_t)(F->j0 - 1 - F->wj)) * img) * f.esize();
      if (whole_rows) { if (pread_all(S.fd, pin, (size_t)nl * band * f.esize(), first)) return ff_io_error(c, "restore_interior", n, S, 0); }
      else for (int k = 0; k < nl; k++) if (pread_all(S.fd, pin + (size_t)k * band * f.esize(), band * f.esize(), first + (uint64_t)k * jmg * img * f.esize())) return ff_io_error(c, "restore_interior", n, S, 0);
      if (ff_send(c, F, (size_t)nl * band * f.esize())) return ff_io_error(c, "restore_interior", n, S, 1);
      const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((rows + 3) / 4), (unsigned)nl);
      double *to = onz ? F->zdev : dst;
      if (f.type == 5) LAUNCHN(c, "k_rst_unpack", k_rst_unpack<float>, grid, blk2(), to, (const void *)F->stage, cols, rows, rows, (int)img, F->i0 - 1 - F->wi, k0);
      else LAUNCHN(c, "k_rst_unpack", k_rst_unpack<double>, grid, blk2(), to, (const void *)F->stage, cols, rows, rows, (int)img, F->i0 - 1 - F->wi, k0);
    }
    if (onz) launch_ztosig_window(c, dst, 1, F->zdev, F->zdev + F->zwin + 2 * F->zwork, F->zdev + F->zwin, F->zdev + F->zwin + F->zwork, F->zks, F->wi, F->we, F->wj, F->wn);
  }
  return POMGPU_OK;
}

// ---- the restore rate from a z-level file (read_restore_tau_interior_pnetcdf, io_pnetcdf.F:3053-3107, and the ztosig behind it that
// bounds_forcing.f:1049-1051, :1076-1079 keep commented) ---------------------------------------------------------------------------------
// `z` (ks levels) and `tau` (ks, jm_global, im_global), with or without a leading record dimension.  The rate that goes with T/S record n
// is record n of the file; a file with one record (or no record dimension) is steady and serves every n.  Registered beside the three
// forcing files: the same header parser and checks, the same pinned buffers, the window and the work arrays of the z-level clim file.
static std::string rate_check(const RHeader &H, FSource &S, uint64_t ks, uint64_t jmg, uint64_t img) {
  const RVar *v = NULL;
  for (const RVar &x : H.vars) if (x.name == FF_RATE[0]) { v = &x; break; }
  if (!v) return std::string("variable tau is absent");
  if (v->dimids.size() != 3) return ff_check(H, S, FF_RATE, {{ks, jmg, img}}, 1);   // a leading record dimension, unlimited or fixed
  if (v->type != 5 && v->type != 6) return "variable tau has NetCDF type " + std::to_string(v->type) + ", neither NC_FLOAT (5) nor NC_DOUBLE (6)";
  if (H.dimlen[v->dimids[0]] != ks || H.dimlen[v->dimids[1]] != jmg || H.dimlen[v->dimids[2]] != img)
    return "variable tau has the dimension lengths " + lengths_of(H, *v) + ", wanted ([records, ]" + std::to_string(ks) + ", " + std::to_string(jmg) + ", " + std::to_string(img) + ")";
  FVar f;
  f.name = FF_RATE[0]; f.type = v->type; f.begin = v->begin;
  f.slab = f.esize() * ks * jmg * img;
  f.rec = false; f.stride = f.slab; f.nfixed = 1;
  if (f.begin > S.fsize || f.slab > S.fsize - f.begin)
    return "variable tau (1 records of " + std::to_string(f.slab) + " bytes from " + std::to_string(f.begin) + ") reaches beyond the file's " + std::to_string(S.fsize) + " bytes: a truncated file";
  S.v.assign(1, f);
  S.numrecs = H.numrecs;
  return std::string();
}
extern "C" int pomgpu_set_restore_rate_file(pomgpu_ctx *c, const char *path, const pomgpu_file_meta *m) {
  if (!c) return POMGPU_EINVAL;
  if (!path || !m) return fail(c, POMGPU_EINVAL, "set_restore_rate_file: %s", path ? "no file meta was given" : "no path was given (NULL)");
  (void)hipSetDevice(c->device);
  const KP &P = c->P;
  if (c->flags & POMGPU_CTX_2D) return fail(c, POMGPU_EINVAL, "set_restore_rate_file: %s: not on a 2-D context", path);
  if (P.im < 4 || P.jm < 4) return fail(c, POMGPU_EINVAL, "set_restore_rate_file: %s: a rate file needs a tile of at least 4 x 4 cells, this one has %d x %d", path, P.im, P.jm);
  // ztosig's fill-in looks at all four neighbours: one more column / row towards every neighbour of the tile, as for a z-level clim file
  const int wi = !P.W, we = !P.E, wj = !P.S, wn = !P.N;
  if (m->i0 - wi < 1 || m->j0 - wj < 1 || m->i0 + P.im - 1 + we > m->im_global || m->j0 + P.jm - 1 + wn > m->jm_global)
    return fail(c, POMGPU_EINVAL, "set_restore_rate_file: %s: the tile (%d..%d, %d..%d) with its window lines towards every neighbour does not fit the global grid %d x %d", path,
                m->i0, m->i0 + P.im - 1, m->j0, m->j0 + P.jm - 1, m->im_global, m->jm_global);
  FFiles *old = FF(c);
  if (old && (old->im_global != m->im_global || old->jm_global != m->jm_global || old->i0 != m->i0 || old->j0 != m->j0))
    return fail(c, POMGPU_EINVAL, "set_restore_rate_file: %s: files are registered under another global grid or tile origin", path);
  const uint64_t img = (uint64_t)m->im_global, jmg = (uint64_t)m->jm_global;
  FSource S;
  S.path = path;
  S.fd = open(path, O_RDONLY);
  if (S.fd < 0) return fail(c, POMGPU_EINVAL, "set_restore_rate_file: cannot open %s", path);
  struct stat sb;
  if (fstat(S.fd, &sb)) { (void)close(S.fd); return fail(c, POMGPU_EINVAL, "set_restore_rate_file: cannot stat %s", path); }
  S.fsize = (uint64_t)sb.st_size;
  RHeader H;
  std::string what;
  if (ff_header(S.fd, S.fsize, H, what) < 0) { (void)close(S.fd); return fail(c, POMGPU_EINVAL, "set_restore_rate_file: %s is not a rate file this library reads: %s", path, what.c_str()); }
  std::vector<double> zlev;
  std::string why = z_levels(H, S, "z", zlev);
  if (why.empty()) why = rate_check(H, S, (uint64_t)zlev.size(), jmg, img);
  if (!why.empty()) { (void)close(S.fd); return fail(c, POMGPU_EINVAL, "set_restore_rate_file: %s: %s", path, why.c_str()); }
  // ---- accepted: the buffers and the table every fetch uses (no allocation inside a step) ----
  FFiles *F = old ? old : new FFiles();
  const size_t ks = zlev.size();
  const size_t band2 = (size_t)(P.jm + wj + wn) * (size_t)img * 8;   // one level's band of the window's rows at the file's full width, doubles
  size_t need = (SW(c, IO_CHUNK_KB) && SWV(c, IO_CHUNK_KB) > 0 ? (size_t)SWV(c, IO_CHUNK_KB) << 10 : (size_t)64 << 20);
  if (need < band2) need = band2;
  if (need > band2 * ks) need = band2 * ks;
  int bad = ff_reserve(c, F, need);
  const size_t rwin = ks * (size_t)(P.im + wi + we) * (size_t)(P.jm + wj + wn), rwork = ks * P.n2;
  double *rnew = NULL;
  if (!bad) {
    std::vector<double> tab(4 * ks);
    ztosig_table(zlev.data(), (int)ks, tab.data());
    if (hipMalloc((void **)&rnew, (rwin + 2 * rwork + 4 * ks) * sizeof(double)) != hipSuccess ||
        hipMemcpyAsync(rnew + rwin + 2 * rwork, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {          // (and an earlier fetch has stopped mapping out of the old buffers)
      bad = 1;
      if (rnew) (void)hipFree(rnew);
      rnew = NULL;
    }
  }
  c->frc_files = F;
  if (bad) {
    (void)close(S.fd);
    (void)hipGetLastError();
    if (!old) pomgpu_ff_free(c);
    return fail(c, POMGPU_ENOMEM, "set_restore_rate_file: %s: no memory for the read buffers (%zu bytes, twice pinned) and the window", path, need);
  }
  if (F->rdev) (void)hipFree(F->rdev);
  F->rdev = rnew;
  F->rks = (int)ks; F->rwi = wi; F->rwe = we; F->rwj = wj; F->rwn = wn;
  F->rwin = rwin; F->rwork = rwork;
  F->im_global = m->im_global; F->jm_global = m->jm_global; F->i0 = m->i0; F->j0 = m->j0;
  if (F->s[3].fd >= 0) (void)close(F->s[3].fd);
  F->s[3] = S;
  const FVar &f = F->s[3].v[0];
  F->rsteady = f.rec ? S.numrecs == 1 : f.nfixed == 1;
  c->tau_gen++;                                                   // what the arrays were made from before is not this file's
  c->rate_in_f = 0;
  return POMGPU_OK;
}
int pomgpu_ff_rate_steady(pomgpu_ctx *c) { return FF(c)->rsteady; }
int pomgpu_ff_rate_have(pomgpu_ctx *c, int n) {
  FFiles *F = FF(c);
  if (n < 1) return fail(c, POMGPU_EINVAL, "restore_interior: rate record %d", n);
  return ff_have(c, F->s[3], "restore_interior (rate)", F->rsteady ? 1 : n, {0});
}
// record n of `tau`: all rks levels over the tile's window into the window buffer, then k_ztosig straight into the mirror taurstrf -- every
// cell of (1:im, 1:jm) on all kb levels, the padding beyond keeps what k_restore_load has put there; on the stream the step is enqueued on
int pomgpu_ff_fetch_rate(pomgpu_ctx *c, int n) {
  FFiles *F = FF(c);
  FSource &S = F->s[3];
  const KP &P = c->P;
  const int rec = F->rsteady ? 1 : n;
  const uint64_t img = (uint64_t)F->im_global, jmg = (uint64_t)F->jm_global;
  const int rows = P.jm + F->rwj + F->rwn, cols = P.im + F->rwi + F->rwe, nlev = F->rks;
  const size_t band = (size_t)rows * (size_t)img;               // values of one level's band
  const bool whole_rows = (uint64_t)rows == jmg;
  const FVar &f = S.v[0];
  const int lev_per_run = (int)(F->cap / (band * f.esize())) < nlev ? (int)(F->cap / (band * f.esize())) : nlev;
  for (int k0 = 0; k0 < nlev; k0 += lev_per_run) {
    const int nl = nlev - k0 < lev_per_run ? nlev - k0 : lev_per_run;
    unsigned char *pin = ff_buffer(F);
    if (!pin) return ff_io_error(c, "restore_interior (rate)", n, S, 1);
    const uint64_t first = f.begin + (uint64_t)(rec - 1) * f.stride + (((uint64_t)k0 * jmg + (uint64_t)(F->j0 - 1 - F->rwj)) * img) * f.esize();
    if (whole_rows) { if (pread_all(S.fd, pin, (size_t)nl * band * f.esize(), first)) return ff_io_error(c, "restore_interior (rate)", n, S, 0); }
    else for (int k = 0; k < nl; k++) if (pread_all(S.fd, pin + (size_t)k * band * f.esize(), band * f.esize(), first + (uint64_t)k * jmg * img * f.esize())) return ff_io_error(c, "restore_interior (rate)", n, S, 0);
    if (ff_send(c, F, (size_t)nl * band * f.esize())) return ff_io_error(c, "restore_interior (rate)", n, S, 1);
    const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((rows + 3) / 4), (unsigned)nl);
    if (f.type == 5) LAUNCHN(c, "k_rst_unpack", k_rst_unpack<float>, grid, blk2(), F->rdev, (const void *)F->stage, cols, rows, rows, (int)img, F->i0 - 1 - F->rwi, k0);
    else LAUNCHN(c, "k_rst_unpack", k_rst_unpack<double>, grid, blk2(), F->rdev, (const void *)F->stage, cols, rows, rows, (int)img, F->i0 - 1 - F->rwi, k0);
  }
  double *taurstrf = c->P.b3 + (size_t)P3_taurstrf * c->P.a3;
  launch_ztosig_window(c, taurstrf, 0, F->rdev, F->rdev + F->rwin + 2 * F->rwork, F->rdev + F->rwin, F->rdev + F->rwin + F->rwork, F->rks, F->rwi, F->rwe, F->rwj, F->rwn);
  return POMGPU_OK;
}

// ---- ztosig: z-level T or S onto the sigma levels (initialize.f:547-595 with splinc :598-638 and splint :641-667) -----------------------
// One column per lane, threadIdx.x -> i, the level loops in the thread.  ks goes up to splinc's nmax = 300, so the column's vectors do
// not live in registers: tin (the filled-in source, splinc's y) and u / y2 are two work arrays of this call laid out like the source,
// (i, j, k), so that a wavefront touches one contiguous row piece per level; a lane reads back only what it stored itself.  What
// depends on zs alone -- sig, p and the decomposition's y2(i) = (sig-1.)/p (:613-615) -- comes in `tab` (zs, sig, p, y2, ks values each),
// formed once per call by ztosig_table with the same fp64 expressions.
//   fill-in (:564-572): from the RAW source only -- no lane reads what another has stored -- one level ahead of the decomposition, which
//     needs y(i+1); amax1 is the REAL(4) intrinsic: the neighbour maximum reaches tin rounded to single; 0.01 is a REAL(4) literal
//   natural spline (yp1 = ypn = 2.d30): y2(1) = u(1) = 0, qn = un = 0, the reference's order and association throughout
//   splint: its bisection as written, on the table (a**3 = a*a*a, h**2 = h*h)
// All kb levels are stored (level kb is an extrapolation), rounded once to the storage type.  Columns on the frame of (1:im, 1:jm) and
// those with h <= 1.0 get the +0.0 of `t = 0.` (:558); k_ztosig_edges makes the copies of :589-592 after the exchange of :586.
#define POMGPU_ZTOSIG_NMAX 300
static void ztosig_table(const double *zs, int ks, double *tab) {
  double *x = tab, *sg = tab + ks, *pp = tab + 2 * (size_t)ks, *d2 = tab + 3 * (size_t)ks;
  for (int i = 0; i < ks; i++) { x[i] = zs[i]; sg[i] = 0.; pp[i] = 0.; d2[i] = 0.; }
  for (int i = 1; i < ks - 1; i++) {
    const double sig = (x[i] - x[i - 1]) / (x[i + 1] - x[i - 1]);
    const double p = sig * d2[i - 1] + (double)2.f;
    sg[i] = sig; pp[i] = p;
    d2[i] = (sig - (double)1.f) / p;
  }
}
// Where the source and the result live: the source as doubles, `sp` values per row and `sl` per level, the tile's cell (1,1) at `so`
// (the stand-alone call: the tile's own array; the file readers: the tile's WINDOW, one more column / row towards every neighbour); the
// result `op` values per row and `ol` per level (a mirror, or the (im,jm,kb) restore record).  Columns ilo..ihi x jlo..jhi are mapped
// from their own source column.  fuse = 0: every other cell of (1:im, 1:jm) gets zero and the caller exchanges and copies the edges.
// fuse = 1 (the file readers, which post no message round): the range reaches the ghost lines towards neighbours -- formed from the
// window with the owner's arithmetic, which is what the exchange would bring -- and stops one line short of a physical edge, whose
// cells map the column next to them across every physical edge they lie on: what the four copies leave there, corners included.
struct ZtsGeo { int sp, op, ilo, ihi, jlo, jhi, fuse; size_t sl, so, ol; };
template <class TO>
__global__ void k_ztosig(KP P, TO *out, const double *src, const double *tab, double *wa, double *wb, int ks, ZtsGeo g) {
  const int i = TID_I, j = TID_J;
  if (i > P.im || j > P.jm) return;
  const int is = i < g.ilo ? g.ilo : (i > g.ihi ? g.ihi : i), js = j < g.jlo ? g.jlo : (j > g.jhi ? g.jhi : j);
  const double hc = F2(h, is, js);
  TO *const oc = out + (size_t)(j - 1) * g.op + (size_t)(i - 1);
  if ((!g.fuse && (is != i || js != j)) || !(hc > (double)1.f)) {
    for (int k = 0; k < P.kb; k++) oc[(size_t)k * g.ol] = (TO)0.;
    return;
  }
  const double *xs = tab, *sg = tab + ks, *pp = tab + 2 * (size_t)ks, *d2 = tab + 3 * (size_t)ks;
  const size_t o = IX2(i, j), lv = P.n2;
  const double *const sc = src + g.so + (size_t)(js - 1) * g.sp + (size_t)(is - 1);
  const double miss = (double)0.01f;
  auto raw = [&](int k) {                                       // tin(k) before the copy from above; k is 0-based
    const double *s = sc + (size_t)k * g.sl;
    double v = s[0];
    if (xs[k] <= hc && v < miss) {
      double m = s[-1];
      m = s[1] > m ? s[1] : m;
      m = s[-(ptrdiff_t)g.sp] > m ? s[-(ptrdiff_t)g.sp] : m;
      m = s[g.sp] > m ? s[g.sp] : m;
      v = (double)(float)m;
    }
    return v;
  };
  double y0 = raw(0), y1 = raw(1), up = 0.;
  if (y1 < miss) y1 = y0;
  wa[o] = y0;
  wb[o] = 0.;
  for (int n = 1; n < ks - 1; n++) {
    double yn = raw(n + 1);
    if (yn < miss) yn = y1;
    const double u = ((double)6.f * ((yn - y1) / (xs[n + 1] - xs[n]) - (y1 - y0) / (xs[n] - xs[n - 1])) / (xs[n + 1] - xs[n - 1]) - sg[n] * up) / pp[n];
    wa[(size_t)n * lv + o] = y1;
    wb[(size_t)n * lv + o] = u;
    up = u; y0 = y1; y1 = yn;
  }
  wa[(size_t)(ks - 1) * lv + o] = y1;
  const double qn = (double)0.f, un = 0.;
  double y2 = (un - qn * up) / (qn * d2[ks - 2] + (double)1.f);
  wb[(size_t)(ks - 1) * lv + o] = y2;
  for (int k = ks - 2; k >= 0; k--) {
    y2 = d2[k] * y2 + wb[(size_t)k * lv + o];
    wb[(size_t)k * lv + o] = y2;
  }
  for (int k = 1; k <= P.kb; k++) {
    const double x = -F1(zz, k) * hc;
    int klo = 1, khi = ks;
    while (khi - klo > 1) {
      const int kk = (khi + klo) / 2;
      if (xs[kk - 1] > x) khi = kk; else klo = kk;
    }
    const double xl = xs[klo - 1], xh = xs[khi - 1], hh = xh - xl;
    const double a = (xh - x) / hh, b = (x - xl) / hh;
    const size_t ql = (size_t)(klo - 1) * lv + o, qh = (size_t)(khi - 1) * lv + o;
    oc[(size_t)(k - 1) * g.ol] = (TO)(a * wa[ql] + b * wa[qh] + ((a * a * a - a) * wb[ql] + (b * b * b - b) * wb[qh]) * (hh * hh) / (double)6.f);
  }
}
// The copies onto physical edges (:589-592: west, east, south, north).  One lane per frame cell and level; a cell takes the value the
// sequence leaves there: the cell next to it across every physical edge it lies on -- never a cell this kernel writes, so the four
// statements' order shows only in which cell a corner ends up with, and that is this one.
__global__ void k_ztosig_edges(KP P, double *t) {
  const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x), k = (int)blockIdx.y + 1;
  int i, j;
  if (q < P.im) { i = q + 1; j = 1; }
  else if (q < 2 * P.im) { i = q - P.im + 1; j = P.jm; }
  else if (q < 2 * P.im + P.jm) { i = 1; j = q - 2 * P.im + 1; }
  else if (q < 2 * (P.im + P.jm)) { i = P.im; j = q - 2 * P.im - P.jm + 1; }
  else return;
  const int is = (i == 1 && P.W) ? 2 : ((i == P.im && P.E) ? P.imm1 : i), js = (j == 1 && P.S) ? 2 : ((j == P.jm && P.N) ? P.jmm1 : j);
  if (is != i || js != j) G3(t, i, j, k) = G3(t, is, js, k);
}
// the interior of ztosig into the mirror `t`; zs: ks host doubles (vetted), src: host (im_local, jm_local, ks).  Synchronous: the source
// and the work arrays are this call's.  The caller exchanges t and calls launch_ztosig_edges
int launch_ztosig(pomgpu_ctx *c, double *t, const double *zs, int ks, const double *src) {
  const KP &P = c->P;
  const size_t vol = (size_t)ks * P.n2;
  std::vector<double> tab(4 * (size_t)ks);
  ztosig_table(zs, ks, tab.data());
  double *dev = NULL;                                            // source, tin, u / y2, table
  if (hipMalloc((void **)&dev, (3 * vol + tab.size()) * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return POMGPU_ENOMEM; }
  int rc = POMGPU_OK;
  if (hipMemcpyAsync(dev, src, vol * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(dev + 3 * vol, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = POMGPU_EHIP;
  const ZtsGeo g = {P.iml, P.iml, 2, P.imm1, 2, P.jmm1, 0, P.n2, 0, P.n2};
  if (!rc) LAUNCHN(c, "k_ztosig", k_ztosig<pomgpu_st>, grid2(P), blk2(), P, (pomgpu_st *)t, (const double *)dev, (const double *)(dev + 3 * vol), dev + vol, dev + 2 * vol, ks, g);
  if (hipStreamSynchronize(c->stream) != hipSuccess) rc = POMGPU_EHIP;
  (void)hipFree(dev);
  return rc;
}
void launch_ztosig_edges(pomgpu_ctx *c, double *t) {
  const KP &P = c->P;
  LAUNCH(c, k_ztosig_edges, dim3((unsigned)((2 * (P.im + P.jm) + 63) / 64), (unsigned)P.kb, 1), dim3(64, 1, 1), P, t);
}
// ztosig for the file readers: the source is the tile's window (wi, we, wj, wn: one more line towards the west, east, south, north
// neighbour), every cell of (1:im, 1:jm) comes out of the one kernel (ZtsGeo, fuse = 1); enqueued on c->cur, no message round
// record = 0: `out` is a mirror; 1: the (im, jm, kb) restore record, plain doubles in every build
static void launch_ztosig_window(pomgpu_ctx *c, double *out, int record, const double *zsrc, const double *tab, double *wa, double *wb, int ks, int wi, int we, int wj, int wn) {
  const KP &P = c->P;
  const int wim = P.im + wi + we, wjm = P.jm + wj + wn;
  ZtsGeo g = {wim, P.iml, wi ? 1 : 2, we ? P.im : P.imm1, wj ? 1 : 2, wn ? P.jm : P.jmm1, 1, (size_t)wim * wjm, (size_t)wj * wim + wi, P.n2};
  if (record) {
    g.op = P.im; g.ol = (size_t)P.im * P.jm;
    LAUNCHN(c, "k_ztosig", k_ztosig<double>, grid2(P), blk2(), P, out, zsrc, tab, wa, wb, ks, g);
  } else LAUNCHN(c, "k_ztosig", k_ztosig<pomgpu_st>, grid2(P), blk2(), P, (pomgpu_st *)out, zsrc, tab, wa, wb, ks, g);
}

// ---- ztosig for the lines of a lateral record (bounds_forcing.f:636-716: the commented blocks behind read_boundary_conditions_pnetcdf) ----
// The block spreads a line, temp.east say, across the tile -- ts1(i,j,k) = t_e(j,k), hs(i,j) = h(imm1,j) --, calls ztosig and keeps the
// column im/2 (south: the row jm/2).  The source does not vary across the line, so every sampled column is the same ztosig column per line
// point `a`: depth hl(a) (east h(imm1,a), south h(a,2), west h(2,a), north h(a,jmm1)); of the four neighbours of the fill-in two are the
// point's own raw value and two the raw values of the points a-1 and a+1, in the order of amax1's arguments (:567-568).
//   k_ztosig_line: one line point per lane, threadIdx.x along the line, blockIdx.y the line of the job, the level loops in the thread and
//   k_ztosig's march (fill-in one level ahead of the decomposition, ztosig_table, splint's bisection as written).  tin and u / y2 live in
//   two work arrays laid out (point, level), the point contiguous, one slice per line; a lane reads back only what it stored itself.
//   The raw source (fmt 0: doubles; 1 / 2: the file's big-endian NC_FLOAT / NC_DOUBLE) holds `sp` values per level, point 1 at `so`.  A
//   lane reads the raw values of as-1, as, as+1 alone, as = its point moved into lo..hi: lo = 2 / hi = n-1 at a physical end, whose point
//   so redoes the column of the point next to it (the copies of :589-592, zeros included), and 1 / n towards a neighbour tile, whose ghost
//   point is formed from the window point beyond it with the owner's arithmetic and the owner's depth, which h's ghost cell holds -- what
//   the exchange of :586 would bring.  Every load is unconditional (the three addresses are inside the source for every lane that is
//   not beyond the line); points beyond n, up to the record's npad, and those with hl <= 1.0 get +0.0 on all kb levels.
static ZtlLine ztosig_line_of(const KP &P, int edge, double *out, const void *src, int fmt, int sp, int so) {
  const bool alongj = edge == 0 || edge == 2;
  const int n = alongj ? P.jm : P.im, npad = alongj ? P.jml : P.iml;
  const int plo = alongj ? P.S : P.W, phi = alongj ? P.N : P.E;
  return ZtlLine{out, src, fmt, edge, n, npad, plo ? 2 : 1, phi ? n - 1 : n, sp, so, npad};
}
__device__ __forceinline__ double ztl_raw(const void *p, int fmt, size_t q) {
  if (fmt == 1) return CdfRaw<float>::get(p, q);                   // fmt is the line's: uniform across the workgroup
  if (fmt == 2) return CdfRaw<double>::get(p, q);
  return ((const double *)p)[q];
}
__global__ void k_ztosig_line(KP P, ZtlJob job, const double *tab, double *wa, double *wb, int ks, int pitch) {
  const ZtlLine &L = job.l[blockIdx.y];
  const int a = TID_I;
  if (a > L.npad) return;
  const int as = a < L.lo ? L.lo : (a > L.hi ? L.hi : a);
  const bool alongj = L.edge == 0 || L.edge == 2;
  const int hi = L.edge == 0 ? P.imm1 : (L.edge == 2 ? 2 : as), hj = L.edge == 1 ? 2 : (L.edge == 3 ? P.jmm1 : as);
  const double hc = F2(h, hi, hj);
  double *const oc = L.out + (size_t)(a - 1);
  if (a > L.n || !(hc > (double)1.f)) {
    for (int k = 0; k < P.kb; k++) oc[(size_t)k * L.op] = 0.;
    return;
  }
  const double *xs = tab, *sg = tab + ks, *pp = tab + 2 * (size_t)ks, *d2 = tab + 3 * (size_t)ks;
  const size_t lv = (size_t)pitch, o = (size_t)blockIdx.y * (size_t)ks * lv + (size_t)(a - 1);
  const size_t sc = (size_t)L.so + (size_t)(as - 1);
  const double miss = (double)0.01f;
  auto raw = [&](int k) {                                       // tin(k) before the copy from above; k is 0-based
    const size_t q = (size_t)k * (size_t)L.sp + sc;
    const double v = ztl_raw(L.src, L.fmt, q), vl = ztl_raw(L.src, L.fmt, q - 1), vh = ztl_raw(L.src, L.fmt, q + 1);
    // amax1(tb(i-1,j,k), tb(i+1,j,k), tb(i,j-1,k), tb(i,j+1,k)): along j the first two are the point's own value, along i the last two
    const double n0 = alongj ? v : vl, n1 = alongj ? v : vh, n2 = alongj ? vl : v, n3 = alongj ? vh : v;
    double m = n0;
    m = n1 > m ? n1 : m;
    m = n2 > m ? n2 : m;
    m = n3 > m ? n3 : m;
    return (xs[k] <= hc && v < miss) ? (double)(float)m : v;
  };
  double y0 = raw(0), y1 = raw(1), up = 0.;
  if (y1 < miss) y1 = y0;
  wa[o] = y0;
  wb[o] = 0.;
  for (int n = 1; n < ks - 1; n++) {
    double yn = raw(n + 1);
    if (yn < miss) yn = y1;
    const double u = ((double)6.f * ((yn - y1) / (xs[n + 1] - xs[n]) - (y1 - y0) / (xs[n] - xs[n - 1])) / (xs[n + 1] - xs[n - 1]) - sg[n] * up) / pp[n];
    wa[(size_t)n * lv + o] = y1;
    wb[(size_t)n * lv + o] = u;
    up = u; y0 = y1; y1 = yn;
  }
  wa[(size_t)(ks - 1) * lv + o] = y1;
  const double qn = (double)0.f, un = 0.;
  double y2 = (un - qn * up) / (qn * d2[ks - 2] + (double)1.f);
  wb[(size_t)(ks - 1) * lv + o] = y2;
  for (int k = ks - 2; k >= 0; k--) {
    y2 = d2[k] * y2 + wb[(size_t)k * lv + o];
    wb[(size_t)k * lv + o] = y2;
  }
  for (int k = 1; k <= P.kb; k++) {
    const double x = -F1(zz, k) * hc;
    int klo = 1, khi = ks;
    while (khi - klo > 1) {
      const int kk = (khi + klo) / 2;
      if (xs[kk - 1] > x) khi = kk; else klo = kk;
    }
    const double xl = xs[klo - 1], xh = xs[khi - 1], hh = xh - xl;
    const double a_ = (xh - x) / hh, b = (x - xl) / hh;
    const size_t ql = (size_t)(klo - 1) * lv + o, qh = (size_t)(khi - 1) * lv + o;
    oc[(size_t)(k - 1) * L.op] = a_ * wa[ql] + b * wa[qh] + ((a_ * a_ * a_ - a_) * wb[ql] + (b * b * b - b) * wb[qh]) * (hh * hh) / (double)6.f;
  }
}
// the lines of `job` (nlines of them; wa, wb: nlines slices of ks * pitch values each), enqueued on c->cur
static void launch_ztosig_lines(pomgpu_ctx *c, const ZtlJob &job, int nlines, const double *tab, double *wa, double *wb, int ks, int pitch) {
  LAUNCH(c, k_ztosig_line, dim3((unsigned)((pitch + 63) / 64), (unsigned)nlines, 1), dim3(64, 1, 1), c->P, job, tab, wa, wb, ks, pitch);
}
// One line on its own (pomgpu_ztosig_line): zs: ks host doubles (vetted); src: host, ks levels of npad + 2 values, point a at a (0-based),
// so that the window points sit at 0 and n + 1; out: host, kb levels of npad values.  Launched as the fetch launches it; synchronous
int launch_ztosig_line(pomgpu_ctx *c, int edge, const double *zs, int ks, const double *src, double *out) {
  const KP &P = c->P;
  const int npad = (edge == 0 || edge == 2) ? P.jml : P.iml;
  const size_t nsrc = (size_t)ks * (npad + 2), nwork = (size_t)ks * npad, nout = (size_t)P.kb * npad;
  std::vector<double> tab(4 * (size_t)ks);
  ztosig_table(zs, ks, tab.data());
  double *dev = NULL;                                            // source, table, tin, u / y2, result
  if (hipMalloc((void **)&dev, (nsrc + tab.size() + 2 * nwork + nout) * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return POMGPU_ENOMEM; }
  double *dtab = dev + nsrc, *wa = dtab + tab.size(), *wb = wa + nwork, *dout = wb + nwork;
  int rc = POMGPU_OK;
  if (hipMemcpyAsync(dev, src, nsrc * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = POMGPU_EHIP;
  if (!rc) {
    ZtlJob job;
    for (int l = 0; l < 4; l++) job.l[l] = ztosig_line_of(P, edge, dout, dev, 0, npad + 2, 1);
    launch_ztosig_lines(c, job, 1, dtab, wa, wb, ks, npad);
    if (hipMemcpyAsync(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = POMGPU_EHIP;
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess) rc = POMGPU_EHIP;
  (void)hipFree(dev);
  return rc;
}

// ---- a cold start from the reference's input files (pomgpu_cold_start) ---------------------------------------------------------------
// initialize.f:24-36 after read_input: initialize_arrays, read_grid (read_grid_pnetcdf io_pnetcdf.F:2085-2263, initialize.f:317-389),
// initial_conditions (read_initial_ts_pnetcdf :2771-2842, read_clim_ts_pnetcdf :2845-2909, initialize.f:392-463), update_initial
// (:466-521) and bottom_friction (:524-544) without PnetCDF.  The headers go through parse_header / ff_check; the data path is the
// restart reader's (raw big-endian bands through two pinned buffers, one staging buffer, kernels behind each copy on a copy stream).
// What needs sin or log (cor, cbc) is formed on the host with libm from the band while it sits in the pinned buffer; dz, dzz likewise.
namespace {
struct CVar { uint32_t type = 0; uint64_t begin = 0; unsigned es = 0; };   // a fixed-size variable of the grid file
struct CPlane { const char *name; int slot; };
const CPlane CS_PLANES[13] = {{"dx", P2_dx}, {"dy", P2_dy}, {"lon_rho", P2_east_e}, {"lat_rho", P2_north_e}, {"lon_u", P2_east_u}, {"lat_u", P2_north_u},
                              {"lon_v", P2_east_v}, {"lat_v", P2_north_v}, {"lon_psi", P2_east_c}, {"lat_psi", P2_north_c}, {"angle", P2_rot}, {"h", P2_h},
                              {"fsm", P2_fsm}};
const char *const CS_INIT[2] = {"T", "S"};
const unsigned CS_REAL = (1u << 5) | (1u << 6), CS_MASK = CS_REAL | (1u << 1) | (1u << 3) | (1u << 4);   // NC_FLOAT NC_DOUBLE / also NC_BYTE NC_SHORT NC_INT
// value q of a raw big-endian array of NetCDF type `type` on the host (the kernels' cold_raw below)
double host_raw(unsigned type, const void *p, size_t q) {
  if (type == 6) { uint64_t u; memcpy(&u, (const char *)p + q * 8, 8); u = __builtin_bswap64(u); double x; memcpy(&x, &u, 8); return x; }
  if (type == 5) { uint32_t u; memcpy(&u, (const char *)p + q * 4, 4); u = __builtin_bswap32(u); float x; memcpy(&x, &u, 4); return (double)x; }
  if (type == 4) { uint32_t u; memcpy(&u, (const char *)p + q * 4, 4); return (double)(int32_t)__builtin_bswap32(u); }
  if (type == 3) { const unsigned char *b = (const unsigned char *)p + q * 2; return (double)(int16_t)(uint16_t)((b[0] << 8) | b[1]); }
  return (double)((const signed char *)p)[q];
}
// `name` as a variable of the lengths `want` (at_least: one dimension of at least want[0]), of a type in `types`, no record variable, inside the file
std::string cold_fixed(const RHeader &H, uint64_t fsize, const char *name, const std::vector<uint64_t> &want, bool at_least, unsigned types, CVar &out) {
  const RVar *v = NULL;
  for (const RVar &x : H.vars) if (x.name == name) { v = &x; break; }
  if (!v) return std::string("variable ") + name + " is absent";
  if (v->type > 6 || !((types >> v->type) & 1u))
    return std::string("variable ") + name + " has NetCDF type " + std::to_string(v->type) + (types == CS_REAL ? ", neither NC_FLOAT (5) nor NC_DOUBLE (6)" : ", none of NC_BYTE (1), NC_SHORT (3), NC_INT (4), NC_FLOAT (5), NC_DOUBLE (6)");
  uint64_t count = 1;
  bool same = v->dimids.size() == want.size();
  for (size_t d = 0; d < v->dimids.size(); d++) {
    const uint64_t len = H.dimlen[v->dimids[d]];
    if (len == 0) return std::string("variable ") + name + " is a record variable (unlimited dimension)";
    if (__builtin_mul_overflow(count, len, &count)) count = UINT64_MAX / 8;
    if (same && (at_least ? len < want[d] : len != want[d])) same = false;
  }
  if (!same) {
    std::string w = at_least ? "(>= " : "(";
    for (size_t d = 0; d < want.size(); d++) w += (d ? ", " : "") + std::to_string(want[d]);
    return std::string("variable ") + name + " has the dimension lengths " + lengths_of(H, *v) + ", wanted " + w + ")";
  }
  out.type = v->type; out.begin = v->begin; out.es = NC_TYPE_BYTES[v->type];
  if (v->begin > fsize || count * out.es > fsize - v->begin)
    return std::string("variable ") + name + " (" + std::to_string(count * out.es) + " bytes at " + std::to_string(v->begin) + ") reaches beyond the file's " + std::to_string(fsize) + " bytes";
  return std::string();
}
}  // namespace

__device__ __forceinline__ double cold_raw(unsigned type, const void *p, size_t q) {
  if (type == 6) return CdfRaw<double>::get(p, q);
  if (type == 5) return CdfRaw<float>::get(p, q);
  if (type == 4) return (double)(int)__builtin_bswap32(((const unsigned *)p)[q]);
  if (type == 3) { const unsigned char *b = (const unsigned char *)p + q * 2; return (double)(short)(unsigned short)((b[0] << 8) | b[1]); }
  return (double)((const signed char *)p)[q];
}
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
  const double x = cold_raw(type, src, (size_t)b * (size_t)pitch + (size_t)(c0 + a));
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
// k_cdf_unpack for either real type: gridDim.z levels of Tclim / Sclim into the mirror (dst: the first of those levels)
template <class T>
__global__ void k_cold_vol(pomgpu_st *dst, const void *src, int im, int jm, int iml, size_t n2, int rows, int pitch, int c0) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x), j = (int)(blockIdx.y * blockDim.y + threadIdx.y), k = (int)blockIdx.z;
  if (i >= im || j >= jm) return;
  dst[(size_t)k * n2 + (size_t)j * iml + i] = (pomgpu_st)CdfRaw<T>::get(src, ((size_t)k * rows + j) * (size_t)pitch + (size_t)(c0 + i));
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
// the z levels of an init (`Level`) or clim (`z`) file: a 1-D NC_FLOAT / NC_DOUBLE variable of 2..300 finite, strictly increasing values
static std::string z_levels(const RHeader &H, const FSource &S, const char *name, std::vector<double> &zs) {
  const RVar *v = NULL;
  for (const RVar &x : H.vars) if (x.name == name) { v = &x; break; }
  if (!v) return std::string("variable ") + name + " (the z levels) is absent";
  if (v->dimids.size() != 1) return std::string("variable ") + name + " has " + std::to_string(v->dimids.size()) + " dimensions, wanted the one of the z levels";
  const uint64_t ks = H.dimlen[v->dimids[0]];
  if (ks < 2 || ks > POMGPU_ZTOSIG_NMAX) return std::string("variable ") + name + " holds " + std::to_string(ks) + " z levels, wanted 2..300";
  CVar cv;
  std::string why = cold_fixed(H, S.fsize, name, {ks}, false, CS_REAL, cv);
  if (!why.empty()) return why;
  std::vector<unsigned char> raw((size_t)ks * cv.es);
  if (pread_all(S.fd, raw.data(), raw.size(), cv.begin)) return std::string("I/O error (") + name + ")";
  zs.resize((size_t)ks);
  for (size_t k = 0; k < ks; k++) {
    zs[k] = host_raw(cv.type, raw.data(), k);
    if (!__builtin_isfinite(zs[k]) || (k && !(zs[k] > zs[k - 1])))
      return std::string("variable ") + name + " is not finite and strictly increasing at level " + std::to_string(k + 1) + " (" + std::to_string(zs[k]) + ")";
  }
  return std::string();
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

extern "C" int pomgpu_cold_start(pomgpu_ctx *c, const char *grid, const char *init, const char *clim, const pomgpu_file_meta *m, pomgpu_cold_info *info) {
  if (!c || !grid || !init || !clim || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  { const int rcw = pomgpu_io_wait(c); if (rcw) return rcw; }  // a file this context is still writing
  const KP &P = c->P;
  if (c->flags & POMGPU_CTX_2D) return fail(c, POMGPU_EINVAL, "cold_start: not on a 2-D context");
  const int wi = P.W ? 0 : 1, wj = P.S ? 0 : 1;                // one more column / row on the low side of a tile with a neighbour there
  const int zin[2] = {c->z_init, c->z_clim};                   // pomgpu_set_z_inputs: T, S / Tclim, Sclim are on z levels and go through ztosig,
  const int we = (zin[0] || zin[1]) && !P.E ? 1 : 0, wn = (zin[0] || zin[1]) && !P.N ? 1 : 0;   // whose fill-in looks at the neighbour on the high side too
  if (m->i0 - wi < 1 || m->j0 - wj < 1 || m->i0 + P.im - 1 + we > m->im_global || m->j0 + P.jm - 1 + wn > m->jm_global)
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
    if (ff_header(F[q].fd, F[q].fsize, H[q], what) < 0) { drop(); return fail(c, POMGPU_EINVAL, "cold_start: %s is not a %s file this library reads: %s", paths[q], kind[q], what.c_str()); }
  }
  auto refuse = [&](int q, const std::string &why) { drop(); return fail(c, POMGPU_EINVAL, "cold_start: %s: %s", paths[q], why.c_str()); };
  // grid
  CVar vz, vzz, vp[13];
  {
    std::string why = cold_fixed(H[0], F[0].fsize, "z", {kb}, true, CS_REAL, vz);
    if (why.empty()) why = cold_fixed(H[0], F[0].fsize, "zz", {kb}, true, CS_REAL, vzz);
    for (int q = 0; q < 13 && why.empty(); q++) why = cold_fixed(H[0], F[0].fsize, CS_PLANES[q].name, {jmg, img}, false, q == 12 ? CS_MASK : CS_REAL, vp[q]);
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
    cor_mid = cor_of(host_raw(vlat.type, raw, 0));
    if (cor_mid == 0.) return refuse(0, "Coriolis problem: cor(im/2, jm/2) of this tile is zero (lat_rho = " + std::to_string(host_raw(vlat.type, raw, 0)) + ")");
  }
  // masks are 0 or 1 (the kernels fold repeated mask multiplies; pomgpu_upload checks the same): the tile's window of fsm, read ahead
  {
    const CVar &vf = vp[12];
    std::vector<unsigned char> row((size_t)(P.im + wi) * vf.es);
    for (int j = 0; j < P.jm + wj; j++) {
      const uint64_t cell = (uint64_t)(m->j0 - 1 - wj + j) * img + (uint64_t)(m->i0 - 1 - wi);
      if (pread_all(F[0].fd, row.data(), row.size(), vf.begin + cell * vf.es)) return refuse(0, "I/O error (fsm)");
      for (int i = 0; i < P.im + wi; i++) {
        const double x = host_raw(vf.type, row.data(), (size_t)i);
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
      for (int k = 0; k < P.kb; k++) x[k] = host_raw(v.type, raw.data(), (size_t)k);
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
  size_t cap = SW(c, IO_CHUNK_KB) && SWV(c, IO_CHUNK_KB) > 0 ? (size_t)SWV(c, IO_CHUNK_KB) << 10 : (size_t)64 << 20;   // bytes per buffer
  if (cap > band3 * (size_t)P.kb) cap = band3 * (size_t)P.kb;
  if (cap < band2) cap = band2;
  const size_t nwin = (size_t)(P.im + 1) * (size_t)(P.jm + 1);
  unsigned char *pin[2] = {NULL, NULL}, *stage = NULL;
  double *win = NULL;                                            // dx, dy, fsm over the window
  if (!bad && hipMalloc((void **)&win, 3 * nwin * sizeof(double)) != hipSuccess) bad = 2;
  // z-level input: the window of one variable as doubles, ztosig's two work arrays and the table of either file (cdf_out.hip's end)
  const int wim = P.im + wi + we, wjm = P.jm + wj + wn;
  const size_t ksz[2] = {zlev[0].size(), zlev[1].size()}, ksmax = ksz[0] > ksz[1] ? ksz[0] : ksz[1];
  const size_t zwin = ksmax * (size_t)wim * (size_t)wjm, zwork = ksmax * P.n2;
  double *zdev = NULL;
  std::vector<double> ztab[2];
  if (!bad && ksmax && hipMalloc((void **)&zdev, (zwin + 2 * zwork + 8 * ksmax) * sizeof(double)) != hipSuccess) bad = 2;
  for (int q = 0; q < 2 && !bad; q++) {
    if (!ksz[q]) continue;
    ztab[q].resize(4 * ksz[q]);
    ztosig_table(zlev[q].data(), (int)ksz[q], ztab[q].data());
    if (hipMemcpyAsync(zdev + zwin + 2 * zwork + (size_t)q * 4 * ksmax, ztab[q].data(), ztab[q].size() * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) bad = 2;
  }
#ifdef POMGPU_EMU
  if (!bad && hipMalloc((void **)&pin[0], cap) != hipSuccess) bad = 2;
  stage = pin[0];
  hipStream_t rs = c->stream;
#else
  hipStream_t rs = NULL;
  hipEvent_t ev[2] = {NULL, NULL};                              // the copy out of pin[b] has completed
  if (!bad && (hipHostMalloc((void **)&pin[0], cap, hipHostMallocDefault) != hipSuccess || hipHostMalloc((void **)&pin[1], cap, hipHostMallocDefault) != hipSuccess ||
               hipMalloc((void **)&stage, cap) != hipSuccess || hipStreamCreateWithFlags(&rs, hipStreamNonBlocking) != hipSuccess ||
               hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) != hipSuccess))
    bad = 2;
  int used[2] = {0, 0};
#endif
  if (hipStreamSynchronize(c->stream) != hipSuccess && !bad) bad = 2;   // the zeroes precede the first store of the copy stream
  const hipStream_t cur0 = c->cur;
  c->cur = rs;
  int b = 0;
  // nl bands of `bytes` each, `stride` bytes apart in the file, into the free pinned buffer and on their way to the staging buffer
  auto fetch = [&](int fd, uint64_t first, size_t bytes, uint64_t stride, int nl) {
#ifndef POMGPU_EMU
    if (used[b] && hipEventSynchronize(ev[b]) != hipSuccess) { bad = 2; return; }
#endif
    if (stride == bytes) { if (pread_all(fd, pin[b], (size_t)nl * bytes, first)) bad = 1; }
    else for (int k = 0; k < nl && !bad; k++) if (pread_all(fd, pin[b] + (size_t)k * bytes, bytes, first + (uint64_t)k * stride)) bad = 1;
#ifndef POMGPU_EMU
    if (!bad && (hipMemcpyAsync(stage, pin[b], (size_t)nl * bytes, hipMemcpyHostToDevice, rs) != hipSuccess || hipEventRecord(ev[b], rs) != hipSuccess)) bad = 2;
    if (!bad) used[b] = 1;
#endif
  };
  auto flip = [&]() {
#ifndef POMGPU_EMU
    b ^= 1;
#endif
  };
  const int c0 = m->i0 - 1 - wi;                                 // the file column (0-based) of the window's first
  for (int q = 0; q < 13 && !bad; q++) {                         // the planes of the grid file, rows j0-wj .. j0+jm-1
    const CVar &v = vp[q];
    const size_t bytes = (size_t)(P.jm + wj) * (size_t)img * v.es;
    fetch(F[0].fd, v.begin + (uint64_t)(m->j0 - 1 - wj) * img * v.es, bytes, bytes, 1);
    if (bad) break;
    if (&v == &vlat || &v == &vh) {                              // cor (initialize.f:349) and cbc (:536-540) on the host, from the band in the pinned buffer
      const double zk = 1. + b1[(size_t)P1_zz * P.kb + (P.kbm1 - 1)];
      for (int j = 0; j < P.jm; j++)
        for (int i = 0; i < P.im; i++) {
          const double x = host_raw(v.type, pin[b], (size_t)(j + wj) * (size_t)img + (size_t)(m->i0 - 1 + i));
          if (&v == &vlat) hcor[(size_t)j * P.iml + i] = cor_of(x);
          else {
            const double t = c->con.kappa / log(zk * x / c->con.z0b), cb = t * t;
            hcbc[(size_t)j * P.iml + i] = fmin(c->con.cbcmax, fmax(c->con.cbcmin, cb));
          }
        }
    }
    double *w = q == 0 ? win : (q == 1 ? win + nwin : (q == 12 ? win + 2 * nwin : NULL));
    LAUNCH(c, k_cold_plane, dim3((unsigned)((P.im + wi + 63) / 64), (unsigned)((P.jm + wj + 3) / 4), 1), blk2(), P.b2 + (size_t)CS_PLANES[q].slot * P.n2, w, (const void *)stage,
           (unsigned)v.type, P.im, P.jm, P.iml, wi, wj, (int)img, c0);
    flip();
  }
  for (int q = 0; q < 4 && !bad; q++) {                          // T, S (record 1, levels 1..kbm1), Tclim, Sclim (record 10, kb levels)
    const bool ini = q < 2;
    const FVar &f = ini ? F[1].v[q] : F[2].v[q - 2];
    const int onz = zin[ini ? 0 : 1];                            // all ks levels over the window, then ztosig; else the sigma levels over the tile
    const int zq = ini ? 0 : 1, nlv = onz ? (int)ksz[zq] : (ini ? P.kbm1 : P.kb), rows = onz ? wjm : P.jm;
    const size_t bytes = (size_t)rows * (size_t)img * f.esize();
    const uint64_t stride = jmg * img * f.esize();
    const uint64_t base = f.begin + (ini ? 0 : 9 * f.stride) + (uint64_t)(m->j0 - 1 - (onz ? wj : 0)) * img * f.esize();
    int per = (int)(cap / bytes);
    if (per > nlv) per = nlv;
    for (int k0 = 0; k0 < nlv && !bad; k0 += per) {
      const int nl = nlv - k0 < per ? nlv - k0 : per;
      fetch(ini ? F[1].fd : F[2].fd, base + (uint64_t)k0 * stride, bytes, stride, nl);
      if (bad) break;
      const dim3 g((unsigned)((P.im + 63) / 64), (unsigned)((P.jm + 3) / 4), (unsigned)nl);
      if (onz) {
        const dim3 gw((unsigned)((wim + 63) / 64), (unsigned)((wjm + 3) / 4), (unsigned)nl);
        if (f.type == 5) LAUNCHN(c, "k_rst_unpack", k_rst_unpack<float>, gw, blk2(), zdev, (const void *)stage, wim, wjm, wjm, (int)img, c0, k0);
        else LAUNCHN(c, "k_rst_unpack", k_rst_unpack<double>, gw, blk2(), zdev, (const void *)stage, wim, wjm, wjm, (int)img, c0, k0);
      } else if (ini) {
        if (f.type == 5) LAUNCHN(c, "k_cold_ts", k_cold_ts<float>, g, blk2(), P, q, (const void *)stage, P.jm, (int)img, m->i0 - 1, k0);
        else LAUNCHN(c, "k_cold_ts", k_cold_ts<double>, g, blk2(), P, q, (const void *)stage, P.jm, (int)img, m->i0 - 1, k0);
      } else {
        pomgpu_st *dst = (pomgpu_st *)(P.b3 + (size_t)(q == 2 ? P3_tclim : P3_sclim) * P.a3) + (size_t)k0 * P.n2;
        if (f.type == 5) LAUNCHN(c, "k_cold_vol", k_cold_vol<float>, g, blk2(), dst, (const void *)stage, P.im, P.jm, P.iml, P.n2, P.jm, (int)img, m->i0 - 1);
        else LAUNCHN(c, "k_cold_vol", k_cold_vol<double>, g, blk2(), dst, (const void *)stage, P.im, P.jm, P.iml, P.n2, P.jm, (int)img, m->i0 - 1);
      }
      flip();
    }
    if (onz && !bad) {
      double *t = P.b3 + (size_t)(q == 0 ? P3_tb : (q == 1 ? P3_sb : (q == 2 ? P3_tclim : P3_sclim))) * P.a3;
      launch_ztosig_window(c, t, 0, zdev, zdev + zwin + 2 * zwork + (size_t)zq * 4 * ksmax, zdev + zwin, zdev + zwin + zwork, nlv, wi, we, wj, wn);
      if (ini) LAUNCH(c, k_cold_zts, grid3(P, P.kb), blk2(), P, q);
    }
  }
  c->cur = cur0;
  if (hipStreamSynchronize(rs) != hipSuccess && !bad) bad = 2;
#ifndef POMGPU_EMU
  if (ev[0]) (void)hipEventDestroy(ev[0]);
  if (ev[1]) (void)hipEventDestroy(ev[1]);
  if (rs) (void)hipStreamDestroy(rs);
  if (pin[0]) (void)hipHostFree(pin[0]);
  if (pin[1]) (void)hipHostFree(pin[1]);
  if (stage) (void)hipFree(stage);
#else
  (void)hipFree(pin[0]);
#endif
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
  if (zdev) (void)hipFree(zdev);
  if (bad || c->launch_err) {
    if (bad == 2) (void)hipGetLastError();
    return fail(c, bad == 1 ? POMGPU_EINVAL : POMGPU_EHIP, bad == 1 ? "cold_start: I/O error on %s, %s or %s (the state is unspecified)" : "cold_start: a HIP call failed while reading %s, %s or %s (the state is unspecified)", grid, init, clim);
  }
  if (info) { info->cflmin = cflmin; info->period = c->con.period; }
  return POMGPU_OK;
}
