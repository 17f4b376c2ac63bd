// cdf_io.hpp -- what the units that read NetCDF classic files share (cdf_in.hip, frc_files.hip, ztosig.hip; cdf_out.hip for the tile check).
// The first part is plain C++ -- the header parser, the variable checker, the band preads -- and is all a host program sees that defines
// CDF_IO_HOST_ONLY (tools/check_cdf_header.cpp); the second part needs pomgpu_internal.hpp: the raw-value decoder, the unpack kernel, the
// pinned two-buffer band reader, the level-run loop, the z-level window and the declarations that cross the units.
#pragma once
#include <unistd.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

// ---- the header of a classic file (CDF-1 or CDF-2), parsed as it stands: dimension list, attributes skipped, every variable's type,
// dimension ids and `begin`.  A file written by PnetCDF itself aligns its data section differently from this library's writer and may hold
// its variables in another order, so readers find variables by name and check everything before they change anything.
struct RVar { std::string name; std::vector<uint32_t> dimids; uint32_t type = 0; uint64_t begin = 0; };
struct RHeader { std::vector<uint64_t> dimlen; std::vector<RVar> vars; uint32_t numrecs = 0; };   // numrecs: records written so far (the forcing files)
struct Cur {                                                    // big-endian cursor over the bytes read so far
  const unsigned char *p; size_t n, at = 0; bool shortfall = false;
  bool need(size_t k) { if (k > n - at) { shortfall = true; return false; } return true; }
  uint32_t u32() { if (!need(4)) return 0; uint32_t v = 0; for (int q = 0; q < 4; q++) v = (v << 8) | p[at + q]; at += 4; return v; }
  uint64_t u64() { if (!need(8)) return 0; uint64_t v = 0; for (int q = 0; q < 8; q++) v = (v << 8) | p[at + q]; at += 8; return v; }
  void skip(uint64_t k) { k = (k + 3) & ~(uint64_t)3; if (need(k)) at += k; }
  std::string name() { const uint32_t len = u32(); std::string s; if (need(((size_t)len + 3) & ~(size_t)3)) { s.assign((const char *)p + at, len); at += ((size_t)len + 3) & ~(size_t)3; } return s; }
};
static const unsigned NC_TYPE_BYTES[7] = {0, 1, 1, 2, 4, 4, 8};   // byte, char, short, int, float, double
// 0 = parsed, 1 = more bytes needed, -1 = not a classic header (why: `what`)
static inline int parse_atts(Cur &c, std::string &what) {
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
static inline int parse_header(const unsigned char *buf, size_t n, RHeader &H, std::string &what) {
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
static inline std::string lengths_of(const RHeader &H, const RVar &v) {
  std::string s = "(";
  for (size_t d = 0; d < v.dimids.size(); d++) { if (d) s += ", "; const uint64_t len = H.dimlen[v.dimids[d]]; s += len ? std::to_string(len) : std::string("unlimited"); }
  return s + ")";
}
static inline int pread_all(int fd, void *buf, size_t n, uint64_t off) {
  char *p = (char *)buf;
  while (n) { const ssize_t r = pread(fd, p, n, (off_t)off); if (r <= 0) return -1; p += r; off += (uint64_t)r; n -= (size_t)r; }
  return 0;
}
// nl bands of `bytes` each, `stride` bytes apart in the file from `first`, back to back into dst: one pread where the bands touch
static inline int read_bands(int fd, unsigned char *dst, uint64_t first, size_t bytes, uint64_t stride, int nl) {
  if (stride == bytes) return pread_all(fd, dst, (size_t)nl * bytes, first);
  for (int k = 0; k < nl; k++) if (pread_all(fd, dst + (size_t)k * bytes, bytes, first + (uint64_t)k * stride)) return -1;
  return 0;
}
// the header of `fd`, whole, read in growing prefixes: 0 = parsed, -1 = refused, -2 = I/O error (why: `what`)
static inline int read_header(int fd, uint64_t fsize, RHeader &H, std::string &what) {
  std::vector<unsigned char> hb;
  int rc = 1;
  for (size_t want = 1 << 16; rc == 1; want *= 4) {
    const size_t n = (size_t)(want < fsize ? want : fsize);
    hb.resize(n);
    if (n && pread_all(fd, hb.data(), n, 0)) { what = "I/O error (header)"; return -2; }
    rc = parse_header(hb.data(), n, H, what);
    if (rc == 1 && n == fsize) { what = fsize ? "the file ends inside its header" : "the file is empty"; rc = -1; }
  }
  return rc;
}

// ---- one named variable against what its reader asks for.  Empty string = accepted, *out set; else the refusal's text.
const unsigned NC_ONLY_DOUBLE = 1u << 6, NC_REAL = (1u << 5) | (1u << 6), NC_NUMBER = NC_REAL | (1u << 1) | (1u << 3) | (1u << 4);   // also NC_BYTE NC_SHORT NC_INT
struct VarWant {
  enum How { EXACT, AT_LEAST, ONE_VALUE };                      // ONE_VALUE: a scalar or any number of dimensions of length 1
  unsigned types;                                               // bit t: the NetCDF type t is accepted
  std::vector<uint64_t> len;                                    // the wanted dimension lengths, slowest first (behind the record dimension, if rec)
  How how;
  bool whole;                                                   // one block inside the file: no unlimited dimension, begin + size <= fsize
  bool rec;                                                     // a leading record dimension: the unlimited one, or a fixed one of at least min_rec
  uint64_t min_rec;
  const char *open;                                             // how the message opens the wanted lengths, where the mode's own is not it
  // one block of these lengths inside the file (the restart, grid and level variables)
  static VarWant fixed(unsigned types, std::vector<uint64_t> len, How how = EXACT) { return VarWant{types, std::move(len), how, true, false, 1, NULL}; }
  // these lengths behind a leading record dimension; where the records lie in the file is the caller's to check (ff_check)
  static VarWant record(unsigned types, std::vector<uint64_t> len, uint64_t min_rec) { return VarWant{types, std::move(len), EXACT, false, true, min_rec, NULL}; }
  // these lengths and nothing else: an unlimited dimension is a wrong length, the file's end is the caller's to check (the rate file)
  static VarWant shape(unsigned types, std::vector<uint64_t> len, const char *open) { return VarWant{types, std::move(len), EXACT, false, false, 1, open}; }
};
// ", not NC_DOUBLE (6)" / ", neither A nor B" / ", none of A, B, C": the accepted types of a mask, as a refusal names them
static inline std::string type_names(unsigned types) {
  static const char *const NAME[7] = {"", "NC_BYTE (1)", "NC_CHAR (2)", "NC_SHORT (3)", "NC_INT (4)", "NC_FLOAT (5)", "NC_DOUBLE (6)"};
  std::vector<const char *> n;
  for (int t = 1; t <= 6; t++) if ((types >> t) & 1u) n.push_back(NAME[t]);
  if (n.size() == 1) return std::string(", not ") + n[0];
  if (n.size() == 2) return std::string(", neither ") + n[0] + " nor " + n[1];
  std::string s = ", none of ";
  for (size_t q = 0; q < n.size(); q++) s += std::string(q ? ", " : "") + n[q];
  return s;
}
static inline const RVar *find_var(const RHeader &H, const char *name) { for (const RVar &v : H.vars) if (v.name == name) return &v; return NULL; }
static inline std::string check_var(const RHeader &H, uint64_t fsize, const char *name, const VarWant &w, const RVar **out) {
  const std::string var = std::string("variable ") + name;
  const RVar *v = find_var(H, name);
  if (!v) return var + " is absent";
  if (v->type > 6 || !((w.types >> v->type) & 1u))
    return var + " has NetCDF type " + std::to_string(v->type) + type_names(w.types);
  const size_t lead = w.rec ? 1 : 0;
  uint64_t count = 1;
  bool same = v->dimids.size() == w.len.size() + lead;
  for (size_t d = 0; d < v->dimids.size(); d++) {
    const uint64_t len = H.dimlen[v->dimids[d]];
    if (w.whole && len == 0) return var + " is a record variable (unlimited dimension)";
    if (__builtin_mul_overflow(count, len, &count)) count = UINT64_MAX / 8;   // a hostile header: saturate, the checks below refuse it
    if (!same) continue;
    if (d < lead) same = len == 0 || len >= w.min_rec;
    else same = w.how == VarWant::AT_LEAST ? len >= w.len[d - lead] : len == w.len[d - lead];
  }
  if (w.how == VarWant::ONE_VALUE ? count != 1 : !same) {
    std::string t = w.open ? w.open : (w.rec ? (w.min_rec > 1 ? "(>= " + std::to_string(w.min_rec) : std::string("(records")) : std::string(w.how == VarWant::AT_LEAST ? "(>= " : "("));
    for (size_t d = 0; d < w.len.size(); d++) t += (d || w.rec ? ", " : "") + std::to_string(w.len[d]);
    return var + " has the dimension lengths " + lengths_of(H, *v) + ", wanted " + (w.how == VarWant::ONE_VALUE ? std::string("one value") : t + ")");
  }
  const uint64_t bytes = count * NC_TYPE_BYTES[v->type];
  if (w.whole && (v->begin > fsize || bytes > fsize - v->begin))
    return var + " (" + std::to_string(bytes) + " bytes at " + std::to_string(v->begin) + ") reaches beyond the file's " + std::to_string(fsize) + " bytes";
  *out = v;
  return std::string();
}

#ifndef CDF_IO_HOST_ONLY
#include "pomgpu.h"
#include "pomgpu_internal.hpp"

// the tile with wi, we, wj, wn more lines towards its west, east, south, north neighbour lies inside the global grid
static inline bool tile_fits(const pomgpu_file_meta *m, const KP &P, int wi, int we, int wj, int wn) {
  return m->i0 - wi >= 1 && m->j0 - wj >= 1 && m->i0 + P.im - 1 + we <= m->im_global && m->j0 + P.jm - 1 + wn <= m->jm_global;
}

// ---- one raw big-endian value: the compile-time form for the kernels with one real type per launch, cdf_raw for the five number types.
// A kernel's source is aligned to its type (the staging buffer, bands of whole values) and is read with one typed load; host code may
// hand in any address.
template <class U> static __host__ __device__ __forceinline__ U raw_load(const void *p, size_t q) {
#ifdef __HIP_DEVICE_COMPILE__
  return ((const U *)p)[q];
#else
  U u;
  __builtin_memcpy(&u, (const char *)p + q * sizeof(U), sizeof(U));
  return u;
#endif
}
template <class T> struct CdfRaw;
template <> struct CdfRaw<float> {
  static __host__ __device__ __forceinline__ double get(const void *p, size_t q) {
    const unsigned u = __builtin_bswap32(raw_load<unsigned>(p, q));
    float x;
    __builtin_memcpy(&x, &u, 4);
    return (double)x;                                           // exact, what get_vara_double does with an NC_FLOAT variable
  }
};
template <> struct CdfRaw<double> {
  static __host__ __device__ __forceinline__ double get(const void *p, size_t q) {
    const unsigned long long u = __builtin_bswap64(raw_load<unsigned long long>(p, q));
    double x;
    __builtin_memcpy(&x, &u, 8);
    return x;
  }
};
// value q of an array of NetCDF type `type`, on the host and in the kernels
static __host__ __device__ __forceinline__ double cdf_raw(unsigned type, const void *p, size_t q) {
  if (type == 6) return CdfRaw<double>::get(p, q);
  if (type == 5) return CdfRaw<float>::get(p, q);
  if (type == 4) return (double)(int)__builtin_bswap32(raw_load<unsigned>(p, q));
  if (type == 3) { const unsigned char *b = (const unsigned char *)p + q * 2; return (double)(short)(unsigned short)((b[0] << 8) | b[1]); }
  return (double)((const signed char *)p)[q];
}

// ---- the unpack kernel: gridDim.z levels of a band (raw values in `src`, `rows` rows per level, `pitch` values per row, the first wanted
// column at c0) into dst, dl values per level and dp per row.  One lane, one value: threadIdx.x runs along i, so a wavefront loads a
// contiguous piece of a file row and stores a contiguous piece of the destination's row, rounded to TDst as an upload rounds
// (pomgpu_st: the mirrors of blk3d; double: blk2d, the restore record, a z-level window).
template <class TSrc, class TDst>
__global__ void k_cdf_unpack(TDst *dst, const void *src, int im, int jm, size_t dl, int dp, int rows, int pitch, int c0) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x), j = (int)(blockIdx.y * blockDim.y + threadIdx.y), k = (int)blockIdx.z;
  if (i >= im || j >= jm) return;
  dst[(size_t)k * dl + (size_t)j * dp + i] = (TDst)CdfRaw<TSrc>::get(src, ((size_t)k * rows + j) * (size_t)pitch + (size_t)(c0 + i));
}
// nl levels of im x jm values of the NetCDF real type `type` (5 or 6, checked with the header); `label`: the call site's name in a profile
template <class TDst>
static inline void launch_cdf_unpack(pomgpu_ctx *c, const char *label, unsigned type, TDst *dst, const void *src, int im, int jm, int nl, size_t dl, int dp, int rows, int pitch, int c0) {
  const dim3 grid((unsigned)((im + 63) / 64), (unsigned)((jm + 3) / 4), (unsigned)nl);
  if (type == 5) LAUNCHN(c, label, (k_cdf_unpack<float, TDst>), grid, blk2(), dst, src, im, jm, dl, dp, rows, pitch, c0);
  else LAUNCHN(c, label, (k_cdf_unpack<double, TDst>), grid, blk2(), dst, src, im, jm, dl, dp, rows, pitch, c0);
}

// ---- raw bytes on their way to the device: two pinned buffers filled in turn, one device buffer their copies land in, an event per
// pinned buffer (the copy out of it has completed).  Copies and the kernels behind them go to c->cur.  Two lifetimes: one call with a
// copy stream of its own (open .. release: the restart and cold-start readers, which put c->cur on that stream) and the context's
// (reserve, growing; the forcing files, on whatever stream the step is enqueued on).  The host emulation has one buffer and no copy.
struct BandReader {
  unsigned char *pin[2] = {NULL, NULL}, *stage = NULL;
  size_t cap = 0;                                               // bytes of each
  hipStream_t own = NULL;
  int b = 0;
#ifndef POMGPU_EMU
  hipEvent_t ev[2] = {NULL, NULL};
  int used[2] = {0, 0};
#endif
  void drop() {
#ifndef POMGPU_EMU
    for (int q = 0; q < 2; q++) { if (pin[q]) (void)hipHostFree(pin[q]); pin[q] = NULL; used[q] = 0; }
    if (stage) (void)hipFree(stage);
#else
    if (pin[0]) (void)hipFree(pin[0]);
    pin[0] = NULL;
#endif
    stage = NULL;
    cap = 0;
  }
  // buffers of at least `need` bytes each; the caller has seen to it that no copy out of the old ones is in flight.  1 = a HIP call failed
  int reserve(size_t need) {
    if (cap >= need) return 0;
    drop();
#ifndef POMGPU_EMU
    if (hipHostMalloc((void **)&pin[0], need, hipHostMallocDefault) != hipSuccess || hipHostMalloc((void **)&pin[1], need, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&stage, need) != hipSuccess) return 1;
    for (int q = 0; q < 2; q++) if (!ev[q] && hipEventCreateWithFlags(&ev[q], hipEventDisableTiming) != hipSuccess) return 1;
#else
    if (hipMalloc((void **)&pin[0], need) != hipSuccess) return 1;
    stage = pin[0];
#endif
    cap = need;
    return 0;
  }
  // for one call: the buffers and a non-blocking stream for the caller to put c->cur on (the emulation: the context's stream)
  int open(pomgpu_ctx *c, size_t need) {
#ifndef POMGPU_EMU
    return reserve(need) || hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess;
#else
    own = c->stream;
    return reserve(need);
#endif
  }
  // the pinned buffer free for the next preads, once the copy of its last run has left it; NULL = a HIP call failed
  unsigned char *acquire() {
#ifndef POMGPU_EMU
    if (used[b] && hipEventSynchronize(ev[b]) != hipSuccess) return NULL;
#endif
    return pin[b];
  }
  // the acquired buffer's first `bytes` to `stage`, in stream order behind the kernels that read the last run; the host may go on READING
  // the pinned bytes until it acquires this buffer again.  1 = a HIP call failed
  int send(pomgpu_ctx *c, size_t bytes) {
#ifndef POMGPU_EMU
    if (hipMemcpyAsync(stage, pin[b], bytes, hipMemcpyHostToDevice, c->cur) != hipSuccess || hipEventRecord(ev[b], c->cur) != hipSuccess) return 1;
    used[b] = 1;
    b ^= 1;
#else
    (void)c; (void)bytes;
#endif
    return 0;
  }
  void release() {
#ifndef POMGPU_EMU
    for (int q = 0; q < 2; q++) { if (ev[q]) (void)hipEventDestroy(ev[q]); ev[q] = NULL; }
    if (own) (void)hipStreamDestroy(own);
#endif
    own = NULL;
    drop();
  }
};
// bytes of a run of whole levels: the switch IO_CHUNK_KB (64 MiB without it), at most `hi`, at least `lo` (one level's band)
static inline size_t io_run_bytes(pomgpu_ctx *c, size_t lo, size_t hi) {
  size_t run = SW(c, IO_CHUNK_KB) && SWV(c, IO_CHUNK_KB) > 0 ? (size_t)SWV(c, IO_CHUNK_KB) << 10 : (size_t)64 << 20;
  if (run > hi) run = hi;
  return run < lo ? lo : run;
}
// nlev levels, one band of `bytes` each and `stride` bytes apart in the file from `first`, in runs of as many whole levels as a buffer
// holds: preads, the copy, then launch(k0, nl) for the levels k0 .. k0+nl-1 now on their way to R.stage.  0, 1 = I/O error, 2 = a HIP call failed
template <class Launch>
static inline int read_levels(pomgpu_ctx *c, BandReader &R, int fd, uint64_t first, size_t bytes, uint64_t stride, int nlev, Launch launch) {
  const int per = (int)(R.cap / bytes) < nlev ? (int)(R.cap / bytes) : nlev;
  for (int k0 = 0; k0 < nlev; k0 += per) {
    const int nl = nlev - k0 < per ? nlev - k0 : per;
    unsigned char *pin = R.acquire();
    if (!pin) return 2;
    if (read_bands(fd, pin, first + (uint64_t)k0 * stride, bytes, stride, nl)) return 1;
    if (R.send(c, (size_t)nl * bytes)) return 2;
    launch(k0, nl);
  }
  return 0;
}

// ---- a source on z levels as ztosig sees it (ztosig.hip): the tile's WINDOW -- wi, we, wj, wn more lines towards the west, east,
// south, north neighbour, because the fill-in looks at all four -- of one variable as doubles, ztosig's two work arrays and its table,
// in one allocation.  Cold start maps two files with level sets of their own through one window: table q, ks[q] levels.
struct ZWindow {
  int ks[2] = {0, 0}, wi = 0, we = 0, wj = 0, wn = 0;
  double *dev = NULL;
  size_t nwin = 0, nwork = 0;                                   // values of the window / of one work array, at the larger ks
  std::vector<double> host_tab;                                 // the tables as uploaded (the copy is asynchronous)
  int kmax() const { return ks[0] > ks[1] ? ks[0] : ks[1]; }
  int rows(const KP &P) const { return P.jm + wj + wn; }
  int cols(const KP &P) const { return P.im + wi + we; }
  double *win() const { return dev; }
  double *wa() const { return dev + nwin; }
  double *wb() const { return dev + nwin + nwork; }
  const double *tab(int q) const { return dev + nwin + 2 * nwork + (size_t)q * 4 * (size_t)kmax(); }
  // the allocation and the tables of zs0 (and zs1; empty: none) enqueued on c->stream; 1 = a HIP call failed (nothing is kept)
  int alloc(pomgpu_ctx *c, int wi_, int we_, int wj_, int wn_, const std::vector<double> &zs0, const std::vector<double> &zs1 = std::vector<double>());
  void free() { if (dev) (void)hipFree(dev); dev = NULL; }
};

// ---- what crosses the units
struct FVar {                                                   // one variable a record reader asks for, as the header describes it
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
extern const char *const FF_CLIM[2];
// frc_files.hip: one source's record variables against what its reader asks for: `want[q]` = the dimension lengths after the record dimension;
// min_rec: records a fixed first dimension must at least have.  Empty string = accepted, S.v filled
std::string ff_check(const RHeader &H, FSource &S, const char *const *names, const std::vector<std::vector<uint64_t>> &want, uint64_t min_rec);
// ztosig.hip
#define POMGPU_ZTOSIG_NMAX 300
// the z levels of an init (`Level`) or clim, lbry, rate (`z`) file: a 1-D NC_FLOAT / NC_DOUBLE variable of 2..300 finite, strictly increasing values
std::string z_levels(const RHeader &H, const FSource &S, const char *name, std::vector<double> &zs);
void ztosig_table(const double *zs, int ks, double *tab);
// every cell of (1:im, 1:jm) from the window Z holds, with table q; record = 0: `out` is a mirror; 1: the (im, jm, kb) restore record
void launch_ztosig_window(pomgpu_ctx *c, double *out, int record, const ZWindow &Z, int q);
// the lines of an lbry file on z levels
struct ZtlLine { double *out; const void *src; int fmt, edge, n, npad, lo, hi, sp, so, op; };
struct ZtlJob { ZtlLine l[8]; };                                // temp, salt of up to four sides
ZtlLine ztosig_line_of(const KP &P, int edge, double *out, const void *src, int fmt, int sp, int so);
void launch_ztosig_lines(pomgpu_ctx *c, const ZtlJob &job, int nlines, const double *tab, double *wa, double *wb, int ks, int pitch);
#endif
