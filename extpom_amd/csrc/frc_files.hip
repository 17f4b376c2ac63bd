// frc_files.hip -- forcing records from the files (pomgpu_set_forcing_files, pomgpu_set_restore_rate_file, pomgpu_set_water_files).
// read_wind_pnetcdf, read_heat_pnetcdf, read_surface_pnetcdf (io_pnetcdf.F:2912-2998, :3110-3224), read_boundary_conditions_pnetcdf
// (:3393-3621) and read_restore_ts_interior_pnetcdf (:3275-3333) without PnetCDF.  The host names the files once; the schedule code of
// pomgpu_api.hip (frc_read, lat_read, restore_prepare) asks for record n when the step needs it, and the fetch below puts it where
// the setter of the same record would have put it: the tile's band of raw big-endian values with pread into a pinned buffer, one copy
// to the device on the stream the step is being enqueued on, and a kernel that swaps bytes, widens, converts units, tapers the wind
// and scatters.  Nothing here waits for the device but the reuse of a pinned buffer (an event per buffer).
#include <fcntl.h>
#include <sys/stat.h>

#include "cdf_io.hpp"
#define fail pomgpu_fail

struct FFiles {
  FSource s[4];                                                 // sfrc, lbry, clim; [3]: the restore rate (pomgpu_set_restore_rate_file)
  int im_global = 0, jm_global = 0, i0 = 1, j0 = 1;
  BandReader rd;                                                // sized at registration, never inside a step; copies on c->cur
  ZWindow z;                                                    // a clim file on z levels (pomgpu_set_z_inputs); z.ks[0] = 0: it is on the sigma levels
  // the lbry file's sides that are ON (pomgpu_set_lateral_sides, as registered) and what s[1].v[j] is: lq[j], LatSrc's number, lnv of them
  int lsides = 0, lnv = 0, lq[20];
  // an lbry file on z levels (pomgpu_set_z_lateral): its level count, the window points of the east and west lines (lwj, lwn: towards the
  // south, north neighbour) and of the south and north lines (lwi, lwe), and one allocation: ztosig's table, then the two work arrays of
  // eight lines (temp, salt of four sides)
  int lks = 0, lwi = 0, lwe = 0, lwj = 0, lwn = 0;
  double *ldev = NULL;
  // the rate file: `tau` on the levels of its `z`, always through ztosig; rsteady: it holds one record (or has no record dimension), which
  // serves every record number
  ZWindow r;
  int rsteady = 0;
  // the water files (pomgpu_set_water_files): record n is the ONE record of <wprefix>.water.NNNN.nc, opened when the schedule asks for it
  std::string wprefix;
  int won = 0;
};
static const char *const FF_WHAT[3] = {"sfrc", "lbry", "clim"};
static const char *const FF_SFRC[6] = {"sustr", "svstr", "shflux", "swrad", "SST", "SSS"};
static const char *const FF_LBRY[20] = {"zeta.east",  "u.east",  "v.east",  "temp.east",  "salt.east",  "zeta.south", "u.south", "v.south", "temp.south", "salt.south",   // LatSrc's numbers
                                        "zeta.west",  "u.west",  "v.west",  "temp.west",  "salt.west",  "zeta.north", "u.north", "v.north", "temp.north", "salt.north"};
const char *const FF_CLIM[2] = {"Tclim", "Sclim"};
static const char *const FF_RATE[1] = {"tau"};

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
// pomgpu_set_forcing_record fills.  Kind 3 is water (read_water_pnetcdf, :3227-3272): one source, neither converted nor tapered, into the
// record pomgpu_set_water_record fills.  Thread mapping of k_cdf_unpack: threadIdx.x runs along i.
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
// (the tile's jm or im values per level): src 5 * side + (0 zeta, 1 u, 2 v, 3 temp, 4 salt), side 0 east, 1 south, 2 west, 3 north -- the
// edge numbers of k_ztosig_line; f32 bit q: that variable is NC_FLOAT.  `sides` (pomgpu_set_lateral_sides, bit = side; a kernel argument:
// every side's branch is uniform across the grid): a side that is ON takes its four (., kb) arrays and its elevation line from the file;
// one that is OFF has t s from the line of tclim, sclim next to it (i = 1, i = im, j = 1, j = jm: :3606-3614 and the commented :3607-3608,
// :3612-3613), u v zero and its elevation line as the state holds it (:3393-3621 never writes elw, eln).  Everything beyond jm / im: zero,
// but in the elevations, which the reader leaves as they are there.  The arrays of a side in the reader's order: t s u v west and east,
// t s v u north and south.
// zts (an lbry file on z levels): temp / salt of the ON sides hold other levels and are left to k_ztosig_line, which fills those arrays.
// Source q lies at base + off[q] (8-byte aligned); a variable of a side that is OFF has none.  The table reaches the kernel through memory
// -- it travels behind the data in the fetch's one copy -- and not as an argument: twenty sources held in scalar registers beside KP for
// the whole kernel spilled 79 of them; read where a side's loop needs them they spill none.
struct LatSrc { const unsigned char *base; unsigned off[20]; unsigned f32; int zts; };
__device__ __forceinline__ double lat_raw(const LatSrc &s, int q, size_t at) {
  const void *p = s.base + s.off[q];
  return (s.f32 >> q) & 1u ? CdfRaw<float>::get(p, at) : CdfRaw<double>::get(p, at);
}
// level k of the four arrays of `side` (n values each from r) at the point whose place in them is o and in the file's compact level f;
// (ci, cj): the cell of tclim, sclim next to the point
__device__ __forceinline__ void lat_four(const KP &P, const LatSrc &s, int sides, int side, double *r, size_t n, size_t o, size_t f, bool in, int ci, int cj, int k) {
  const int q = 5 * side, qa = q + ((side & 1) ? 2 : 1), qb = q + ((side & 1) ? 1 : 2);   // south, north: v before u
  if ((sides >> side) & 1) {
    if (!s.zts) {
      r[o] = in ? lat_raw(s, q + 3, f) : 0.;
      r[n + o] = in ? lat_raw(s, q + 4, f) : 0.;
    }
    r[2 * n + o] = in ? lat_raw(s, qa, f) : 0.;
    r[3 * n + o] = in ? lat_raw(s, qb, f) : 0.;
  } else {
    r[o] = in ? (double)F3(tclim, ci, cj, k) : 0.;
    r[n + o] = in ? (double)F3(sclim, ci, cj, k) : 0.;
    r[2 * n + o] = 0.;
    r[3 * n + o] = 0.;
  }
}
__global__ void k_lat_unpack(KP P, double *__restrict__ rec, const LatSrc *__restrict__ sp, int sides) {
  const LatSrc &s = *sp;
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
      lat_four(P, s, sides, 2, rec, njk, o, f, in, 1, a, k);
    }
    for (int k = 1; k <= kb; k++) {                               // (a loop per side: either needs the sources of one side alone)
      const size_t o = (size_t)(k - 1) * jml + (a - 1), f = (size_t)(k - 1) * P.jm + (a - 1);
      lat_four(P, s, sides, 0, rec + 4 * njk, njk, o, f, in, P.im, a, k);
    }
    e[a - 1] = (sides & 4) && in ? lat_raw(s, 10, (size_t)(a - 1)) : BD1(elw, a);
    e[jml + a - 1] = (sides & 1) && in ? lat_raw(s, 0, (size_t)(a - 1)) : BD1(ele, a);
  } else {
    const int a = t - jml + 1;
    const bool in = a <= P.im;
    double *r = rec + 8 * njk;
    for (int k = 1; k <= kb; k++) {
      const size_t o = (size_t)(k - 1) * iml + (a - 1), f = (size_t)(k - 1) * P.im + (a - 1);
      lat_four(P, s, sides, 3, r, nik, o, f, in, a, P.jm, k);
    }
    for (int k = 1; k <= kb; k++) {
      const size_t o = (size_t)(k - 1) * iml + (a - 1), f = (size_t)(k - 1) * P.im + (a - 1);
      lat_four(P, s, sides, 1, r + 4 * nik, nik, o, f, in, a, 1, k);
    }
    e[2 * (size_t)jml + a - 1] = (sides & 8) && in ? lat_raw(s, 15, (size_t)(a - 1)) : BD1(eln, a);
    e[2 * (size_t)jml + iml + a - 1] = (sides & 2) && in ? lat_raw(s, 5, (size_t)(a - 1)) : BD1(els, a);
  }
}
// the variables of the ON sides in the order they are looked up -- the elevations, then u v temp salt of every side; the sides east,
// south, west, north -- as LatSrc's numbers into lq; their count
static int lat_vars(int sides, int *lq) {
  int n = 0;
  for (int sd = 0; sd < 4; sd++) if ((sides >> sd) & 1) lq[n++] = 5 * sd;
  for (int sd = 0; sd < 4; sd++) if ((sides >> sd) & 1) for (int v = 1; v <= 4; v++) lq[n++] = 5 * sd + v;
  return n;
}

static FFiles *FF(pomgpu_ctx *c) { return (FFiles *)c->frc_files; }
int pomgpu_ff_has(pomgpu_ctx *c, int src) { return c->frc_files && FF(c)->s[src].fd >= 0; }
void pomgpu_ff_free(pomgpu_ctx *c) {
  FFiles *F = FF(c);
  if (!F) return;
  for (FSource &s : F->s) if (s.fd >= 0) (void)close(s.fd);
  F->rd.release();
  F->z.free();
  if (F->ldev) (void)hipFree(F->ldev);
  F->r.free();
  delete F;
  c->frc_files = NULL;
}
// One source's record variables against what its reader asks for (cdf_io.hpp): the file's record size here, each variable through check_var,
// then where its records lie and whether they are all inside the file
std::string ff_check(const RHeader &H, FSource &S, const char *const *names, const std::vector<std::vector<uint64_t>> &want, uint64_t min_rec) {
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
    const std::string why = check_var(H, S.fsize, name, VarWant::record(NC_REAL, want[q], min_rec), &v);
    if (!why.empty()) return why;
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

// the read buffers grown to `need` bytes each (never inside a step); 1 = a HIP call failed
static int ff_reserve(pomgpu_ctx *c, FFiles *F, size_t need) {
  if (F->rd.cap >= need) return 0;
  const int bad = hipStreamSynchronize(c->stream) != hipSuccess;   // (a second registration: earlier fetches may still be copying)
  if (!(F->rd.reserve(need) | bad)) return 0;
  F->rd.cap = 0;
  return 1;
}

extern "C" int pomgpu_set_forcing_files(pomgpu_ctx *c, const char *sfrc, const char *lbry, const char *clim, const pomgpu_file_meta *m) {
  if (!c || !m) return POMGPU_EINVAL;
  (void)hipSetDevice(c->device);
  const KP &P = c->P;
  if (!tile_fits(m, P, 0, 0, 0, 0))
    return fail(c, POMGPU_EINVAL, "set_forcing_files: the tile (%d..%d, %d..%d) does not fit the global grid %d x %d", m->i0, m->i0 + P.im - 1, m->j0,
                m->j0 + P.jm - 1, m->im_global, m->jm_global);
  if (P.im < 3 || P.jm < 3) return fail(c, POMGPU_EINVAL, "set_forcing_files: the wind taper needs a tile of at least 3 x 3 cells");
  // a clim file on z levels (pomgpu_set_z_inputs): ztosig's fill-in looks at all four neighbours, so the monthly fetch reads one more column / row
  // towards every neighbour of the tile
  const int zc = clim && c->z_clim, wi = zc && !P.W, we = zc && !P.E, wj = zc && !P.S, wn = zc && !P.N;
  if (!tile_fits(m, P, wi, we, wj, wn))
    return fail(c, POMGPU_EINVAL, "set_forcing_files: %s: the tile (%d..%d, %d..%d) with its window lines towards every neighbour does not fit the global grid %d x %d", clim,
                m->i0, m->i0 + P.im - 1, m->j0, m->j0 + P.jm - 1, m->im_global, m->jm_global);
  // an lbry file on z levels (pomgpu_set_z_lateral): the fill-in of a line point looks at the points before and after it, so the fetch reads one
  // more point of temp / salt towards every neighbour of the tile: .east / .west towards the south and north one, .south / .north towards the
  // west and east one
  const int zl = lbry && c->z_lbry, lwi = zl && !P.W, lwe = zl && !P.E, lwj = zl && !P.S, lwn = zl && !P.N;
  // the lbry file's variables: those of the sides that are ON (pomgpu_set_lateral_sides), a side's along j (east, west) or i
  int lq[20];
  const int sides = c->lbry_sides, lnv = lat_vars(sides, lq);
  const size_t nej = (size_t)((sides & 1) + ((sides >> 2) & 1)), nei = (size_t)(((sides >> 1) & 1) + ((sides >> 3) & 1));
  if (zl && (P.im < 4 || P.jm < 4)) return fail(c, POMGPU_EINVAL, "set_forcing_files: %s: a z-level lbry file needs a tile of at least 4 x 4 cells, this one has %d x %d", lbry, P.im, P.jm);
  if (!tile_fits(m, P, lwi, lwe, lwj, lwn))
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
    if (read_header(S.fd, S.fsize, H, what) < 0) { drop(); return fail(c, POMGPU_EINVAL, "set_forcing_files: %s is not a %s file this library reads: %s", paths[q], FF_WHAT[q], what.c_str()); }
    std::string why;
    if (q == 0) why = ff_check(H, S, FF_SFRC, std::vector<std::vector<uint64_t>>(6, {jmg, img}), 1);
    else if (q == 1) {
      if (zl) why = z_levels(H, S, "z", llev);
      const uint64_t kl = zl && why.empty() ? (uint64_t)llev.size() : kb;   // temp, salt on the levels of z; u, v stay on the sigma levels
      const char *names[20];
      std::vector<std::vector<uint64_t>> want;
      for (int j = 0; j < lnv; j++) {
        const int var = lq[j] % 5;
        const uint64_t len = (lq[j] / 5) & 1 ? img : jmg;
        names[j] = FF_LBRY[lq[j]];
        if (var == 0) want.push_back({len});
        else want.push_back({var >= 3 ? kl : kb, len});
      }
      if (why.empty()) why = ff_check(H, S, names, want, 1);
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
  const size_t run = io_run_bytes(c, band2, band2 * nlevmax);
  size_t need = 2 * band2;                                        // sfrc: two variables' bands
  const size_t lpts = nej * (size_t)P.jm + nei * (size_t)P.im;    // an lbry record: the elevation line and four arrays of every side that is ON
  const size_t lat = 8 * lpts + 4 * 8 * (size_t)P.kb * lpts + sizeof(LatSrc);   // (k_lat_unpack's table goes behind the data)
  if (need < lat) need = lat;
  const size_t lks = llev.size();                                 // a z-level lbry record: two of the four arrays of such a side on lks levels over the window
  const size_t latz = 8 * lpts + 2 * 8 * (size_t)P.kb * lpts + 2 * 8 * lks * (lpts + 2 * (nej + nei)) + sizeof(LatSrc);
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
  ZWindow znew;
  if (!bad && paths[2] && zks && (znew.alloc(c, wi, we, wj, wn, zlev) || hipStreamSynchronize(c->stream) != hipSuccess)) { bad = 1; znew.free(); }
  const size_t lpitch = (size_t)(P.jml > P.iml ? P.jml : P.iml);
  double *lnew = NULL;
  if (!bad && lks) {
    std::vector<double> tab(4 * lks);
    ztosig_table(llev.data(), (int)lks, tab.data());
    if (hipMalloc((void **)&lnew, (4 * lks + 2 * 8 * lks * lpitch) * sizeof(double)) != hipSuccess ||   // the table, tin and u / y2 of eight lines
        hipMemcpyAsync(lnew, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {           // (and an earlier fetch has stopped mapping out of the old buffers)
      bad = 1;
      if (lnew) (void)hipFree(lnew);
      lnew = NULL;
      znew.free();
    }
  }
  if (!bad && paths[1]) {
    if (F->ldev && !lks && hipStreamSynchronize(c->stream) != hipSuccess) { bad = 1; znew.free(); }
    else {
      if (F->ldev) (void)hipFree(F->ldev);
      F->ldev = lnew;
      F->lks = (int)lks; F->lwi = lwi; F->lwe = lwe; F->lwj = lwj; F->lwn = lwn;
      F->lsides = sides; F->lnv = lnv;
      for (int j = 0; j < lnv; j++) F->lq[j] = lq[j];
    }
  }
  if (!bad && paths[2]) {
    if (F->z.dev && hipStreamSynchronize(c->stream) != hipSuccess) bad = 1;   // an earlier fetch may still be mapping out of the old buffers
    F->z.free();
    F->z = znew;
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
static int ff_have(pomgpu_ctx *c, FSource &S, const char *who, int n, const int *which, int nwhich) {
  for (int pass = 0; pass < 2; pass++) {
    bool ok = n >= 1;
    for (int w = 0; w < nwhich; w++) {
      const FVar &f = S.v[which[w]];
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
static int ff_have(pomgpu_ctx *c, FSource &S, const char *who, int n, std::initializer_list<int> which) { return ff_have(c, S, who, n, which.begin(), (int)which.size()); }
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
  // SSS is read by the reference and dropped (bounds_forcing.f:978-979): read here only where pomgpu_set_surface_sss wants it
  const int va = 2 * kind, vb = 2 * kind + 1, nvar = kind == 2 && !c->sss_on ? 1 : 2;
  int rc = nvar == 1 ? ff_have(c, S, who[kind], n, {va}) : ff_have(c, S, who[kind], n, {va, vb});
  if (rc) return rc;
  const int sl = n % 4;
  unsigned char *pin = F->rd.acquire();
  if (!pin) return ff_io_error(c, who[kind], n, S, 1);
  const size_t half = (size_t)P.jm * (size_t)F->im_global * 8;   // where the second variable's band starts (8-byte aligned whatever the types)
  for (int q = 0; q < nvar; q++) {
    const FVar &f = S.v[q ? vb : va];
    const uint64_t at = f.begin + (uint64_t)(n - 1) * f.stride + (uint64_t)(F->j0 - 1) * (uint64_t)F->im_global * f.esize();
    if (pread_all(S.fd, pin + q * half, (size_t)P.jm * (size_t)F->im_global * f.esize(), at)) return ff_io_error(c, who[kind], n, S, 0);
  }
  if (F->rd.send(c, nvar == 2 ? 2 * half : half)) return ff_io_error(c, who[kind], n, S, 1);
  double *da = c->frc_dev[kind][sl][0], *db = c->frc_dev[kind][sl][1];
  const void *sa = F->rd.stage, *sb = nvar == 2 ? (const void *)(F->rd.stage + half) : NULL;
  const bool fa = S.v[va].type == 5, fb = nvar == 2 && S.v[vb].type == 5;
  const int pitch = F->im_global, i0 = F->i0 - 1;
  if (fa && fb) LAUNCHN(c, "k_frc_unpack", (k_frc_unpack<float, float>), grid2(P), blk2(), P, kind, da, db, sa, sb, pitch, i0);
  else if (fa) LAUNCHN(c, "k_frc_unpack", (k_frc_unpack<float, double>), grid2(P), blk2(), P, kind, da, db, sa, sb, pitch, i0);
  else if (fb) LAUNCHN(c, "k_frc_unpack", (k_frc_unpack<double, float>), grid2(P), blk2(), P, kind, da, db, sa, sb, pitch, i0);
  else LAUNCHN(c, "k_frc_unpack", (k_frc_unpack<double, double>), grid2(P), blk2(), P, kind, da, db, sa, sb, pitch, i0);
  c->frc_n[kind][sl] = n;
  return POMGPU_OK;
}
// ---- water (read_water_pnetcdf, io_pnetcdf.F:3227-3272): '(a,''in/'',a,''.water.'',i4.4,''.nc'')', one file per record and in it `w` as
// (jm_global, im_global), found by name.  Nothing is opened at registration: the schedule (pomgpu_water) names the record, the file is opened,
// checked by the shared header parser and check_var, its band read and unpacked into the slot pomgpu_set_water_record(n, ...) fills, and closed.
extern "C" int pomgpu_set_water_files(pomgpu_ctx *c, const char *prefix, const pomgpu_file_meta *m) {
  if (!c) return POMGPU_EINVAL;
  if (!prefix || !m) return fail(c, POMGPU_EINVAL, "set_water_files: %s", prefix ? "no file meta was given" : "no prefix was given (NULL)");
  (void)hipSetDevice(c->device);
  const KP &P = c->P;
  if (!tile_fits(m, P, 0, 0, 0, 0))
    return fail(c, POMGPU_EINVAL, "set_water_files: the tile (%d..%d, %d..%d) does not fit the global grid %d x %d", m->i0, m->i0 + P.im - 1, m->j0,
                m->j0 + P.jm - 1, m->im_global, m->jm_global);
  FFiles *old = FF(c);
  if (old && (old->im_global != m->im_global || old->jm_global != m->jm_global || old->i0 != m->i0 || old->j0 != m->j0))
    return fail(c, POMGPU_EINVAL, "set_water_files: %s: files are registered under another global grid or tile origin", prefix);
  FFiles *F = old ? old : new FFiles();
  const size_t need = (size_t)P.jm * (size_t)m->im_global * 8;    // the tile's band of rows at the file's full width, doubles
  int bad = ff_reserve(c, F, need);
  for (int sl = 0; sl < 4 && !bad; sl++)                          // the slots the setter would have allocated: a step allocates nothing
    if (!c->wat_dev[sl] && hipMalloc((void **)&c->wat_dev[sl], sizeof(double) * (size_t)P.im * P.jm) != hipSuccess) bad = 1;
  c->frc_files = F;
  if (bad) {
    (void)hipGetLastError();
    if (!old) pomgpu_ff_free(c);
    return fail(c, POMGPU_ENOMEM, "set_water_files: %s: no memory for the read buffers (%zu bytes, twice pinned)", prefix, need);
  }
  F->im_global = m->im_global; F->jm_global = m->jm_global; F->i0 = m->i0; F->j0 = m->j0;
  F->wprefix = prefix;
  F->won = 1;
  for (int sl = 0; sl < 4; sl++) c->wat_n[sl] = 0;                // records the setter left are not the files'
  c->wat_on = 1;
  return POMGPU_OK;
}
int pomgpu_ff_has_water(pomgpu_ctx *c) { return c->frc_files && FF(c)->won; }
int pomgpu_ff_fetch_water(pomgpu_ctx *c, int n) {
  FFiles *F = FF(c);
  const KP &P = c->P;
  if (n < 0 || n > 9999) return fail(c, POMGPU_EINVAL, "water: record %d has no file name (%s.water.NNNN.nc: 0..9999)", n, F->wprefix.c_str());
  char num[16];
  snprintf(num, sizeof num, "%04d", n);
  FSource S;
  S.path = F->wprefix + ".water." + num + ".nc";
  S.fd = open(S.path.c_str(), O_RDONLY);
  if (S.fd < 0) return fail(c, POMGPU_EINVAL, "water: cannot open %s", S.path.c_str());
  struct Closer { int fd; ~Closer() { (void)close(fd); } } closer{S.fd};
  struct stat sb;
  if (fstat(S.fd, &sb)) return fail(c, POMGPU_EINVAL, "water: cannot stat %s", S.path.c_str());
  S.fsize = (uint64_t)sb.st_size;
  RHeader H;
  std::string what;
  if (read_header(S.fd, S.fsize, H, what) < 0) return fail(c, POMGPU_EINVAL, "water: %s is not a water file this library reads: %s", S.path.c_str(), what.c_str());
  const RVar *v = NULL;
  const std::string why = check_var(H, S.fsize, "w", VarWant::fixed(NC_REAL, {(uint64_t)F->jm_global, (uint64_t)F->im_global}), &v);
  if (!why.empty()) return fail(c, POMGPU_EINVAL, "water: %s: %s", S.path.c_str(), why.c_str());
  const unsigned esize = v->type == 5 ? 4u : 8u;
  const int sl = n % 4;
  unsigned char *pin = F->rd.acquire();
  if (!pin) return ff_io_error(c, "water", n, S, 1);
  const size_t bytes = (size_t)P.jm * (size_t)F->im_global * esize;
  if (pread_all(S.fd, pin, bytes, v->begin + (uint64_t)(F->j0 - 1) * (uint64_t)F->im_global * esize)) return ff_io_error(c, "water", n, S, 0);
  if (F->rd.send(c, bytes)) return ff_io_error(c, "water", n, S, 1);
  const void *sa = F->rd.stage, *sb0 = NULL;
  double *da = c->wat_dev[sl], *db = NULL;
  const int pitch = F->im_global, i0 = F->i0 - 1;
  if (v->type == 5) LAUNCHN(c, "k_frc_unpack", (k_frc_unpack<float, float>), grid2(P), blk2(), P, 3, da, db, sa, sb0, pitch, i0);
  else LAUNCHN(c, "k_frc_unpack", (k_frc_unpack<double, double>), grid2(P), blk2(), P, 3, da, db, sa, sb0, pitch, i0);
  c->wat_n[sl] = n + 1;
  return POMGPU_OK;
}
// record n of the lateral file into the slot pomgpu_set_lateral_record(n, ...) fills
int pomgpu_ff_fetch_lateral(pomgpu_ctx *c, int n) {
  FFiles *F = FF(c);
  FSource &S = F->s[1];
  const KP &P = c->P;
  const int nv = F->lnv;                                          // the variables of the sides that are ON: S.v[j] is LatSrc's F->lq[j]
  int all[20];
  for (int j = 0; j < nv; j++) all[j] = j;
  int rc = ff_have(c, S, "lateral_bc", n, all, nv);
  if (rc) return rc;
  const int sl = n % 4;
  unsigned char *pin = F->rd.acquire();
  if (!pin) return ff_io_error(c, "lateral_bc", n, S, 1);
  LatSrc src;
  src.f32 = 0;
  for (int q = 0; q < 20; q++) src.off[q] = 0;
  size_t at = 0, off[20];
  // a z-level lbry file: temp, salt of every such side on all lks levels over the line and its window points, mapped by k_ztosig_line behind k_lat_unpack
  const int onz = F->lks > 0;
  int cnt[20], wlo[20];
  for (int j = 0; j < nv; j++) {
    const FVar &f = S.v[j];
    const int q = F->lq[j], var = q % 5;
    const bool alongj = !((q / 5) & 1);                          // east, west: the tile's jm values from j0; else im values from i0
    const bool zq = onz && var >= 3;
    const int nlev = var == 0 ? 1 : (zq ? F->lks : P.kb);
    wlo[j] = zq ? (alongj ? F->lwj : F->lwi) : 0;
    cnt[j] = (alongj ? P.jm : P.im) + wlo[j] + (zq ? (alongj ? F->lwn : F->lwe) : 0);
    const uint64_t glen = alongj ? (uint64_t)F->jm_global : (uint64_t)F->im_global, first = (uint64_t)((alongj ? F->j0 : F->i0) - 1 - wlo[j]);
    const size_t len = (size_t)cnt[j] * f.esize();
    const uint64_t base = f.begin + (uint64_t)(n - 1) * f.stride + first * f.esize();
    off[j] = at;
    if (read_bands(S.fd, pin + at, base, len, glen * f.esize(), nlev)) return ff_io_error(c, "lateral_bc", n, S, 0);
    at += (len * nlev + 7) & ~(size_t)7;
    if (f.type == 5) src.f32 |= 1u << q;
  }
  for (int j = 0; j < nv; j++) src.off[F->lq[j]] = (unsigned)off[j];
  src.base = F->rd.stage;
  src.zts = onz;
  memcpy(pin + at, &src, sizeof src);                             // the table travels behind the data, in the one copy
  if (F->rd.send(c, at + sizeof src)) return ff_io_error(c, "lateral_bc", n, S, 1);
  const int nt = P.jml + P.iml;
  LAUNCH(c, k_lat_unpack, dim3((unsigned)((nt + 63) / 64), 1, 1), dim3(64, 1, 1), P, c->lat_dev[sl], (const LatSrc *)(F->rd.stage + at), F->lsides);
  if (onz) {                                                     // t s of every such side: the record's first two arrays of it, one launch
    const size_t njk = (size_t)P.jml * P.kb, nik = (size_t)P.iml * P.kb;
    const int pitch = P.jml > P.iml ? P.jml : P.iml;
    const size_t first4[4] = {4 * njk, 8 * njk + 4 * nik, 0, 8 * njk};   // where the four arrays of east, south, west, north start
    ZtlJob job;
    int nl = 0;
    for (int j = 0; j < nv; j++) {
      const int q = F->lq[j], sd = q / 5, var = q % 5;
      if (var < 3) continue;
      double *out = c->lat_dev[sl] + first4[sd] + (size_t)(var - 3) * ((sd & 1) ? nik : njk);
      job.l[nl++] = ztosig_line_of(P, sd, out, src.base + src.off[q], S.v[j].type == 5 ? 1 : 2, cnt[j], wlo[j]);
    }
    for (int l = nl; l < 8; l++) job.l[l] = job.l[0];
    const size_t work = 8 * (size_t)F->lks * pitch;              // one work array: eight lines' slices (sized at registration)
    launch_ztosig_lines(c, job, nl, F->ldev, F->ldev + 4 * (size_t)F->lks, F->ldev + 4 * (size_t)F->lks + work, F->lks, pitch);
  }
  c->lat_n[sl] = n;
  return POMGPU_OK;
}
// nlev levels of record `rec` of the volume f over Z's window (an empty Z: over the tile), as doubles to `to`; read_levels' result
static int ff_fetch_volume(pomgpu_ctx *c, FFiles *F, const FSource &S, const FVar &f, int rec, const ZWindow &Z, int nlev, double *to) {
  const KP &P = c->P;
  const uint64_t img = (uint64_t)F->im_global, jmg = (uint64_t)F->jm_global;
  const int rows = Z.rows(P), cols = Z.cols(P);
  const uint64_t first = f.begin + (uint64_t)(rec - 1) * f.stride + (uint64_t)(F->j0 - 1 - Z.wj) * img * f.esize();
  return read_levels(c, F->rd, S.fd, first, (size_t)rows * (size_t)img * f.esize(), jmg * img * f.esize(), nlev, [&](int k0, int nl) {
    launch_cdf_unpack(c, "k_rst_unpack", f.type, to + (size_t)k0 * rows * cols, F->rd.stage, cols, rows, nl, (size_t)rows * cols, cols, rows, (int)img, F->i0 - 1 - Z.wi);
  });
}
// Tclim, Sclim of month mod(n+9,12)+1 (io_pnetcdf.F:3316) into rec_t[0], rec_s[0], the (im,jm,kb) records k_restore_load reads
int pomgpu_ff_fetch_restore(pomgpu_ctx *c, int n) {
  FFiles *F = FF(c);
  FSource &S = F->s[2];
  if (n < 1) return fail(c, POMGPU_EINVAL, "restore_interior: record %d", n);
  const int month = (n + 9) % 12 + 1;
  int rc = ff_have(c, S, "restore_interior", month, {0, 1});
  if (rc) return rc;
  // a z-level clim file: all its levels over the tile's window into the window buffer, then ztosig into the record, in the unpack kernel's place
  const int onz = F->z.ks[0] > 0;
  for (int q = 0; q < 2; q++) {
    double *dst = q ? c->rec_s[0] : c->rec_t[0];
    rc = ff_fetch_volume(c, F, S, S.v[q], month, F->z, onz ? F->z.ks[0] : c->P.kb, onz ? F->z.win() : dst);
    if (rc) return ff_io_error(c, "restore_interior", n, S, rc == 2);
    if (onz) launch_ztosig_window(c, dst, 1, F->z, 0);
  }
  return POMGPU_OK;
}

// ---- the restore rate from a z-level file (read_restore_tau_interior_pnetcdf, io_pnetcdf.F:3053-3107, and the ztosig behind it that
// bounds_forcing.f:1049-1051, :1076-1079 keep commented) ---------------------------------------------------------------------------------
// `z` (ks levels) and `tau` (ks, jm_global, im_global), with or without a leading record dimension.  The rate that goes with T/S record n
// is record n of the file; a file with one record (or no record dimension) is steady and serves every n.  Registered beside the three
// forcing files: the same header parser and checks, the same pinned buffers, the window and the work arrays of the z-level clim file.
static std::string rate_check(const RHeader &H, FSource &S, uint64_t ks, uint64_t jmg, uint64_t img) {
  const RVar *v = find_var(H, FF_RATE[0]);
  if (v && v->dimids.size() != 3) return ff_check(H, S, FF_RATE, {{ks, jmg, img}}, 1);   // a leading record dimension, unlimited or fixed
  const std::string why = check_var(H, S.fsize, FF_RATE[0], VarWant::shape(NC_REAL, {ks, jmg, img}, "([records, ]"), &v);
  if (!why.empty()) return why;
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
  if (!tile_fits(m, P, wi, we, wj, wn))
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
  if (read_header(S.fd, S.fsize, H, what) < 0) { (void)close(S.fd); return fail(c, POMGPU_EINVAL, "set_restore_rate_file: %s is not a rate file this library reads: %s", path, what.c_str()); }
  std::vector<double> zlev;
  std::string why = z_levels(H, S, "z", zlev);
  if (why.empty()) why = rate_check(H, S, (uint64_t)zlev.size(), jmg, img);
  if (!why.empty()) { (void)close(S.fd); return fail(c, POMGPU_EINVAL, "set_restore_rate_file: %s: %s", path, why.c_str()); }
  // ---- accepted: the buffers and the table every fetch uses (no allocation inside a step) ----
  FFiles *F = old ? old : new FFiles();
  const size_t ks = zlev.size();
  const size_t band2 = (size_t)(P.jm + wj + wn) * (size_t)img * 8;   // one level's band of the window's rows at the file's full width, doubles
  const size_t need = io_run_bytes(c, band2, band2 * ks);
  int bad = ff_reserve(c, F, need);
  ZWindow rnew;                                                   // (the synchronise: an earlier fetch has stopped mapping out of the old buffers)
  if (!bad && (rnew.alloc(c, wi, we, wj, wn, zlev) || hipStreamSynchronize(c->stream) != hipSuccess)) { bad = 1; rnew.free(); }
  c->frc_files = F;
  if (bad) {
    (void)close(S.fd);
    (void)hipGetLastError();
    if (!old) pomgpu_ff_free(c);
    return fail(c, POMGPU_ENOMEM, "set_restore_rate_file: %s: no memory for the read buffers (%zu bytes, twice pinned) and the window", path, need);
  }
  F->r.free();
  F->r = rnew;
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
// record n of `tau`: all its levels over the tile's window into the window buffer, then k_ztosig straight into the mirror taurstrf -- every
// cell of (1:im, 1:jm) on all kb levels, the padding beyond keeps what k_restore_load has put there; on the stream the step is enqueued on
int pomgpu_ff_fetch_rate(pomgpu_ctx *c, int n) {
  FFiles *F = FF(c);
  FSource &S = F->s[3];
  const int rc = ff_fetch_volume(c, F, S, S.v[0], F->rsteady ? 1 : n, F->r, F->r.ks[0], F->r.win());
  if (rc) return ff_io_error(c, "restore_interior (rate)", n, S, rc == 2);
  launch_ztosig_window(c, c->P.b3 + (size_t)P3_taurstrf * c->P.a3, 0, F->r, 0);
  return POMGPU_OK;
}
