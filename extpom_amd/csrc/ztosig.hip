// ztosig.hip -- z-level T or S onto the sigma levels (initialize.f:547-595 with splinc :598-638 and splint :641-667): the stand-alone
// calls behind pomgpu_ztosig / pomgpu_ztosig_line, and the window and line forms the file readers of cdf_in.hip and frc_files.hip enqueue.
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
#include "cdf_io.hpp"

void ztosig_table(const double *zs, int ks, double *tab) {
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
void launch_ztosig_window(pomgpu_ctx *c, double *out, int record, const ZWindow &Z, int q) {
  const KP &P = c->P;
  const int wim = Z.cols(P), wjm = Z.rows(P), ks = Z.ks[q];
  const double *zsrc = Z.win(), *tab = Z.tab(q);
  double *wa = Z.wa(), *wb = Z.wb();
  ZtsGeo g = {wim, P.iml, Z.wi ? 1 : 2, Z.we ? P.im : P.imm1, Z.wj ? 1 : 2, Z.wn ? P.jm : P.jmm1, 1, (size_t)wim * wjm, (size_t)Z.wj * wim + Z.wi, P.n2};
  if (record) {
    g.op = P.im; g.ol = (size_t)P.im * P.jm;
    LAUNCHN(c, "k_ztosig", k_ztosig<double>, grid2(P), blk2(), P, out, zsrc, tab, wa, wb, ks, g);
  } else LAUNCHN(c, "k_ztosig", k_ztosig<pomgpu_st>, grid2(P), blk2(), P, (pomgpu_st *)out, zsrc, tab, wa, wb, ks, g);
}
int ZWindow::alloc(pomgpu_ctx *c, int wi_, int we_, int wj_, int wn_, const std::vector<double> &zs0, const std::vector<double> &zs1) {
  const KP &P = c->P;
  ks[0] = (int)zs0.size(); ks[1] = (int)zs1.size();
  wi = wi_; we = we_; wj = wj_; wn = wn_;
  const size_t km = (size_t)kmax();
  nwin = km * (size_t)cols(P) * (size_t)rows(P);
  nwork = km * P.n2;
  host_tab.assign(8 * km, 0.);
  if (hipMalloc((void **)&dev, (nwin + 2 * nwork + (ks[1] ? 8 : 4) * km) * sizeof(double)) != hipSuccess) { dev = NULL; return 1; }
  for (int q = 0; q < 2; q++) {
    if (!ks[q]) continue;
    double *t = host_tab.data() + (size_t)q * 4 * km;
    ztosig_table((q ? zs1 : zs0).data(), ks[q], t);
    if (hipMemcpyAsync((double *)tab(q), t, 4 * (size_t)ks[q] * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) { free(); return 1; }
  }
  return 0;
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
ZtlLine ztosig_line_of(const KP &P, int edge, double *out, const void *src, int fmt, int sp, int so) {
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
void launch_ztosig_lines(pomgpu_ctx *c, const ZtlJob &job, int nlines, const double *tab, double *wa, double *wb, int ks, int pitch) {
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
    for (int l = 0; l < 8; l++) job.l[l] = ztosig_line_of(P, edge, dout, dev, 0, npad + 2, 1);
    launch_ztosig_lines(c, job, 1, dtab, wa, wb, ks, npad);
    if (hipMemcpyAsync(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = POMGPU_EHIP;
  }
  if (hipStreamSynchronize(c->stream) != hipSuccess) rc = POMGPU_EHIP;
  (void)hipFree(dev);
  return rc;
}

// the z levels of a file, vetted (cdf_io.hpp)
std::string z_levels(const RHeader &H, const FSource &S, const char *name, std::vector<double> &zs) {
  const RVar *v = find_var(H, name);
  if (!v) return std::string("variable ") + name + " (the z levels) is absent";
  if (v->dimids.size() != 1) return std::string("variable ") + name + " has " + std::to_string(v->dimids.size()) + " dimensions, wanted the one of the z levels";
  const uint64_t ks = H.dimlen[v->dimids[0]];
  if (ks < 2 || ks > POMGPU_ZTOSIG_NMAX) return std::string("variable ") + name + " holds " + std::to_string(ks) + " z levels, wanted 2..300";
  std::string why = check_var(H, S.fsize, name, VarWant::fixed(NC_REAL, {ks}), &v);
  if (!why.empty()) return why;
  std::vector<unsigned char> raw((size_t)ks * NC_TYPE_BYTES[v->type]);
  if (pread_all(S.fd, raw.data(), raw.size(), v->begin)) return std::string("I/O error (") + name + ")";
  zs.resize((size_t)ks);
  for (size_t k = 0; k < ks; k++) {
    zs[k] = cdf_raw(v->type, raw.data(), k);
    if (!__builtin_isfinite(zs[k]) || (k && !(zs[k] > zs[k - 1])))
      return std::string("variable ") + name + " is not finite and strictly increasing at level " + std::to_string(k + 1) + " (" + std::to_string(zs[k]) + ")";
  }
  return std::string();
}
