// k_tile.hip -- column-marching stencil kernels and the derived 2-D coefficient arrays.
//
// Profile of the first-cut cell kernels on MI355X (2048x1536x50): a cell of advt2 issued 56 global
// loads (each i+-1 / j+-1 neighbour a separate 512-byte wavefront request) and evaluated every face
// flux twice; the kernels ran at ~1.4-1.9 TB/s of algorithmic traffic, bound by the L1/TA request
// rate and fp64 divides, not by HBM.  A row-marching version (a wavefront walks a strip of rows at one
// level) moved the bottleneck to L2-miss traffic: the 14 two-dimensional coefficient operands of a
// cell were re-fetched for every level (31 GB per launch against 7.5 GB algorithmic).  The kernels
// here let a thread own the water column (i,j) instead; see the comment above k_advt2_col.
#include "pomgpu_internal.hpp"


// ---- derived 2-D coefficients -------------------------------------------------------------------
__global__ void k_coef_static(KP P) {
  const int i = TID_I, j = TID_J;
  if (i > P.iml || j > P.jml) return;
  const int iw = i > 1 ? i - 1 : 1, js = j > 1 ? j - 1 : 1;
  P.m8[IX2(i, j)] = (unsigned char)((F2(fsm, i, j) != 0. ? 1 : 0) | (F2(dum, i, j) != 0. ? 2 : 0) | (F2(dvm, i, j) != 0. ? 4 : 0));
  K2(HSX, i, j) = F2(h, i, j) + F2(h, iw, j);
  K2(HSY, i, j) = F2(h, i, j) + F2(h, i, js);
  K2(DYSX, i, j) = F2(dy, i, j) + F2(dy, iw, j);
  K2(DXSX, i, j) = F2(dx, i, j) + F2(dx, iw, j);
  K2(DXSY, i, j) = F2(dx, i, j) + F2(dx, i, js);
  K2(DYSY, i, j) = F2(dy, i, j) + F2(dy, i, js);
  K2(DX4, i, j) = F2(dx, i, j) + F2(dx, iw, j) + F2(dx, i, js) + F2(dx, iw, js);
  K2(DY4, i, j) = F2(dy, i, j) + F2(dy, iw, j) + F2(dy, i, js) + F2(dy, iw, js);
  const int ie = i < P.iml ? i + 1 : P.iml, jn = j < P.jml ? j + 1 : P.jml;
  K2(CVA, i, j) = F2(dy, ie, j) - F2(dy, iw, j);
  K2(CVB, i, j) = F2(dx, i, jn) - F2(dx, i, js);
  K2(R2DXSX, i, j) = 2.0 / (F2(dx, i, j) + F2(dx, iw, j));
  K2(R2DYSY, i, j) = 2.0 / (F2(dy, i, j) + F2(dy, i, js));
  K2(RDX, i, j) = 1.0 / F2(dx, i, j);
  K2(RDY, i, j) = 1.0 / F2(dy, i, j);
  // reciprocals of the vertical grid arrays (divi(), pomgpu_internal.hpp); 1/0 = inf where dz, dzz are 0 (level kb): never used
  if (j == 1)
    for (int n = i - 1; n < POM_NBLK1D * P.kb; n += P.iml) P.r1[n] = 1.0 / P.b1[n];
}
__global__ void k_coef_dt(KP P) {
  const int i = TID_I, j = TID_J;
  if (i > P.iml || j > P.jml) return;
  const int iw = i > 1 ? i - 1 : 1, js = j > 1 ? j - 1 : 1;
  K2(CMX, i, j) = 0.25 * (F2(dy, iw, j) + F2(dy, i, j)) * (F2(dt, iw, j) + F2(dt, i, j));
  K2(CMY, i, j) = 0.25 * (F2(dx, i, js) + F2(dx, i, j)) * (F2(dt, i, js) + F2(dt, i, j));
  K2(DTSX, i, j) = F2(dt, i, j) + F2(dt, iw, j);
  K2(DTSY, i, j) = F2(dt, i, j) + F2(dt, i, js);
  K2(DT4, i, j) = F2(dt, i, j) + F2(dt, iw, j) + F2(dt, i, js) + F2(dt, iw, js);
}
// uvm: also the depth means advance.f:375-392 gives u, v (C2_UCOR, C2_VCOR; utf, vtf are final once the external mode is done), with
// the reference's division; UVM_MARK where it corrects nothing: i = 1 for u, j = 1 for v, and beyond (im, jm)
__global__ void k_coef_eta(KP P, int uvm) {
  const int i = TID_I, j = TID_J;
  if (i > P.iml || j > P.jml) return;
  K2(HEA, i, j) = (F2(h, i, j) + F2(etb, i, j)) * F2(art, i, j);
  K2(HFA, i, j) = (F2(h, i, j) + F2(etf, i, j)) * F2(art, i, j);
  if (uvm) {
    const unsigned long long mb = UVM_MARK;
    double mark;
    __builtin_memcpy(&mark, &mb, sizeof mark);
    const int iw = i > 1 ? i - 1 : 1, js = j > 1 ? j - 1 : 1;
    const double cu = (F2(utb, i, j) + F2(utf, i, j)) / (F2(dt, i, j) + F2(dt, iw, j));     // advance.f:375-382
    const double cv = (F2(vtb, i, j) + F2(vtf, i, j)) / (F2(dt, i, j) + F2(dt, i, js));     // :385-392
    K2(UCOR, i, j) = (i >= 2 && i <= P.im && j <= P.jm) ? cu : mark;
    K2(VCOR, i, j) = (j >= 2 && j <= P.jm && i <= P.im) ? cv : mark;
  }
}

// ---- advt2, nitera == 1 -- solver.f:577-731 with smol_adif's mask (:1898-1900) --------------------
__device__ __forceinline__ pomgpu_ct upw_(pomgpu_ct m, pomgpu_ct lo, pomgpu_ct hi) {     // solver.f:631-635
  return CT(0.5) * ((m + fabs(m)) * lo + (m - fabs(m)) * hi);
}
// the values of k_advt2_col, k_advq_col, k_advct_col and k_advuv_col are pomgpu_ct: fp32 in the fp32-arithmetic variant
// (pomgpu_internal.hpp), where every 2-D coefficient is narrowed once per column, before the level loop
struct FaceT { pomgpu_ct adv, dif; };
// ---- advt2, nitera == 1, COLUMN-MARCHING version -----------------------------------------------------
// PMC profile of the row-marching kernel above (2048x1536x50): 31 GB of L2-miss traffic per launch
// against 7.5 GB algorithmic -- the 14 two-dimensional coefficient operands of a cell are re-fetched
// for every level -- and ~1e9 L1 line accesses.  Here a thread owns the water column (i,j):
//   * all 2-D coefficients of its three faces live in registers for the whole column;
//   * the level loop is software-pipelined: iteration L issues the loads of level L+1, evaluates
//     the faces of level L from registers filled one iteration earlier, and finishes level L-1
//     (whose bottom face is the top face of level L, evaluated once);
//   * west operands and the east face come from the neighbour lane of a halo-lane wavefront
//     (pomgpu_internal.hpp): no lane ever loads in the middle of an iteration -- vmcnt counts in
//     order, so such a load would wait for the whole prefetch batch of the next level.
// Per cell: 13 512-byte wavefront loads (was 56 in the cell kernel), 3 face evaluations
// in x/y (was 4) and 1 in z (was 2).
// NF = 2 advances T and S in ONE pass (advance.f:431-432 calls advt2 twice): u, v, w, aam and the face
// coefficients are read once for both fields.
// rtf (RTF launches alone, the last member: the others keep their place in the kernel's arguments): see k_advt2_col
struct TFields { const double *fb[2], *f[2], *fcl[2]; double *ff[2]; unsigned long long *rtf; };
// Operands of a level.  Shared with the rows above and below through the workgroup's LDS slab (RowShare,
// pomgpu_internal.hpp), in this order: fb[0..NF-1], fclim[0..NF-1], aam, v; this row only: u, w.
// c: the wavefront's own row, h: its share of the two rows outside the workgroup.
template <int NF> struct LevT { pomgpu_ct c[2 * NF + 2], o[2], h[ROWSHARE_SLOTS(2 * NF + 2)]; };
template <int NS> struct NbrT { pomgpu_ct s[NS], n[NS]; };
struct CoefT { pomgpu_ct cm, hs, msk, ds_num; InvDc den; };   // mass-flux coefficient, h sum, mask, metric sums of one face
__device__ __forceinline__ CoefT coef_x(const KP &P, int i, int j) {
  CoefT c; c.cm = K2(CMX, i, j); c.hs = K2(HSX, i, j); c.msk = F2(dum, i, j); c.ds_num = K2(DYSX, i, j); c.den = inv_of(CT(K2(DXSX, i, j))); return c;
}
__device__ __forceinline__ CoefT coef_y(const KP &P, int i, int j) {
  CoefT c; c.cm = K2(CMY, i, j); c.hs = K2(HSY, i, j); c.msk = F2(dvm, i, j); c.ds_num = K2(DXSY, i, j); c.den = inv_of(CT(K2(DYSY, i, j))); return c;
}
// face between a "lo" cell (west / south) and a "hi" cell; vel = u or v on that face
__device__ __forceinline__ FaceT advt2_face(const pomgpu_ct tprni, const CoefT &c, pomgpu_ct vel, pomgpu_ct fb_hi, pomgpu_ct fb_lo, pomgpu_ct fc_hi,
                                            pomgpu_ct fc_lo, pomgpu_ct am_hi, pomgpu_ct am_lo) {
  FaceT f;
  f.adv = upw_(c.cm * vel, fb_lo, fb_hi);
  const pomgpu_ct am = CT(0.5) * (am_hi + am_lo);
  f.dif = divi(-am * c.hs * tprni * ((fb_hi - fc_hi) - (fb_lo - fc_lo)) * c.msk * c.ds_num * CT(0.5), c.den);
  return f;
}
#if COL_WX != 1
#error "the row-sharing column kernels keep one wavefront per workgroup row (COL_WX == 1)"
#endif
// What keeps the level loop a pipeline (each item was a stall in the ISA of the first version):
//   * every load of a level is issued in ONE batch a whole iteration before its first use, and NO memory instruction sits
//     inside a branch: where control flow joins, the compiler no longer knows how many operations are outstanding and
//     waits for vmcnt(0), i.e. for the batch it has just issued.  Lanes / iterations with nothing to store aim outside
//     the buffer (BOFF_NONE, dropped by the hardware); the last iterations re-request level kbm1;
//   * dz(k) comes through the constant address space (scalar load) -- as a vector load it queued behind the batch;
//   * buffer addressing: no vector instruction computes an address; two register sets alternate as current / next
//     level (no copies); divisors that are fixed along the column are inverted once (divi).
// UM: u, v in memory still lack the depth-mean correction of advance.f:365-393 (KP::uvm, uvm_fix in pomgpu_internal.hpp): applied to
// u of the own column and to v before it enters the slab -- the own row's with the lane's coefficients, the share of a row outside the
// workgroup with that row's; the east face travels through the lane shift as before.  Every level this kernel loads is <= kbm1.
// RTF (the T / S launch of mode_internal alone, launch_advt2x2_col): where does fb's in-place round trip through fb - fclim
// (solver.f:691,715), which k_ts_update applies to what it loads, change a bit?  The lane that owns a column holds both operands of
// every level 1..kbm1 and forms fb - fclim anyway: (fb - fclim) + fclim is compared with fb bit for bit, the wavefront's 64 answers
// (T's or S's) are one lane mask, and lane 0 stores that word to A.rtf -- one per (level, row, 62-column block), bit = lane,
// RT_WORD below.  k_ts_update reads tclim, sclim only where a bit is set (by Sterbenz's lemma fb - fclim is exact for fclim/2 <= fb <=
// 2 fclim: a field next to its climatology sets none).  The store follows the loop's discipline: every lane, every iteration, the
// offset selected.  The emulated build, one lane at a time, ORs its bit into the word its block's first owned lane has started.
template <int NF, bool UM = false, bool RTF = false>
__global__ void __launch_bounds__(64 * LDS_ROWS) k_advt2_col(KP P, TFields A) {
  constexpr int NS = 2 * NF + 2, NH = ROWSHARE_SLOTS(NS), AM = 2 * NF, VV = 2 * NF + 1;
  HALO_XCD_DECODE_R(LDS_ROWS)                                           // a workgroup outside the grid leaves as a whole
  const int r = WAVE_UNIFORM((int)threadIdx.y), j0w = j - r;
  const bool jrow = j <= P.jml;                             // rows beyond the tile shadow row jml and store nothing
  const int jc = jrow ? j : P.jml;
  const bool icol = jrow && (lane >= 1 && lane <= 62 && i0 <= P.iml);   // this lane owns an output column
#ifdef POMGPU_EMU
  if (!icol) return;
#endif
  const int i = i0 < 1 ? 1 : (i0 > P.iml ? P.iml : i0);          // halo / padding lanes shadow a valid column
  const int iw = i > 1 ? i - 1 : 1, ie = i < P.iml ? i + 1 : P.iml;
  const int js = jc > 1 ? jc - 1 : 1, jn = jc < P.jml ? jc + 1 : P.jml;
  const bool in = icol && (i >= 2 && i <= P.imm1 && jc >= 2 && jc <= P.jmm1);
  const pomgpu_ct fsm = F2(fsm, i, jc);
  // column-resident coefficients of the west, south and north faces and of the cell
  const CoefT cw = coef_x(P, i, jc), cs = coef_y(P, i, jc), cn = coef_y(P, i, jn);
  const pomgpu_ct art = F2(art, i, jc), hea = K2(HEA, i, jc);
  const InvDc hfa = inv_of(CT(K2(HFA, i, jc)));
  const pomgpu_ct tprni = P.tprni, dti2 = P.dti2;
  BufA bs[NS], bo[2], bff[NF], bh[NH];
  const double *ps[NS];
#pragma unroll
  for (int f = 0; f < NF; f++) { ps[f] = A.fb[f]; ps[NF + f] = A.fcl[f]; bff[f] = BUF3(A.ff[f]); }
  ps[AM] = P.aamc; ps[VV] = A3(v); bo[0] = BUF3(A3(u)); bo[1] = BUF3(A3(w));
#pragma unroll
  for (int x = 0; x < NS; x++) bs[x] = BUF3(ps[x]);
  const RowShare<NS> S = rowshare_setup<NS>(P, r, j, j0w, i);
#pragma unroll
  for (int q = 0; q < NH; q++) bh[q] = BUF3(rowshare_pick<NS>(ps, S.hop[q]));
  const UvmC mu = UM ? uvm_of<0>(P, i, jc) : uvm_none(), mv = UM ? uvm_of<1>(P, i, jc) : uvm_none();
  UvmC mh[NH];
#pragma unroll
  for (int q = 0; q < NH; q++) mh[q] = UM ? rowshare_uvm<1, NS, LDS_ROWS>(P, S, q, VV, j0w, i) : uvm_none();
  const unsigned oc = BOFF2(i, jc), lvb = LVB;
  const unsigned ost = in ? oc : BOFF_NONE;
  const int rt_nbx = RT_NBX(P);
  const BufA brtf = buf2_of((const double *)A.rtf, RTF ? (size_t)P.kbm1 * P.jml * rt_nbx : 0);
  const unsigned ortf = (RTF && jrow && lane == 0) ? (unsigned)((jc - 1) * rt_nbx + (i0 - lane) / 62) * 8u : BOFF_NONE, lvrtf = (unsigned)(P.jml * rt_nbx) * 8u;
#ifndef POMGPU_EMU
  __shared__ pomgpu_ct slab[2][NS][ROWSHARE_ROWS][64];
#else
  const unsigned os = BOFF2(i, js), on = BOFF2(i, jn);
#endif
  auto load = [&](LevT<NF> &L, unsigned lv) {
#pragma unroll
    for (int x = 0; x < NS; x++) L.c[x] = bldc(bs[x], oc, lv);
    L.o[0] = bldc(bo[0], oc, lv); L.o[1] = bldc(bo[1], oc, lv);
#pragma unroll
    for (int q = 0; q < NH; q++) L.h[q] = bldc(bh[q], S.hoff[q], lv);
  };
  pomgpu_ct f1[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) f1[f] = G3(A.f[f], i, jc, 1);
  const int kbm1 = P.kbm1;
  // carried from level L-1 to its completion in iteration L
  pomgpu_ct p_adv[NF], p_dif[NF], p_fb[NF], p_zu[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) p_adv[f] = p_dif[f] = p_fb[f] = p_zu[f] = 0.;
  // one iteration: request level L+1 into `nxt`, park level L (`cur`) in the slab, evaluate its faces, finish level L-1.
  // (Tried: parking a level one iteration ahead, the level itself re-read from the slab, one register set less -- the
  // barrier then waits for nobody less than an iteration behind, but the LDS round trip of the own row sits in front of
  // every level's arithmetic: 3-5 % slower.)
  auto step = [&](const int L, const int par, const LevT<NF> &cur, LevT<NF> &nxt) {
    load(nxt, (unsigned)(L < kbm1 ? L : kbm1 - 1) * lvb);     // the last iterations re-request level kbm1
    NbrT<NS> nb;
    const pomgpu_ct v_c = uvm_fix(cur.c[VV], mv);
#ifndef POMGPU_EMU
#pragma unroll
    for (int x = 0; x < NS; x++) slab[par][x][r + 1][lane] = x == VV ? v_c : cur.c[x];
#pragma unroll
    for (int q = 0; q < NH; q++) slab[par][S.hop[q]][S.hrow[q]][lane] = uvm_fix(cur.h[q], mh[q]);
    __syncthreads();
#pragma unroll
    for (int x = 0; x < NS; x++) { nb.s[x] = slab[par][x][S.ss][lane]; nb.n[x] = slab[par][x][S.sn][lane]; }
#else
    const unsigned lvc = (unsigned)((L <= kbm1 ? L : kbm1) - 1) * lvb;
#pragma unroll
    for (int x = 0; x < NS; x++) { nb.s[x] = bldc(bs[x], os, lvc); nb.n[x] = bldc(bs[x], on, lvc); }
    nb.s[VV] = uvm_fix(nb.s[VV], uvm_of<1>(P, i, js)); nb.n[VV] = uvm_fix(nb.n[VV], uvm_of<1>(P, i, jn));
#endif
    const pomgpu_ct am_c = cur.c[AM], u_c = uvm_fix(cur.o[0], mu), w_c = cur.o[1];
    const pomgpu_ct am_w = halo_w(am_c, [&] { return G3(P.aamc, iw, jc, L); });
    InvDc dzk; dzk.b = dzk.y = 0.;
    if (L >= 2) { dzk.b = F1(dz, L - 1); dzk.y = R1(dz, L - 1); }
    if constexpr (RTF) {                                    // cur holds level min(L, kbm1); padding and halo lanes answer 0
      bool ch = false;
#pragma unroll
      for (int f = 0; f < NF; f++) ch = ch || rt_changes(cur.c[f], cur.c[NF + f]);
      const unsigned lvw = (unsigned)WAVE_UNIFORM(L - 1) * lvrtf;
#ifndef POMGPU_EMU
      bst2u(brtf, L <= kbm1 ? ortf : BOFF_NONE, lvw, __ballot(icol && ch));
#else
      if (L <= kbm1) {
        unsigned long long &wd = A.rtf[RT_WORD(P, i, jc, L)];
        wd = (lane == 1 ? 0ull : wd) | ((unsigned long long)ch << lane);
      }
      (void)brtf; (void)ortf; (void)lvw;
#endif
    }
#pragma unroll
    for (int f = 0; f < NF; f++) {
      const pomgpu_ct fb_c = cur.c[f], fc_c = cur.c[NF + f];
      pomgpu_ct zu = 0.;                                                           // top face of level L (0 below kbm1)
      pomgpu_ct s_adv = 0., s_dif = 0.;
      if (L <= kbm1) {
        const pomgpu_ct fb_w = halo_w(fb_c, [&] { return G3(A.fb[f], iw, jc, L); });
        const pomgpu_ct fc_w = halo_w(fc_c, [&] { return G3(A.fcl[f], iw, jc, L); });
        const FaceT xw = advt2_face(tprni, cw, u_c, fb_c, fb_w, fc_c, fc_w, am_c, am_w);
        auto east = [&] {                                   // emulation only: the east face from memory
          return advt2_face(tprni, coef_x(P, ie, jc), uvm_ld<0>(P, ie, jc, L), G3(A.fb[f], ie, jc, L), fb_c, G3(A.fcl[f], ie, jc, L), fc_c,
                            G3(P.aamc, ie, jc, L), am_c);
        };
        FaceT xe;
        xe.adv = halo_e(xw.adv, [&] { return east().adv; });
        xe.dif = halo_e(xw.dif, [&] { return east().dif; });
        const FaceT ys = advt2_face(tprni, cs, v_c, fb_c, nb.s[f], fc_c, nb.s[NF + f], am_c, nb.s[AM]);
        const FaceT yn = advt2_face(tprni, cn, nb.n[VV], nb.n[f], fb_c, nb.n[NF + f], fc_c, nb.n[AM], am_c);
        s_adv = xe.adv - xw.adv + yn.adv - ys.adv;                                            // solver.f:670-671
        s_dif = xe.dif - xw.dif + yn.dif - ys.dif;                                            // :721-722
        zu = (L == 1) ? w_c * f1[f] * art : upw_(w_c, fb_c, p_fb[f]) * art;                   // :646-662
      }
      {                                                     // finish level L-1: its bottom face is this level's top face
        pomgpu_ct rr = p_adv[f] + divi(p_zu[f] - zu, dzk);                                    // :670-672
        rr = divi(p_fb[f] * hea - dti2 * rr, hfa);                                            // :673-674
        rr = rr * fsm;                                                                        // :1899
        rr = rr - divi(dti2 * p_dif[f], hfa);                                                 // :721-723
        // every lane stores, every iteration: lanes without an interior column (and the first iteration, which has
        // no finished level yet) aim outside the buffer and the hardware drops the store
        bstc(bff[f], (L >= 2 && L <= kbm1 + 1) ? ost : BOFF_NONE, (unsigned)(L >= 2 ? L - 2 : 0) * lvb, rr);
      }
      p_adv[f] = s_adv; p_dif[f] = s_dif; p_fb[f] = fb_c; p_zu[f] = zu;
    }
  };
  // two register sets take turns as "current" and "next" level: no copy between iterations
  LevT<NF> ra, rb;
  load(ra, 0u);
  rb = ra;
  for (int L = 1; L <= kbm1 + 1; L += 2) {
    step(L, 1, ra, rb);
    step(L + 1, 0, rb, ra);                                 // for even kbm1 one iteration too many: its stores aim outside the buffer
  }
  // :1899 on what the loop did not write: level kb everywhere, every level of the rim cells.  AFTER the loop: a load
  // inside it (even one only rim lanes execute) makes the compiler wait for vmcnt(0) where the paths join
  if (icol) {
    for (int k = in ? P.kb : 1; k <= P.kb; k++) {
#pragma unroll
      for (int f = 0; f < NF; f++) G3(A.ff[f], i, jc, k) = CT(G3(A.ff[f], i, jc, k)) * fsm;
    }
  }
}

// ---- advq, flux + step fused (single tile) -- solver.f:411-477 -----------------------------------------
// Same structure as k_advt2_col: column-resident face coefficients, software-pipelined level loop,
// neighbour-lane operands.  The reference exchanges xflux/yflux between the flux and the step
// loops (:458-459); with all neighbours -1 that exchange is a no-op and the two halves fuse: the
// fluxes never reach memory.  Used only when the context has no exchange hook (one tile).
// NF = 2 advances q2 and q2l in ONE pass (advance.f:407-408 calls advq twice): u, v, w, aam and every
// face coefficient are read once for both -- 12.5 array passes instead of 2 x 9.5.
struct QFields { const double *q[2], *qb[2]; double *qf[2]; };
// operands of a level, shared through the workgroup's LDS slab in this order: q[0..NF-1], qb[0..NF-1], aam, v; own row only: u, w
// (NO = 1: the kernel forms w itself, see WF below, and only u remains)
template <int NF, int NO = 2> struct LevQa { pomgpu_ct c[2 * NF + 2], o[NO], h[ROWSHARE_SLOTS(2 * NF + 2)]; };
struct CoefQ { pomgpu_ct dts, hs, msk, ds_num; InvDc den; };
__device__ __forceinline__ CoefQ coefq_x(const KP &P, int i, int j) {
  CoefQ c; c.dts = K2(DTSX, i, j); c.hs = K2(HSX, i, j); c.msk = F2(dum, i, j); c.den = inv_of(CT(K2(DXSX, i, j))); c.ds_num = K2(DYSX, i, j); return c;
}
__device__ __forceinline__ CoefQ coefq_y(const KP &P, int i, int j) {
  CoefQ c; c.dts = K2(DTSY, i, j); c.hs = K2(HSY, i, j); c.msk = F2(dvm, i, j); c.den = inv_of(CT(K2(DYSY, i, j))); c.ds_num = K2(DXSY, i, j); return c;
}
// flux through the face between a "lo" (west/south) and a "hi" cell at w-level k (:428-453)
__device__ __forceinline__ pomgpu_ct advq_face(const CoefQ &c, pomgpu_ct q_hi, pomgpu_ct q_lo, pomgpu_ct vel_k, pomgpu_ct vel_km1, pomgpu_ct am_hi_k,
                                               pomgpu_ct am_lo_k, pomgpu_ct am_hi_m, pomgpu_ct am_lo_m, pomgpu_ct qb_hi, pomgpu_ct qb_lo) {
  pomgpu_ct x = CT(.125) * (q_hi + q_lo) * c.dts * (vel_k + vel_km1);
  x = x - divi(CT(.25) * (am_hi_k + am_lo_k + am_hi_m + am_lo_m) * c.hs * (qb_hi - qb_lo) * c.msk, c.den);
  return CT(.5) * c.ds_num * x;
}
// loop discipline and row sharing as in k_advt2_col
//
// WF: the kernel forms w on its way down instead of loading it -- vertvl (solver.f:1970-2021) with the fsm mask of bcondorl(5), as
// k_vertvl_rs (k_vert.hip) runs it in front of this kernel in mode_internal.  That routine is a running sum down the same levels on
// the same lanes, over operands this march already holds: u of the own row on all 64 lanes (the east neighbour's is one lane away), v
// and v(i,j+1) from the slab, and the previous level's copies of them.  Iteration L forms w(L) from level L-1's u_e, u, v_n, v, stores
// it where the kernel used to load it, and multiplies the STORED value -- masked on levels 1..kbm1, rounded to the storage type --
// with q(L): what the unfused kernel reads back.  The chain is fp64 (vertvl is fp64 in the fp32-storage build too) with
// k_vertvl_rs's expressions in k_vertvl_rs's order; nobody reads a neighbour column's w here, so no workgroup waits for another.
// Rim columns get vertvl's tail (w = w * fsm on levels 1..kbm1) after the loop.  The fp32-arithmetic variant, whose stencil kernels
// hold no fp64 arithmetic, does not instantiate WF and keeps the vertvl launch (POMGPU_W_FUSE).
// UM: as in k_advt2_col -- u, v corrected as they are loaded (levels 1..kbm1), w formed from the corrected values as vertvl follows
// advance.f:365-393
template <int NF, bool WF = false, bool UM = false>
__global__ void __launch_bounds__(64 * LDS_ROWS) k_advq_col(KP P, QFields A, int zero_else) {
  constexpr int NS = 2 * NF + 2, NH = ROWSHARE_SLOTS(NS), AM = 2 * NF, VV = 2 * NF + 1;
  typedef LevQa<NF, WF ? 1 : 2> Lev;
  HALO_XCD_DECODE_R(LDS_ROWS)
  const int r = WAVE_UNIFORM((int)threadIdx.y), j0w = j - r;
  const bool jrow = j <= P.jml;
  const int jc = jrow ? j : P.jml;
  const bool icol = jrow && (lane >= 1 && lane <= 62 && i0 <= P.iml);
#ifdef POMGPU_EMU
  if (!icol) return;
#endif
  const int i = i0 < 1 ? 1 : (i0 > P.iml ? P.iml : i0);
  const int iw = i > 1 ? i - 1 : 1, ie = i < P.iml ? i + 1 : P.iml;
  const int js = jc > 1 ? jc - 1 : 1, jn = jc < P.jml ? jc + 1 : P.jml;
  const bool in = icol && (i >= 2 && i <= P.imm1 && jc >= 2 && jc <= P.jmm1);
  const CoefQ cw = coefq_x(P, i, jc), cs = coefq_y(P, i, jc), cn = coefq_y(P, i, jn);
  const pomgpu_ct art = F2(art, i, jc), hea = K2(HEA, i, jc);
  const InvDc hfa = inv_of(CT(K2(HFA, i, jc)));
  const int kb = P.kb, kbm1 = P.kbm1;
  BufA bs[NS], bo[2], bqf[NF], bh[NH];
  const double *ps[NS];
#pragma unroll
  for (int f = 0; f < NF; f++) { ps[f] = A.q[f]; ps[NF + f] = A.qb[f]; bqf[f] = BUF3(A.qf[f]); }
  ps[AM] = P.aamc; ps[VV] = A3(v); bo[0] = BUF3(A3(u)); bo[1] = BUF3(A3(w));
#pragma unroll
  for (int x = 0; x < NS; x++) bs[x] = BUF3(ps[x]);
  const RowShare<NS> S = rowshare_setup<NS>(P, r, j, j0w, i);
#pragma unroll
  for (int q = 0; q < NH; q++) bh[q] = BUF3(rowshare_pick<NS>(ps, S.hop[q]));
  const UvmC mu = UM ? uvm_of<0>(P, i, jc) : uvm_none(), mv = UM ? uvm_of<1>(P, i, jc) : uvm_none();
  UvmC mh[NH];
#pragma unroll
  for (int q = 0; q < NH; q++) mh[q] = UM ? rowshare_uvm<1, NS, LDS_ROWS>(P, S, q, VV, j0w, i) : uvm_none();
  const unsigned oc = BOFF2(i, jc), lvb = LVB;
  // interior columns get the new value, every other owned column a zero (zero_else) or nothing
  const unsigned ost = in ? oc : ((zero_else && icol) ? oc : BOFF_NONE);
  const unsigned ostw = in ? oc : BOFF_NONE;                // w: interior columns only, as k_vertvl_rs stores it
#ifndef POMGPU_EMU
  __shared__ pomgpu_ct slab[2][NS][ROWSHARE_ROWS][64];
#else
  const unsigned os = BOFF2(i, js), on = BOFF2(i, jn);
#endif
  // WF: vertvl's column constants and start value (k_vertvl_rs: the same expressions in the same order)
  double vv_cw = 0., vv_ce = 0., vv_cs = 0., vv_cn = 0., vv_det = 0., vv_m = 0., wk = 0.;
  InvD vv_area; vv_area.b = vv_area.y = 0.;
  if constexpr (WF) {
    vv_m = F2(fsm, i, jc);
    const double dyc = F2(dy, i, jc), dtc = F2(dt, i, jc), dxc = F2(dx, i, jc);
    const double dyw = halo_w(dyc, [&] { return F2(dy, iw, jc); }), dtw = halo_w(dtc, [&] { return F2(dt, iw, jc); });
    const double dye = halo_e(dyc, [&] { return F2(dy, ie, jc); }), dte = halo_e(dtc, [&] { return F2(dt, ie, jc); });
    vv_cw = .25 * (dyc + dyw) * (dtc + dtw);
    vv_ce = .25 * (dye + dyc) * (dte + dtc);
    vv_cs = .25 * (dxc + F2(dx, i, js)) * (dtc + F2(dt, i, js));
    vv_cn = .25 * (F2(dx, i, jn) + dxc) * (F2(dt, i, jn) + dtc);
    vv_area = inv_of(dxc * dyc);
    vv_det = (F2(etf, i, jc) - F2(etb, i, jc)) / P.dti2;
    wk = 0.5 * (F2(vfluxb, i, jc) + F2(vfluxf, i, jc));                                      // :2004
  }
  auto load = [&](Lev &L, int k) {
    const unsigned lv = (unsigned)WAVE_UNIFORM(k - 1) * lvb;
#pragma unroll
    for (int x = 0; x < NS; x++) L.c[x] = bldc(bs[x], oc, lv);
    L.o[0] = bldc(bo[0], oc, lv);
    if constexpr (!WF) L.o[1] = bldc(bo[1], oc, lv);
#pragma unroll
    for (int q = 0; q < NH; q++) L.h[q] = bldc(bh[q], S.hoff[q], lv);
  };
  pomgpu_ct u_m = 0., v_m = 0., vn_m = 0., am_m = 0., ams_m = 0., amn_m = 0.;   // u, v, v(j+1), aam (c, s, n) of level L-1
  pomgpu_ct am_w_prv = 0.;                    // aam(i-1,j,L-1) as seen by this lane
  pomgpu_ct ue_m = 0.;                        // WF: u(i+1,j,L-1)
  pomgpu_ct wq_pp[NF], wq_p[NF];              // w*q of levels L-2 and L-1
  pomgpu_ct xe_p[NF], xw_p[NF], yn_p[NF], ys_p[NF], qb_p[NF];   // faces and qb of level L-1, waiting for w(L)*q(L)
#pragma unroll
  for (int f = 0; f < NF; f++) wq_pp[f] = wq_p[f] = xe_p[f] = xw_p[f] = yn_p[f] = ys_p[f] = qb_p[f] = 0.;
  auto step = [&](const int L, const int par, const Lev &cur, Lev &nxt) {
    load(nxt, L + 1 <= kb ? L + 1 : kb);                    // the last iterations re-request level kb
    NbrT<NS> nb;
    const bool lcor = L <= kbm1;                            // level kb of u, v is never corrected
    const pomgpu_ct v_c = uvm_fix(cur.c[VV], mv, lcor), u_c = uvm_fix(cur.o[0], mu, lcor);
#ifndef POMGPU_EMU
#pragma unroll
    for (int x = 0; x < NS; x++) slab[par][x][r + 1][lane] = x == VV ? v_c : cur.c[x];
#pragma unroll
    for (int q = 0; q < NH; q++) slab[par][S.hop[q]][S.hrow[q]][lane] = uvm_fix(cur.h[q], mh[q], lcor);
    __syncthreads();
#pragma unroll
    for (int x = 0; x < NS; x++) { nb.s[x] = slab[par][x][S.ss][lane]; nb.n[x] = slab[par][x][S.sn][lane]; }
#else
    const unsigned lvc = (unsigned)((L <= kb ? L : kb) - 1) * lvb;
#pragma unroll
    for (int x = 0; x < NS; x++) { nb.s[x] = bldc(bs[x], os, lvc); nb.n[x] = bldc(bs[x], on, lvc); }
    nb.s[VV] = uvm_fix(nb.s[VV], uvm_of<1>(P, i, js), lcor); nb.n[VV] = uvm_fix(nb.n[VV], uvm_of<1>(P, i, jn), lcor);
#endif
    const pomgpu_ct am_c = cur.c[AM];
    const pomgpu_ct am_s = nb.s[AM], am_n = nb.n[AM], v_n = nb.n[VV];
    const pomgpu_ct am_w = halo_w(am_c, [&] { return G3(P.aamc, iw, jc, L); });
    pomgpu_ct w_c, ue_c = 0.;
    if constexpr (WF) {
      ue_c = halo_e(u_c, [&] { return uvm_ld<0>(P, ie, jc, L); });
      // w(L) from level L-1 (solver.f:2006-2014); selects, no branch: iteration 1 keeps the start value.  The running sum is never masked
      const double wn = wk + F1(dz, L >= 2 ? L - 1 : 1) *
                             (divi(vv_ce * (double)ue_m - vv_cw * (double)u_m + vv_cn * (double)vn_m - vv_cs * (double)v_m, vv_area) + vv_det);
      wk = L >= 2 ? wn : wk;
      const double wst = L <= kbm1 ? wk * vv_m : wk;        // bcondorl(5)'s mask on levels 1..kbm1
      bst(bo[1], ostw, (unsigned)WAVE_UNIFORM(L - 1) * lvb, wst);
      w_c = CT((pomgpu_st)wst);                             // what the unfused kernel loads: the stored value
    } else {
      w_c = cur.o[1];
    }
    const int k = L - 1;                                    // level completed in this iteration
    InvDc dz2; dz2.b = dz2.y = 0.;
    if (k >= 2 && k <= kbm1) { dz2.b = CT(F1(dz, k)) + CT(F1(dz, k - 1)); dz2.y = CT(1.0) / dz2.b; }
#pragma unroll
    for (int f = 0; f < NF; f++) {
      const pomgpu_ct q_c = cur.c[f], qb_c = cur.c[NF + f];
      pomgpu_ct xe_c = 0., xw_c = 0., yn_c = 0., ys_c = 0.;
      if (L >= 2 && L <= kbm1) {
        const pomgpu_ct q_w = halo_w(q_c, [&] { return G3(A.q[f], iw, jc, L); });
        const pomgpu_ct qb_w = halo_w(qb_c, [&] { return G3(A.qb[f], iw, jc, L); });
        const pomgpu_ct xw = advq_face(cw, q_c, q_w, u_c, u_m, am_c, am_w, am_m, am_w_prv, qb_c, qb_w);
        xw_c = xw;
        xe_c = halo_e(xw, [&] {                             // emulation only: the east face from memory
          return advq_face(coefq_x(P, ie, jc), G3(A.q[f], ie, jc, L), q_c, uvm_ld<0>(P, ie, jc, L), uvm_ld<0>(P, ie, jc, L - 1), G3(P.aamc, ie, jc, L), am_c,
                           G3(P.aamc, ie, jc, L - 1), am_m, G3(A.qb[f], ie, jc, L), qb_c);
        });
        ys_c = advq_face(cs, q_c, nb.s[f], v_c, v_m, am_c, am_s, am_m, ams_m, qb_c, nb.s[NF + f]);
        yn_c = advq_face(cn, nb.n[f], q_c, v_n, vn_m, am_n, am_c, amn_m, am_m, nb.n[NF + f], qb_c);
      }
      const pomgpu_ct wq_c = w_c * q_c;
      {
        pomgpu_ct rr = 0.;
        if (in && k >= 2 && k <= kbm1) {
          rr = divi((wq_pp[f] - wq_c) * art, dz2) + xe_p[f] - xw_p[f] + yn_p[f] - ys_p[f];    // :465-468
          rr = divi(hea * qb_p[f] - CT(P.dti2) * rr, hfa);                                    // :469-471
        }
        // levels 2..kbm1 of interior columns: the new value; with zero_else every other owned cell (levels 1..kb-1 here,
        // kb below): zero; everything else aims outside the buffer
        const bool lev_in = (k >= 2 && k <= kbm1);
        const unsigned o = (k >= 1) ? (lev_in ? ost : ((zero_else && icol) ? oc : BOFF_NONE)) : BOFF_NONE;
        bstc(bqf[f], o, (unsigned)WAVE_UNIFORM(k >= 1 ? k - 1 : 0) * lvb, rr);
      }
      wq_pp[f] = wq_p[f]; wq_p[f] = wq_c; qb_p[f] = qb_c;
      xe_p[f] = xe_c; xw_p[f] = xw_c; yn_p[f] = yn_c; ys_p[f] = ys_c;
    }
    am_w_prv = am_w;
    if constexpr (WF) ue_m = ue_c;
    u_m = u_c; v_m = v_c; vn_m = v_n; am_m = am_c; ams_m = am_s; amn_m = am_n;
  };
  Lev ra, rb;
  load(ra, 1);
  rb = ra;
  for (int L = 1; L <= kb; L += 2) {
    step(L, 1, ra, rb);
    if (L + 1 <= kb) step(L + 1, 0, rb, ra);                // uniform for the whole workgroup (barrier inside)
  }
  if (icol && zero_else) {
#pragma unroll
    for (int f = 0; f < NF; f++) G3(A.qf[f], i, jc, kb) = 0.;
  }
  if constexpr (WF) {                                       // rim columns: the mask of bcondorl(5) alone (k_vertvl_rs's tail).  After the loop, as in k_advt2_col
    if (icol && !in && i0 <= P.im && jc <= P.jm)
      for (int k = 1; k <= kbm1; k++) F3(w, i, jc, k) = F3(w, i, jc, k) * vv_m;
  }
}

// ---- advct, all three phases fused (single tile) -- solver.f:201-408 ------------------------------------
// The reference forms curv, xflux, yflux, exchanges them, forms advx and a second set of fluxes,
// exchanges, forms advy: 27 array passes through the three cell kernels of k_adv.hip (PMC: 33.7 GB per
// launch against 8.8 GB for "read u,v,ub,vb,aam, write advx,advy").  With all neighbours -1 nothing is
// exchanged and every flux is a function of the five operands around (i,j,k), so the fluxes stay in
// registers.  There is no vertical coupling; the level loop exists to keep the 28 two-dimensional
// coefficients of a column in registers and to have the next level's 15 row loads in flight.
//
// Lane map: a wavefront covers 64 consecutive columns but only lanes 1..62 own an output column;
// lanes 0 and 63 are HALO lanes that load their column and feed the shuffles (lane 0 supplies the
// west operands / west face flux of lane 1, lane 63 the east operands / corner flux of lane 62), so
// no lane ever needs a mid-iteration fallback load (vmcnt is in-order) and no flux is evaluated
// from memory.  Wave w covers columns 62w .. 62w+63.
// the same quantities evaluated from memory (emulation fallbacks only); i, j inside the tile
// am: the array that holds the aam being read (its slot, or the spare array while k_advct_col<*, true> reads it there)
__device__ double advct_xf_mem(const KP &P, const double *am, int i, int j, int k) {                 // x-eq. xflux, 2<=j
  if (i < 2 || i > P.imm1) return 0.;
  double xf = .125 * (K2(DTSX, i + 1, j) * F3(u, i + 1, j, k) + K2(DTSX, i, j) * F3(u, i, j, k)) * (F3(u, i + 1, j, k) + F3(u, i, j, k));
  xf = xf - F2(dt, i, j) * G3(am, i, j, k) * 2. * (F3(ub, i + 1, j, k) - F3(ub, i, j, k)) / F2(dx, i, j);
  return F2(dy, i, j) * xf;
}
__device__ double advct_curv_mem(const KP &P, int i, int j, int k) {
  if (i < 2 || i > P.imm1 || j < 2 || j > P.jmm1) return 0.;
  return .25 * ((F3(v, i, j + 1, k) + F3(v, i, j, k)) * K2(CVA, i, j) - (F3(u, i + 1, j, k) + F3(u, i, j, k)) * K2(CVB, i, j)) / F2(art, i, j);
}
__device__ double advct_xg_mem(const KP &P, const double *am, int i, int j, int k) {                 // y-eq. xflux at corner (i,j), 2<=i, 2<=j<=jmm1
  double xg = .125 * (K2(DTSX, i, j) * F3(u, i, j, k) + K2(DTSX, i, j - 1) * F3(u, i, j - 1, k)) * (F3(v, i, j, k) + F3(v, i - 1, j, k));
  const double dtaam = .25 * K2(DT4, i, j) * (G3(am, i, j, k) + G3(am, i - 1, j, k) + G3(am, i, j - 1, k) + G3(am, i - 1, j - 1, k));
  const double dy4 = K2(DY4, i, j);
  xg = xg - dtaam * ((F3(ub, i, j, k) - F3(ub, i, j - 1, k)) / dy4 + (F3(vb, i, j, k) - F3(vb, i - 1, j, k)) / K2(DX4, i, j));
  return .25 * dy4 * xg;
}
__device__ double advct_yf_mem(const KP &P, const double *am, int i, int j, int k) {                 // x-eq. yflux at corner (i,j), 2<=i<=imm1, 2<=j
  double yf = .125 * (K2(DTSY, i, j) * F3(v, i, j, k) + K2(DTSY, i - 1, j) * F3(v, i - 1, j, k)) * (F3(u, i, j, k) + F3(u, i, j - 1, k));
  const double dtaam = .25 * K2(DT4, i, j) * (G3(am, i, j, k) + G3(am, i - 1, j, k) + G3(am, i, j - 1, k) + G3(am, i - 1, j - 1, k));
  const double dx4 = K2(DX4, i, j);
  yf = yf - dtaam * ((F3(ub, i, j, k) - F3(ub, i, j - 1, k)) / K2(DY4, i, j) + (F3(vb, i, j, k) - F3(vb, i - 1, j, k)) / dx4);
  return .25 * dx4 * yf;
}
__device__ double advct_yg_mem(const KP &P, const double *am, int i, int j, int k) {                 // y-eq. yflux at the centre of (i,j), 2<=i, 2<=j<=jmm1
  double yg = .125 * (K2(DTSY, i, j + 1) * F3(v, i, j + 1, k) + K2(DTSY, i, j) * F3(v, i, j, k)) * (F3(v, i, j + 1, k) + F3(v, i, j, k));
  yg = yg - F2(dt, i, j) * G3(am, i, j, k) * 2. * (F3(vb, i, j + 1, k) - F3(vb, i, j, k)) / F2(dy, i, j);
  return F2(dx, i, j) * yg;
}
// advct on tiles without exchanging whole intermediate arrays.  What a tile cannot form itself is little: advx(2,j)
// needs xflux(1,j) and curv(1,j) (solver.f:284-301), advy(i,2) needs the y-equation's yflux(i,1) and curv(i,1)
// (:374-391) -- in the reference they arrive with the exchanges of curv, xflux, yflux (:229, :279, :369).  Here the
// neighbour evaluates just those lines (k_advct_edge: its column imm1 / row jmm1, the same formulas on the same
// operands) and sends them east / north in one small message; k_advct_col then runs as on a single tile and
// k_advct_fix redoes advx(2,:) and advy(:,2) with the received values.  Message layout: curv, then the flux,
// each kbm1 x jm (east) or kbm1 x im (north), level-major.
__global__ void k_advct_edge(KP P, double *to_e, double *to_n) {
  const int t = TID_I, k = (int)blockIdx.y + 1;
  if (k > P.kbm1) return;
  if (to_e && t <= P.jm) {
    const size_t o = (size_t)(k - 1) * P.jm + (size_t)(t - 1);
    to_e[o] = advct_curv_mem(P, P.imm1, t, k);
    to_e[(size_t)P.kbm1 * P.jm + o] = t >= 2 ? advct_xf_mem(P, A3(aam), P.imm1, t, k) : 0.;
  }
  if (to_n && t <= P.im) {
    const size_t o = (size_t)(k - 1) * P.im + (size_t)(t - 1);
    to_n[o] = advct_curv_mem(P, t, P.jmm1, k);
    to_n[(size_t)P.kbm1 * P.im + o] = t >= 2 ? advct_yg_mem(P, A3(aam), t, P.jmm1, k) : 0.;
  }
}
__global__ void k_advct_fix(KP P, const double *from_w, const double *from_s) {
  const int t = TID_I, k = (int)blockIdx.y + 1;
  if (k > P.kbm1) return;
  if (from_w && t >= 2 && t <= P.jmm1) {                     // advx(2,j,k), j = t
    const int j = t;
    const size_t o = (size_t)(k - 1) * P.jm + (size_t)(j - 1);
    const double cv_w = from_w[o], xf_w = from_w[(size_t)P.kbm1 * P.jm + o];
    const double xf = advct_xf_mem(P, A3(aam), 2, j, k), yf_n = advct_yf_mem(P, A3(aam), 2, j + 1, k), yf_c = advct_yf_mem(P, A3(aam), 2, j, k);
    const double cv = advct_curv_mem(P, 2, j, k);
    const double ctx = cv * F2(dt, 2, j) * (F3(v, 2, j + 1, k) + F3(v, 2, j, k));
    const double ctx_w = cv_w * F2(dt, 1, j) * (F3(v, 1, j + 1, k) + F3(v, 1, j, k));
    double ax = xf - xf_w + yf_n - yf_c;                                                         // :284-288
    ax = ax - F2(aru, 2, j) * .25 * (ctx + ctx_w);                                               // :291-301
    F3(advx, 2, j, k) = ax;
  }
  if (from_s && t >= 2 && t <= P.imm1) {                     // advy(i,2,k), i = t
    const int i = t;
    const size_t o = (size_t)(k - 1) * P.im + (size_t)(i - 1);
    const double cv_s = from_s[o], yg_s = from_s[(size_t)P.kbm1 * P.im + o];
    const double xg_e = advct_xg_mem(P, A3(aam), i + 1, 2, k), xg = advct_xg_mem(P, A3(aam), i, 2, k), yg_c = advct_yg_mem(P, A3(aam), i, 2, k);
    const double cv = advct_curv_mem(P, i, 2, k);
    double ay = xg_e - xg + yg_c - yg_s;                                                         // :374-378
    ay = ay + F2(arv, i, 2) * .25 * (cv * F2(dt, i, 2) * (F3(u, i + 1, 2, k) + F3(u, i, 2, k)) +
                                     cv_s * F2(dt, i, 1) * (F3(u, i + 1, 1, k) + F3(u, i, 1, k)));     // :381-391
    F3(advy, i, 2, k) = ay;
  }
}
// sum2d: also leave the vertical integrals adx2d, ady2d of advance.f:152-168 (k_vint) -- the column is here anyway
// Operands of a level, all five shared through the workgroup's LDS slab (rows j-1, j, j+1): u, v, ub, vb, aam.
// Loop discipline and row sharing as in k_advt2_col.
// sum2d bit 1 (one tile): also leave su = sum_k u(k)*dz(k), sv = sum_k v(k)*dz(k) of every owned column (C2_USUM, C2_VSUM), the sums
// advance.f:365-372 forms at the head of mode_internal -- nothing writes u, v between here and there -- in that loop's order, fp64
// ROWS rows per workgroup: 8 (LDS_ROWS) on large grids; 4 on low tiles, where a launch is only three or four rounds of workgroups and two
// workgroups per compute unit leave the last round fuller (launch_advct_col)
// AAM (one tile, lateral_viscosity's aam_fused; never in the fp32-arithmetic variant, POMGPU_AAM_FUSE): iteration k also forms the NEW
// aam(i,j,k) of advance.f:122-136 from the raw u, v it holds -- three more east shifts: u(i+1,j+1), v(i+1,j), v(i+1,j+1) -- with
// aam_point_r (pomgpu_internal.hpp, the expression k_aam_pair evaluates), and stores it to aam_w, which is never the array being read
// (ps[AM] = KP::aamc): this launch reads the old aam of rows and columns other workgroups own.  Every owned cell of levels 1..kbm1 is
// stored, the rim rows and columns with the old value as loaded, so that aam_w is the whole current aam afterwards.  aam2d (advance.f:
// 158-168) is one more running sum, of the value as stored (rounded to the storage type), in k_vint's order, fp64 in every build.
template <int ROWS> struct LevCaT { pomgpu_ct c[5], h[(2 * 5 + ROWS - 1) / ROWS]; };
template <int ROWS, bool AAM = false>
__global__ void __launch_bounds__(64 * ROWS) k_advct_col(KP P, int sum2d, double *aam_w) {
  constexpr int NS = 5, NH = (2 * NS + ROWS - 1) / ROWS, U = 0, V = 1, UB = 2, VB = 3, AM = 4;
  typedef LevCaT<ROWS> LevCa;
  HALO_XCD_DECODE_R(ROWS)                                               // i0: 1-based column of this lane (0 for the very first halo lane)
#ifdef POMGPU_WGTIME                                        // developer build (tools/wg_times.py): when does each workgroup run, and where?
  const unsigned long long wgt0 = wall_clock64();
#endif
  const int r = WAVE_UNIFORM((int)threadIdx.y), j0w = j - r;
  const bool jvalid = j <= P.jml;                           // rows beyond the tile shadow row jml and store nothing
  const int jc = jvalid ? j : P.jml;
  const bool out = jvalid && (lane >= 1 && lane <= 62 && i0 <= P.iml);
#ifdef POMGPU_EMU
  if (!out) return;
#endif
  const int i = i0 < 1 ? 1 : (i0 > P.iml ? P.iml : i0);
  const int iw = i > 1 ? i - 1 : 1, ie = i < P.iml ? i + 1 : P.iml;
  const int js = jc > 1 ? jc - 1 : 1, jn = jc < P.jml ? jc + 1 : P.jml;
  const bool jrow = (jc >= 2 && jc <= P.jmm1);
  const bool iin = (i0 >= 2 && i0 <= P.imm1);
  const bool in = out && iin && jrow;
  const int kb = P.kb, kbm1 = P.kbm1;
  double ax2 = 0., ay2 = 0.;                                // the vertical sums stay fp64 in every build: they feed the external mode
#if POMGPU_UVM_ONLOAD
  double su2 = 0., sv2 = 0.;
#endif
  double am2 = 0.;                                          // AAM: sum_k aam(k)*dz(k) of the new aam
  // column-resident coefficients
  const pomgpu_ct dtsx_c = K2(DTSX, i, jc), dtsx_s = K2(DTSX, i, js);
  const pomgpu_ct dtsx_e = halo_e(dtsx_c, [&] { return K2(DTSX, ie, jc); });
  const pomgpu_ct dtsy_c = K2(DTSY, i, jc), dtsy_n = K2(DTSY, i, jn), dtsy_s = K2(DTSY, i, js);
  const pomgpu_ct dtsy_w = halo_w(dtsy_c, [&] { return K2(DTSY, iw, jc); });
  const pomgpu_ct dtsy_nw = halo_w(dtsy_n, [&] { return K2(DTSY, iw, jn); });
  const pomgpu_ct dt4_c = K2(DT4, i, jc), dt4_n = K2(DT4, i, jn);
  const pomgpu_ct dx4_c = K2(DX4, i, jc), dx4_n = K2(DX4, i, jn);
  const InvDc dy4_c = inv_of(CT(K2(DY4, i, jc))), dy4_n = inv_of(CT(K2(DY4, i, jn))), idx4_c = inv_of(dx4_c), idx4_n = inv_of(dx4_n);
  const pomgpu_ct dt_c = F2(dt, i, jc), dy_c = F2(dy, i, jc), dx_c = F2(dx, i, jc);
  const pomgpu_ct dt_s = F2(dt, i, js), dx_s = F2(dx, i, js);
  const InvDc idx_c = inv_of(dx_c), idy_c = inv_of(dy_c), idy_s = inv_of(CT(F2(dy, i, js)));
  const pomgpu_ct cva_c = K2(CVA, i, jc), cvb_c = K2(CVB, i, jc);
  const pomgpu_ct cva_s = K2(CVA, i, js), cvb_s = K2(CVB, i, js);
  const InvDc art_c = inv_of(CT(F2(art, i, jc))), art_s = inv_of(CT(F2(art, i, js)));
  const pomgpu_ct aru = F2(aru, i, jc), arv = F2(arv, i, jc);
  const bool srow = (jc - 1 >= 2);                          // row j-1 carries y-eq. fluxes / curv
  const bool curvx = (i0 >= (P.W ? 3 : 2)), curvy = (jc >= (P.S ? 3 : 2));
  BufA bs[NS], bh[NH];
  const double *ps[NS] = {A3(u), A3(v), A3(ub), A3(vb), AAM ? P.aamc : A3(aam)};
#pragma unroll
  for (int x = 0; x < NS; x++) bs[x] = BUF3(ps[x]);
  const BufA bax = BUF3(A3(advx)), bay = BUF3(A3(advy)), baw = BUF3(AAM ? aam_w : A3(advx));
  const RowShare<NS, ROWS> S = rowshare_setup<NS, ROWS>(P, r, j, j0w, i);
#pragma unroll
  for (int q = 0; q < NH; q++) bh[q] = BUF3(rowshare_pick<NS>(ps, S.hop[q]));
  const unsigned oc = BOFF2(i, jc), lvb = LVB;
  const unsigned ost = (out && jrow) ? oc : BOFF_NONE;      // rim rows are zeroed after the loop
  const unsigned osta = out ? oc : BOFF_NONE;               // AAM: every owned cell, rim rows included
#ifndef POMGPU_EMU
  __shared__ pomgpu_ct slab[2][NS][ROWS + 3][64];
#else
  const unsigned os = BOFF2(i, js), on = BOFF2(i, jn);
#endif
  auto load = [&](LevCa &L, int k) {
    const unsigned lv = (unsigned)WAVE_UNIFORM(k - 1) * lvb;
#pragma unroll
    for (int x = 0; x < NS; x++) L.c[x] = bldc(bs[x], oc, lv);
#pragma unroll
    for (int q = 0; q < NH; q++) L.h[q] = bldc(bh[q], S.hoff[q], lv);
  };
  auto step = [&](const int k, const int par, const LevCa &cur, LevCa &nxt) {
    load(nxt, k + 1 <= kbm1 ? k + 1 : kbm1);                // in flight during this iteration (the last one re-requests level kbm1)
    NbrT<NS> nb;
#ifndef POMGPU_EMU
#pragma unroll
    for (int x = 0; x < NS; x++) slab[par][x][r + 1][lane] = cur.c[x];
#pragma unroll
    for (int q = 0; q < NH; q++) slab[par][S.hop[q]][S.hrow[q]][lane] = cur.h[q];
    __syncthreads();
#pragma unroll
    for (int x = 0; x < NS; x++) { nb.s[x] = slab[par][x][S.ss][lane]; nb.n[x] = slab[par][x][S.sn][lane]; }
#else
    const unsigned lvc = (unsigned)(k - 1) * lvb;
#pragma unroll
    for (int x = 0; x < NS; x++) { nb.s[x] = bldc(bs[x], os, lvc); nb.n[x] = bldc(bs[x], on, lvc); }
#endif
    const pomgpu_ct u_c = cur.c[U], v_c = cur.c[V], ub_c = cur.c[UB], vb_c = cur.c[VB], am_c = cur.c[AM];
    const pomgpu_ct u_s = nb.s[U], v_s = nb.s[V], ub_s = nb.s[UB], vb_s = nb.s[VB], am_s = nb.s[AM];
    const pomgpu_ct u_n = nb.n[U], v_n = nb.n[V], ub_n = nb.n[UB], vb_n = nb.n[VB], am_n = nb.n[AM];
    const pomgpu_ct u_e = halo_e(u_c, [&] { return F3(u, ie, jc, k); });
    const pomgpu_ct u_se = halo_e(u_s, [&] { return F3(u, ie, js, k); });
    const pomgpu_ct ub_e = halo_e(ub_c, [&] { return F3(ub, ie, jc, k); });
    const pomgpu_ct v_w = halo_w(v_c, [&] { return F3(v, iw, jc, k); });
    const pomgpu_ct v_nw = halo_w(v_n, [&] { return F3(v, iw, jn, k); });
    const pomgpu_ct vb_w = halo_w(vb_c, [&] { return F3(vb, iw, jc, k); });
    const pomgpu_ct vb_nw = halo_w(vb_n, [&] { return F3(vb, iw, jn, k); });
    const pomgpu_ct am_w = halo_w(am_c, [&] { return G3(ps[AM], iw, jc, k); });
    const pomgpu_ct am_sw = halo_w(am_s, [&] { return G3(ps[AM], iw, js, k); });
    const pomgpu_ct am_nw = halo_w(am_n, [&] { return G3(ps[AM], iw, jn, k); });
    // x-equation xflux at the cell centre (:233-239, :257-262, :275); 0 outside 2..imm1
    pomgpu_ct xf = 0., cv = 0.;
    if (iin) {
      xf = CT(.125) * (dtsx_e * u_e + dtsx_c * u_c) * (u_e + u_c);
      xf = xf - divi(dt_c * am_c * CT(2.) * (ub_e - ub_c), idx_c);
      xf = dy_c * xf;
      cv = divi(CT(.25) * ((v_n + v_c) * cva_c - (u_e + u_c) * cvb_c), art_c);                     // :217-227
    }
    const pomgpu_ct ctx = cv * dt_c * (v_n + v_c);                                                // :296-297
    const pomgpu_ct xf_w = halo_w(xf, [&] { return advct_xf_mem(P, ps[AM], i - 1, jc, k); });
    const pomgpu_ct ctx_w = halo_w(ctx, [&] {
      return advct_curv_mem(P, i - 1, jc, k) * F2(dt, i - 1, jc) * (F3(v, i - 1, jc + 1, k) + F3(v, i - 1, jc, k));
    });
    // corner (i,j): y-flux of the x-equation and x-flux of the y-equation share dtaam and the shear bracket
    const pomgpu_ct dtaam = CT(.25) * dt4_c * (am_c + am_w + am_s + am_sw);                           // :264-266
    const pomgpu_ct br = divi(ub_c - ub_s, dy4_c) + divi(vb_c - vb_w, idx4_c);
    pomgpu_ct yf_c = CT(.125) * (dtsy_c * v_c + dtsy_w * v_w) * (u_c + u_s);                          // :244-250
    yf_c = yf_c - dtaam * br;                                                                  // :267-272
    yf_c = CT(.25) * dx4_c * yf_c;                                                                 // :276-277
    pomgpu_ct xg = CT(.125) * (dtsx_c * u_c + dtsx_s * u_s) * (v_c + v_w);                            // :322-328
    xg = xg - dtaam * br;                                                                      // :348-353
    xg = CT(.25) * dy4_c.b * xg;                                                                   // :363-364
    const pomgpu_ct xg_e = halo_e(xg, [&] { return advct_xg_mem(P, ps[AM], i + 1, jc, k); });
    // corner (i,j+1): y-flux of the x-equation only
    const pomgpu_ct dtaam_n = CT(.25) * dt4_n * (am_n + am_nw + am_c + am_w);
    pomgpu_ct yf_n = CT(.125) * (dtsy_n * v_n + dtsy_nw * v_nw) * (u_n + u_c);
    yf_n = yf_n - dtaam_n * (divi(ub_n - ub_c, dy4_n) + divi(vb_n - vb_nw, idx4_n));
    yf_n = CT(.25) * dx4_n * yf_n;
    // y-equation yflux at the centres of rows j and j-1 (:333-339, :355-358, :365)
    pomgpu_ct yg_c = CT(.125) * (dtsy_n * v_n + dtsy_c * v_c) * (v_n + v_c);
    yg_c = yg_c - divi(dt_c * am_c * CT(2.) * (vb_n - vb_c), idy_c);
    yg_c = dx_c * yg_c;
    pomgpu_ct yg_s = 0., cv_s = 0.;
    if (srow) {
      yg_s = CT(.125) * (dtsy_c * v_c + dtsy_s * v_s) * (v_c + v_s);
      yg_s = yg_s - divi(dt_s * am_s * CT(2.) * (vb_c - vb_s), idy_s);
      yg_s = dx_s * yg_s;
      if (iin) cv_s = divi(CT(.25) * ((v_c + v_s) * cva_s - (u_se + u_s) * cvb_s), art_s);
    }
    pomgpu_ct ax = 0., ay = 0.;
    if (in) {
      ax = xf - xf_w + yf_n - yf_c;                                                            // :284-288
      if (curvx) ax = ax - aru * CT(.25) * (ctx + ctx_w);                                          // :291-301
      ay = xg_e - xg + yg_c - yg_s;                                                            // :374-378
      if (curvy) ay = ay + arv * CT(.25) * (cv * dt_c * (u_e + u_c) + cv_s * dt_s * (u_se + u_s));   // :381-391
    }
    const unsigned lv = (unsigned)WAVE_UNIFORM(k - 1) * lvb;
    bstc(bax, ost, lv, ax);
    bstc(bay, ost, lv, ay);
    const double dzk = F1(dz, k);
    ax2 = ax2 + ax * dzk;
    ay2 = ay2 + ay * dzk;
#if POMGPU_UVM_ONLOAD
    su2 = su2 + (double)u_c * dzk;                                                             // advance.f:365-372
    sv2 = sv2 + (double)v_c * dzk;
#endif
#if POMGPU_AAM_FUSE
    if constexpr (AAM) {                                                                       // advance.f:122-136, :158-168
      const double u_ne = halo_e(u_n, [&] { return F3(u, ie, jn, k); });
      const double v_e = halo_e(v_c, [&] { return F3(v, ie, jc, k); });
      const double v_ne = halo_e(v_n, [&] { return F3(v, ie, jn, k); });
      double an = am_c;                                     // off the interior: the old value, as loaded
      if (in) an = aam_point_r(P, idx_c, idy_c, u_c, u_e, u_n, u_ne, u_s, u_se, v_c, v_n, v_e, v_ne, v_w, v_nw);
      bstc(baw, osta, lv, an);
      am2 = am2 + (double)(pomgpu_st)an * dzk;              // the value as stored: what k_vint would read back
    }
#endif
  };
  LevCa ra, rb;
#ifdef POMGPU_EMU
  if (jrow) {                                               // the emulation's neighbour fallbacks reach beyond a rim row
#endif
  load(ra, 1);
  rb = ra;
  for (int k = 1; k <= kbm1; k += 2) {
    step(k, 1, ra, rb);
    if (k + 1 <= kbm1) step(k + 1, 0, rb, ra);              // uniform for the whole workgroup (barrier inside)
  }
#ifdef POMGPU_EMU
  }
#if POMGPU_UVM_ONLOAD
  else {                                                    // a rim row's sums: the march above does not run there in the emulation
    for (int k = 1; k <= kbm1; k++) { su2 = su2 + (double)F3(u, i, jc, k) * F1(dz, k); sv2 = sv2 + (double)F3(v, i, jc, k) * F1(dz, k); }
  }
#endif
  if (AAM && !jrow)                                         // ... nor its copy of the old aam and its share of aam2d
    for (int k = 1; k <= kbm1; k++) {
      const double an = bldc(bs[AM], oc, (unsigned)(k - 1) * lvb);
      bstc(baw, osta, (unsigned)(k - 1) * lvb, an);
      am2 = am2 + (double)(pomgpu_st)an * F1(dz, k);
    }
#endif
#if POMGPU_UVM_ONLOAD
  if (out && (sum2d & 2)) { K2(USUM, i, jc) = su2; K2(VSUM, i, jc) = sv2; }
#endif
  if (out) {
    if (jrow) {
      F3(advx, i, jc, kb) = 0.; F3(advy, i, jc, kb) = 0.;
    } else {                                                // rim rows: advx = advy = 0 (solver.f:211,:317)
      for (int k = 1; k <= kb; k++) { F3(advx, i, jc, k) = 0.; F3(advy, i, jc, k) = 0.; }
    }
    if (sum2d & 1) { F2(adx2d, i, jc) = jrow ? ax2 : 0.; F2(ady2d, i, jc) = jrow ? ay2 : 0.; }
    if (AAM) F2(aam2d, i, jc) = (i <= P.im && jc <= P.jm) ? am2 : 0.;   // the cells and values k_vint(only_aam) writes
  }
#ifdef POMGPU_WGTIME
  __syncthreads();
  if (threadIdx.y == 0 && lane == 0) {                      // four doubles per workgroup into wr (a diagnostic array nothing reads here)
    double *rec = (double *)(P.b3 + (size_t)P3_wr * P.a3) + 4 * (size_t)L__;
    rec[0] = (double)wgt0; rec[1] = (double)wall_clock64();
    rec[2] = (double)__builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_ID: wave, simd, pipe, cu, sh, se ...
    rec[3] = (double)__builtin_amdgcn_s_getreg((31 << 11) | 20);    // XCC_ID
  }
#endif
}

// ---- advu + advv in one pass -- solver.f:734-788, :791-845 --------------------------------------------
// The two leapfrog steps share w, u, v: read together they cost 9 array reads + 2 writes instead of
// 2 x (7 + 1) through the fused solve kernels of k_vert.hip, and the tridiagonal solves that follow
// (k_profuv_reg) then need only their right-hand side and km.  Column-marching, halo-lane wavefronts:
// the level loop carries the vertical fluxes, the (i-1) / (i+1) operands are neighbour-lane values.
// Columns outside the interior get the reference's left-over vertical flux (:744-751, :801-808).
// Operands of iteration k.  Shared with the rows next to this one through the workgroup's LDS slabs: w, u, v of level
// k+1 (c: own row, h: this wavefront's share of the two rows outside the workgroup); own row only, level k: ub, vb, advx,
// advy, drhox, drhoy.  The row south of u and the row north of v are needed at level k -- one level behind what is being
// parked -- so the slabs rotate through THREE buffers: level L lives in slab (L-1) % 3, iteration k fills the slab of
// level k+1 and reads that of level k, and the slab it will overwrite two iterations later is out of everybody's reach
// behind two barriers.  (PMC before: 14.8 array passes of HBM-side traffic for 11 algorithmic -- the three neighbour rows
// were never L2 hits.)
struct LevUV { pomgpu_ct c[3], h[ROWSHARE_SLOTS(3)], ub, vb, advx, advy, drhox, drhoy; };
// Same loop discipline as k_advt2_col: one batch of loads per level, issued a whole iteration ahead and never inside a
// branch, stores of lanes without an output column aimed outside the buffer, buffer addressing, two register sets.
// UM: as in k_advt2_col -- u, v corrected as they are loaded and before they enter a slab (levels 1..kbm1; the last iteration loads
// level kb, which nothing uses); a halo job may carry u or v: it takes that component's coefficients of the row it loads
template <bool UM>
__global__ void __launch_bounds__(64 * LDS_ROWS) k_advuv_col(KP P) {
  constexpr int NS = 3, NH = ROWSHARE_SLOTS(NS), W = 0, U = 1, V = 2;
  HALO_XCD_DECODE_R(LDS_ROWS)
  const int r = WAVE_UNIFORM((int)threadIdx.y), j0w = j - r;
  const bool jvalid = j <= P.jm;                            // rows beyond the tile shadow row jm and store nothing
  const int jc = j <= P.jml ? j : P.jml;
  const bool out = jvalid && (lane >= 1 && lane <= 62 && i0 <= P.im);
#ifdef POMGPU_EMU
  if (!out) return;
#endif
  const int i = i0 < 1 ? 1 : (i0 > P.iml ? P.iml : i0);
  const int iw = i > 1 ? i - 1 : 1, ie = i < P.iml ? i + 1 : P.iml;
  const int js = jc > 1 ? jc - 1 : 1, jn = jc < P.jml ? jc + 1 : P.jml;
  const bool in = out && (i >= 2 && i <= P.imm1 && jc >= 2 && jc <= P.jmm1);
  const int kb = P.kb, kbm1 = P.kbm1;
  // column-resident coefficients (in the fp32-arithmetic variant every 2-D operand is narrowed first: no fp64 operation)
#define C2_(name, i, j) CT(F2(name, i, j))
  const pomgpu_ct aru = F2(aru, i, jc), arv = F2(arv, i, jc), dti2 = P.dti2;
  const pomgpu_ct dt_c = F2(dt, i, jc), dt_w = F2(dt, iw, jc), dt_s = F2(dt, i, js);
  const pomgpu_ct cd_c = C2_(cor, i, jc) * dt_c, cd_s = C2_(cor, i, js) * dt_s;              // cor*dt of this column and of (i,j-1)
  const pomgpu_ct hcu = CT(P.grav) * CT(.125) * (dt_c + dt_w) *
                        (C2_(egf, i, jc) - C2_(egf, iw, jc) + C2_(egb, i, jc) - C2_(egb, iw, jc) + (C2_(e_atmos, i, jc) - C2_(e_atmos, iw, jc)) * CT(2.)) *
                        (C2_(dy, i, jc) + C2_(dy, iw, jc));                                     // :765-770
  const pomgpu_ct hcv = CT(P.grav) * CT(.125) * (dt_c + dt_s) *
                        (C2_(egf, i, jc) - C2_(egf, i, js) + C2_(egb, i, jc) - C2_(egb, i, js) + (C2_(e_atmos, i, jc) - C2_(e_atmos, i, js)) * CT(2.)) *
                        (C2_(dx, i, jc) + C2_(dx, i, js));                                      // :822-827
  const pomgpu_ct hb = C2_(h, i, jc) + C2_(etb, i, jc), hf = C2_(h, i, jc) + C2_(etf, i, jc);
  const pomgpu_ct sau = (hb + C2_(h, iw, jc) + C2_(etb, iw, jc)) * aru;                       // :758
  const pomgpu_ct sav = (hb + C2_(h, i, js) + C2_(etb, i, js)) * arv;                       // :815
  const InvDc sdu = inv_of((hf + C2_(h, iw, jc) + C2_(etf, iw, jc)) * aru), sdv = inv_of((hf + C2_(h, i, js) + C2_(etf, i, js)) * arv);   // :781, :838
#undef C2_
  BufA bs[NS], bh[NH];
  const double *ps[NS] = {A3(w), A3(u), A3(v)};
#pragma unroll
  for (int x = 0; x < NS; x++) bs[x] = BUF3(ps[x]);
  const BufA bub = BUF3(A3(ub)), bvb = BUF3(A3(vb)), bax = BUF3(A3(advx)), bay = BUF3(A3(advy)), bdx = BUF3(A3(drhox)), bdy = BUF3(A3(drhoy)),
             buf = BUF3(A3(uf)), bvf = BUF3(A3(vf));
  const RowShare<NS> S = rowshare_setup<NS>(P, r, j, j0w, i);
#pragma unroll
  for (int q = 0; q < NH; q++) bh[q] = BUF3(rowshare_pick<NS>(ps, S.hop[q]));
  const UvmC mu = UM ? uvm_of<0>(P, i, jc) : uvm_none(), mv = UM ? uvm_of<1>(P, i, jc) : uvm_none();
  UvmC mh[NH];
#pragma unroll
  for (int q = 0; q < NH; q++)
    mh[q] = !UM ? uvm_none() : (S.hop[q] == U ? rowshare_uvm<0, NS, LDS_ROWS>(P, S, q, U, j0w, i) : rowshare_uvm<1, NS, LDS_ROWS>(P, S, q, V, j0w, i));
  const unsigned oc = BOFF2(i, jc), lvb = LVB;
  const unsigned ost = out ? oc : BOFF_NONE;
#ifndef POMGPU_EMU
  __shared__ pomgpu_ct slab[3][NS][ROWSHARE_ROWS][64];
#else
  const unsigned os = BOFF2(i, js), on = BOFF2(i, jn);
#endif
  auto load = [&](LevUV &L, int k) {                        // shared operands of level k+1, own-row operands of level k
    const unsigned lv = (unsigned)WAVE_UNIFORM(k - 1) * lvb, lv1 = lv + lvb;
#pragma unroll
    for (int x = 0; x < NS; x++) L.c[x] = bldc(bs[x], oc, lv1);
#pragma unroll
    for (int q = 0; q < NH; q++) L.h[q] = bldc(bh[q], S.hoff[q], lv1);
    L.ub = bldc(bub, oc, lv);  L.vb = bldc(bvb, oc, lv);
    L.advx = bldc(bax, oc, lv); L.advy = bldc(bay, oc, lv); L.drhox = bldc(bdx, oc, lv); L.drhoy = bldc(bdy, oc, lv);
  };
  // lcor: the level being parked is one of 1..kbm1.  u_o, v_o: the own column's corrected values, as they went into the slab
  auto park = [&](const pomgpu_ct (&cv)[3], const pomgpu_ct (&hv)[NH], const int sl, const bool lcor, pomgpu_ct &u_o, pomgpu_ct &v_o) {
    u_o = uvm_fix(cv[U], mu, lcor); v_o = uvm_fix(cv[V], mv, lcor);
#ifndef POMGPU_EMU
    slab[sl][W][r + 1][lane] = cv[W]; slab[sl][U][r + 1][lane] = u_o; slab[sl][V][r + 1][lane] = v_o;
#pragma unroll
    for (int q = 0; q < NH; q++) slab[sl][S.hop[q]][S.hrow[q]][lane] = uvm_fix(hv[q], mh[q], lcor);
#endif
  };
  // level 1 of u, v (and w, unused) into slab 0: what the first iteration reads as its "level k" neighbours
  pomgpu_ct u_k, v_k;                                       // u, v of this column at level k
  {
    pomgpu_ct c1[3], h1[NH];
#pragma unroll
    for (int x = 0; x < NS; x++) c1[x] = bldc(bs[x], oc, 0u);
#pragma unroll
    for (int q = 0; q < NH; q++) h1[q] = bldc(bh[q], S.hoff[q], 0u);
    park(c1, h1, 0, true, u_k, v_k);
  }
  pomgpu_ct fu_k = 0., fv_k = 0.;                              // vertical fluxes at level k (0 at the surface)
  auto step = [&](const int k, const int sl, const LevUV &c, LevUV &nxt) {   // sl = k % 3: the slab of level k+1
    load(nxt, k + 1 <= kbm1 ? k + 1 : kbm1);                // in flight during this iteration (the last one re-requests level kbm1)
    pomgpu_ct u_c, v_c;                                     // level k+1
    park(c.c, c.h, sl, k + 1 <= kbm1, u_c, v_c);
    const int slm = sl == 0 ? 2 : sl - 1;                   // the slab of level k
#ifndef POMGPU_EMU
    __syncthreads();
    const pomgpu_ct w_s = slab[sl][W][S.ss][lane], u_s = slab[slm][U][S.ss][lane], v_n = slab[slm][V][S.sn][lane];
#else
    const pomgpu_ct w_s = bldc(bs[W], os, (unsigned)k * lvb), u_s = uvm_fix(bldc(bs[U], os, (unsigned)(k - 1) * lvb), uvm_of<0>(P, i, js)),
                    v_n = uvm_fix(bldc(bs[V], on, (unsigned)(k - 1) * lvb), uvm_of<1>(P, i, jn));
#endif
    const pomgpu_ct w_c = c.c[W];
    const pomgpu_ct w_w = halo_w(w_c, [&] { return F3(w, iw, jc, k + 1); });
    const pomgpu_ct tc = cd_c * (v_n + v_k);                                                // cor*dt*(v(i,j+1,k)+v(i,j,k))
    const pomgpu_ct tw = halo_w(tc, [&] { return F2(cor, iw, jc) * F2(dt, iw, jc) * (uvm_ld<1>(P, iw, jn, k) + uvm_ld<1>(P, iw, jc, k)); });
    const pomgpu_ct u_e = halo_e(u_k, [&] { return uvm_ld<0>(P, ie, jc, k); });
    const pomgpu_ct u_se = halo_e(u_s, [&] { return uvm_ld<0>(P, ie, js, k); });
    // vertical fluxes at level k+1 (:744-751, :801-808); zero below kbm1, and where the column has no west / south neighbour
    pomgpu_ct fu_n = 0., fv_n = 0.;
    if (k + 1 <= kbm1) {
      if (i >= 2) fu_n = CT(.25) * (w_c + w_w) * (u_c + u_k);
      if (jc >= 2) fv_n = CT(.25) * (w_c + w_s) * (v_c + v_k);
    }
    pomgpu_ct ru = fu_k, rv = fv_k;                                                         // outside the interior: the flux itself
    if (in) {
      InvDc dzk; dzk.b = F1(dz, k); dzk.y = R1(dz, k);
      ru = divi(sau * c.ub - CT(2.) * dti2 * (c.advx + divi((fu_k - fu_n) * aru, dzk) - aru * CT(.25) * (tc + tw) + hcu + c.drhox), sdu);   // :758-782
      rv = divi(sav * c.vb -
                    CT(2.) * dti2 * (c.advy + divi((fv_k - fv_n) * arv, dzk) + arv * CT(.25) * (cd_c * (u_e + u_k) + cd_s * (u_se + u_s)) + hcv + c.drhoy),
                sdv);                                                                       // :815-839
    }
    const unsigned lv = (unsigned)WAVE_UNIFORM(k - 1) * lvb;
    bstc(buf, ost, lv, ru);
    bstc(bvf, ost, lv, rv);
    fu_k = fu_n; fv_k = fv_n;
    u_k = u_c; v_k = v_c;
  };
  LevUV ra, rb;
  load(ra, 1);
  rb = ra;
  for (int k = 1; k <= kbm1; k += 6) {                      // six iterations: two register sets x three slabs
    step(k, 1, ra, rb);
    if (k + 1 <= kbm1) step(k + 1, 2, rb, ra);
    if (k + 2 <= kbm1) step(k + 2, 0, ra, rb);
    if (k + 3 <= kbm1) step(k + 3, 1, rb, ra);
    if (k + 4 <= kbm1) step(k + 4, 2, ra, rb);
    if (k + 5 <= kbm1) step(k + 5, 0, rb, ra);
  }
  if (out) { F3(uf, i, jc, kb) = 0.; F3(vf, i, jc, kb) = 0.; }
}

// ---- launchers ------------------------------------------------------------------------------------
void launch_coef_static(pomgpu_ctx *c) { LAUNCH(c, k_coef_static, grid2(c->P), blk2(), c->P); }
void launch_coef_dt(pomgpu_ctx *c) { LAUNCH(c, k_coef_dt, grid2(c->P), blk2(), c->P); }
void launch_coef_eta(pomgpu_ctx *c, int uvm) { LAUNCH(c, k_coef_eta, grid2(c->P), blk2(), c->P, uvm); }
void launch_advq_col(pomgpu_ctx *c, const double *q, const double *qb, double *qf, int zero_else) {
  QFields A; A.q[0] = A.q[1] = q; A.qb[0] = A.qb[1] = qb; A.qf[0] = A.qf[1] = qf;
  LAUNCHN(c, "k_advq_col", (k_advq_col<1>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, A, zero_else);
}
void launch_advq2_col(pomgpu_ctx *c, const double *q, const double *qb, double *qf, const double *ql, const double *qlb, double *qlf, int zero_else) {
  QFields A; A.q[0] = q; A.qb[0] = qb; A.qf[0] = qf; A.q[1] = ql; A.qb[1] = qlb; A.qf[1] = qlf;
  LAUNCHN(c, "k_advq2_col", (k_advq_col<2>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, A, zero_else);
}
// the same pass with vertvl (mask of bcondorl(5) included) inside its march: w is written, not read (mode_internal on one tile).
// Not in the fp32-arithmetic variant (POMGPU_W_FUSE, pomgpu_internal.hpp)
#if POMGPU_W_FUSE
void launch_advq2w_col(pomgpu_ctx *c, const double *q, const double *qb, double *qf, const double *ql, const double *qlb, double *qlf, int zero_else) {
  QFields A; A.q[0] = q; A.qb[0] = qb; A.qf[0] = qf; A.q[1] = ql; A.qb[1] = qlb; A.qf[1] = qlf;
#if POMGPU_UVM_ONLOAD
  if (c->P.uvm) { LAUNCHN(c, "k_advq2_col", (k_advq_col<2, true, true>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, A, zero_else); return; }
#endif
  LAUNCHN(c, "k_advq2_col", (k_advq_col<2, true>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, A, zero_else);
}
#endif
// aam_w (lateral_viscosity, aam_fused): the march also forms the new aam into aam_w and leaves aam2d; advct_aam_fused of the event profile
// counts these launches, a count without events as profq_ld_store
void launch_advct_col(pomgpu_ctx *c, int sum2d, double *aam_w) {
  // low tiles (a tile of an 8- or 4-tile split of 2048x1536): 4-row workgroups, two per compute unit
  const bool rows4 = SW(c, ADVCT_ROWS4) || (!SW(c, ADVCT_ROWS8) && c->P.jml <= 400 && c->exch);
  sum2d = (sum2d ? 1 : 0) | (POMGPU_UVM_ONLOAD && !c->exch && !c->tp.on && !c->wide.on && !(c->flags & POMGPU_CTX_2D) ? 2 : 0);   // bit 1: the depth sums of u, v (one tile)
#if POMGPU_AAM_FUSE
  if (aam_w) {                                              // one tile only: the 4-row shape is for low tiles
    if (c->prof_on) {
      const int s = pomgpu_prof_slot(c, "advct_aam_fused");
      if (s >= 0) (c->parent ? c->parent : c)->prof[s].launches++;
    }
    LAUNCHN(c, "k_advct_col", (k_advct_col<LDS_ROWS, true>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, sum2d, aam_w);
    return;
  }
#endif
  if (rows4) LAUNCHN(c, "k_advct_col", (k_advct_col<4>), grid1_halo_r(c->P, 4), blk_col_r(4), c->P, sum2d, (double *)NULL);
  else LAUNCHN(c, "k_advct_col", (k_advct_col<LDS_ROWS>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, sum2d, (double *)NULL);
}
// with sum2d the column kernel has left adx2d, ady2d (advance.f:152-168) from its own advx(2,:), advy(:,2): redo the
// two lines from the corrected values, in the column kernel's order of summation
__global__ void k_advct_fix2d(KP P, int west, int south) {
  const int t = TID_I;
  if (west && t >= 2 && t <= P.jmm1) {
    double a = 0.;
#pragma unroll 8
    for (int k = 1; k <= P.kbm1; k++) a = a + F3(advx, 2, t, k) * F1(dz, k);
    F2(adx2d, 2, t) = a;
  }
  if (south && t >= 2 && t <= P.imm1) {
    double a = 0.;
#pragma unroll 8
    for (int k = 1; k <= P.kbm1; k++) a = a + F3(advy, t, 2, k) * F1(dz, k);
    F2(ady2d, t, 2) = a;
  }
}
void launch_advct_fix2d(pomgpu_ctx *c, int west, int south) {
  const KP &P = c->P;
  const int len = P.im > P.jm ? P.im : P.jm;
  LAUNCH(c, k_advct_fix2d, dim3((len + 63) / 64, 1, 1), dim3(64, 1, 1), c->P, west, south);
}
void launch_advct_edge(pomgpu_ctx *c, double *to_e, double *to_n) {
  const KP &P = c->P;
  const int len = P.im > P.jm ? P.im : P.jm;
  LAUNCH(c, k_advct_edge, dim3((len + 63) / 64, P.kbm1, 1), dim3(64, 1, 1), c->P, to_e, to_n);
}
void launch_advct_fix(pomgpu_ctx *c, const double *from_w, const double *from_s) {
  const KP &P = c->P;
  const int len = P.im > P.jm ? P.im : P.jm;
  LAUNCH(c, k_advct_fix, dim3((len + 63) / 64, P.kbm1, 1), dim3(64, 1, 1), c->P, from_w, from_s);
}
void launch_advuv_col(pomgpu_ctx *c) {
#if POMGPU_UVM_ONLOAD
  if (c->P.uvm) { LAUNCHN(c, "k_advuv_col", (k_advuv_col<true>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P); return; }
#endif
  LAUNCHN(c, "k_advuv_col", (k_advuv_col<false>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P);
}
void launch_advt2_rows(pomgpu_ctx *c, const double *fb, const double *f, const double *fc, double *ff) {
  {
    TFields A; A.fb[0] = A.fb[1] = fb; A.f[0] = A.f[1] = f; A.fcl[0] = A.fcl[1] = fc; A.ff[0] = A.ff[1] = ff; A.rtf = NULL;
#if POMGPU_UVM_ONLOAD   // an odd passive tracer on one tile: u, v still lack the depth-mean correction (the T / S pair never comes here with KP::uvm up)
    if (c->P.uvm) { LAUNCHN(c, "k_advt2_col", (k_advt2_col<1, true>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, A); return; }
#endif
    LAUNCHN(c, "k_advt2_col", (k_advt2_col<1>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, A);
  }
}
// rtf (the T / S pair of mode_internal on one tile; NULL: passive tracers, tiles): where the round trip of tb, sb changes bits (RTF)
void launch_advt2x2_col(pomgpu_ctx *c, const double *tb, const double *t, const double *tc, double *tf, const double *sb, const double *s_,
                        const double *sc, double *sf, unsigned long long *rtf) {
  TFields A; A.fb[0] = tb; A.f[0] = t; A.fcl[0] = tc; A.ff[0] = tf; A.fb[1] = sb; A.f[1] = s_; A.fcl[1] = sc; A.ff[1] = sf; A.rtf = rtf;
  if (rtf) {
#if POMGPU_UVM_ONLOAD
    if (c->P.uvm) { LAUNCHN(c, "k_advt2x2_col", (k_advt2_col<2, true, true>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, A); return; }
#endif
    LAUNCHN(c, "k_advt2x2_col", (k_advt2_col<2, false, true>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, A);
    return;
  }
#if POMGPU_UVM_ONLOAD
  if (c->P.uvm) { LAUNCHN(c, "k_advt2x2_col", (k_advt2_col<2, true>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, A); return; }
#endif
  LAUNCHN(c, "k_advt2x2_col", (k_advt2_col<2>), grid1_halo_r(c->P, LDS_ROWS), blk_col_r(LDS_ROWS), c->P, A);
}
