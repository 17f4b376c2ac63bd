/* include/pomgpu.h -- C ABI of the MI355X hot path of extPOM's mode-split time step.
 *
 * The reference has no plugin registry: its boundary is the Fortran external-procedure ABI plus
 * COMMON blocks (reference pom/pom.f:17-19 calls `advance`; every hot routine is an argument-less
 * subroutine working on the blocks of pom.h_dist:46-640).  This library keeps that shape:
 *
 *   - state crosses the boundary as whole COMMON blocks in the reference's own layout
 *     (include/pom_layout.h), handed over by address and mirrored in HBM;
 *   - every hot-path routine of the reference has an entry point of the same name
 *     (pomgpu_<name>) and the same argument meaning; routines whose Fortran actual arguments are
 *     COMMON arrays (advq, advt1, advt2, dens, proft: advance.f:407-408,426-430,439-440,454) take
 *     the HOST address of that array -- exactly what the Fortran caller passes by reference -- and
 *     the library translates it to the device mirror;
 *   - errors follow the reference's convention: a routine sets error_status=1 in blkcon and
 *     reports on stderr (advance.f:118-119,631-637); in addition every entry point returns 0 on
 *     success and a negative pomgpu_status otherwise (HIP failures map to POMGPU_EHIP and also
 *     set error_status=1).
 *
 * All entry points are plain C: pointers, ints and doubles only.  One context = one tile = one GPU.
 * The library never frees or reallocates host arrays; it owns only its device mirrors and stream.
 */
#ifndef POMGPU_H
#define POMGPU_H
#include <stddef.h>
#include "pom_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pomgpu_ctx pomgpu_ctx;

enum pomgpu_status {
  POMGPU_OK = 0,
  POMGPU_EINVAL = -1,   /* bad argument / unsupported option (message in pomgpu_last_error) */
  POMGPU_EHIP = -2,     /* a HIP runtime call failed */
  POMGPU_ENOMEM = -3,
  POMGPU_ENODEV = -4    /* no usable GPU: the hot path has no CPU fallback */
};

/* Tile description: blksiz + blkpar of the reference (pom.h_dist:46-54,58-78). */
typedef struct pomgpu_dims {
  int im, jm, kb;                         /* active extents */
  int im_local, jm_local;                 /* leading dimensions of every array */
  int n_west, n_east, n_south, n_north;   /* neighbour ranks, -1 = physical edge (parallel_mpi.f:111-119) */
} pomgpu_dims;

/* ---- life cycle ------------------------------------------------------------------------- */
/* `stream` is a hipStream_t (or NULL for the library's own stream) passed as void* so that this
 * header needs no HIP include. */
int  pomgpu_create(pomgpu_ctx **ctx, const pomgpu_dims *dims, int device, void *stream);
void pomgpu_destroy(pomgpu_ctx *ctx);
const char *pomgpu_last_error(const pomgpu_ctx *ctx);
int  pomgpu_sync(pomgpu_ctx *ctx);
void *pomgpu_stream(pomgpu_ctx *ctx);
/* The stream the library is enqueueing on at this moment.  Outside a callback this is pomgpu_stream(); inside a transport
 * callback it is the stream of the message round being served -- pomgpu_stream(), or the library's second stream for the rounds
 * that run beside the kernels (the early part of the wide exchange, the rim rounds, wr): a mover that enqueues its copies must
 * enqueue them THERE (or complete them before it returns), else the unpack kernel that follows on that stream does not wait
 * for them. */
void *pomgpu_current_stream(pomgpu_ctx *ctx);

/* ---- state transfer (pomgpu_upload_state / pomgpu_download_state of SURVEY 8b) ---------- */
/* Whole blocks; any pointer may be NULL to skip that block.  `bdry` is the bdry block
 * (pom.h_dist:532-608).  `lramp` is blklog. */
int pomgpu_upload(pomgpu_ctx *ctx, const double *blk1d, const double *blk2d, const double *blk3d,
                  const double *bdry, const pom_blkcon *con, int lramp);
int pomgpu_download(pomgpu_ctx *ctx, double *blk1d, double *blk2d, double *blk3d, double *bdry,
                    pom_blkcon *con);
/* Single arrays, addressed by their slot in the block (enum pom_slot2d / pom_slot3d). */
int pomgpu_upload_2d(pomgpu_ctx *ctx, int slot2d, const double *host);
int pomgpu_upload_3d(pomgpu_ctx *ctx, int slot3d, const double *host);
int pomgpu_download_2d(pomgpu_ctx *ctx, int slot2d, double *host);
int pomgpu_download_3d(pomgpu_ctx *ctx, int slot3d, double *host);
/* blkcon only (iint, time, ramp ... change every step on the host side of the reference). */
int pomgpu_set_con(pomgpu_ctx *ctx, const pom_blkcon *con, int lramp);
int pomgpu_get_con(pomgpu_ctx *ctx, pom_blkcon *con);
/* Register the host base addresses of blk2d/blk3d so that array arguments given as host
 * addresses (Fortran by-reference actuals) can be translated to device mirrors. */
int pomgpu_bind_host(pomgpu_ctx *ctx, const double *host_blk2d, const double *host_blk3d);
/* Relaxation targets that the reference's restore_interior reads through
 * read_restore_ts_interior_pnetcdf(n,kb,tr,sr) (bounds_forcing.f:1040,1060): record n (1-based),
 * arrays dimensioned (im,jm,kb).  Copied to the device.  Refused (POMGPU_EINVAL) once the records come from a file
 * (pomgpu_set_forcing_files). */
int pomgpu_set_restore_record(pomgpu_ctx *ctx, int n, const double *tr, const double *sr);
/* The restore RATE as a field -- a sponge: taurstr(i,j,k) in 1/day, which the reference keeps in COMMON and never fills (it assigns
 * taurstrf = 1./trst and leaves read_restore_tau_interior_pnetcdf + ztosig commented, bounds_forcing.f:1049-1051, :1076-1079).
 * pomgpu_set_restore_rate_record: `tau`, (im,jm,kb) on the sigma levels, is the rate that goes with T/S record n (1..POMGPU_MAXREC; same
 * lifetime and copy as pomgpu_set_restore_record).  Refused (POMGPU_EINVAL) once the rate comes from a file.
 * pomgpu_set_restore_rate_file: the reference's reader without PnetCDF, registered like the files of pomgpu_set_forcing_files (its parser,
 * checks, pinned buffers; of `meta` only im_global, jm_global, i0, j0; not collective, no message round).  Classic NetCDF (CDF-1 / CDF-2),
 * variables BY NAME: `z`, 1-D NC_FLOAT / NC_DOUBLE, ks values, 2 <= ks <= 300, finite and strictly increasing; `tau`, NC_FLOAT / NC_DOUBLE,
 * (ks, jm_global, im_global) with or without a leading record dimension (unlimited or fixed).  Anything else -- a file shorter than its
 * header says, a tile whose window (one more column / row towards every neighbour) does not fit the grid, im or jm below 4, a NULL path --
 * is refused before anything changes, with POMGPU_EINVAL, error_status = 1 and the file and the cause in pomgpu_last_error.  Buffers and
 * ztosig's table are allocated here; a step allocates nothing.
 * The rate that accompanies T/S record n is record n (1-based) of the file; a file with exactly one record, or without a record dimension,
 * serves every n, is read and mapped once, and later loads skip both.  A record beyond the file's count or end fails that step before any
 * slot is written.
 * A load of record n in restore_interior (T/S by setter or from the clim file alike) assigns taurstrf = 1./trst over the whole padded array
 * as ever, then (a) with a rate file: the ks levels of the tile's window are mapped by ztosig (initialize.f:547-595) straight into the
 * mirror taurstrf -- all kb levels of (1:im, 1:jm), the +0.0 of dry and rim columns and the copies onto physical edges included, the padding
 * keeps 1./trst; on the stream of the step; the fp32 builds round once at the store -- or (b) with a rate record n: taurstrf(1:im,1:jm,1:kb)
 * = tau, or (c) neither: nothing more.  Two properties of the map are the reference's own: a rate below the REAL(4) 0.01 on a level the
 * depth covers counts as MISSING and is filled from the neighbour maximum or the level above (a sponge's edge creeps by a cell), and the
 * natural spline may undershoot below zero.  A host that wants exact rates uses the sigma-level setter. */
int pomgpu_set_restore_rate_record(pomgpu_ctx *ctx, int n, const double *tau);   /* pomgpu_set_restore_rate_file: declared beside pomgpu_set_forcing_files */
/* Device address of a mirror (for halo exchange by the caller, e.g. RCCL send/recv).  An address of a 3-D array stays valid until
 * pomgpu_destroy -- pomgpu_tune_placement, which moves those arrays, refuses once one has been handed out.  Through an address the
 * caller reads and writes behind the library's back: a pending wr (see pomgpu_run) is formed before the address is returned, and from
 * then on the context forms wr at the end of every step.  An address of taurstrb or taurstrf ends what the library knows about the restore
 * rate for good: every step reads both arrays from then on. */
double *pomgpu_device_2d(pomgpu_ctx *ctx, int slot2d);
double *pomgpu_device_3d(pomgpu_ctx *ctx, int slot3d);

/* ---- halo exchange hook (replaces exchange2d_mpi / exchange3d_mpi, parallel_mpi.f:154-351) */
/* Called on the library's stream order: `dev` is the DEVICE address of the first level to
 * exchange, leading dimensions (im_local, jm_local), `nz` levels (1 for 2-D).  `count` arrays are
 * exchanged at one program point (the caller may batch them into one message per neighbour).
 * NULL hook = single tile (all neighbours -1: every exchange is a no-op, parallel_mpi.f:171). */
typedef void (*pomgpu_exchange_fn)(void *user, double *const *dev, const int *nz, int count);
int pomgpu_set_exchange(pomgpu_ctx *ctx, pomgpu_exchange_fn fn, void *user);

/* order2d_mpi / order3d_mpi of baropg_mcc (parallel_mpi.f:353-480, called at solver.f:958-959): the
 * 4th-order pressure gradient needs ONE more ghost column to the west and ghost row to the south.  The
 * library packs what the reference sends -- column im_local-2 / row jm_local-2 of d and of rho-rmean --
 * into device buffers and asks the hook to move them: `send_east` (n_east doubles) goes to the eastern
 * neighbour, which receives it as `recv_west`; `send_north` (n_north) to the northern one, received as
 * `recv_south`.  A tile without the respective neighbour skips that transfer (its recv buffer is not
 * read).  NULL hook = single tile. */
typedef void (*pomgpu_order_fn)(void *user, const double *send_east, int n_east, const double *send_north, int n_north,
                                double *recv_west, double *recv_south);
int pomgpu_set_order_exchange(pomgpu_ctx *ctx, pomgpu_order_fn fn, void *user);

/* ---- surface forcing on the device (bounds_forcing.f:871-983, called from advance.f:77-93) ---------------
 * wind and heat keep two records (…b, …f members of blk2d) and interpolate linearly in time; surface sets the
 * SST without interpolation.  The records come from the files named with pomgpu_set_forcing_files (below), or -- a source without a
 * file -- from the host's readers (read_wind_pnetcdf, read_heat_pnetcdf,
 * read_surface_pnetcdf: io_pnetcdf.F:2912,3110,3170): the host hands the library the pair of (im,jm) fields
 * of record n -- kind 0 = wind (wu, wv), 1 = heat (shf, swr), 2 = surface (sst, sss) -- before the step whose
 * wind / heat / surface call asks for it; the last four records per kind are kept.  pomgpu_get_time must have
 * set the step's time.  A record that was not supplied: error_status = 1, POMGPU_EINVAL.  Refused (POMGPU_EINVAL) once the
 * surface records come from a file. */
int pomgpu_set_forcing_record(pomgpu_ctx *ctx, int kind, int n, const double *a, const double *b);
int pomgpu_wind(pomgpu_ctx *ctx);              /* bounds_forcing.f:871-912 */
int pomgpu_heat(pomgpu_ctx *ctx);              /* bounds_forcing.f:915-960 */
int pomgpu_surface(pomgpu_ctx *ctx);           /* bounds_forcing.f:963-983 */
int pomgpu_surface_forcing(pomgpu_ctx *ctx);   /* advance.f:77-93: wind, heat, [water,] surface */
/* ":979 ssurf(1:im,1:jm) = sss", which the reference keeps commented: on != 0 makes pomgpu_surface load ssurf from the record's second
 * field (SSS of the sfrc file, `b` of a kind-2 record) beside tsurf -- what proft's salt solve reads at nbcs = 3.  Off (the default):
 * ssurf is never written. */
int pomgpu_set_surface_sss(pomgpu_ctx *ctx, int on);

/* ---- water: the fresh-water flux wssurf (bounds_forcing.f:986-1020; the call at advance.f:89 is commented in the reference) -------------
 * proft's salt solve reads wssurf at nbcs = 1 (solver.f:1566-1574, advance.f:440).  pomgpu_water restates `water` as written: twater = 1.
 * day, iwater = int(86400 / dti); at iint == 1 record iint / iwater goes into wssurff; when iint == 1 or mod(iint, iwater) == 0, wssurfb =
 * wssurff over (1:im, 1:jm) and record (iint + iwater) / iwater goes into wssurff; then wssurf = fold * wssurfb + fnew * wssurff with fnew
 * = time / twater - int(time / twater), fold = 1. - fnew.  Three differences from wind and heat: (1) cont_bry is not in the schedule;
 * (2) the record number carries no "+ 1" -- records count from 0, which the first step reads unless dti is a day or more; (3) there is
 * no "iint /= iend" guard: a run whose last step is a multiple of iwater needs one more record.  The record is neither converted nor
 * tapered.  Off by default: the first pomgpu_set_water_record or pomgpu_set_water_files switches it on, pomgpu_set_water(ctx, 0) off
 * again.  While on, pomgpu_surface_forcing calls pomgpu_water between heat and surface, and pomgpu_advance / pomgpu_run call it alone
 * where no surface source is registered.  iwater < 1 and a record that cannot be had: POMGPU_EINVAL, error_status = 1, before any mirror or record
 * slot is written (the shift is not made either).
 * Records: pomgpu_set_water_record hands over the one (im,jm) field read_water_pnetcdf(n, ...) (io_pnetcdf.F:3227-3272) would deliver, n
 * >= 0, the last four are kept; or pomgpu_set_water_files names <prefix>.water.NNNN.nc -- the reference's '(a,''in/'',a,''.water.'',
 * i4.4,''.nc'')' with prefix = <wrk_pth>in/<netcdf_file> -- each file ONE record: `w` as (jm_global, im_global), found by name, NC_FLOAT
 * or NC_DOUBLE, other dimensions and variables tolerated.  The file of record n is opened when the schedule asks for it, checked like
 * every other file this library reads, its band unpacked by the kernel of the surface records, and closed; n > 9999 has no file name.
 * Every rank reads its own window (meta's i0, j0): no message round.  The setter is refused once files are registered. */
int pomgpu_set_water_record(pomgpu_ctx *ctx, int n, const double *w);   /* pomgpu_set_water_files: declared beside pomgpu_set_forcing_files */
int pomgpu_set_water(pomgpu_ctx *ctx, int on);
int pomgpu_water(pomgpu_ctx *ctx);             /* bounds_forcing.f:986-1020 */

/* lateral_bc on the device (bounds_forcing.f:593-868): records every 1/24 day, the same shift / load /
 * interpolate pattern on the open-boundary arrays of `bdry`, plus the depth integrals uab?f, vab?f, uabe, uabw,
 * vabn, vabs.  The host's reader (read_boundary_conditions_pnetcdf, io_pnetcdf.F:3393) fills 20 arrays: tbwf sbwf
 * ubwf vbwf tbef sbef ubef vbef tbnf sbnf vbnf ubnf tbsf sbsf vbsf ubsf elw ele eln els -- hand them over in this
 * order, each in the shape of the bdry member it lands in ((jm_local,kb), (im_local,kb), (jm_local), (im_local)).  Refused
 * (POMGPU_EINVAL) once the lateral records come from a file (pomgpu_set_forcing_files). */
int pomgpu_set_lateral_record(pomgpu_ctx *ctx, int n, const double *const *arrays20);
int pomgpu_lateral_bc(pomgpu_ctx *ctx);

/* Pack / unpack helpers for the hook (one kernel launch per direction instead of one copy per
 * array and edge).  dir 0 = east/west phase, 1 = north/south phase.  pack: the edge the western
 * (southern) neighbour needs -- column 2 (row 2) of every array -- goes to `to_lo`, column im-1
 * (row jm-1) to `to_hi`, arrays concatenated, each nz x jm (nz x im) doubles, level-major.  unpack:
 * `from_lo` (sent by the western / southern neighbour) lands in column 1 (row 1), `from_hi` in
 * column im (row jm).  A NULL buffer skips that side.  Buffers are device memory. */
int pomgpu_halo_pack(pomgpu_ctx *ctx, double *const *dev, const int *nz, int count, int dir, double *to_lo, double *to_hi);
int pomgpu_halo_unpack(pomgpu_ctx *ctx, double *const *dev, const int *nz, int count, int dir, const double *from_lo,
                       const double *from_hi);
/* The same exchange in ONE round with up to eight neighbours (half the message rounds per exchange point):
 * buffer tables in the order W E S N SW SE NW NE, NULL = no such neighbour.  pack8: column 2 / im-1 (jm values
 * per level) to W / E, row 2 / jm-1 (im values) to S / N, the cells (2,2), (im-1,2), (2,jm-1), (im-1,jm-1) to
 * SW, SE, NW, NE.  unpack8: what W / E sent lands in column 1 / im over the rows no N/S neighbour's row owns,
 * what S / N sent in row 1 / jm over the columns no W/E neighbour's column owns, the diagonal cells in the
 * four corners -- the ghost cells end up exactly as after the reference's two phases. */
int pomgpu_halo_pack8(pomgpu_ctx *ctx, double *const *dev, const int *nz, int count, double *const *to);
int pomgpu_halo_unpack8(pomgpu_ctx *ctx, double *const *dev, const int *nz, int count, const double *const *from);

/* ---- the library's own exchange: transport (replaces the MPI layer under exchange2d/3d_mpi, order2d/3d_mpi) --
 * With a transport the library serves every exchange point itself -- pack8, ONE message round with up to eight
 * neighbours, unpack8, all on its stream, no host code in between -- and the hooks above are not needed.
 * neighbours8: ranks in the order W E S N SW SE NW NE, -1 = none (W E S N must agree with pomgpu_dims).
 *
 * pomgpu_rccl_init: the production transport, grouped ncclSend / ncclRecv (RCCL, xGMI between the GPUs of a node)
 * enqueued on the library's stream.  The reference side is parallel_mpi.f:124-151 (initialize_mpi: communicator,
 * rank, size): one rank obtains `id128` (128 bytes) from pomgpu_rccl_unique_id and distributes it with whatever
 * the host has (MPI_Bcast in the Fortran driver), then every rank calls pomgpu_rccl_init.  librccl is opened at
 * run time (`librccl_path`, NULL = "librccl.so"), so the library has no link-time dependency on it.
 *
 * pomgpu_set_transport: a callback mover for hosts without RCCL between the ranks (tests: ranks sharing one GPU,
 * host threads).  It must deliver send[d][0..scount[d]) to neighbour d -- which receives it as recv[OPP(d)] --
 * and fill recv[d][0..rcount[d]) with what neighbour d sent towards OPP(d); buffers are device memory, the work
 * must be ordered after what is already enqueued on pomgpu_current_stream() (the stream of the round: pomgpu_stream(), or the
 * library's second stream, whose earlier work has completed when the callback is called) and before what follows there.  fn == NULL removes
 * the transport (and the wide-halo external mode with it). */
typedef void (*pomgpu_transport_fn)(void *user, const double *const *send, const size_t *scount, double *const *recv,
                                    const size_t *rcount);
int pomgpu_set_transport(pomgpu_ctx *ctx, const int *neighbours8, pomgpu_transport_fn fn, void *user);
int pomgpu_rccl_available(const char *librccl_path);   /* POMGPU_OK if librccl opens and has every entry point; no GPU call, not collective */
int pomgpu_rccl_unique_id(void *id128, const char *librccl_path);
int pomgpu_rccl_init(pomgpu_ctx *ctx, const void *id128, int rank, int nranks, const int *neighbours8,
                     const char *librccl_path);
/* Message rounds on the library's SECOND stream (the early part of the wide exchange; the rim rounds: advct's edge lines, advx + advy + aam, w,
 * the turbulence arrays and T / S / rho behind the kernels that produce them, the two velocity exchanges that end mode_internal; wr -- nine of
 * a full step's ten rounds) are a decision every rank of
 * the decomposition must take alike: a rank that kept them on the first stream while its neighbours moved them would post
 * its rounds in another order on another communicator, and the job would hang.  pomgpu_rccl_init agrees on it itself,
 * BEFORE anything collective depends on a rank's own answer: one ncclAllReduce(min) over the first communicator of every
 * rank's (a) willingness to split a second communicator off (ncclCommSplit present, second stream created, neither
 * POMGPU_NO_OVERLAP nor POMGPU_NO_SIDE_COMM in the switches its context was created under), (b) POMGPU_WR_MAIN unset, and
 * (c) a digest of the switches that choose which message rounds exist -- ranks started with different switch sets are all
 * refused with a message (POMGPU_EHIP) instead of hanging later; only if ALL ranks are willing does any of them enter
 * ncclCommSplit, and a second all-reduce settles whether every split succeeded.  With a callback mover the library cannot
 * reach the other ranks: side rounds stay OFF until the host has reduced pomgpu_transport_side_capable() (this rank: 0 =
 * cannot, 1 = can but wants wr on the main stream, 2 = can) to its minimum over ALL ranks and handed the result to
 * pomgpu_transport_side_agree() on every rank, after pomgpu_set_transport and before pomgpu_set_wide_external.  agreed = 0
 * is accepted with any transport.  pomgpu_switch_digest: the digest of (c), for such hosts to compare over their ranks. */
int pomgpu_transport_side_capable(pomgpu_ctx *ctx);
int pomgpu_transport_side_agree(pomgpu_ctx *ctx, int agreed);
/* A callback mover that ENQUEUES its work on pomgpu_current_stream() (device-to-device copies between contexts that share a GPU,
 * ordered by events) says so here (ordered = 1, after pomgpu_set_transport): the library then calls it for a round of the second
 * stream without completing that stream first -- such a mover runs beside the kernels like the RCCL transport does.  Default 0:
 * the callback finds the second stream's earlier work completed (movers that stage through the host). */
int pomgpu_transport_stream_ordered(pomgpu_ctx *ctx, int ordered);
unsigned pomgpu_switch_digest(pomgpu_ctx *ctx);
/* how many ranks RCCL itself reports for the communicator (ncclCommCount): 0 without the RCCL transport, -1 if unknown */
int pomgpu_rccl_nranks(pomgpu_ctx *ctx);
/* message rounds served by the transport since it was set (measurement) */
long pomgpu_exchange_rounds(pomgpu_ctx *ctx);
/* ... of them on the library's second stream (the early part of the wide exchange, the rim rounds, wr): beside kernels, not between them */
long pomgpu_exchange_rounds_side(pomgpu_ctx *ctx);

/* Wide-halo external mode (needs a transport).  It starts in pomgpu_mode_interaction and ends with the
 * pomgpu_mode_external call of the last substep (iext = isplit) -- the reference's own sequence in `advance`, and
 * pomgpu_advance / pomgpu_run, get it without change; in between the tile's 2-D arrays are not current (any other
 * entry point or download fetches them first).  The reference exchanges
 * 1-cell halos six times per external substep (advance.f:233,292-293,348-349; solver.f:60-61,70,111-112,121) --
 * ~180 of the ~200 message rounds of an internal step, each a few microseconds of data.  With on != 0 the 2-D part
 * of the step (advave and the tail of mode_interaction, all isplit substeps of mode_external) runs on a copy of
 * the tile extended by w = isplit + 4 cells towards every neighbour: ONE wide exchange per internal step brings
 * the neighbours' cells, the substeps run without any exchange (the band of stale cells at the rim of the extended
 * tile grows by one cell per substep, so after isplit substeps the tile and its ghost cells are still exact),
 * and the result is copied back -- the tile's arrays,
 * ghost cells included, hold bit for bit what the reference's exchanges would have left there.
 * Collective: every rank calls it with the same `on` and the smallest active extents (im, jm) over ALL tiles of
 * the decomposition; when a tile could be narrower than w + 3 cells every rank gets POMGPU_EINVAL and the
 * per-point exchanges stay in use. */
int pomgpu_set_wide_external(pomgpu_ctx *ctx, int on, int min_im, int min_jm);

/* ---- the hot path: orchestration (advance.f) -------------------------------------------- */
int pomgpu_get_time(pomgpu_ctx *ctx);            /* advance.f:62-75  */
/* With the wide-halo mode and side-stream rounds agreed, pomgpu_lateral_viscosity also starts the EARLY part of the wide
 * exchange on the second stream, and pomgpu_mode_interaction then sends only the late part: what the early part has moved (ua, va,
 * uab, vab, el, elb, d, the surface fluxes, wubot, wvbot, the open-boundary lines) is not moved again.  Between the two calls the host
 * therefore leaves the 2-D state alone: no forcing setters (pomgpu_set_forcing_record / _lateral_record, pomgpu_surface_forcing,
 * pomgpu_lateral_bc -- advance.f:14-18 runs them BEFORE lateral_viscosity), no writes through pomgpu_device_2d; pomgpu_upload and
 * pomgpu_upload_2d are allowed if EVERY rank makes them (they end the early part's validity, and pomgpu_mode_interaction then gathers
 * everything in one round -- on one rank only that would be unequal message counts).  The reference's own sequence (advance.f:14-21) and
 * pomgpu_advance satisfy this by construction.
 * pomgpu_lateral_viscosity and pomgpu_mode_internal also post the rim rounds (advct's edge lines; w, the turbulence arrays, T / S / rho and
 * the two velocity exchanges of mode_internal) on the second stream; whatever looks at the state afterwards waits for them by itself. */
int pomgpu_lateral_viscosity(pomgpu_ctx *ctx);   /* advance.f:96-141 */
int pomgpu_mode_interaction(pomgpu_ctx *ctx);    /* advance.f:144-202 */
/* advance.f:205-353; uses blkcon.iext.  One call per substep, as the reference makes them (advance.f:27-29).  PAIRING: on a
 * tile large enough for the two-substeps-per-pass kernel an ODD substep is held back (the call returns POMGPU_OK with nothing
 * launched) until the next call: if that is substep iext + 1 the two run as one pass and elf, uaf, vaf are stored for the
 * SECOND substep only (nobody reads the first's: the reference overwrites them in the next call); any other entry point, a
 * download or pomgpu_sync first runs the held substep alone (with its elf, uaf, vaf stored) under the scalars of the LAST
 * pomgpu_set_con -- do not change blkcon between the two calls of a pair.  If the held substep fails when it finally runs,
 * the context is marked failed: error_status = 1 and the next entry point / pomgpu_get_con reports it. */
int pomgpu_mode_external(pomgpu_ctx *ctx);
int pomgpu_mode_internal(pomgpu_ctx *ctx);       /* advance.f:356-537 */
/* advance.f:611-641; any of the out pointers may be NULL.  Synchronises the stream.  Reads vaf alone: unlike the other entry points
 * outside pomgpu_advance it does NOT bring the lazily kept 3-D arrays (wr, rho's round trip, trstr / srstr / taurstr, the interior of
 * uf / vf) up to date, so a
 * host that calls it after every pomgpu_mode_internal, as advance.f:57 does, pays for none of them. */
int pomgpu_check_velocity(pomgpu_ctx *ctx, double *vamax, int *imax, int *jmax);
/* domain_stats (advance.f:644-756), the sums behind print_section, reduced on the device (deterministic
 * tree; no state download).  out[8] = vtot, atot, mtot, stot, tavg, savg, eavg, ekin in the reference's
 * argument order.  sums_only != 0: this tile's partial sums as they stand before sum0d_mpi (out[4] =
 * sum(tb*dvol), out[6] = sum(et*darea), out[5] = 0) -- the caller reduces over ranks and forms the averages
 * exactly as the reference does on my_task 0; sums_only == 0: the single-task result. */
int pomgpu_domain_stats(pomgpu_ctx *ctx, double *out, int sums_only);
/* ---- output and restart files without PnetCDF (io_pnetcdf.F:57-410, :1661-2083) -----------------------------
 * NetCDF "64-bit offset" (CDF-2) files with the reference's dimensions, variables, order, types and attribute
 * texts, written directly.  Every rank writes its (im,jm) patch at (i0,j0) = (i_global(1), j_global(1)) of the
 * global grid; the rank with create = 1 lays the file out first (the caller puts a barrier between it and the
 * others).  stats: the eight domain_stats values after the rank reduction (NULL: this tile's own).  The file
 * names are the caller's (the reference builds them from wrk_pth, netcdf_file / write_rst_file and the counter). */
typedef struct pomgpu_file_meta {
  const char *title;          /* blkchar title */
  const char *time_start;     /* blkchar time_start: "days since <time_start>" */
  int im_global, jm_global;
  int i0, j0;                 /* 1-based global indices of the tile's (1,1) */
  int create;                 /* 1: create the file and write header + scalars + own patch; 0: own patch only */
  const double *stats;        /* vtot atot mtot stot tavg savg eavg ekin, or NULL */
} pomgpu_file_meta;
/* The two writers return once the file is laid out and a snapshot of its arrays has been taken on the device; a host
 * thread brings the snapshot over on a copy stream and writes it while the model goes on.  pomgpu_io_wait joins it and
 * returns its status (pomgpu_sync, the next write and pomgpu_destroy call it too). */
int pomgpu_io_wait(pomgpu_ctx *ctx);
int pomgpu_write_output(pomgpu_ctx *ctx, const char *path, const pomgpu_file_meta *meta);    /* write_output_pnetcdf */
int pomgpu_write_restart(pomgpu_ctx *ctx, const char *path, const pomgpu_file_meta *meta);   /* write_restart_pnetcdf */
/* read_restart_pnetcdf (io_pnetcdf.F:2420-2768) without PnetCDF: the 18 2-D and 19 3-D variables of the restart file are found BY
 * NAME in a classic NetCDF file (CDF-1 or CDF-2; order, extra variables, attributes and dimension names do not matter), and the
 * tile's (im,jm) patch at (i0,j0) of each lands in X(1:im,1:jm[,1:kb]) of its mirror -- cells beyond (im,jm) of a trimmed tile and
 * every other array keep what they held; then d = h + el, dt = h + et over the same cells, blkcon time0 = time = the file's `time`,
 * and cont_bry = int(the file's `iint`) if cont_bry was non-zero at the call.  *time0_out / *iint_out (either may be NULL) return the
 * two scalars.  Of `meta` only im_global, jm_global, i0, j0 are used.  Synchronous: the state is complete when the call returns; a
 * file this context is still writing is joined first, and whatever the library keeps lazily is completed before mirrors are
 * overwritten.  The host only reads raw big-endian runs into pinned buffers and copies them over; the byte reversal and the scatter
 * into the mirrors are a kernel (in the fp32-storage variants it rounds the 3-D arrays as an upload does).
 * Refused with POMGPU_EINVAL, error_status = 1 and the cause in pomgpu_last_error, BEFORE any mirror is written: a variable that is
 * absent, not NC_DOUBLE, a record variable or of other dimension lengths than (kb, jm_global, im_global) / (jm_global, im_global);
 * a file shorter than a variable's begin + size; any other magic (CDF-5, HDF5); a tile that does not fit the global grid.  An I/O
 * error half way leaves the state unspecified (error_status = 1). */
int pomgpu_read_restart(pomgpu_ctx *ctx, const char *path, const pomgpu_file_meta *meta, double *time0_out, double *iint_out);   /* read_restart_pnetcdf */

/* A cold start without PnetCDF: what initialize (initialize.f:24-36) does after read_input -- initialize_arrays, read_grid,
 * initial_conditions, update_initial, bottom_friction -- from the reference's three input files, on the device.
 * grid: <...>.grid.nc (io_pnetcdf.F:2113-2156): z, zz (at least kb values) and dx dy lon_rho lat_rho lon_u lat_u lon_v lat_v lon_psi
 * lat_psi angle h fsm as (jm_global, im_global); init: <...>.init.nc (:2800-2810): an unlimited dimension, a variable Level, and T, S as
 * (record, Level >= kb-1, jm_global, im_global), of which record 1 and levels 1..kb-1 are read; clim: <...>.clim.nc (:2875-2878): Tclim,
 * Sclim as (record, kb, jm_global, im_global) with at least 10 records, of which record 10 is read (initialize.f:407).  Classic NetCDF
 * (CDF-1 or CDF-2), every variable found BY NAME, NC_FLOAT or NC_DOUBLE (fsm also NC_BYTE, NC_SHORT, NC_INT).
 * Precondition: blkcon holds read_input's constants (pomgpu_set_con, or an upload of con alone).  Of `meta` only im_global, jm_global,
 * i0, j0 are used; every rank of a decomposition names the same files with its own i0, j0 -- not collective: a tile with a west / south
 * neighbour reads ONE more column / row on its low side and forms dum, dvm, aru, arv of its ghost line from it, where the reference
 * exchanges them (io_pnetcdf.F:2255-2256, initialize.f:370-371).  baropg_mcc (npg = 2) posts its own order exchange as ever.
 * The call completes what the library keeps lazily, joins a file still being written, ZEROES blk2d, blk3d and bdry (the COMMON blocks
 * at program start), sets the readers' defaults (dx = dy = h = 1 over the padded arrays) and then fills the state as the reference does:
 * dz dzz, cor, period (from THIS tile's cor(im/2, jm/2), as the reference computes it), art aru arv, dum dvm, d dt, tb sb t s (level
 * kb stays +0.0: the reference copies an uninitialised automatic array there), tsurf ssurf, the eight boundary arrays tbe .. sbs,
 * rfe = rfw = rfn = rfs = 1, tclim sclim, rmean and rho (dens), update_initial with baropg / baropg_mcc by npg, drx2d dry2d, cbc.
 * cor and cbc (sin, log) and dz, dzz are formed on the host with libm; everything else is kernels behind the copies of raw big-endian
 * bands (the restart reader's loop: POMGPU_IO_CHUNK_KB applies; the fp32-storage variants round 3-D arrays as an upload does).
 * time, time0, iint, the record slots and a registration by pomgpu_set_forcing_files stay untouched.  Synchronous.
 * info (may be NULL): cflmin = this tile's min of cfl over cfl > 0 (parallel_mpi.f:493-499; huge(), what minval gives, if there is none; the caller
 * reduces over ranks and prints the warning) and period.
 * Refused with POMGPU_EINVAL, error_status = 1 and file and cause in pomgpu_last_error, BEFORE any mirror, slot or blkcon member
 * changes: another magic (CDF-5, HDF5), a missing or misshapen variable, a file shorter than begin + size, a tile outside the global
 * grid, cor(im/2, jm/2) == 0 (the reference stops there, initialize.f:354-355), npg other than 1 or 2 (:506-508), a value of fsm in
 * the tile's window other than 0 or 1 (the kernels fold mask multiplies; pomgpu_upload refuses the same).  An I/O error half
 * way leaves the state unspecified (error_status = 1). */
typedef struct pomgpu_cold_info {
  double cflmin;
  double period;
} pomgpu_cold_info;
int pomgpu_cold_start(pomgpu_ctx *ctx, const char *grid, const char *init, const char *clim, const pomgpu_file_meta *meta,
                      pomgpu_cold_info *info);
/* Z-level input (a context setting; default 0 / 0: the files hold sigma levels, everything above as it stands).  init_on_z: pomgpu_cold_start
 * takes the init file as z-level data -- what the reference's commented call sites (initialize.f:410-422, io_pnetcdf.F:2805-2817) are for:
 * `Level` must be a 1-D NC_FLOAT / NC_DOUBLE variable of ks values, 2 <= ks <= 300, finite and strictly increasing (metres, positive down),
 * T and S (record, ks, jm_global, im_global); record 1, ALL ks levels, is read over the tile's window and tb, sb are the ztosig of it
 * (pomgpu_ztosig below), all kb levels -- level kb is the spline's extrapolation, not +0.0 -- and t, s, tsurf, ssurf and the eight boundary
 * lines follow from tb, sb as initialize.f:437-460 and update_initial have them.  clim_on_z: the same for Tclim, Sclim as (record, ks,
 * jm_global, im_global) with the levels in the clim file's variable `z` (io_pnetcdf.F:2858); record 10 is read; the two files may have
 * different levels.  Still no message round: ztosig's fill-in looks at all four neighbours of a column, so a tile reads one more column /
 * row towards EVERY neighbour, forms its ghost lines with the owner's arithmetic where the reference exchanges t (initialize.f:586), and
 * makes the copies onto physical edges only where it has no neighbour.  Every cell of a tile is the single tile's result on that window.
 * More refusals of pomgpu_cold_start, before anything changes: the level variable absent, not 1-D, of another type, outside 2..300 values,
 * not finite and strictly increasing; T / S / Tclim / Sclim with another level count than it; a tile whose window does not fit the grid.
 * pomgpu_set_forcing_files under clim_on_z: the clim check wants `z` and (ks, jm_global, im_global) with at least 12 records; restore_interior's
 * monthly fetch reads the window's ks levels and maps them into the (im,jm,kb) record in place of the plain unpack, on the stream the step is
 * enqueued on, with buffers allocated at registration (a step still allocates nothing); t_w s_w t_n s_n come from the tclim, sclim mirrors as
 * ever.  This call refuses (POMGPU_EINVAL) to change clim_on_z once a clim file is registered.  Z-level .lbry.nc files
 * (bounds_forcing.f:636-716) are pomgpu_set_z_lateral's, below. */
int pomgpu_set_z_inputs(pomgpu_ctx *ctx, int init_on_z, int clim_on_z);
/* Z-level lateral files (a context setting; default 0: the lbry file holds sigma levels, today's behaviour bit for bit and refusal for
 * refusal) -- what the reference's commented blocks behind read_boundary_conditions_pnetcdf (bounds_forcing.f:636-716, :757-836) are for.
 * Under lbry_on_z pomgpu_set_forcing_files wants of the lbry file: `z`, a 1-D NC_FLOAT / NC_DOUBLE variable of ks values, 2 <= ks <= 300,
 * finite and strictly increasing; temp.east salt.east as (record, ks, jm_global), temp.south salt.south as (record, ks, im_global); zeta, u
 * and v as ever (the reference maps T and S only).  lateral_bc's fetch reads the four variables on all ks levels over the tile's line and
 * one more point towards every neighbour, and maps each line onto the sigma levels into the record's tbe sbe / tbs sbs with the line form of
 * ztosig (pomgpu_ztosig_line below: east with h(imm1,j), south with h(i,2)), behind the unpack of everything else, on the stream the step is
 * enqueued on, with buffers allocated at registration.  Every rank maps every line with its own h, as the reference does; no message round.
 * t_w s_w t_n s_n come from the tclim, sclim mirrors as ever.  More refusals of pomgpu_set_forcing_files, before anything changes: `z`
 * absent, not 1-D, of another type, outside 2..300 values, not finite and strictly increasing; one of the four variables with another
 * level count than it; a tile whose window does not fit the grid; im or jm below 4.  This call refuses (POMGPU_EINVAL) to change the
 * setting once an lbry file is registered. */
int pomgpu_set_z_lateral(pomgpu_ctx *ctx, int lbry_on_z);
/* Which of the four open boundaries the lbry file feeds (a context setting; default EAST|SOUTH: today's behaviour bit for bit and refusal
 * for refusal).  read_boundary_conditions_pnetcdf (io_pnetcdf.F:3393-3621) reads the .east and .south variables only, takes t_w s_w t_n s_n
 * from line i = 1 / j = jm of tclim sclim (:3606-3614), leaves u_w v_w u_n v_n zero and never writes elw eln; its commented look-ups for
 * west and north (:3458-3463, :3474-3479, :3491-3498), its commented tclim fall-backs for east and south (:3607-3608, :3612-3613) and the
 * commented z-level blocks for all four sides (bounds_forcing.f:657-716, :777-836) show the four-sided reader this setting completes;
 * lateral_bc (bounds_forcing.f:841-865), bcond(2) (:47-78) and bcond(4) (:175-229) are four-sided already.
 * Variable names follow the reference's active pattern <var>.<side>: zeta.west u.west v.west temp.west salt.west, and the same with .north
 * (the commented 'west.u' / 'tw' are an older spelling and are not accepted); zeta.west is (record, jm_global), the other .west variables
 * (record, kb, jm_global), zeta.north (record, im_global), the other .north variables (record, kb, im_global) -- the shapes of .east and
 * .south --, each NC_FLOAT or NC_DOUBLE, found by name, CDF-1 or CDF-2, the record dimension unlimited or fixed.
 * A side that is ON: its elevation line is the tile's piece of zeta.<side> over 1:jm / 1:im and untouched beyond, as ele els are today;
 * its four (., kb) arrays are the tile's pieces of temp salt u v, zero beyond jm / im, in the reader's argument order (t_w s_w u_w v_w ...
 * t_n s_n v_n u_n ...: v before u on north and south).
 * A side that is OFF: t s are the line of tclim sclim next to that side -- i = 1, i = im, j = 1, j = jm of the TILE, as the reference's
 * statements are per rank --, u v are zero, the elevation line is left as the state holds it, and the file's variables of that side are
 * not looked up at all: the file need not hold them, and if it does they are ignored, as extra variables are.  For west and north OFF is
 * the reference's live code, for east and south its commented code.
 * Every rank reads every ON side with its own i0, j0, as the reference does: not collective, no message round.
 * Under pomgpu_set_z_lateral(1) temp / salt of every ON side are on the levels of the file's `z` and are mapped into the record by the
 * line form of ztosig with that side's edge number (0 east h(imm1,j), 1 south h(i,2), 2 west h(2,j), 3 north h(i,jmm1)), all lines in one
 * launch; one window point is read towards every neighbour (.east / .west towards the south and north one, .south / .north towards the
 * west and east one); u v zeta stay on sigma levels; OFF sides take the tclim line as above.
 * pomgpu_set_forcing_files checks the header for the variables of the ON sides only (up to twenty), names the variable in every refusal
 * and refuses before anything is kept; a fetch looks for its record in the ON sides' variables.
 * Refused with POMGPU_EINVAL and the cause in pomgpu_last_error: `sides` outside 1..15; a change of the mask once an lbry file is
 * registered. */
enum { POMGPU_SIDE_EAST = 1, POMGPU_SIDE_SOUTH = 2, POMGPU_SIDE_WEST = 4, POMGPU_SIDE_NORTH = 8 };
int pomgpu_set_lateral_sides(pomgpu_ctx *ctx, int sides);

/* The forcing files without PnetCDF: read_wind_pnetcdf, read_heat_pnetcdf, read_surface_pnetcdf (io_pnetcdf.F:2912-3224),
 * read_boundary_conditions_pnetcdf (:3393-3621), read_restore_ts_interior_pnetcdf (:3275-3333).  The host names the files once --
 * sfrc: <...>.sfrc.nc (sustr svstr shflux swrad SST SSS), lbry: <...>.lbry.nc (zeta u v temp salt, each .east and .south), clim:
 * <...>.clim.nc (Tclim Sclim); any of them may be NULL: that source stays as it is (records by setter, or constant forcing) -- and from
 * then on pomgpu_wind / _heat / _surface, pomgpu_lateral_bc and restore_interior take record n (restore: month mod(n+9,12)+1) from the
 * file when their own schedule asks for it: the tile's rows with pread into one of two pinned buffers, one copy and one kernel on the
 * stream, which swaps bytes, widens NC_FLOAT, converts units (wind -x/1025., heat -x/rhoref/3986.), tapers the wind against the tile's
 * dum / dvm (:2966-2995) and builds the lateral record (t_w s_w t_n s_n from tclim sclim, u_w v_w u_n v_n zero, elw eln untouched).  The
 * host is held up for the preads alone.  A registered sfrc / lbry file makes pomgpu_advance / pomgpu_run call surface_forcing /
 * lateral_bc; the setters of a source that has a file are refused.  Of `meta` only im_global, jm_global, i0, j0 are used; every rank of a
 * decomposition names the same files with its own i0, j0 -- not collective, no message round.
 * The call opens each file and checks its header: classic NetCDF (CDF-1 or CDF-2), every variable found BY NAME, NC_FLOAT or NC_DOUBLE,
 * the record number as the slowest dimension (the unlimited one, or a fixed one), then (jm_global, im_global) in sfrc; (jm_global),
 * (im_global), (kb, jm_global), (kb, im_global) in lbry; (kb, jm_global, im_global) with at least 12 records in clim.  Anything else
 * -- and a file shorter than the records its header counts, a tile outside the global grid -- is refused with POMGPU_EINVAL,
 * error_status = 1 and the cause in pomgpu_last_error; nothing is registered then and no mirror or record slot changes.  At a fetch, a
 * record beyond the file's count or end (looked at once more: the file may have grown) fails that step the same way, before the record
 * slot is written. */
int pomgpu_set_forcing_files(pomgpu_ctx *ctx, const char *sfrc, const char *lbry, const char *clim, const pomgpu_file_meta *meta);
/* the restore rate's file: see pomgpu_set_restore_rate_record above */
int pomgpu_set_restore_rate_file(pomgpu_ctx *ctx, const char *path, const pomgpu_file_meta *meta);
/* the water files: see pomgpu_water above */
int pomgpu_set_water_files(pomgpu_ctx *ctx, const char *prefix, const pomgpu_file_meta *meta);

/* One internal step for the current blkcon.iint: get_time, [surface_forcing, lateral_bc -- once the host has named
 * forcing files or supplied forcing / lateral records, see above; skipped otherwise: constant forcing; water inside surface_forcing, or
 * alone where no surface source is registered, once water is on], lateral_viscosity,
 * mode_interaction, isplit x mode_external, mode_internal, check_velocity (advance.f:6-59 minus print and
 * output, which stay on the host).  Does not synchronise: a record fetched from a file holds the host for its preads only. */
int pomgpu_advance(pomgpu_ctx *ctx);
/* nsteps x { iint = iint+1; advance }  (pom.f:17-19).  Does not synchronise.  On several tiles with the second stream agreed
 * (pomgpu_rccl_init / pomgpu_transport_side_agree) every step but the last of the call leaves realvertvl (solver.f:2024-2067) and the
 * exchange of wr (:2055) to the step that follows: they run on the second stream beside that step's external substeps -- wr has
 * no reader on the hot path.  The last step of the call does both at once, so after the call the state is complete.  Like every
 * call that posts message rounds, every rank makes it with the same nsteps.
 * wr ON ONE TILE (a context without exchange hook, transport or wide-halo mode): wr is a diagnostic that no routine of the step reads,
 * so pomgpu_mode_internal -- called directly, by pomgpu_advance or by pomgpu_run -- ends without realvertvl and only notes that wr is
 * due.  wr is "current" in the sense of every other lazily kept array: whatever looks at the mirrors or overwrites them from outside
 * the step -- pomgpu_download*, pomgpu_upload*, pomgpu_device_2d / _3d, the two file writers, pomgpu_read_restart,
 * pomgpu_tune_placement, pomgpu_domain_stats, every stand-alone kernel entry point below, a pomgpu_set_con that changes dti2 -- first
 * forms the wr of the last completed step, bit for bit what realvertvl at the end of that step would have stored (between two
 * mode_internal nothing writes w, u, v, dt, et, etb, and et holds what etf held, advance.f:525-534).  Steps that follow each other
 * unobserved never form it.  pomgpu_realvertvl itself reads etf as the reference does and replaces whatever was due.
 * POMGPU_WR_NODEFER restores realvertvl at the end of every step.
 * uf, vf ON ONE TILE (the same kind of context, kb in 6..64, im and jm >= 8, no address handed out by pomgpu_device_2d / _3d): profu,
 * profv and the filter of advance.f:469-514 are one kernel on the interior (5 <= i <= im-3, 5 <= j <= jm-3), which leaves the step with
 * u = uf, v = vf there without storing uf, vf (levels 1..kbm1).  Nothing in the step reads them before the next advq rewrites both
 * arrays whole, so the copy u -> uf, v -> vf is kept lazily like wr: the same callers as above (all but pomgpu_set_con) make it first,
 * and the next pomgpu_mode_internal that runs its 3-D part drops it.  POMGPU_UV_NOFUSE keeps the two kernels apart.
 * l, dtef ON ONE TILE (the same kind of context, no address handed out by pomgpu_device_2d / _3d): profq forms both for its two solves
 * and nothing else in the step reads them; the next profq rewrites both whole (solver.f:1338-1352, :1388).  They cannot be formed
 * afterwards (l = |q2lb / q2b| takes the old q2b, q2lb, which the filter overwrites), so there is nothing lazy about them: a step of
 * pomgpu_run that another step of the SAME call follows does not store them, the last step of every call does, and so do
 * pomgpu_advance, pomgpu_mode_internal, pomgpu_profq and every context on tiles, always.  After every call that returns POMGPU_OK
 * the two arrays are those of the last completed step, with nothing for an observer to wait for.  A step in front of one that asks
 * for a forcing or lateral record stores them as well (one step per record interval): a pomgpu_run that ends at a record the file or
 * the host does not have leaves the whole state of its last completed step.  A pomgpu_run that FAILS in step k < nsteps for another
 * reason (a refused launch, a failed copy) leaves l, dtef of an earlier step (the last one that stored) beside the other arrays;
 * blkcon.error_status is set in that case anyway.  POMGPU_LD_EAGER stores them in every step. */
int pomgpu_run(pomgpu_ctx *ctx, int nsteps);

/* Where the 3-D arrays live (no counterpart in the reference; optional).  The same kernels on the same bytes run up to 6 %
 * faster or slower with where in HBM their arrays lie; which places are good differs from process to process and cannot be seen from
 * user space, but is reproducible inside one process.  This call MEASURES it: blk3d and the 3-D scratch arrays move into one
 * allocation with room in front, up to max_try layouts (a start offset, and the arrays at their distance or 256 MiB further apart) are tried with one untimed and `steps` timed internal steps each (real
 * steps: the model advances by ntried x (steps + 1); results do not depend on where an array lives) and the fastest is kept.  ms_out / front_mib_out /
 * pad_mib_out (max_try entries each, may be NULL): what each trial took per step, how far into the allocation blk3d started and how much
 * further apart than their size its arrays were; *ntried = 0 when nothing was
 * tried (arrays below 64 MiB, no memory for the move).  On several tiles the trial steps post message rounds: every rank makes the
 * call alike (same steps, same max_try) and keeps its own best.  Needs the arrays' size plus the room again while it moves in.
 * The placement survives pomgpu_upload: a host that wants its run to start from an untouched state tunes on the initial state
 * and uploads it again (state and blkcon) before its first step.
 * The call MOVES the 3-D arrays (and frees the allocations they lived in): every address obtained from pomgpu_device_3d before it
 * would dangle, so the call refuses (POMGPU_EINVAL) once pomgpu_device_3d has been used on the context -- tune first, take addresses
 * afterwards.  It also refuses while the time-mean output is on (pomgpu_set_mean_output: the trial steps would be accumulated) -- tune
 * first, switch the mean on afterwards; that is checked before "nothing tried".  If a move fails half way (a HIP error inside it) the mirrors no longer hold the state: error_status = 1 and every later
 * hot-path call on this context returns POMGPU_EHIP; destroy it and upload the state into a new one. */
int pomgpu_tune_placement(pomgpu_ctx *ctx, int steps, int max_try, double *ms_out, long *front_mib_out, long *pad_mib_out, int *ntried, int *kept);

/* ---- time-mean output (no counterpart in the reference; optional, off by default: with it off every byte is as without it) --------------
 * pomgpu_write_output copies uab vab elb u v t s rho w as they stand at the step of the call; a snapshot every iprint steps aliases whatever
 * is faster than iprint * dti.  With the mean on, the library keeps one fp64 accumulator per field -- the nine above, which are the variables
 * of the output file that depend on time -- laid out like the field's mirror, and one integer count.
 * pomgpu_set_mean_output: on != 0 allocates the accumulators (3 x n2 + 6 x n3 doubles) and sets every one of them to +0.0 and the count to 0;
 * if they exist already it zeroes them and the count.  on == 0 frees them.  Nothing else but pomgpu_write_output_mean resets them: not an
 * upload, not pomgpu_read_restart, not pomgpu_cold_start -- a host that replaces the state inside an interval switches the mean on again.
 * The accumulators are not in the restart file, whose schema is the reference's: a job that restarts inside an output interval loses that
 * interval's partial sums.  Refused with POMGPU_EINVAL: the fp32-storage variants (which refuse pomgpu_write_output too), a 2-D-only context.
 * pomgpu_tune_placement refuses while the mean is on -- its trial steps are real steps and would count: tune first, switch the mean on afterwards.
 * pomgpu_mean_accumulate: the step's accumulation -- every accumulator becomes acc + x, ONE fp64 add per cell, in step order, x being what
 * pomgpu_download would show at that moment (read from wherever it lives: no lazily kept array is formed for it, no message round is posted;
 * one kernel launch for the nine fields).  pomgpu_advance and pomgpu_run make the call themselves behind mode_internal, where advance.f:38
 * writes, while the mean is on; the entry point is for hosts that string the routines together (the Fortran `advance`): call it after
 * pomgpu_mode_internal.  POMGPU_EINVAL while the mean is off.
 * pomgpu_mean_count: the steps accumulated since the switch or the last mean file; -1 while the mean is off.
 * pomgpu_mean_download: acc / (double)count -- one IEEE division per cell, not a multiplication by a reciprocal -- of one accumulated array
 * (is3d, slot: enum pom_slot2d / pom_slot3d) into `host`, n2 or n3 doubles in the mirror's shape.  Padding cells, and cells beyond (im, jm) of
 * a trimmed tile, may hold anything.  Resets nothing.  POMGPU_EINVAL: a slot that is not accumulated, count 0, the mean off.
 * pomgpu_write_output_mean: pomgpu_write_output's file, byte for byte in the header -- dimensions, variables, attributes, offsets, `time` and
 * the statistics as of the call; every reader of an output file reads it -- with the MEANS as the values of the nine fields.  Same asynchronous
 * writer; the snapshot of the nine is taken by a kernel that stores acc / count into it and +0.0 into the accumulator in the same pass, on
 * the kernels' stream: steps enqueued right after the call accumulate into clean sums while the file is still being written.  The count
 * returns to 0.  On tiles every rank writes its patch, as pomgpu_write_output does.  Count 0 at the call: POMGPU_EINVAL, error_status = 1, the
 * cause in pomgpu_last_error; no file is touched, nothing changes. */
int pomgpu_set_mean_output(pomgpu_ctx *ctx, int on);
int pomgpu_mean_accumulate(pomgpu_ctx *ctx);
int pomgpu_mean_count(pomgpu_ctx *ctx);
int pomgpu_mean_download(pomgpu_ctx *ctx, int is3d, int slot, double *host);
int pomgpu_write_output_mean(pomgpu_ctx *ctx, const char *path, const pomgpu_file_meta *meta);

/* ---- passive tracers (no counterpart in the reference; optional, off by default: with none registered every byte and every launch is as
 * without them) ------------------------------------------------------------------------------------------------------------------------
 * Up to POMGPU_MAXTRACERS fields that the flow carries and mixes as it does T and S -- dye, age, a first-order decaying constituent --
 * and that never act on the flow: with tracers registered every other array keeps the bits it has without them.  The reference's users
 * add such a field by repeating the advt / proft / bcond(4) / filter lines of mode_internal for it; that is what the library does, per
 * tracer n = 1..ntr, inside pomgpu_mode_internal whenever the 3-D body runs (advance.f:362; mode 3 and mode 4), behind advance.f:454 and
 * in front of :459, with the run's own nadv nitera tprni smoth umol dti2 and the u v w aam kh etb etf of that moment:
 *   1. advt1 / advt2(trb, tr, trclim, trf) as for T, level kb of trb (tr) and the fb - fclim + fclim round trip included;
 *   2. only with a source array or lam != 0: trf = trf + dti2 * (q - lam * trb) on (1:im, 1:jm, 1:kbm1), four separate fp64 operations;
 *   3. the exchange of advance.f:436;   4. proft(trf, wtrsurf, trsurf, nbc);
 *   5. bcond(4)'s lines for T with trf, tr, trb[ewns] in place of uf, t, tb[ewns], and its mask on levels 1..kbm1;
 *   6. tr = tr + .5*smoth*(trf + trb - 2.*tr); trb = tr; tr = trf on the whole arrays.  No restore_interior, no dens.
 * The work array trf is the library's own; its level kb is +0.0.  Tracers are not in the output, restart or mean files (their schemas are
 * the reference's): they have a file family of their own, below (pomgpu_write_tracers, pomgpu_read_tracers).  pomgpu_upload,
 * pomgpu_cold_start and pomgpu_read_restart do not touch them.
 * pomgpu_set_tracers: n > 0 allocates n tracers (or keeps the allocation of a context that has n already) and sets every array of theirs
 * to +0.0, nbc to 1, lam to 0, no source; n == 0 frees them.  POMGPU_EINVAL: n outside 0..POMGPU_MAXTRACERS, the fp32-storage variants, a
 * 2-D-only context.
 * pomgpu_tracer_upload / _download: array `which` of tracer n (1-based), HOST doubles in the shape of the array it stands for: TRB TR
 * CLIM SOURCE as tb (n3 doubles), WSURF SURF as wtsurf (n2), BE BW as tbe (jm_local x kb), BN BS as tbn (im_local x kb).  Uploading CLIM or
 * SOURCE gives the tracer an array of its own; a NULL host for either returns it to the default (the shared zero array / no source), and
 * downloading a default delivers zeros.  POMGPU_EINVAL: no tracers registered, n outside 1..ntr, an unknown `which`, a NULL host otherwise.
 * pomgpu_tracer_set: the surface condition (1: the flux wtrsurf, 3: the value trsurf; 2 and 4, the short-wave forms, are refused) and the
 * decay rate lam (1/s).  pomgpu_tracer_count: the number registered.
 * pomgpu_tune_placement refuses while tracers are registered -- its trial steps are real steps and would move them. */
#define POMGPU_MAXTRACERS 8
enum pomgpu_tracer_array {
  POMGPU_TR_TRB = 0, POMGPU_TR_TR = 1, POMGPU_TR_CLIM = 2, POMGPU_TR_SOURCE = 3, POMGPU_TR_WSURF = 4, POMGPU_TR_SURF = 5,
  POMGPU_TR_BE = 6, POMGPU_TR_BW = 7, POMGPU_TR_BN = 8, POMGPU_TR_BS = 9
};
int pomgpu_set_tracers(pomgpu_ctx *ctx, int n);
int pomgpu_tracer_count(pomgpu_ctx *ctx);
int pomgpu_tracer_upload(pomgpu_ctx *ctx, int n, int which, const double *host);
int pomgpu_tracer_download(pomgpu_ctx *ctx, int n, int which, double *host);
int pomgpu_tracer_set(pomgpu_ctx *ctx, int n, int nbc, double lam);
/* ---- tracer files, means and inventory (off unless called: with no tracers registered, or with these entry points unused, every byte
 * and every launch is as without them) ----------------------------------------------------------------------------------------------------
 * pomgpu_tracer_get: nbc and lam of tracer n as pomgpu_tracer_set (or a file) left them; either pointer may be NULL.
 * pomgpu_tracer_stats: the inventory, out[4 * (n-1) + 0..3] = tot avg min max of tracer n, reduced on the device in one pass over the
 * columns for all tracers (two launches, a fixed-shape tree, no atomics: same launch, same bits).  tot = sum trb * dx*dy*fsm*dt*dz(k) over
 * 2:imm1 x 2:jmm1, k = 1..kbm1 -- domain_stats' sum(tb*dvol) with trb in tb's place, so tile sums add up under the host's rank reduction;
 * avg = tot / vtot with vtot from the same pass (0 where vtot is 0); min, max of tr over the cells of (1:im, 1:jm, 1:kbm1) with fsm != 0.
 * Time mean: while the mean is on (pomgpu_set_mean_output) AND tracers are registered the library keeps one more fp64 accumulator of n3
 * doubles per tracer, with a count of their own.  pomgpu_set_mean_output(1) creates and zeroes them for the tracers registered then;
 * pomgpu_set_tracers(n > 0) while the mean is on creates them anew at +0.0 with count 0 (it zeroes the tracers themselves) and leaves the
 * nine fields' sums and count alone; pomgpu_set_tracers(0) and pomgpu_set_mean_output(0) free them.  pomgpu_mean_accumulate -- called by
 * pomgpu_advance / pomgpu_run as before -- adds tr of every tracer with ONE fp64 add per cell: the nine fields' kernel launched once more
 * with the tracers' table, i.e. ONE added launch per step whatever the number of tracers, and none without tracers or with the mean off.
 * pomgpu_tracer_mean_count: steps accumulated, -1 while there are no tracer accumulators.  pomgpu_tracer_mean_download: acc / (double)count
 * of tracer n, n3 doubles shaped like tr; resets nothing; POMGPU_EINVAL at count 0 or without accumulators.
 * pomgpu_write_tracers: one CDF-2 file of `kind`, laid out and written as pomgpu_write_output writes (meta->create, every rank its patch,
 * asynchronous, joined by pomgpu_io_wait); NN is the tracer number, two digits; everything is NC_DOUBLE.
 *   POMGPU_TRFILE_RESTART  description "tracer restart file"; dimensions time = 1, z = kb, y, x; iint (scalar), time {time}, ntr (scalar);
 *     nbcNN, lamNN (scalars) per tracer; then per tracer trNN, trbNN, trfNN (z, y, x), all kb levels, as pomgpu_tracer_download shows them
 *     and trf straight from the work array: trf survives between steps unmasked and smol_adif reads its edge lines when nitera > 1, so
 *     trb and tr alone are not the state of the run.
 *   POMGPU_TRFILE_OUTPUT  description "tracer output file"; the output file's dimensions time, z, zz, y, x; time; per tracer totNN avgNN
 *     minNN maxNN {time}; z, zz; per tracer trNN (time, zz, y, x).  trstats: 4 * ntr rank-reduced values in pomgpu_tracer_stats' order,
 *     as meta->stats is for the output file; NULL: this tile's own.
 *   POMGPU_TRFILE_OUTPUT_MEAN  the same file with acc / count in place of trNN: one kernel pass stores the quotient into the snapshot and
 *     +0.0 into the accumulator, the tracers' count returns to 0; `time` and the statistics are as of the call.  Count 0 or no accumulators:
 *     POMGPU_EINVAL, no file touched, nothing changed.
 * POMGPU_EINVAL too: no tracers registered, an unknown kind, a tile that does not fit the global grid, the fp32-storage variants.
 * pomgpu_read_tracers: a classic NetCDF file (CDF-1 or CDF-2) into the registered tracers; variables are found BY NAME, order, extra
 * variables and attributes do not matter.  For n = 1..ntr trNN is required: NC_DOUBLE, not a record variable, (kb, jm_global, im_global).
 * trbNN / trfNN are optional and an absent one takes trNN's values (a file with trNN alone is an initial file any tool can write); a
 * present one must have trNN's type and shape.  nbcNN / lamNN are optional and applied as pomgpu_tracer_set would; nbc other than 1 or 3 is
 * refused.  Tracers of the file beyond ntr are ignored.  The tile's (im, jm) patch at (i0, j0) lands in X(1:im, 1:jm, 1:kb); cells
 * beyond keep what they held; clim source wsurf surf be bw bn bs, the flow and every accumulator are not touched.  *time_out / *iint_out
 * (either may be NULL) return the file's `time` / `iint`, 0 where absent; they are applied to nothing.  The data path is
 * pomgpu_read_restart's -- pinned bands, a copy stream -- with one kernel behind each copy that reverses the staged bytes once and stores
 * them to one, two or three arrays.  No message round: on tiles every rank reads its own patch, ghost lines included.  Every refusal
 * comes BEFORE any array changes, with POMGPU_EINVAL, error_status = 1 and the cause in pomgpu_last_error: no tracers registered; a
 * required variable absent, of another type or shape, or a record variable; a file shorter than a variable's begin + size; any other
 * magic (CDF-5, HDF5); a tile that does not fit the global grid; the fp32-storage variants; a 2-D-only context. */
enum { POMGPU_TRFILE_RESTART = 0, POMGPU_TRFILE_OUTPUT = 1, POMGPU_TRFILE_OUTPUT_MEAN = 2 };
int pomgpu_write_tracers(pomgpu_ctx *ctx, const char *path, const pomgpu_file_meta *meta, int kind, const double *trstats);
int pomgpu_read_tracers(pomgpu_ctx *ctx, const char *path, const pomgpu_file_meta *meta, double *time_out, double *iint_out);
int pomgpu_tracer_stats(pomgpu_ctx *ctx, double *out);            /* 4 * ntr doubles: tot avg min max per tracer */
int pomgpu_tracer_get(pomgpu_ctx *ctx, int n, int *nbc, double *lam);
int pomgpu_tracer_mean_count(pomgpu_ctx *ctx);                    /* -1: no tracer accumulators */
int pomgpu_tracer_mean_download(pomgpu_ctx *ctx, int n, double *host);   /* acc / count, n3 doubles */

/* ---- Lagrangian floats (no counterpart in the reference; optional, off by default: with none registered every byte and every launch is as
 * without them, and with some every other array keeps its bits) -----------------------------------------------------------------------------
 * Water parcels that the model's own u, v, w of every internal step carry: surface drifters, larval or spill trajectories.  A float is
 *   x, y    index coordinates of the grid: the centre of cell (i, j) is x = i, y = j; u(i,j,k) sits at (i - 0.5, j), v(i,j,k) at (i, j - 0.5),
 *           w and t at (i, j);
 *   sig     sigma in [-1, 0];
 *   status  POMGPU_FLOAT_ACTIVE, _EXITED (it left 2..im-1 x 2..jm-1; the position is where it left) or _LOST (a position that was not
 *           finite, or admitted on land);   kind  0 follows w, 1 keeps its sigma (a surface drifter is sig = 0, kind = 1);
 *   id      an int the library carries and never reads.
 * The state is a structure of arrays: three arrays of n doubles and three of n ints, n <= POMGPU_MAXFLOATS.
 * Interpolation.  L(p, q, f) = p + f * (q - p).  A field point's horizontal cell: for u xs = x + 0.5, i0 = floor(xs), fx = xs - i0,
 * j0 = floor(y), fy = y - j0; for v the same with y + 0.5; for cell-centre fields floor(x), floor(y); i1 = i0 + 1, j1 = j0 + 1.  Every
 * coordinate is limited to [0, im + 1] ([0, jm + 1]) by fmax then fmin before it becomes an integer and every index to 1..im (1..jm) after
 * the fractions are formed, so no position or velocity addresses memory outside the arrays.  Vertically u v t s live on zz: level 1 alone
 * for sig >= zz(1), level kbm1 alone for sig <= zz(kbm1), else the k with zz(k) >= sig > zz(k+1) and fz = (zz(k) - sig) / (zz(k) - zz(k+1));
 * w lives on z: the k in 1..kbm1 with z(k) >= sig > z(k+1) and the same fz with z.  A value is L in i, then in j, per level, then in k.
 * The velocity in index space is V(x, y, sig) = (U / DXU, V / DYV, W / D): DXU the bilinear interpolant, over u's four corners, of
 * 0.5 * (dx(i,j) + dx(max(i-1,1),j)), DYV likewise of dy and j - 1 over v's, D that of dt at cell centres (w is the sigma velocity).
 * The step, for ACTIVE floats, is one midpoint step of length dti with the fields frozen:
 *   (a1,b1,c1) = V(x,y,sig); xm = x + .5*dti*a1, ym alike, sm = sig + .5*dti*c1 (kind 1: sig) limited to [-1, 0]; (a2,b2,c2) = V(xm,ym,sm);
 *   xn = x + dti*a2, yn alike, sn = sig + dti*c2 (kind 1: sig); sn > 0 reflects to -sn, sn < -1 to -2 - sn, then sn is limited to [-1, 0].
 * Then, in this order: xn, yn or sn (as summed, before its limits) not finite: LOST, position kept; the containing cell (floor(xn + 0.5),
 * floor(yn + 0.5)) outside 2..im-1 x 2..jm-1: EXITED, xn yn sn stored; fsm of that cell 0: x, y kept, sig = sn, the float stays active and
 * tries again; otherwise xn yn sn stored.  pomgpu_advance / pomgpu_run make the step behind pomgpu_mean_accumulate and in front of
 * check_velocity in every step whose 3-D body ran (mode 3 and 4, not the first step of a run from rest; in mode 2 floats rest), with u v
 * w dt as that step left them: ONE launch (k_float_step) per step, none without floats.  pomgpu_float_step is the stage alone, for a host
 * that strings the routines together (after pomgpu_mode_internal and pomgpu_mean_accumulate).
 * pomgpu_float_upload: n floats from host arrays; kind NULL = all 0, id NULL = 0..n-1; n == 0 frees them.  The positions are admitted by
 * the step's classification: not finite or on land LOST, outside EXITED.  Replaces whatever was registered.
 * pomgpu_float_download: any pointer may be NULL.  pomgpu_float_count: the number registered.
 * pomgpu_float_sample: out[q * n + f], q = 0..4: lon lat depth t s of float f, whatever its status -- lon, lat bilinear in east_e, north_e
 * at cell centres; depth = et + sig * dt of the containing cell (indices limited like every index); t, s from that cell's column alone,
 * linear in sigma on zz as above, so that land zeros never mix in.
 * pomgpu_write_floats: one CDF-2 file, description "float file": dimension nfloat; iint, time (scalars, NC_DOUBLE); x y sig lon lat depth
 * t s (nfloat) NC_DOUBLE; status kind id (nfloat) NC_INT.  Output and checkpoint in one; written synchronously (68 MB for a million
 * floats) behind pomgpu_io_wait.  meta->title and time_start are used, the tile members are not.
 * pomgpu_read_floats: registers the floats of a classic file (CDF-1 or CDF-2) as pomgpu_float_upload would.  x y sig are found by name and
 * required: NC_DOUBLE, one shared 1-D length, not record variables, inside the file; status kind id are optional (NC_INT, that length),
 * anything else is ignored: a file with x y sig alone is an initial file any tool can write.  A stored status other than ACTIVE is kept
 * over the admission's verdict.  *time_out / *iint_out (either may be NULL) return the file's `time` / `iint`, 0 where absent, applied to
 * nothing.
 * Refused with POMGPU_EINVAL, error_status = 1 and the cause in pomgpu_last_error, before anything changes: n outside 0..POMGPU_MAXFLOATS;
 * a NULL position array; a context with any neighbour in pomgpu_dims -- floats live on a single tile, moving them between ranks takes a
 * message round a step; the fp32-storage variants; a 2-D-only context; step, sample or write with no floats registered; for the reader
 * also a file it cannot open, any other magic, a required variable absent, of another type or shape, a record variable or one that
 * reaches beyond the file, more than POMGPU_MAXFLOATS floats.  pomgpu_tune_placement refuses while floats are registered -- its trial
 * steps are real steps and would move them.  pomgpu_upload, pomgpu_cold_start and pomgpu_read_restart do not touch the floats. */
#define POMGPU_MAXFLOATS (1 << 26)
enum { POMGPU_FLOAT_ACTIVE = 0, POMGPU_FLOAT_EXITED = 1, POMGPU_FLOAT_LOST = 2 };
int pomgpu_float_upload(pomgpu_ctx *ctx, int n, const double *x, const double *y, const double *sig, const int *kind, const int *id);
int pomgpu_float_count(pomgpu_ctx *ctx);
int pomgpu_float_download(pomgpu_ctx *ctx, double *x, double *y, double *sig, int *status, int *kind, int *id);
int pomgpu_float_step(pomgpu_ctx *ctx);
int pomgpu_float_sample(pomgpu_ctx *ctx, double *out5n);
int pomgpu_write_floats(pomgpu_ctx *ctx, const char *path, const pomgpu_file_meta *meta);
int pomgpu_read_floats(pomgpu_ctx *ctx, const char *path, const pomgpu_file_meta *meta, double *time_out, double *iint_out);

/* ---- tides: harmonic open-boundary forcing and harmonic analysis (no counterpart in the reference; optional, off by default: with no
 * table registered every byte and every launch is as without them) ---------------------------------------------------------------------------
 * One table of nc <= POMGPU_MAXTIDES constituents, omega[c] in rad/s, serves the forcing and the analysis.
 * pomgpu_set_tides(ctx, nc, omega, sides, lines, meta): nc == 0 clears the table (and switches the analysis off).  sides: the POMGPU_SIDE_*
 * bits of the open boundaries that carry a tide (0: a table for the analysis alone).  lines[4 * s + q], s = 0 east, 1 south, 2 west, 3 north
 * (the order of the bits), q = 0..3 = elC elS unC unS: HOST arrays of nc x n_global doubles, constituent-major, n_global = jm_global for east /
 * west and im_global for south / north -- the GLOBAL line, the same on every rank; entries of an OFF side are not looked at; unC, unS may be
 * NULL: zero.  elC elS are elevation coefficients in metres, unC unS those of the depth-mean NORMAL velocity in m/s in the model's +i / +j
 * sense (not "outward").  meta: im_global jm_global i0 j0 are used; the library cuts the tile's stretch and, in the wide-halo external mode,
 * the extended tile's -- no message round, and the boundary messages carry nothing new.  The lines are copied; the call synchronises.
 * The value of constituent c is C * cos(omega[c] * t) + S * sin(omega[c] * t); amplitude A and Greenwich-style phase g in degrees,
 * A * cos(omega * t - g), are C = A cos g, S = A sin g (the Python and Fortran layers convert on the host).
 * Where the tide enters: bcond(2) of substep iext of internal step iint (bounds_forcing.f:43-83).  Where the reference reads elw(j) the library
 * reads e = elw(j), then e = e + (elC[c][j] * cw[c] + elS[c][j] * sw[c]) for c = 0 .. nc-1 in that order; uabw(j) alike with unC unS; the
 * other three sides alike with ele uabe, els vabs, eln vabn.  The tangential values (vabw vabe uabs uabn) are untouched.  The STORED boundary
 * arrays are never modified: a download gives what lateral_bc or the host left.  ramp, dum, dvm act afterwards as they do without a tide, so
 * lramp ramps the tide too.  Every path of the external mode does this, also the stand-alone pomgpu_mode_external and pomgpu_bcond(2).
 * Phasors: cw[c] = cos(omega[c] * t), sw[c] = sin(omega[c] * t), t = (time0 * 86400. + dti * (double)(iint - 1)) + dte * (double)iext seconds,
 * evaluated in fp64 ON THE HOST with the C library, as cor is.  pomgpu_tide_phasors(ctx, iint, iext, out) returns them, out[2c] = cw[c],
 * out[2c + 1] = sw[c].  A step's isplit x nc x 2 phasors reach the device as the arguments of ONE launch per internal step (k_tide_table,
 * while isplit * nc <= 240 -- isplit 30 at nc 8; a longer table takes one launch per 480 doubles); nothing is added per substep and
 * pomgpu_run stays free of host-device synchronisation.
 * pomgpu_tide_count: nc.
 * Harmonic analysis.  pomgpu_set_harmonic_analysis(ctx, on, every): from now on, at the end of every internal step with iint % every == 0 --
 * in pomgpu_advance / pomgpu_run behind the floats' stage and in front of check_velocity, in every mode -- ONE launch (k_harm_accum) adds f,
 * f * cn[c] and f * sn[c] of f = elb, uab, vab (what the mean output samples, read from the current generation) to 1 + 2 nc fp64 planes per
 * field, cn[c] = cos(omega[c] * t_n), sn[c] = sin(omega[c] * t_n), t_n = time0 * 86400. + dti * (double)iint from the host as kernel
 * arguments.  The host adds the outer product of the same basis b = [1, cn0, sn0, cn1, sn1, ...] to the (2 nc + 1)^2 normal matrix, row by
 * row.  on = 1 (again) zeroes sums, matrix and count; on = 0 frees them.  No lazily kept array is formed by the stage.
 * pomgpu_harmonic_accumulate: the stage alone, for a host that strings the routines together (after pomgpu_mode_internal); it samples
 * whatever iint says, `every` is the caller's business there.
 * pomgpu_harmonic_count: samples so far, -1 while off.  pomgpu_harmonic_sums(ctx, field, out): field 0 elb, 1 uab, 2 vab; out = (2 nc + 1)
 * planes of im_local x jm_local doubles, plane p = the sum of f * b[p].  pomgpu_harmonic_matrix(ctx, out, t2): the matrix, row-major, and
 * t2[0], t2[1] = t_n of the first and last sample (t2 may be NULL).  pomgpu_harmonic_solve(ctx, field, coef): the host inverts the matrix
 * (Gauss-Jordan with partial pivoting, fp64), a second kernel (k_harm_solve) applies the inverse per cell: coef = 2 nc + 1 planes, the mean,
 * then C and S of every constituent: f ~ mean + sum C cos(omega t) + S sin(omega t); amplitude hypot(C, S), phase g = atan2(S, C).
 * pomgpu_harmonic_reset: zeroes sums, matrix and count.  Nothing else resets them.
 * Refused with POMGPU_EINVAL, error_status = 1 and the cause in pomgpu_last_error, before anything changes: nc outside 0..POMGPU_MAXTIDES; a
 * NULL omega or meta with nc > 0; an omega or coefficient that is not finite; a NULL elevation line of an ON side; a tile stretch (or the
 * extended tile's) outside the global line; the two fp32 study builds; the analysis with no table, every < 1, or a singular matrix (fewer
 * samples than unknowns).  pomgpu_tune_placement refuses while a tide table or the analysis is on -- its trial steps are real steps.
 * pomgpu_write_harmonics: one CDF-2 file through the asynchronous patch writer (every rank its patch, as pomgpu_write_output), description
 * "harmonics file": dimensions ncon y x; omega(ncon), count, t_first, t_last (scalars, seconds), and for f = elb uab vab: f_mean(y,x),
 * f_amp(ncon,y,x), f_pha(ncon,y,x), all NC_DOUBLE; the phase is g of A cos(omega t - g) in degrees in [0, 360), formed on the device
 * (k_harm_constants: hypot and atan2 of k_harm_solve's C and S).  Writing resets nothing.  Refused like pomgpu_harmonic_solve.
 * pomgpu_set_tide_file: registers the table of a classic file (CDF-1 or CDF-2) as pomgpu_set_tides would.  omega(ncon), NC_DOUBLE, and per side
 * that has them el_amp.<side> el_pha.<side> and optionally un_amp.<side> un_pha.<side>, <side> = east south west north, each (ncon, jm_global |
 * im_global) NC_DOUBLE, amplitude and phase in degrees, are found by name; a side without el lines is OFF; anything else in the file is ignored.
 * The conversion is C = A cos(g pi / 180), S = A sin(g pi / 180) with the C library.  Refused before anything changes: a file it cannot open,
 * any other magic, omega absent or not one dimension of 1..POMGPU_MAXTIDES, an amplitude without its phase, un lines without el lines, a variable
 * of another type or shape, a record variable, one that reaches beyond the file; then pomgpu_set_tides' own refusals.
 * Not built: the Fortran wrappers and the driver's flags, sums that survive a restart, 3-D currents, nodal corrections, the tidal potential. */
#define POMGPU_MAXTIDES 8
int pomgpu_set_tides(pomgpu_ctx *ctx, int nc, const double *omega, int sides, const double *const *lines16, const pomgpu_file_meta *meta);
int pomgpu_tide_count(pomgpu_ctx *ctx);
int pomgpu_tide_phasors(pomgpu_ctx *ctx, int iint, int iext, double *out2nc);
int pomgpu_set_harmonic_analysis(pomgpu_ctx *ctx, int on, int every);
int pomgpu_harmonic_accumulate(pomgpu_ctx *ctx);
int pomgpu_harmonic_count(pomgpu_ctx *ctx);
int pomgpu_harmonic_sums(pomgpu_ctx *ctx, int field, double *out);
int pomgpu_harmonic_matrix(pomgpu_ctx *ctx, double *out, double *t2);
int pomgpu_harmonic_solve(pomgpu_ctx *ctx, int field, double *coef);
int pomgpu_harmonic_reset(pomgpu_ctx *ctx);
int pomgpu_write_harmonics(pomgpu_ctx *ctx, const char *path, const pomgpu_file_meta *meta);
int pomgpu_set_tide_file(pomgpu_ctx *ctx, const char *path, const pomgpu_file_meta *meta);

/* ---- the hot path: kernels (solver.f, bounds_forcing.f), device-resident ---------------- */
int pomgpu_advave(pomgpu_ctx *ctx);              /* solver.f:6-198   */
int pomgpu_advct(pomgpu_ctx *ctx);               /* solver.f:201-408 */
int pomgpu_advq(pomgpu_ctx *ctx, const double *qb, const double *q, const double *qf);   /* :411-477 */
int pomgpu_advt1(pomgpu_ctx *ctx, const double *fb, const double *f, const double *fclim, const double *ff); /* :480-574 */
int pomgpu_advt2(pomgpu_ctx *ctx, const double *fb, const double *f, const double *fclim, const double *ff); /* :577-731 */
/* smol_adif(xmassflux,ymassflux,zwflux,ff) (solver.f:1880-1967) is the ONE routine of SURVEY 8(b)'s export list without an
 * entry point: its three flux arguments are automatic (stack) arrays of advt2 (solver.f:588-590), never COMMON arrays, so a
 * host has nothing to pass by reference; it runs inside pomgpu_advt2 (nitera > 1: k_advt2_smol; nitera = 1: fused away). */
int pomgpu_advu(pomgpu_ctx *ctx);                /* solver.f:734-788 */
int pomgpu_advv(pomgpu_ctx *ctx);                /* solver.f:791-845 */
int pomgpu_baropg(pomgpu_ctx *ctx);              /* solver.f:848-940 */
int pomgpu_baropg_mcc(pomgpu_ctx *ctx);          /* solver.f:943-1159 (npg = 2) */
int pomgpu_dens(pomgpu_ctx *ctx, const double *si, const double *ti, const double *rhoo); /* :1162-1209 */
/* ztosig(zs,tb,zz,h,t,...) (initialize.f:547-595) with splinc / splint (:598-667): the vertical natural-cubic-spline mapping of z-level
 * temperature or salinity onto the sigma levels -- the routine behind the reference's commented call sites initialize.f:410-422.
 * zs: ks HOST doubles, the z levels in metres, positive down; src: the HOST array (im_local, jm_local, ks) in the reference's layout, the
 * tile's own ghost cells included (the reference's `tb` argument, a caller's temporary: it is uploaded for the call); t: the HOST address
 * of a 3-D COMMON array, mapped to its mirror like every array argument.  h and zz are the mirrors', the four neighbours the context's.
 * On X(1:im, 1:jm): t = 0, then every column 2 <= i <= im-1, 2 <= j <= jm-1 with h > 1.0 fills its missing values (< 0.01) from the four
 * RAW neighbours where zs(k) <= h -- amax1 is the REAL(4) intrinsic: the maximum arrives rounded to single precision -- and from the
 * level above, and is splined onto -zz(k)*h for ALL kb levels (level kb is an extrapolation); the ghost lines of t go through the
 * exchange hook / transport (nothing on one tile), then the copies onto physical edges, west east south north.  Bit for bit what the
 * reference's compiled routine leaves; the fp32-storage variants compute in fp64 and round once at the store.
 * Refused with POMGPU_EINVAL, error_status = 1 and the cause in pomgpu_last_error before t changes: ks outside 2..300 (splinc's nmax), zs
 * not finite or not strictly increasing, t not a blk3d array of the bound host block.  Synchronous. */
int pomgpu_ztosig(pomgpu_ctx *ctx, const double *zs, int ks, const double *src, const double *t);
/* ztosig for one lateral line (bounds_forcing.f:636-716): the block spreads the line across the tile, calls ztosig with the depth
 * hs = h(imm1,j) (edge 0, east), h(i,2) (1, south), h(2,j) (2, west) or h(i,jmm1) (3, north) and keeps the column im/2 / the row jm/2.  The
 * source does not vary across the line, so each line point is one ztosig column: of the fill-in's four neighbours two are the point's own
 * raw value, two the raw values of the points before and after it.  n_local = jm_local (east, west) or im_local (south, north), n = jm or im.
 * zs: ks HOST doubles; src: HOST, ks levels of n_local + 2 doubles each, line point a (1-based) at index a of its level: index 0 and
 * index n + 1 are the window points beyond the line's ends, ignored at a physical end, where the point takes the finished value of the
 * point next to it (zeros included); out: HOST, kb levels of n_local doubles, points beyond n zero, filled when the call returns.  h, zz
 * and the neighbours are the context's; no mirror changes and no message round is posted (a ghost end is formed from the window point
 * with the owner's arithmetic).  Refused with POMGPU_EINVAL as pomgpu_ztosig refuses ks and zs; also edge outside 0..3, im or jm below 4. */
int pomgpu_ztosig_line(pomgpu_ctx *ctx, int edge, const double *zs, int ks, const double *src, double *out);
/* The scalar device functions that restate host arithmetic, run as the kernels run them (tests; no counterpart in the reference).
 * in: nin HOST arrays of n doubles, out: n HOST doubles; the arrays are uploaded, one kernel computes one element per lane, the result
 * is copied back on the context's stream.  No mirror changes.  Synchronous.
 *   POMGPU_PROBE_DIVI      a, b                      divi(a, inv_of(b)): the quotient from the stored reciprocal, fp64
 *   POMGPU_PROBE_DIVI_F32  a, b                      the same in fp32: a and b are narrowed on the device, the quotient widened
 *   POMGPU_PROBE_GPOW15    x                         gpow15(x): glibc 2.35's pow(x, 1.5) as dens calls it
 *   POMGPU_PROBE_RAD_Q     swrad, r, omr, x1, x2     proft_rad_q(...): proft's short-wave term, the REAL(16) expression rounded once
 * Refused with POMGPU_EINVAL and the cause in pomgpu_last_error, before anything is allocated or launched: an unknown op, nin other than
 * the op's number of inputs, n outside 1..2^22, a NULL pointer. */
enum { POMGPU_PROBE_DIVI = 0, POMGPU_PROBE_DIVI_F32 = 1, POMGPU_PROBE_GPOW15 = 2, POMGPU_PROBE_RAD_Q = 3 };
int pomgpu_math_probe(pomgpu_ctx *ctx, int op, long n, const double *const *in, int nin, double *out);
int pomgpu_profq(pomgpu_ctx *ctx);               /* solver.f:1212-1538 */
int pomgpu_proft(pomgpu_ctx *ctx, const double *f, const double *wfsurf, const double *fsurf, int nbc); /* :1541-1683 */
int pomgpu_profu(pomgpu_ctx *ctx);               /* solver.f:1686-1780 */
int pomgpu_profv(pomgpu_ctx *ctx);               /* solver.f:1783-1877 */
int pomgpu_vertvl(pomgpu_ctx *ctx);              /* solver.f:1970-2021 */
int pomgpu_realvertvl(pomgpu_ctx *ctx);          /* solver.f:2024-2067 */
int pomgpu_bcond(pomgpu_ctx *ctx, int idx);      /* bounds_forcing.f:6-328   (idx 1,2,4,5,6) */
int pomgpu_bcondorl(pomgpu_ctx *ctx, int idx);   /* bounds_forcing.f:331-590 (idx 3,5) */
int pomgpu_restore_interior(pomgpu_ctx *ctx);    /* bounds_forcing.f:1023-1121 */

/* ---- measurement ------------------------------------------------------------------------ */
/* Per-kernel device time measured with HIP events on the library's stream.  Between
 * pomgpu_prof_begin and pomgpu_prof_end every launch is bracketed by events; pomgpu_prof_get
 * returns, for kernel number `k` (0 <= k < pomgpu_prof_count()), its name, launch count and
 * total milliseconds. */
int pomgpu_prof_begin(pomgpu_ctx *ctx);
/* Two phases are always bracketed as well, whatever the filter: "phase_step" (one pomgpu_advance, on the kernels' stream) and
 * "phase_external" (its isplit mode_external substeps); internal mode = the difference.
 * restrict the bracketing to one kernel (its name, e.g. "k_profq"); NULL or "" = every kernel */
int pomgpu_prof_filter(pomgpu_ctx *ctx, const char *kernel_name);
int pomgpu_prof_end(pomgpu_ctx *ctx);
int pomgpu_prof_count(pomgpu_ctx *ctx);
int pomgpu_prof_get(pomgpu_ctx *ctx, int k, const char **name, long *launches, double *total_ms);

/* developer switches are read from the environment ONCE, at pomgpu_create; this changes one of a live
 * context afterwards (name with or without "POMGPU_", value NULL = unset).  Tools and tests only. */
int pomgpu_debug_switch(pomgpu_ctx *ctx, const char *name, const char *value);
const char *pomgpu_version(void);
/* a digest of the sources this library was built from (measurement bookkeeping: profiles/traffic.json names the build its
 * counters were taken from) */
const char *pomgpu_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* POMGPU_H */
