! pomgpu_iface.f90 -- ISO_C_BINDING view of the C ABI (include/pomgpu.h).
! One interface per entry point; array arguments are passed as the address of the COMMON array
! (c_loc), exactly what the reference's by-reference calls hand to its own kernels.
module pomgpu_iface
  use iso_c_binding
  implicit none
  type, bind(C) :: pomgpu_dims
    integer(c_int) :: im, jm, kb, im_local, jm_local, n_west, n_east, n_south, n_north
  end type
  type(c_ptr), save :: pom_ctx = c_null_ptr
  ! which forcing files the library reads itself (set by pomgpu_open_forcing_files' caller; pom_gpu_main's advance_hot looks at them)
  logical, save :: pom_frc_sfrc = .false., pom_frc_lbry = .false., pom_frc_clim = .false.
  ! the water files <wrk_pth>in/<netcdf_file>.water.NNNN.nc are registered (pomgpu_open_forcing_files found .water.0000.nc): `water` runs
  logical, save :: pom_frc_water = .false.
  ! the init / clim file holds z levels (pomgpu_set_z_inputs): cold_start_files and pomgpu_open_forcing_files pass the two on
  logical, save :: pom_init_on_z = .false., pom_clim_on_z = .false.
  ! temp, salt of the lbry file are on z levels (pomgpu_set_z_lateral): pomgpu_open_forcing_files passes it on
  logical, save :: pom_lbry_on_z = .false.
  ! the open boundaries the lbry file feeds (pomgpu_set_lateral_sides: east 1, south 2, west 4, north 8; the default is the reference's
  ! reader, io_pnetcdf.F:3393-3621): pomgpu_open_forcing_files passes it on
  integer, save :: pom_lbry_sides = 3
  ! the time-mean output is on (pom_output_mean): `advance` accumulates behind mode_internal, write_output_pnetcdf writes the mean file
  logical, save :: pom_mean_on = .false.
  ! the harmonic analysis samples every pom_harm_every-th internal step (pom_harmonics; 0: off): harmonic_step asks it
  integer, save :: pom_harm_every = 0
  type, bind(C) :: pomgpu_file_meta               ! include/pomgpu.h
    type(c_ptr) :: title, time_start
    integer(c_int) :: im_global, jm_global, i0, j0, create
    type(c_ptr) :: stats
  end type
  type, bind(C) :: pomgpu_cold_info               ! include/pomgpu.h
    real(c_double) :: cflmin, period
  end type
  real(c_double), save :: pom_cflmin = 0.d0       ! this rank's cflmin of the last cold_start_files (check_cflmin_mpi reduces it over the ranks)
  interface
    integer(c_int) function pomgpu_create(ctx, dims, device, stream) bind(C, name='pomgpu_create')
      import; type(c_ptr) :: ctx; type(pomgpu_dims) :: dims; integer(c_int), value :: device; type(c_ptr), value :: stream
    end function
    subroutine pomgpu_destroy(ctx) bind(C, name='pomgpu_destroy')
      import; type(c_ptr), value :: ctx
    end subroutine
    integer(c_int) function pomgpu_upload(ctx, b1, b2, b3, bd, con, lramp) bind(C, name='pomgpu_upload')
      import; type(c_ptr), value :: ctx, b1, b2, b3, bd, con; integer(c_int), value :: lramp
    end function
    integer(c_int) function pomgpu_download(ctx, b1, b2, b3, bd, con) bind(C, name='pomgpu_download')
      import; type(c_ptr), value :: ctx, b1, b2, b3, bd, con
    end function
    integer(c_int) function pomgpu_set_con(ctx, con, lramp) bind(C, name='pomgpu_set_con')
      import; type(c_ptr), value :: ctx, con; integer(c_int), value :: lramp
    end function
    integer(c_int) function pomgpu_get_con(ctx, con) bind(C, name='pomgpu_get_con')
      import; type(c_ptr), value :: ctx, con
    end function
    integer(c_int) function pomgpu_bind_host(ctx, h2, h3) bind(C, name='pomgpu_bind_host')
      import; type(c_ptr), value :: ctx, h2, h3
    end function
    integer(c_int) function pomgpu_set_restore_record(ctx, n, tr, sr) bind(C, name='pomgpu_set_restore_record')
      import; type(c_ptr), value :: ctx, tr, sr; integer(c_int), value :: n
    end function
    ! the library's own exchange over RCCL (include/pomgpu.h "transport") and the wide-halo external mode
    integer(c_int) function pomgpu_rccl_unique_id(id128, librccl_path) bind(C, name='pomgpu_rccl_unique_id')
      import; character(kind=c_char) :: id128(128); type(c_ptr), value :: librccl_path
    end function
    integer(c_int) function pomgpu_rccl_init(ctx, id128, rank, nranks, neighbours8, librccl_path) bind(C, name='pomgpu_rccl_init')
      import; type(c_ptr), value :: ctx, librccl_path; character(kind=c_char) :: id128(128)
      integer(c_int), value :: rank, nranks; integer(c_int) :: neighbours8(8)
    end function
    integer(c_int) function pomgpu_set_wide_external(ctx, on, min_im, min_jm) bind(C, name='pomgpu_set_wide_external')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: on, min_im, min_jm
    end function
    ! hosts without RCCL between the ranks: the MPI mover of libpomgpu_mpi.so (extpom_amd/csrc/mpi_mover.c); fcomm = pom_comm
    integer(c_int) function pomgpu_mpi_mover_install(ctx, fcomm, neighbours8) bind(C, name='pomgpu_mpi_mover_install')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: fcomm; integer(c_int) :: neighbours8(8)
    end function
    integer(c_int) function pomgpu_mpi_mover_remove(ctx) bind(C, name='pomgpu_mpi_mover_remove')   ! before pomgpu_host_finalize: frees the pinned staging buffers
      import; type(c_ptr), value :: ctx
    end function
    integer(c_long) function pomgpu_exchange_rounds_side(ctx) bind(C, name='pomgpu_exchange_rounds_side')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_long) function pomgpu_exchange_rounds(ctx) bind(C, name='pomgpu_exchange_rounds')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function pomgpu_tune_placement(ctx, steps, max_try, ms_out, front_mib_out, pad_mib_out, ntried, kept) bind(C, name='pomgpu_tune_placement')
      import; type(c_ptr), value :: ctx, ms_out, front_mib_out, pad_mib_out, ntried, kept; integer(c_int), value :: steps, max_try   ! the five outputs may be c_null_ptr
    end function
    integer(c_int) function pomgpu_sync(ctx) bind(C, name='pomgpu_sync')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function pomgpu_check_velocity(ctx, vamax, imax, jmax) bind(C, name='pomgpu_check_velocity')
      import; type(c_ptr), value :: ctx; real(c_double) :: vamax; integer(c_int) :: imax, jmax
    end function
    integer(c_int) function pomgpu_set_forcing_record(ctx, kind, n, a, b) bind(C, name='pomgpu_set_forcing_record')
      import; type(c_ptr), value :: ctx, a, b; integer(c_int), value :: kind, n
    end function
    integer(c_int) function pomgpu_set_lateral_record(ctx, n, arrays) bind(C, name='pomgpu_set_lateral_record')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: n; type(c_ptr) :: arrays(20)
    end function
    integer(c_int) function pomgpu_set_forcing_files(ctx, sfrc, lbry, clim, meta) bind(C, name='pomgpu_set_forcing_files')
      import; type(c_ptr), value :: ctx, sfrc, lbry, clim; type(pomgpu_file_meta) :: meta   ! any path may be c_null_ptr
    end function
    integer(c_int) function pomgpu_set_water_record(ctx, n, w) bind(C, name='pomgpu_set_water_record')
      import; type(c_ptr), value :: ctx, w; integer(c_int), value :: n   ! n >= 0
    end function
    integer(c_int) function pomgpu_set_water_files(ctx, prefix, meta) bind(C, name='pomgpu_set_water_files')
      import; type(c_ptr), value :: ctx, prefix; type(pomgpu_file_meta) :: meta   ! <prefix>.water.NNNN.nc
    end function
    integer(c_int) function pomgpu_set_water(ctx, on) bind(C, name='pomgpu_set_water')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: on
    end function
    integer(c_int) function pomgpu_set_surface_sss(ctx, on) bind(C, name='pomgpu_set_surface_sss')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: on
    end function
    integer(c_int) function pomgpu_set_restore_rate_record(ctx, n, tau) bind(C, name='pomgpu_set_restore_rate_record')
      import; type(c_ptr), value :: ctx, tau; integer(c_int), value :: n
    end function
    integer(c_int) function pomgpu_set_restore_rate_file(ctx, path, meta) bind(C, name='pomgpu_set_restore_rate_file')
      import; type(c_ptr), value :: ctx, path; type(pomgpu_file_meta) :: meta
    end function
    integer(c_int) function pomgpu_io_wait(ctx) bind(C, name='pomgpu_io_wait')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function pomgpu_write_output(ctx, path, meta) bind(C, name='pomgpu_write_output')
      import; type(c_ptr), value :: ctx, path; type(pomgpu_file_meta) :: meta
    end function
    integer(c_int) function pomgpu_write_output_mean(ctx, path, meta) bind(C, name='pomgpu_write_output_mean')
      import; type(c_ptr), value :: ctx, path; type(pomgpu_file_meta) :: meta
    end function
    integer(c_int) function pomgpu_set_mean_output(ctx, on) bind(C, name='pomgpu_set_mean_output')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: on
    end function
    integer(c_int) function pomgpu_mean_count(ctx) bind(C, name='pomgpu_mean_count')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function pomgpu_mean_download(ctx, is3d, slot, host) bind(C, name='pomgpu_mean_download')
      import; type(c_ptr), value :: ctx, host; integer(c_int), value :: is3d, slot
    end function
    ! passive tracers (include/pomgpu.h): which = enum pomgpu_tracer_array, 0 trb 1 tr 2 clim 3 source 4 wsurf 5 surf 6 be 7 bw 8 bn 9 bs
    integer(c_int) function pomgpu_set_tracers(ctx, n) bind(C, name='pomgpu_set_tracers')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: n
    end function
    integer(c_int) function pomgpu_tracer_count(ctx) bind(C, name='pomgpu_tracer_count')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function pomgpu_tracer_upload(ctx, n, which, host) bind(C, name='pomgpu_tracer_upload')
      import; type(c_ptr), value :: ctx, host; integer(c_int), value :: n, which
    end function
    integer(c_int) function pomgpu_tracer_download(ctx, n, which, host) bind(C, name='pomgpu_tracer_download')
      import; type(c_ptr), value :: ctx, host; integer(c_int), value :: n, which
    end function
    integer(c_int) function pomgpu_tracer_set(ctx, n, nbc, lam) bind(C, name='pomgpu_tracer_set')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: n, nbc; real(c_double), value :: lam
    end function
    ! the tracers' files, means and inventory (include/pomgpu.h): kind 0 restart, 1 output, 2 output mean; trstats: 4 x ntr rank-reduced
    ! values (tot avg min max per tracer) or c_null_ptr; time_out / iint_out may be c_null_ptr
    integer(c_int) function pomgpu_write_tracers(ctx, path, meta, kind, trstats) bind(C, name='pomgpu_write_tracers')
      import; type(c_ptr), value :: ctx, path, trstats; type(pomgpu_file_meta) :: meta; integer(c_int), value :: kind
    end function
    integer(c_int) function pomgpu_read_tracers(ctx, path, meta, time_out, iint_out) bind(C, name='pomgpu_read_tracers')
      import; type(c_ptr), value :: ctx, path, time_out, iint_out; type(pomgpu_file_meta) :: meta
    end function
    integer(c_int) function pomgpu_tracer_stats(ctx, out) bind(C, name='pomgpu_tracer_stats')
      import; type(c_ptr), value :: ctx, out   ! out(4, ntr)
    end function
    integer(c_int) function pomgpu_tracer_get(ctx, n, nbc, lam) bind(C, name='pomgpu_tracer_get')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: n; integer(c_int) :: nbc; real(c_double) :: lam
    end function
    integer(c_int) function pomgpu_tracer_mean_count(ctx) bind(C, name='pomgpu_tracer_mean_count')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function pomgpu_tracer_mean_download(ctx, n, host) bind(C, name='pomgpu_tracer_mean_download')
      import; type(c_ptr), value :: ctx, host; integer(c_int), value :: n
    end function
    ! Lagrangian floats (include/pomgpu.h): x y sig doubles, status kind id integers, n of each; kind / id may be c_null_ptr on upload, any
    ! pointer on download; the float file is output and checkpoint in one
    integer(c_int) function pomgpu_float_upload(ctx, n, x, y, sig, kind, id) bind(C, name='pomgpu_float_upload')
      import; type(c_ptr), value :: ctx, x, y, sig, kind, id; integer(c_int), value :: n
    end function
    integer(c_int) function pomgpu_float_count(ctx) bind(C, name='pomgpu_float_count')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function pomgpu_float_download(ctx, x, y, sig, status, kind, id) bind(C, name='pomgpu_float_download')
      import; type(c_ptr), value :: ctx, x, y, sig, status, kind, id
    end function
    integer(c_int) function pomgpu_float_sample(ctx, out) bind(C, name='pomgpu_float_sample')
      import; type(c_ptr), value :: ctx, out   ! out(n, 5): lon lat depth t s
    end function
    integer(c_int) function pomgpu_write_floats(ctx, path, meta) bind(C, name='pomgpu_write_floats')
      import; type(c_ptr), value :: ctx, path; type(pomgpu_file_meta) :: meta
    end function
    integer(c_int) function pomgpu_read_floats(ctx, path, meta, time_out, iint_out) bind(C, name='pomgpu_read_floats')
      import; type(c_ptr), value :: ctx, path, time_out, iint_out; type(pomgpu_file_meta) :: meta
    end function
    ! tides (include/pomgpu.h): lines = 16 pointers, 4 * side + q, side 0 east 1 south 2 west 3 north, q = elC elS unC unS, each (n_global, nc)
    integer(c_int) function pomgpu_set_tides(ctx, nc, omega, sides, lines, meta) bind(C, name='pomgpu_set_tides')
      import; type(c_ptr), value :: ctx, omega, lines; integer(c_int), value :: nc, sides; type(pomgpu_file_meta) :: meta
    end function
    integer(c_int) function pomgpu_set_tide_file(ctx, path, meta) bind(C, name='pomgpu_set_tide_file')
      import; type(c_ptr), value :: ctx, path; type(pomgpu_file_meta) :: meta
    end function
    integer(c_int) function pomgpu_tide_count(ctx) bind(C, name='pomgpu_tide_count')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function pomgpu_set_harmonic_analysis(ctx, on, every) bind(C, name='pomgpu_set_harmonic_analysis')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: on, every
    end function
    integer(c_int) function pomgpu_harmonic_accumulate(ctx) bind(C, name='pomgpu_harmonic_accumulate')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function pomgpu_harmonic_count(ctx) bind(C, name='pomgpu_harmonic_count')
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function pomgpu_write_harmonics(ctx, path, meta) bind(C, name='pomgpu_write_harmonics')
      import; type(c_ptr), value :: ctx, path; type(pomgpu_file_meta) :: meta
    end function
    integer(c_int) function pomgpu_write_restart(ctx, path, meta) bind(C, name='pomgpu_write_restart')
      import; type(c_ptr), value :: ctx, path; type(pomgpu_file_meta) :: meta
    end function
    type(c_ptr) function pomgpu_last_error(ctx) bind(C, name='pomgpu_last_error')   ! a NUL-terminated text of at most 511 characters
      import; type(c_ptr), value :: ctx
    end function
    integer(c_int) function pomgpu_read_restart(ctx, path, meta, time0_out, iint_out) bind(C, name='pomgpu_read_restart')
      import; type(c_ptr), value :: ctx, path, time0_out, iint_out; type(pomgpu_file_meta) :: meta   ! the two outputs may be c_null_ptr
    end function
    integer(c_int) function pomgpu_cold_start(ctx, grid, init, clim, meta, info) bind(C, name='pomgpu_cold_start')
      import; type(c_ptr), value :: ctx, grid, init, clim, info; type(pomgpu_file_meta) :: meta   ! info may be c_null_ptr
    end function
    integer(c_int) function pomgpu_set_z_inputs(ctx, init_on_z, clim_on_z) bind(C, name='pomgpu_set_z_inputs')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: init_on_z, clim_on_z
    end function
    integer(c_int) function pomgpu_set_z_lateral(ctx, lbry_on_z) bind(C, name='pomgpu_set_z_lateral')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: lbry_on_z
    end function
    integer(c_int) function pomgpu_set_lateral_sides(ctx, sides) bind(C, name='pomgpu_set_lateral_sides')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: sides
    end function
    integer(c_int) function pomgpu_domain_stats(ctx, out, sums_only) bind(C, name='pomgpu_domain_stats')
      import; type(c_ptr), value :: ctx; real(c_double) :: out(8); integer(c_int), value :: sums_only
    end function
    integer(c_int) function pomgpu_advq(ctx, qb, q, qf) bind(C, name='pomgpu_advq')
      import; type(c_ptr), value :: ctx, qb, q, qf
    end function
    integer(c_int) function pomgpu_advt1(ctx, fb, f, fclim, ff) bind(C, name='pomgpu_advt1')
      import; type(c_ptr), value :: ctx, fb, f, fclim, ff
    end function
    integer(c_int) function pomgpu_advt2(ctx, fb, f, fclim, ff) bind(C, name='pomgpu_advt2')
      import; type(c_ptr), value :: ctx, fb, f, fclim, ff
    end function
    integer(c_int) function pomgpu_dens(ctx, si, ti, rhoo) bind(C, name='pomgpu_dens')
      import; type(c_ptr), value :: ctx, si, ti, rhoo
    end function
    integer(c_int) function pomgpu_proft(ctx, f, wfsurf, fsurf, nbc) bind(C, name='pomgpu_proft')
      import; type(c_ptr), value :: ctx, f, wfsurf, fsurf; integer(c_int), value :: nbc
    end function
    integer(c_int) function pomgpu_ztosig(ctx, zs, ks, src, t) bind(C, name='pomgpu_ztosig')
      import; type(c_ptr), value :: ctx, zs, src, t; integer(c_int), value :: ks   ! zs(ks), src(im_local,jm_local,ks): the caller's own arrays; t: a COMMON array
    end function
    integer(c_int) function pomgpu_ztosig_line(ctx, edge, zs, ks, src, out) bind(C, name='pomgpu_ztosig_line')
      import; type(c_ptr), value :: ctx, zs, src, out; integer(c_int), value :: edge, ks   ! zs(ks), src(0:n_local+1,ks), out(n_local,kb): the caller's own arrays
    end function
    integer(c_int) function pomgpu_bcond(ctx, idx) bind(C, name='pomgpu_bcond')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: idx
    end function
    integer(c_int) function pomgpu_bcondorl(ctx, idx) bind(C, name='pomgpu_bcondorl')
      import; type(c_ptr), value :: ctx; integer(c_int), value :: idx
    end function
  end interface
  ! the argument-less entry points share one abstract shape
  abstract interface
    integer(c_int) function pomgpu_noarg(ctx) bind(C)
      import; type(c_ptr), value :: ctx
    end function
  end interface
  procedure(pomgpu_noarg), bind(C, name='pomgpu_lateral_viscosity') :: pomgpu_lateral_viscosity
  procedure(pomgpu_noarg), bind(C, name='pomgpu_mode_interaction') :: pomgpu_mode_interaction
  procedure(pomgpu_noarg), bind(C, name='pomgpu_mode_external') :: pomgpu_mode_external
  procedure(pomgpu_noarg), bind(C, name='pomgpu_mode_internal') :: pomgpu_mode_internal
  procedure(pomgpu_noarg), bind(C, name='pomgpu_mean_accumulate') :: pomgpu_mean_accumulate
  procedure(pomgpu_noarg), bind(C, name='pomgpu_float_step') :: pomgpu_float_step
  procedure(pomgpu_noarg), bind(C, name='pomgpu_advave') :: pomgpu_advave
  procedure(pomgpu_noarg), bind(C, name='pomgpu_advct') :: pomgpu_advct
  procedure(pomgpu_noarg), bind(C, name='pomgpu_advu') :: pomgpu_advu
  procedure(pomgpu_noarg), bind(C, name='pomgpu_advv') :: pomgpu_advv
  procedure(pomgpu_noarg), bind(C, name='pomgpu_baropg') :: pomgpu_baropg
  procedure(pomgpu_noarg), bind(C, name='pomgpu_baropg_mcc') :: pomgpu_baropg_mcc
  procedure(pomgpu_noarg), bind(C, name='pomgpu_wind') :: pomgpu_wind
  procedure(pomgpu_noarg), bind(C, name='pomgpu_heat') :: pomgpu_heat
  procedure(pomgpu_noarg), bind(C, name='pomgpu_water') :: pomgpu_water
  procedure(pomgpu_noarg), bind(C, name='pomgpu_surface') :: pomgpu_surface
  procedure(pomgpu_noarg), bind(C, name='pomgpu_lateral_bc') :: pomgpu_lateral_bc
  procedure(pomgpu_noarg), bind(C, name='pomgpu_profq') :: pomgpu_profq
  procedure(pomgpu_noarg), bind(C, name='pomgpu_profu') :: pomgpu_profu
  procedure(pomgpu_noarg), bind(C, name='pomgpu_profv') :: pomgpu_profv
  procedure(pomgpu_noarg), bind(C, name='pomgpu_vertvl') :: pomgpu_vertvl
  procedure(pomgpu_noarg), bind(C, name='pomgpu_realvertvl') :: pomgpu_realvertvl
  procedure(pomgpu_noarg), bind(C, name='pomgpu_restore_interior') :: pomgpu_restore_interior
end module pomgpu_iface
