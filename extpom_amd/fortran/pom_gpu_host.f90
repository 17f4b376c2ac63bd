! pom_gpu_host.f90 -- the hot-path subroutines of the reference under THEIR OWN NAMES, as thin
! Fortran wrappers over the C ABI.  Linking this file (plus pomgpu_iface.f90 and libpomgpu.so)
! instead of the reference's solver.f / advance.f hot routines makes `advance` run on the GPU;
! the reference's driver, initialisation, forcing and I/O keep calling the same names
! (reference pom/advance.f:6-59, pom/solver.f).
!
! State lives in HBM between calls.  pomgpu_upload_state / pomgpu_download_state move whole
! COMMON blocks (after initialisation / forcing updates, before print_section / output / restart:
! SURVEY 8b).  Scalars of blkcon that the host changes every step (iint, iext, time, ramp) are
! pushed before each call; error_status is pulled back after check_velocity, which is where the
! reference tests it (advance.f:631-637).

subroutine pomgpu_host_init(device)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer device
  type(pomgpu_dims) :: dm
  dm%im = im; dm%jm = jm; dm%kb = kb; dm%im_local = im_local; dm%jm_local = jm_local
  dm%n_west = n_west; dm%n_east = n_east; dm%n_south = n_south; dm%n_north = n_north
  if (pomgpu_create(pom_ctx, dm, int(device, c_int), c_null_ptr) /= 0) then
    error_status = 1
    write(6,'(/''Error: pomgpu_create failed (no GPU?)'')')
    stop 1
  end if
end subroutine

! Multi-GPU: what initialize_mpi / distribute_mpi set up for MPI (parallel_mpi.f:124-151, :34-122) is handed to the
! library once: the RCCL communicator (id128 = the 128 bytes rank 0 got from pomgpu_rccl_unique_id and the caller
! broadcast with MPI_Bcast over pom_comm) and the eight neighbour ranks.  From then on every exchange point of the hot
! path is served inside the library (pack, one grouped ncclSend/ncclRecv round, unpack, on its stream), and the 2-D
! external mode runs on a wide-halo copy of the tile (one exchange per internal step) when the tiles are wide enough.
! Call it after pomgpu_upload_state: the extended tile is sized by isplit (the library refuses with isplit = 0).
subroutine pomgpu_host_connect(id128)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  character(kind=c_char) :: id128(128)
  integer(c_int) :: nb(8), rc
  integer :: nranks, min_im, min_jm
  call pomgpu_host_neighbours(nb, nranks, min_im, min_jm)
  rc = pomgpu_rccl_init(pom_ctx, id128, int(my_task, c_int), int(nranks, c_int), nb, c_null_ptr)
  if (rc /= 0) then
    error_status = 1
    write(6,'(/''Error: pomgpu_rccl_init failed'')')
    return
  end if
  rc = pomgpu_set_wide_external(pom_ctx, 1_c_int, int(min_im, c_int), int(min_jm, c_int))   ! EINVAL = tiles too narrow: per-point exchanges stay
end subroutine

! The eight neighbour ranks of this tile in the C ABI's order W E S N SW SE NW NE, the number of tiles, and the extents of
! the smallest tile -- from what distribute_mpi left in blkpar / blksiz (parallel_mpi.f:54-119): the tiles are numbered row
! by row, nproc_x of them per row, the east- / north-most ones are the trimmed ones (:83-87, :98-102).
subroutine pomgpu_host_neighbours(nb, nranks, min_im, min_jm)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer(c_int), intent(out) :: nb(8)
  integer, intent(out) :: nranks, min_im, min_jm
  integer :: px, py, npx, npy
  npx = (im_global - 2 + im_local - 3) / (im_local - 2)        ! tiles in x, y (parallel_mpi.f:54-65)
  npy = (jm_global - 2 + jm_local - 3) / (jm_local - 2)
  px = mod(my_task, npx); py = my_task / npx
  nb(1) = n_west; nb(2) = n_east; nb(3) = n_south; nb(4) = n_north
  nb(5) = -1; nb(6) = -1; nb(7) = -1; nb(8) = -1                ! SW SE NW NE: the tiles across the corners
  if (px > 0 .and. py > 0) nb(5) = my_task - 1 - npx
  if (px < npx - 1 .and. py > 0) nb(6) = my_task + 1 - npx
  if (px > 0 .and. py < npy - 1) nb(7) = my_task - 1 + npx
  if (px < npx - 1 .and. py < npy - 1) nb(8) = my_task + 1 + npx
  nranks = npx * npy
  min_im = min(im_local, im_global - (npx - 1) * (im_local - 2))
  min_jm = min(jm_local, jm_global - (npy - 1) * (jm_local - 2))
end subroutine

! End of the run (the reference: finalize_mpi, pom.f:36): the output / restart file still being written behind the model's
! back is joined -- its status is the run's -- and the device state is released.
subroutine pomgpu_host_finalize
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_io_wait(pom_ctx) /= 0) then
    error_status = 1
    write(6,'(/''Error: an output / restart file could not be written'')')
  end if
  call pomgpu_destroy(pom_ctx)
  pom_ctx = c_null_ptr
end subroutine

subroutine pomgpu_upload_state
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer(c_int) :: lr, rc
  lr = 0
  if (lramp) lr = 1
  rc = pomgpu_upload(pom_ctx, c_loc(dz), c_loc(aam2d), c_loc(aam), c_loc(ele), c_loc(alpha), lr)
  rc = pomgpu_bind_host(pom_ctx, c_loc(aam2d), c_loc(aam))
  if (rc /= 0) error_status = 1
end subroutine

subroutine pomgpu_download_state
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer(c_int) :: rc
  rc = pomgpu_download(pom_ctx, c_loc(dz), c_loc(aam2d), c_loc(aam), c_loc(ele), c_loc(alpha))
  if (rc /= 0) error_status = 1
end subroutine

subroutine pomgpu_push_con
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer(c_int) :: lr, rc
  lr = 0
  if (lramp) lr = 1
  rc = pomgpu_set_con(pom_ctx, c_loc(alpha), lr)
end subroutine

! ---- orchestration (advance.f) ------------------------------------------------------------
subroutine lateral_viscosity
  use pomgpu_iface
  implicit none
  include 'pom.h'
  call pomgpu_push_con
  if (pomgpu_lateral_viscosity(pom_ctx) /= 0) error_status = 1
end subroutine

subroutine mode_interaction
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_mode_interaction(pom_ctx) /= 0) error_status = 1
end subroutine

subroutine mode_external
  use pomgpu_iface
  implicit none
  include 'pom.h'
  call pomgpu_push_con            ! iext is the host's DO variable (advance.f:27)
  if (pomgpu_mode_external(pom_ctx) /= 0) error_status = 1
end subroutine

subroutine mode_internal
  use pomgpu_iface
  implicit none
  include 'pom.h'
  call pomgpu_push_con
  if (pomgpu_mode_internal(pom_ctx) /= 0) error_status = 1
end subroutine

! The time-mean output (no counterpart in the reference): pom_output_mean(.true.) after pomgpu_upload_state -- and after
! pomgpu_tune_placement, which refuses while the mean is on -- makes the library accumulate uab vab elb u v t s rho w every internal step,
! and write_output_pnetcdf (pom_gpu_io.f90) write their means since the last output file in place of the snapshot.  Calling it again
! zeroes the sums; .false. frees them.  mean_accumulate is the step's accumulation: `advance` calls it behind mode_internal, where
! advance.f:38 writes (nothing while the mean is off).
subroutine pom_output_mean(on)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  logical, intent(in) :: on
  if (pomgpu_set_mean_output(pom_ctx, merge(1_c_int, 0_c_int, on)) /= 0) then
    error_status = 1
    pom_mean_on = .false.
  else
    pom_mean_on = on
  end if
end subroutine

! bounds_forcing.f:979 "ssurf(1:im,1:jm) = sss" uncommented: pom_surface_sss(.true.) makes `surface` set ssurf from the record's SSS
! (pomgpu_set_surface_sss), what proft's salt solve reads at nbcs = 3
subroutine pom_surface_sss(on)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  logical, intent(in) :: on
  if (pomgpu_set_surface_sss(pom_ctx, merge(1_c_int, 0_c_int, on)) /= 0) error_status = 1
end subroutine

! Passive tracers (no counterpart in the reference; include/pomgpu.h): pom_tracers(n) after pomgpu_upload_state -- and after
! pomgpu_tune_placement, which refuses while tracers are registered -- gives the context n tracers, all zero; mode_internal then carries
! them with the flow.  pom_tracer_put / pom_tracer_get move one array of tracer n (which: 0 trb 1 tr 2 clim 3 source 4 wsurf 5 surf
! 6 be 7 bw 8 bn 9 bs, shaped like tb, wtsurf, tbe, tbn); pom_tracer_set: nbc 1 (the flux) or 3 (the surface value), the decay rate in 1/s.
! Tracers are not in the reference's output or restart files: they have files of their own, write_tracers_pnetcdf and
! read_tracers_pnetcdf (pom_gpu_io.f90).  pom_tracer_stats: the inventory, out(1:4, n) = tot avg min max of tracer n on THIS rank's tile.
subroutine pom_tracers(n)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer, intent(in) :: n
  if (pomgpu_set_tracers(pom_ctx, int(n, c_int)) /= 0) error_status = 1
end subroutine

subroutine pom_tracer_put(n, which, a)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer, intent(in) :: n, which
  double precision, intent(in), target :: a(*)
  if (pomgpu_tracer_upload(pom_ctx, int(n, c_int), int(which, c_int), c_loc(a)) /= 0) error_status = 1
end subroutine

subroutine pom_tracer_get(n, which, a)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer, intent(in) :: n, which
  double precision, intent(out), target :: a(*)
  if (pomgpu_tracer_download(pom_ctx, int(n, c_int), int(which, c_int), c_loc(a)) /= 0) error_status = 1
end subroutine

subroutine pom_tracer_set(n, nbc, lam)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer, intent(in) :: n, nbc
  double precision, intent(in) :: lam
  if (pomgpu_tracer_set(pom_ctx, int(n, c_int), int(nbc, c_int), real(lam, c_double)) /= 0) error_status = 1
end subroutine

subroutine pom_tracer_stats(out)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  double precision, intent(out), target :: out(4, *)
  if (pomgpu_tracer_stats(pom_ctx, c_loc(out)) /= 0) error_status = 1
end subroutine

subroutine mean_accumulate
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (.not. pom_mean_on) return
  if (pomgpu_mean_accumulate(pom_ctx) /= 0) error_status = 1
end subroutine

! Lagrangian floats (no counterpart in the reference; include/pomgpu.h): pom_floats_put after pomgpu_upload_state -- and after
! pomgpu_tune_placement, which refuses while floats are registered -- registers n floats at the index coordinates x, y (the centre of cell
! (i, j) is x = i, y = j) and sigma sig, kind 0 following w and 1 keeping its sigma, id the caller's number; n = 0 frees them.
! pom_floats_get brings the six arrays back (status: 0 active, 1 exited, 2 lost).  float_step is the floats' stage for a host that strings
! the routines together: call it after mode_internal and mean_accumulate; nothing happens without floats, nor in a step whose
! mode_internal skipped its 3-D part (advance.f:362: the first step of a run from rest, mode 2).  Floats have a file of their own,
! write_floats_pnetcdf and read_floats_pnetcdf (pom_gpu_io.f90).  One tile only: a context with neighbours refuses them.
subroutine pom_floats_put(n, x, y, sig, kind, id)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer, intent(in) :: n
  double precision, intent(in), target :: x(*), y(*), sig(*)
  integer(c_int), intent(in), target :: kind(*), id(*)
  if (pomgpu_float_upload(pom_ctx, int(n, c_int), c_loc(x), c_loc(y), c_loc(sig), c_loc(kind), c_loc(id)) /= 0) error_status = 1
end subroutine

subroutine pom_floats_get(x, y, sig, status, kind, id)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  double precision, intent(out), target :: x(*), y(*), sig(*)
  integer(c_int), intent(out), target :: status(*), kind(*), id(*)
  if (pomgpu_float_download(pom_ctx, c_loc(x), c_loc(y), c_loc(sig), c_loc(status), c_loc(kind), c_loc(id)) /= 0) error_status = 1
end subroutine

subroutine float_step
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_float_count(pom_ctx) <= 0) return
  if ((iint == 1 .and. time0 == 0.d0) .or. mode == 2) return
  if (pomgpu_float_step(pom_ctx) /= 0) error_status = 1
end subroutine

! Tides (no counterpart in the reference; include/pomgpu.h "tides"): pom_tides_put after pomgpu_upload_state -- and after
! pomgpu_tune_placement, which refuses while a table is registered -- registers nc constituents, omega in rad/s, on the open sides named by
! the bits of sides (1 east, 2 south, 4 west, 8 north).  el_amp, el_pha, un_amp, un_pha are (nline, nc, 4), the last index east south west
! north, nline >= max(im_global, jm_global): the GLOBAL lines, the same on every rank, amplitude in metres (un: the depth-mean NORMAL velocity
! in m/s in the model's +i / +j sense) and Greenwich-style phase g in degrees, A cos(omega t - g).  with_un = .false.: un is zero.  nc = 0
! clears the table.  The conversion C = A cos g, S = A sin g is made here on the host.  pom_harmonics(on, every) switches the harmonic
! analysis of elb uab vab on; harmonic_step is its stage for a host that strings the routines together: call it after mode_internal,
! mean_accumulate and float_step.  The files: read_tides_pnetcdf and write_harmonics_pnetcdf (pom_gpu_io.f90).
subroutine pom_tides_put(nc, omega, sides, nline, el_amp, el_pha, un_amp, un_pha, with_un)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer, intent(in) :: nc, sides, nline
  double precision, intent(in), target :: omega(*)
  double precision, intent(in) :: el_amp(nline, max(nc, 1), 4), el_pha(nline, max(nc, 1), 4), un_amp(nline, max(nc, 1), 4), un_pha(nline, max(nc, 1), 4)
  logical, intent(in) :: with_un
  double precision, allocatable, target :: pk(:)   ! the 16 lines the C interface takes, (n_global, nc) contiguous each, one behind the other
  type(c_ptr), target :: lines(16)
  type(pomgpu_file_meta) :: m
  double precision :: gel, gun
  integer :: ks, kc, ka, kn, ko
  m%title = c_null_ptr; m%time_start = c_null_ptr; m%stats = c_null_ptr; m%create = 0
  m%im_global = im_global; m%jm_global = jm_global
  m%i0 = i_global(1); m%j0 = j_global(1)
  if (nc <= 0) then
    if (pomgpu_set_tides(pom_ctx, 0_c_int, c_null_ptr, 0_c_int, c_null_ptr, m) /= 0) error_status = 1
    pom_harm_every = 0                       ! the analysis goes with its table
    return
  end if
  allocate(pk(16*max(im_global, jm_global)*nc))
  pk = 0.d0
  lines = c_null_ptr
  ko = 0
  do ks = 1, 4
    if (iand(sides, ishft(1, ks-1)) == 0) cycle
    kn = jm_global
    if (ks == 2 .or. ks == 4) kn = im_global
    lines(4*(ks-1)+1) = c_loc(pk(ko+1))
    lines(4*(ks-1)+2) = c_loc(pk(ko+kn*nc+1))
    lines(4*(ks-1)+3) = c_loc(pk(ko+2*kn*nc+1))
    lines(4*(ks-1)+4) = c_loc(pk(ko+3*kn*nc+1))
    do kc = 1, nc
      do ka = 1, kn
        gel = el_pha(ka, kc, ks)*(3.14159265358979323846d0/180.d0)
        pk(ko+(kc-1)*kn+ka) = el_amp(ka, kc, ks)*cos(gel)
        pk(ko+kn*nc+(kc-1)*kn+ka) = el_amp(ka, kc, ks)*sin(gel)
        if (with_un) then
          gun = un_pha(ka, kc, ks)*(3.14159265358979323846d0/180.d0)
          pk(ko+2*kn*nc+(kc-1)*kn+ka) = un_amp(ka, kc, ks)*cos(gun)
          pk(ko+3*kn*nc+(kc-1)*kn+ka) = un_amp(ka, kc, ks)*sin(gun)
        end if
      end do
    end do
    ko = ko + 4*kn*nc
  end do
  if (pomgpu_set_tides(pom_ctx, int(nc, c_int), c_loc(omega), int(sides, c_int), c_loc(lines), m) /= 0) error_status = 1
  deallocate(pk)
end subroutine

subroutine pom_harmonics(on, every)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  logical, intent(in) :: on
  integer, intent(in) :: every
  integer(c_int) :: ion
  ion = 0
  if (on) ion = 1
  if (pomgpu_set_harmonic_analysis(pom_ctx, ion, int(every, c_int)) /= 0) then
    error_status = 1
    pom_harm_every = 0
  else
    pom_harm_every = 0
    if (on) pom_harm_every = every
  end if
end subroutine

subroutine harmonic_step
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pom_harm_every <= 0) return
  if (mod(iint, pom_harm_every) /= 0) return
  if (pomgpu_harmonic_accumulate(pom_ctx) /= 0) error_status = 1
end subroutine

subroutine check_velocity
  use pomgpu_iface
  implicit none
  include 'pom.h'
  real(c_double) :: vamax
  integer(c_int) :: imax, jmax, rc
  rc = pomgpu_check_velocity(pom_ctx, vamax, imax, jmax)
  rc = pomgpu_get_con(pom_ctx, c_loc(alpha))     ! brings error_status back
end subroutine

! domain_stats (advance.f:644-756): the tile's sums come from the device; the reduction over ranks and
! the averages are the reference's own lines (sum0d_mpi / bcast0d_mpi stay the host's, parallel_mpi.f:125-151)
subroutine domain_stats(vtot, atot, mtot, stot, tavg, savg, eavg, ekin)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  double precision, intent(out) :: vtot, atot, mtot, stot, tavg, savg, eavg, ekin
  real(c_double) :: o(8)
  if (pomgpu_domain_stats(pom_ctx, o, 1_c_int) /= 0) error_status = 1
  vtot = o(1); atot = o(2); mtot = o(3); stot = o(4); tavg = o(5); savg = 0.d0; eavg = o(7); ekin = o(8)
  call sum0d_mpi(atot, 0)
  call sum0d_mpi(eavg, 0)
  call sum0d_mpi(vtot, 0)
  call sum0d_mpi(mtot, 0)
  call sum0d_mpi(stot, 0)
  call sum0d_mpi(tavg, 0)
  call sum0d_mpi(ekin, 0)
  if (my_task == 0) then
    if (atot /= 0) then
      eavg = eavg/atot
    else
      eavg = 0.
    end if
    if (vtot /= 0) then
      tavg = tavg/vtot
      savg = stot/vtot
    else
      tavg = 0.
      savg = 0.
    end if
  end if
  call bcast0d_mpi(atot, 0)
  call bcast0d_mpi(vtot, 0)
  call bcast0d_mpi(mtot, 0)
  call bcast0d_mpi(stot, 0)
  call bcast0d_mpi(tavg, 0)
  call bcast0d_mpi(savg, 0)
  call bcast0d_mpi(eavg, 0)
  call bcast0d_mpi(ekin, 0)
end subroutine

! ---- kernels (solver.f), reference signatures -----------------------------------------------
subroutine advave
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_advave(pom_ctx) /= 0) error_status = 1
end subroutine
subroutine advct
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_advct(pom_ctx) /= 0) error_status = 1
end subroutine
subroutine advq(qb, q, qf)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  double precision, target :: qb(im_local,jm_local,kb), q(im_local,jm_local,kb), qf(im_local,jm_local,kb)
  if (pomgpu_advq(pom_ctx, c_loc(qb), c_loc(q), c_loc(qf)) /= 0) error_status = 1
end subroutine
subroutine advt1(fb, f, fclim, ff)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  double precision, target :: fb(im_local,jm_local,kb), f(im_local,jm_local,kb)
  double precision, target :: fclim(im_local,jm_local,kb), ff(im_local,jm_local,kb)
  if (pomgpu_advt1(pom_ctx, c_loc(fb), c_loc(f), c_loc(fclim), c_loc(ff)) /= 0) error_status = 1
end subroutine
subroutine advt2(fb, f, fclim, ff)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  double precision, target :: fb(im_local,jm_local,kb), f(im_local,jm_local,kb)
  double precision, target :: fclim(im_local,jm_local,kb), ff(im_local,jm_local,kb)
  if (pomgpu_advt2(pom_ctx, c_loc(fb), c_loc(f), c_loc(fclim), c_loc(ff)) /= 0) error_status = 1
end subroutine
subroutine advu
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_advu(pom_ctx) /= 0) error_status = 1
end subroutine
subroutine advv
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_advv(pom_ctx) /= 0) error_status = 1
end subroutine
subroutine baropg
  use pomgpu_iface
  implicit none
  include 'pom.h'
  call pomgpu_push_con            ! ramp
  if (pomgpu_baropg(pom_ctx) /= 0) error_status = 1
end subroutine
subroutine baropg_mcc
  use pomgpu_iface
  implicit none
  include 'pom.h'
  call pomgpu_push_con            ! ramp
  if (pomgpu_baropg_mcc(pom_ctx) /= 0) error_status = 1
end subroutine
subroutine dens(si, ti, rhoo)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  double precision, target :: si(im_local,jm_local,kb), ti(im_local,jm_local,kb), rhoo(im_local,jm_local,kb)
  if (pomgpu_dens(pom_ctx, c_loc(si), c_loc(ti), c_loc(rhoo)) /= 0) error_status = 1
end subroutine
subroutine profq
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_profq(pom_ctx) /= 0) error_status = 1
end subroutine
subroutine proft(f, wfsurf, fsurf, nbc)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  double precision, target :: f(im_local,jm_local,kb), wfsurf(im_local,jm_local), fsurf(im_local,jm_local)
  integer nbc
  if (pomgpu_proft(pom_ctx, c_loc(f), c_loc(wfsurf), c_loc(fsurf), int(nbc, c_int)) /= 0) error_status = 1
end subroutine
subroutine profu
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_profu(pom_ctx) /= 0) error_status = 1
end subroutine
subroutine profv
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_profv(pom_ctx) /= 0) error_status = 1
end subroutine
subroutine vertvl
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_vertvl(pom_ctx) /= 0) error_status = 1
end subroutine
subroutine realvertvl
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (pomgpu_realvertvl(pom_ctx) /= 0) error_status = 1
end subroutine
subroutine bcond(idx)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer idx
  if (pomgpu_bcond(pom_ctx, int(idx, c_int)) /= 0) error_status = 1
end subroutine
subroutine bcondorl(idx)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer idx
  if (pomgpu_bcondorl(pom_ctx, int(idx, c_int)) /= 0) error_status = 1
end subroutine
subroutine restore_interior
  use pomgpu_iface
  implicit none
  include 'pom.h'
  call pomgpu_push_con
  if (pomgpu_restore_interior(pom_ctx) /= 0) error_status = 1
end subroutine
