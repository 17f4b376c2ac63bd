! pom_gpu_io.f90 -- write_output_pnetcdf, write_restart_pnetcdf and read_restart_pnetcdf (reference pom/io_pnetcdf.F:57-410,
! :1661-2083, :2420-2768) without PnetCDF: the file names are built as the reference builds them, the files themselves (CDF-2, same
! dimensions / variables / attributes) are written by the library straight from the device state
! (pomgpu_write_output / pomgpu_write_restart); every rank writes its patch, rank 0 creates the file first.  With the time-mean output on
! (pom_output_mean, pom_gpu_host.f90) write_output_pnetcdf writes the same file with the means of its nine time-dependent fields.
! read_restart_pnetcdf reads such a file (or one PnetCDF wrote) back into the device state and the COMMON blocks.
! write_tracers_pnetcdf / read_tracers_pnetcdf are the same for the passive tracers' own files (pomgpu_write_tracers, pomgpu_read_tracers).
! cold_start_files is initialize.f:24-36 (initialize_arrays, read_grid, initial_conditions, update_initial, bottom_friction) from the
! reference's grid, init and clim files (pomgpu_cold_start).
! Link instead of the reference's two writers and its restart reader.  pomgpu_barrier_mpi is the integrator's one-liner
! (call mpi_barrier(pom_comm, ierr); nothing on a single rank): this file does not include mpif.h.
subroutine write_output_pnetcdf
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer :: nprint
  character(len=400) :: fname
  nprint = (iint+int(time0*86400./dti))/iprint
  write(fname, '(a,''out/'',a,''.'',i4.4,''.nc'')') trim(wrk_pth), trim(netcdf_file), nprint
  call pomgpu_write_file(fname, 0)
end subroutine

subroutine write_restart_pnetcdf
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer :: nprint
  character(len=400) :: fname
  nprint = (iint+int(time0*86400./dti))/irestart
  write(fname, '(a,''out/'',a,''.'',i4.4,''.nc'')') trim(wrk_pth), trim(write_rst_file), nprint
  call pomgpu_write_file(fname, 1)
end subroutine

subroutine pomgpu_write_file(fname, restart)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  character(len=*), intent(in) :: fname
  integer, intent(in) :: restart
  type(pomgpu_file_meta) :: m
  character(kind=c_char, len=401), target :: cname
  character(kind=c_char, len=41), target :: ctitle
  character(kind=c_char, len=27), target :: cstart
  real(c_double), target :: st(8)
  integer(c_int) :: rc
  integer :: pass
  cname = trim(fname)//c_null_char
  ctitle = trim(title)//c_null_char
  cstart = trim(time_start)//c_null_char
  call pomgpu_push_con
  call domain_stats(st(1), st(2), st(3), st(4), st(5), st(6), st(7), st(8))   ! rank-reduced, as the reference's writer does
  if (my_task == 0) write(*,'(/''writing file '',a)') trim(fname)
  m%title = c_loc(ctitle); m%time_start = c_loc(cstart)
  m%im_global = im_global; m%jm_global = jm_global
  m%i0 = i_global(1); m%j0 = j_global(1)
  m%stats = c_loc(st)
  do pass = 1, 2                                  ! rank 0 lays the file out, then everybody else writes
    m%create = 0
    if (pass == 1 .and. my_task == 0) m%create = 1
    if ((pass == 1) .eqv. (my_task == 0)) then
      if (restart == 0 .and. pom_mean_on) then
        rc = pomgpu_write_output_mean(pom_ctx, c_loc(cname), m)   ! the means since the last output file, in the snapshot's place
      else if (restart == 0) then
        rc = pomgpu_write_output(pom_ctx, c_loc(cname), m)
      else
        rc = pomgpu_write_restart(pom_ctx, c_loc(cname), m)
      end if
      if (rc /= 0) error_status = 1
    end if
    call pomgpu_barrier_mpi                        ! mpi_barrier(pom_comm) on several ranks
  end do
  ! The library returns once the file is laid out and a snapshot of its arrays is taken; a host thread writes it while the
  ! model goes on.  A RESTART file must be whole when this routine returns (the reference's writer is synchronous and
  ! collective, io_pnetcdf.F:1661-2083: a run that dies in the next step must find it), so it is joined here and its
  ! status becomes the run's; an output file is joined by the next write or by pomgpu_host_finalize.
  if (restart /= 0) then
    if (pomgpu_io_wait(pom_ctx) /= 0) error_status = 1
    call pomgpu_barrier_mpi
  end if
end subroutine

! read_restart_pnetcdf (io_pnetcdf.F:2420-2768): the reference calls it from initialize (initialize.f:39); a host without PnetCDF
! calls it after pomgpu_upload_state.  Every rank reads its own patch (no ordering between ranks is needed); afterwards the
! device state AND the COMMON blocks hold what the reference's reader would have left: the 37 restart fields, d, dt, time0, time
! and -- if cont_bry was non-zero -- cont_bry = the file's iint.
subroutine read_restart_pnetcdf
  use pomgpu_iface
  implicit none
  include 'pom.h'
  type(pomgpu_file_meta) :: m
  character(len=400) :: fname
  character(kind=c_char, len=401), target :: cname
  character(kind=c_char), pointer :: msg(:)
  type(c_ptr) :: pm
  integer(c_int) :: rc
  integer :: n
  write(fname, '(a,''in/'',a)') trim(wrk_pth), trim(read_rst_file)
  cname = trim(fname)//c_null_char
  if (my_task == 0) write(*,'(/''reading file '',a)') trim(fname)
  call pomgpu_push_con                             ! cont_bry as read_input left it
  m%title = c_null_ptr; m%time_start = c_null_ptr; m%stats = c_null_ptr; m%create = 0
  m%im_global = im_global; m%jm_global = jm_global
  m%i0 = i_global(1); m%j0 = j_global(1)
  rc = pomgpu_read_restart(pom_ctx, c_loc(cname), m, c_null_ptr, c_null_ptr)
  if (rc /= 0) then                                ! handle_error_pnetcdf, io_pnetcdf.F:43-54: a message and error_status = 1
    error_status = 1                               ! (on the rank that failed: a tile that does not fit is that rank's own finding)
    pm = pomgpu_last_error(pom_ctx)                ! names the file and the cause
    if (c_associated(pm)) then
      call c_f_pointer(pm, msg, (/512/))
      n = 0
      do while (n < 511)
        if (msg(n+1) == c_null_char) exit
        n = n + 1
      end do
      write(*,'(/i4,''] Error: read_restart_pnetcdf: '',511a1)') my_task, msg(1:n)
    end if
    return
  end if
  rc = pomgpu_get_con(pom_ctx, c_loc(alpha))       ! time0, time, cont_bry
  if (rc /= 0) error_status = 1
  call pomgpu_download_state
end subroutine

! The tracers' files (no counterpart in the reference; include/pomgpu.h: pomgpu_write_tracers).  kind 0: the restart kind,
! <wrk_pth>out/<netcdf_file>.tracer.rst.nc, joined before return as write_restart_pnetcdf's file is; kind 1 / 2: the output kind / its
! time-mean form, <wrk_pth>out/<netcdf_file>.tracer.<nnnn>.nc with write_output_pnetcdf's counter.  pomgpu_write_file's two passes: rank 0
! lays the file out, a barrier, everybody else writes.  The statistics are rank-reduced as the reference reduces its own: tot with
! sum0d_mpi and avg = tot / vtot with domain_stats' vtot, min and max with pomgpu_minmax0d_mpi (pom_gpu_mpi.f90; an identity on one rank).
! Nothing happens without tracers.
subroutine write_tracers_pnetcdf(kind)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer, intent(in) :: kind
  type(pomgpu_file_meta) :: m
  character(len=400) :: fname
  character(kind=c_char, len=401), target :: cname
  character(kind=c_char, len=41), target :: ctitle
  character(kind=c_char, len=27), target :: cstart
  real(c_double), target :: ts(4, 8)
  double precision :: vtot, atot, mtot, stot, tavg, savg, eavg, ekin
  type(c_ptr) :: pts
  integer(c_int) :: rc
  integer :: pass, nprint, n, ntr
  ntr = pomgpu_tracer_count(pom_ctx)
  if (ntr <= 0) return
  if (kind == 0) then
    write(fname, '(a,''out/'',a,''.tracer.rst.nc'')') trim(wrk_pth), trim(netcdf_file)
  else
    nprint = (iint+int(time0*86400./dti))/iprint
    write(fname, '(a,''out/'',a,''.tracer.'',i4.4,''.nc'')') trim(wrk_pth), trim(netcdf_file), nprint
  end if
  cname = trim(fname)//c_null_char
  ctitle = trim(title)//c_null_char
  cstart = trim(time_start)//c_null_char
  call pomgpu_push_con
  pts = c_null_ptr
  if (kind /= 0) then
    call domain_stats(vtot, atot, mtot, stot, tavg, savg, eavg, ekin)   ! rank-reduced vtot
    if (pomgpu_tracer_stats(pom_ctx, c_loc(ts)) /= 0) error_status = 1
    do n = 1, ntr
      call sum0d_mpi(ts(1, n), master_task)
      call pomgpu_minmax0d_mpi(ts(3, n), ts(4, n), master_task)
      if (vtot /= 0.d0) then
        ts(2, n) = ts(1, n) / vtot
      else
        ts(2, n) = 0.d0
      end if
    end do
    pts = c_loc(ts)
  end if
  if (my_task == 0) write(*,'(/''writing file '',a)') trim(fname)
  m%title = c_loc(ctitle); m%time_start = c_loc(cstart); m%stats = c_null_ptr
  m%im_global = im_global; m%jm_global = jm_global
  m%i0 = i_global(1); m%j0 = j_global(1)
  do pass = 1, 2                                  ! rank 0 lays the file out, then everybody else writes
    m%create = 0
    if (pass == 1 .and. my_task == 0) m%create = 1
    if ((pass == 1) .eqv. (my_task == 0)) then
      rc = pomgpu_write_tracers(pom_ctx, c_loc(cname), m, int(kind, c_int), pts)
      if (rc /= 0) error_status = 1
    end if
    call pomgpu_barrier_mpi
  end do
  if (kind == 0) then                             ! a restart file is whole when this routine returns
    if (pomgpu_io_wait(pom_ctx) /= 0) error_status = 1
    call pomgpu_barrier_mpi
  end if
end subroutine

! <wrk_pth>in/<netcdf_file>.tracer.nc, where it exists, into the registered tracers (pomgpu_read_tracers): every rank reads its own patch,
! ghost lines included; a file with trNN alone is an initial file.  Call it after pom_tracers.  A refusal is printed as the restart
! reader's is and sets error_status.
subroutine read_tracers_pnetcdf
  use pomgpu_iface
  implicit none
  include 'pom.h'
  type(pomgpu_file_meta) :: m
  character(len=400) :: fname
  character(kind=c_char, len=401), target :: cname
  character(kind=c_char), pointer :: msg(:)
  type(c_ptr) :: pm
  integer(c_int) :: rc
  integer :: n
  logical :: there
  write(fname, '(a,''in/'',a,''.tracer.nc'')') trim(wrk_pth), trim(netcdf_file)
  inquire(file=trim(fname), exist=there)
  if (.not. there) return
  cname = trim(fname)//c_null_char
  if (my_task == 0) write(*,'(/''reading file '',a)') trim(fname)
  m%title = c_null_ptr; m%time_start = c_null_ptr; m%stats = c_null_ptr; m%create = 0
  m%im_global = im_global; m%jm_global = jm_global
  m%i0 = i_global(1); m%j0 = j_global(1)
  rc = pomgpu_read_tracers(pom_ctx, c_loc(cname), m, c_null_ptr, c_null_ptr)
  if (rc /= 0) then
    error_status = 1
    pm = pomgpu_last_error(pom_ctx)                ! names the file and the cause
    if (c_associated(pm)) then
      call c_f_pointer(pm, msg, (/512/))
      n = 0
      do while (n < 511)
        if (msg(n+1) == c_null_char) exit
        n = n + 1
      end do
      write(*,'(/i4,''] Error: read_tracers_pnetcdf: '',511a1)') my_task, msg(1:n)
    end if
  end if
end subroutine

! The float file (no counterpart in the reference; include/pomgpu.h: pomgpu_write_floats): state and samples of the Lagrangian floats,
! output and checkpoint in one.  kind 0: <wrk_pth>out/<netcdf_file>.floats.rst.nc; kind 1: <wrk_pth>out/<netcdf_file>.floats.<nnnn>.nc with
! write_output_pnetcdf's counter.  Floats live on one tile: rank 0 writes the whole file, synchronously.  Nothing happens without floats.
subroutine write_floats_pnetcdf(kind)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  integer, intent(in) :: kind
  type(pomgpu_file_meta) :: m
  character(len=400) :: fname
  character(kind=c_char, len=401), target :: cname
  character(kind=c_char, len=41), target :: ctitle
  character(kind=c_char, len=27), target :: cstart
  integer :: nprint
  if (pomgpu_float_count(pom_ctx) <= 0) return
  if (kind == 0) then
    write(fname, '(a,''out/'',a,''.floats.rst.nc'')') trim(wrk_pth), trim(netcdf_file)
  else
    nprint = (iint+int(time0*86400./dti))/iprint
    write(fname, '(a,''out/'',a,''.floats.'',i4.4,''.nc'')') trim(wrk_pth), trim(netcdf_file), nprint
  end if
  cname = trim(fname)//c_null_char
  ctitle = trim(title)//c_null_char
  cstart = trim(time_start)//c_null_char
  call pomgpu_push_con
  if (my_task == 0) write(*,'(/''writing file '',a)') trim(fname)
  m%title = c_loc(ctitle); m%time_start = c_loc(cstart); m%stats = c_null_ptr; m%create = 1
  m%im_global = im_global; m%jm_global = jm_global
  m%i0 = i_global(1); m%j0 = j_global(1)
  if (pomgpu_write_floats(pom_ctx, c_loc(cname), m) /= 0) error_status = 1
end subroutine

! The tide file (include/pomgpu.h: pomgpu_set_tide_file): <wrk_pth>in/<netcdf_file>.tide.nc, where it exists, registered as pom_tides_put
! would -- omega(ncon) and per side el_amp.<side> el_pha.<side> [un_amp.<side> un_pha.<side>].  A refusal is printed and sets error_status.
subroutine read_tides_pnetcdf
  use pomgpu_iface
  implicit none
  include 'pom.h'
  type(pomgpu_file_meta) :: m
  character(len=400) :: fname
  character(kind=c_char, len=401), target :: cname
  character(kind=c_char), pointer :: msg(:)
  type(c_ptr) :: pm
  integer :: n
  logical :: there
  write(fname, '(a,''in/'',a,''.tide.nc'')') trim(wrk_pth), trim(netcdf_file)
  inquire(file=trim(fname), exist=there)
  if (.not. there) return
  cname = trim(fname)//c_null_char
  if (my_task == 0) write(*,'(/''reading file '',a)') trim(fname)
  m%title = c_null_ptr; m%time_start = c_null_ptr; m%stats = c_null_ptr; m%create = 0
  m%im_global = im_global; m%jm_global = jm_global
  m%i0 = i_global(1); m%j0 = j_global(1)
  if (pomgpu_set_tide_file(pom_ctx, c_loc(cname), m) /= 0) then
    error_status = 1
    pm = pomgpu_last_error(pom_ctx)
    if (c_associated(pm)) then
      call c_f_pointer(pm, msg, (/512/))
      n = 0
      do while (n < 511)
        if (msg(n+1) == c_null_char) exit
        n = n + 1
      end do
      write(*,'(/i4,''] Error: read_tides_pnetcdf: '',511a1)') my_task, msg(1:n)
    end if
  end if
end subroutine

! The harmonics file (pomgpu_write_harmonics): <wrk_pth>out/<netcdf_file>.harmonics.nc, mean, amplitude and phase maps of elb uab vab per
! constituent; every rank writes its patch as in pomgpu_write_file, rank 0 lays the file out first.  Joined before it returns (it is written
! at the end of a run).  Nothing happens while the analysis is off.
subroutine write_harmonics_pnetcdf
  use pomgpu_iface
  implicit none
  include 'pom.h'
  type(pomgpu_file_meta) :: m
  character(len=400) :: fname
  character(kind=c_char, len=401), target :: cname
  character(kind=c_char, len=41), target :: ctitle
  character(kind=c_char, len=27), target :: cstart
  integer :: pass
  if (pomgpu_harmonic_count(pom_ctx) < 0) return
  write(fname, '(a,''out/'',a,''.harmonics.nc'')') trim(wrk_pth), trim(netcdf_file)
  cname = trim(fname)//c_null_char
  ctitle = trim(title)//c_null_char
  cstart = trim(time_start)//c_null_char
  call pomgpu_push_con
  if (my_task == 0) write(*,'(/''writing file '',a)') trim(fname)
  m%title = c_loc(ctitle); m%time_start = c_loc(cstart); m%stats = c_null_ptr
  m%im_global = im_global; m%jm_global = jm_global
  m%i0 = i_global(1); m%j0 = j_global(1)
  do pass = 1, 2
    m%create = 0
    if (pass == 1 .and. my_task == 0) m%create = 1
    if ((pass == 1) .eqv. (my_task == 0)) then
      if (pomgpu_write_harmonics(pom_ctx, c_loc(cname), m) /= 0) error_status = 1
    end if
    call pomgpu_barrier_mpi
  end do
  if (pomgpu_io_wait(pom_ctx) /= 0) error_status = 1
  call pomgpu_barrier_mpi
end subroutine

! <wrk_pth>in/<netcdf_file>.floats.nc, where it exists, registered as pom_floats_put would (pomgpu_read_floats): x y sig are required,
! status kind id optional -- a file with x y sig alone is an initial file any tool can write.  A refusal is printed as the restart reader's
! is and sets error_status.
subroutine read_floats_pnetcdf
  use pomgpu_iface
  implicit none
  include 'pom.h'
  type(pomgpu_file_meta) :: m
  character(len=400) :: fname
  character(kind=c_char, len=401), target :: cname
  character(kind=c_char), pointer :: msg(:)
  type(c_ptr) :: pm
  integer(c_int) :: rc
  integer :: n
  logical :: there
  write(fname, '(a,''in/'',a,''.floats.nc'')') trim(wrk_pth), trim(netcdf_file)
  inquire(file=trim(fname), exist=there)
  if (.not. there) return
  cname = trim(fname)//c_null_char
  if (my_task == 0) write(*,'(/''reading file '',a)') trim(fname)
  m%title = c_null_ptr; m%time_start = c_null_ptr; m%stats = c_null_ptr; m%create = 0
  m%im_global = im_global; m%jm_global = jm_global
  m%i0 = i_global(1); m%j0 = j_global(1)
  rc = pomgpu_read_floats(pom_ctx, c_loc(cname), m, c_null_ptr, c_null_ptr)
  if (rc /= 0) then
    error_status = 1
    pm = pomgpu_last_error(pom_ctx)                ! names the file and the cause
    if (c_associated(pm)) then
      call c_f_pointer(pm, msg, (/512/))
      n = 0
      do while (n < 511)
        if (msg(n+1) == c_null_char) exit
        n = n + 1
      end do
      write(*,'(/i4,''] Error: read_floats_pnetcdf: '',511a1)') my_task, msg(1:n)
    end if
  end if
end subroutine

! initialize.f:24-36 without PnetCDF: what initialize does between read_input and the restart reader -- initialize_arrays, read_grid,
! initial_conditions, update_initial, bottom_friction -- on the device, from <wrk_pth>in/<netcdf_file>.grid.nc, .init.nc and .clim.nc
! (the names of io_pnetcdf.F:2102, :2790, :2865).  Call it after read_input and pomgpu_upload_state (blkcon holds the run's constants;
! the arrays may hold anything).  Every rank reads its own patch and one more column / row towards a west / south neighbour, so no
! exchange is needed; afterwards the device state AND the COMMON blocks hold what the reference would have.  pom_init_on_z / pom_clim_on_z
! (pomgpu_iface): T, S / Tclim, Sclim are on the z levels of `Level` / `z` and are mapped with ztosig, as the reference's commented calls
! (initialize.f:410-422) would; a tile then reads one more line towards EVERY neighbour.  pom_cflmin is this rank's
! cflmin: check_cflmin_mpi (parallel_mpi.f:501-512) reduces it with mpi_min and prints the warning; one rank prints it here.
subroutine cold_start_files
  use pomgpu_iface
  implicit none
  include 'pom.h'
  type(pomgpu_file_meta) :: m
  type(pomgpu_cold_info), target :: info
  character(len=400) :: fname
  character(kind=c_char, len=401), target :: cgrid, cinit, cclim
  character(kind=c_char), pointer :: msg(:)
  type(c_ptr) :: pm
  integer(c_int) :: rc
  integer :: n
  write(fname, '(a,''in/'',a,''.grid.nc'')') trim(wrk_pth), trim(netcdf_file)
  cgrid = trim(fname)//c_null_char
  if (my_task == 0) write(*,'(/''reading file '',a)') trim(fname)
  write(fname, '(a,''in/'',a,''.init.nc'')') trim(wrk_pth), trim(netcdf_file)
  cinit = trim(fname)//c_null_char
  if (my_task == 0) write(*,'(/''reading file '',a)') trim(fname)
  write(fname, '(a,''in/'',a,''.clim.nc'')') trim(wrk_pth), trim(netcdf_file)
  cclim = trim(fname)//c_null_char
  if (my_task == 0) write(*,'(/''reading file '',a)') trim(fname)
  call pomgpu_push_con                             ! read_input's constants
  m%title = c_null_ptr; m%time_start = c_null_ptr; m%stats = c_null_ptr; m%create = 0
  m%im_global = im_global; m%jm_global = jm_global
  m%i0 = i_global(1); m%j0 = j_global(1)
  rc = pomgpu_set_z_inputs(pom_ctx, merge(1_c_int, 0_c_int, pom_init_on_z), merge(1_c_int, 0_c_int, pom_clim_on_z))   ! initialize.f:410-422
  if (rc == 0) rc = pomgpu_cold_start(pom_ctx, c_loc(cgrid), c_loc(cinit), c_loc(cclim), m, c_loc(info))
  if (rc /= 0) then                                ! handle_error_pnetcdf, io_pnetcdf.F:43-54: a message and error_status = 1
    error_status = 1
    pm = pomgpu_last_error(pom_ctx)                ! names the file and the cause
    if (c_associated(pm)) then
      call c_f_pointer(pm, msg, (/512/))
      n = 0
      do while (n < 511)
        if (msg(n+1) == c_null_char) exit
        n = n + 1
      end do
      write(*,'(/i4,''] Error: cold_start_files: '',511a1)') my_task, msg(1:n)
    end if
    return
  end if
  rc = pomgpu_get_con(pom_ctx, c_loc(alpha))       ! period, rfe, rfw, rfn, rfs
  if (rc /= 0) error_status = 1
  call pomgpu_download_state
  pom_cflmin = info%cflmin
  if (n_proc == 1 .and. pom_cflmin < dte) then     ! parallel_mpi.f:504-511
    write(*,'(/a,f5.2,a)') "[!] Specified timestep (", dte, ") is too large."
    write(*,'(a,f5.2,a/)') "    You are strongly advised to make dte smaller than ", pom_cflmin, "."
  end if
end subroutine
