! pom_gpu_forcing_files.f90 -- wind, heat, water, surface and lateral_bc (reference pom/bounds_forcing.f:871-1020, :593-868) for a host WITHOUT
! PnetCDF: link instead of pom_gpu_forcing.f90.  No reader call is left: the library has been told the three input files once
! (pomgpu_open_forcing_files below, called after the upload) and its own schedule code -- the reference's, bounds_forcing.f:884-902,
! :607-613, :740-758 -- reads the record a step asks for on the device (pomgpu_set_forcing_files, include/pomgpu.h).  Each routine is
! pomgpu_push_con (iint, time) and the library routine.
subroutine wind
  use pomgpu_iface
  implicit none
  include 'pom.h'
  call pomgpu_push_con
  if (pomgpu_wind(pom_ctx) /= 0) error_status = 1
end subroutine

subroutine heat
  use pomgpu_iface
  implicit none
  include 'pom.h'
  call pomgpu_push_con
  if (pomgpu_heat(pom_ctx) /= 0) error_status = 1
end subroutine

subroutine water                                     ! bounds_forcing.f:986-1020; nothing unless the water files are registered
  use pomgpu_iface
  implicit none
  include 'pom.h'
  if (.not. pom_frc_water) return
  call pomgpu_push_con
  if (pomgpu_water(pom_ctx) /= 0) error_status = 1
end subroutine

subroutine surface
  use pomgpu_iface
  implicit none
  include 'pom.h'
  call pomgpu_push_con
  if (pomgpu_surface(pom_ctx) /= 0) error_status = 1
end subroutine

subroutine lateral_bc
  use pomgpu_iface
  implicit none
  include 'pom.h'
  call pomgpu_push_con
  if (pomgpu_lateral_bc(pom_ctx) /= 0) error_status = 1
end subroutine

! The three paths as the reference's readers build them (io_pnetcdf.F:2929, :3445, :3289: trim(wrk_pth)//'in/'//trim(netcdf_file)//
! '.sfrc.nc', '.lbry.nc', '.clim.nc'); those that exist are registered, this tile's patch at (i_global(1), j_global(1)).
! have_sfrc / have_lbry / have_clim: which did.  A file that exists and is refused: error_status = 1 and the library's message.
! Next to them '.restore_tau_interior.nc' (io_pnetcdf.F:3067), the restore rate on z levels: registered when it exists
! (pomgpu_set_restore_rate_file); restore_interior then maps the rate that goes with every T/S record it loads.
subroutine pomgpu_open_forcing_files(have_sfrc, have_lbry, have_clim)
  use pomgpu_iface
  implicit none
  include 'pom.h'
  logical, intent(out) :: have_sfrc, have_lbry, have_clim
  type(pomgpu_file_meta) :: m
  character(len=400) :: fname
  character(len=256) :: wp
  character(kind=c_char, len=401), target :: cname(3), rname, wname
  character(len=8), parameter :: suffix(3) = (/ '.sfrc.nc', '.lbry.nc', '.clim.nc' /)
  character(kind=c_char), pointer :: msg(:)
  type(c_ptr) :: p(3), pm
  logical :: have(3), have_rate, have_water
  integer(c_int) :: rc
  integer :: q, n
  wp = wrk_pth                                     ! a namelist without wrk_pth leaves the COMMON member as the loader did: NULs, not blanks
  do n = 1, len(wp)
    if (wp(n:n) == char(0)) wp(n:n) = ' '
  end do
  do q = 1, 3
    write(fname, '(a,''in/'',a,a)') trim(wp), trim(netcdf_file), suffix(q)
    inquire(file=trim(fname), exist=have(q))
    cname(q) = trim(fname)//c_null_char
    p(q) = c_null_ptr
    if (have(q)) p(q) = c_loc(cname(q))
  end do
  have_sfrc = have(1); have_lbry = have(2); have_clim = have(3)
  write(fname, '(a,''in/'',a,a)') trim(wp), trim(netcdf_file), '.restore_tau_interior.nc'
  inquire(file=trim(fname), exist=have_rate)
  rname = trim(fname)//c_null_char
  ! the water files (io_pnetcdf.F:3244: ...'.water.',i4.4,'.nc'): registered when record 0's exists; pom_frc_water makes `water` run
  write(fname, '(a,''in/'',a,''.water.'',i4.4,''.nc'')') trim(wp), trim(netcdf_file), 0
  inquire(file=trim(fname), exist=have_water)
  write(fname, '(a,''in/'',a)') trim(wp), trim(netcdf_file)
  wname = trim(fname)//c_null_char
  pom_frc_water = .false.
  if (.not. any(have) .and. .not. have_rate .and. .not. have_water) return
  m%title = c_null_ptr; m%time_start = c_null_ptr; m%stats = c_null_ptr; m%create = 0
  m%im_global = im_global; m%jm_global = jm_global
  m%i0 = i_global(1); m%j0 = j_global(1)
  rc = 0
  if (have(3)) rc = pomgpu_set_z_inputs(pom_ctx, merge(1_c_int, 0_c_int, pom_init_on_z), merge(1_c_int, 0_c_int, pom_clim_on_z))   ! a z-level clim file: the months go through ztosig
  if (rc == 0 .and. have(2)) rc = pomgpu_set_z_lateral(pom_ctx, merge(1_c_int, 0_c_int, pom_lbry_on_z))   ! a z-level lbry file: every record's temp, salt lines go through ztosig
  if (rc == 0 .and. have(2)) rc = pomgpu_set_lateral_sides(pom_ctx, int(pom_lbry_sides, c_int))   ! the sides the lbry file feeds; the others: tclim, sclim lines
  if (rc == 0 .and. any(have)) rc = pomgpu_set_forcing_files(pom_ctx, p(1), p(2), p(3), m)
  if (rc == 0 .and. have_rate) rc = pomgpu_set_restore_rate_file(pom_ctx, c_loc(rname), m)
  if (rc == 0 .and. have_water) then
    rc = pomgpu_set_water_files(pom_ctx, c_loc(wname), m)
    pom_frc_water = rc == 0
  end if
  if (rc /= 0) then                                ! handle_error_pnetcdf, io_pnetcdf.F:43-54: a message and error_status = 1
    error_status = 1
    have_sfrc = .false.; have_lbry = .false.; have_clim = .false.
    pm = pomgpu_last_error(pom_ctx)
    if (c_associated(pm)) then
      call c_f_pointer(pm, msg, (/512/))
      n = 0
      do while (n < 511)
        if (msg(n+1) == c_null_char) exit
        n = n + 1
      end do
      write(*,'(/i4,''] Error: forcing files: '',511a1)') my_task, msg(1:n)
    end if
  end if
end subroutine
