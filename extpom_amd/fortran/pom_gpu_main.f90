! pom_gpu_main.f90 -- a minimal Fortran driver in the shape of the reference's `program pom`
! (reference pom/pom.f:5-39): take the initial COMMON blocks from a raw dump written by extpom_amd
! (the reference would read them through PnetCDF, which this image lacks), read pom.nml like
! read_input (initialize.f:71-74,173-198), then
!     do iint=1,nsteps: advance
! where `advance_hot` is the reference's sequence (advance.f:6-59) minus print / output, and every
! routine it calls is a pom_gpu_host.f90 wrapper -> C ABI -> HIP kernels.  File forcing: the input
! files <wrk_pth>in/<netcdf_file>.sfrc.nc / .lbry.nc / .clim.nc that exist are read by the library
! itself (pom_gpu_forcing_files.f90); without them the forcing is constant.
! Writes the final blocks back for checking against the oracle (tests/test_fortran_host.py).
!
! A cold start needs no dump: `--cold` sets read_input's constants (initialize.f:80-198), reads pom.nml and has cold_start_files
! (pom_gpu_io.f90) do initialize.f:24-36 on the device from <wrk_pth>in/<netcdf_file>.grid.nc, .init.nc and .clim.nc; the restart
! reader (nread_rst /= 0), the forcing files, the steps and the dump follow as ever.
!
! usage: pom_gpu_main <state.in> <state.out>     (pom.nml in the working directory)
!        pom_gpu_main --cold <state.out> <nsteps>
!        pom_gpu_main --cold-z <state.out> <nsteps>     (T, S and Tclim, Sclim on z levels: mapped with ztosig)
!        ... --cold | --cold-z <state.out> <nsteps> --lbry-z     (temp, salt of the lbry file on z levels: bounds_forcing.f:636-716)
!        ... --cold | --cold-z <state.out> <nsteps> --lbry-sides <n>     (the sides the lbry file feeds: east 1 + south 2 + west 4 + north 8;
!                                                                         default 3, the reference's reader; beside --lbry-z, either first)
!        ... --cold | --cold-z <state.out> <nsteps> --mean     (the time-mean output: every iprint steps write_output_pnetcdf writes
!                                                                <wrk_pth>out/<netcdf_file>.<nnnn>.nc with the means since the last one;
!                                                                beside the other two, in any order)
!        ... --cold | --cold-z <state.out> <nsteps> --sss      (surface sets ssurf from the record's SSS: bounds_forcing.f:979 uncommented)
!        ... --cold | --cold-z <state.out> <nsteps> --tracers <n>     (n passive tracers, pom_tracers: read from <wrk_pth>in/<netcdf_file>.tracer.nc
!                                                                      where it exists; wherever an output file is written,
!                                                                      <wrk_pth>out/<netcdf_file>.tracer.<nnnn>.nc beside it -- the mean kind under
!                                                                      --mean --; <wrk_pth>out/<netcdf_file>.tracer.rst.nc at the end of the run;
!                                                                      beside the other flags, in any order)
!        ... --cold | --cold-z <state.out> <nsteps> --floats   (Lagrangian floats: registered from <wrk_pth>in/<netcdf_file>.floats.nc where it
!                                                                exists; wherever an output file is written, <wrk_pth>out/<netcdf_file>.floats.<nnnn>.nc
!                                                                beside it; <wrk_pth>out/<netcdf_file>.floats.rst.nc at the end of the run)
!        ... --cold | --cold-z <state.out> <nsteps> --tides    (the tide of the open boundaries: the table of <wrk_pth>in/<netcdf_file>.tide.nc)
!        ... --cold | --cold-z <state.out> <nsteps> --harmonics [every]   (the harmonic analysis of elb uab vab with that table, every
!                                                                `every`-th step (default 1); <wrk_pth>out/<netcdf_file>.harmonics.nc at the end
!                                                                of the run; a run whose tide comes in the lbry file names --tides for the table)
! The water files <wrk_pth>in/<netcdf_file>.water.NNNN.nc need no flag: they are registered when record 0000's exists.
program pom_gpu_main
  use pomgpu_iface
  implicit none
  include 'pom.h'
  namelist/pom_nml/ title,wrk_pth,netcdf_file,mode,nadv,nitera,sw,npg,dte,isplit,time_start,nread_rst, &
                    read_rst_file,cont_bry,write_rst,write_rst_file,days,prtd1,prtd2,swtch,ntp,nbct,nbcs
  integer :: nsteps, nrec, n, rc, n2, n3, nbd, ntrac
  double precision :: vtot, atot, mtot, stot, tavg, savg, eavg, ekin
  double precision, allocatable, target :: tr(:,:,:,:), sr(:,:,:,:)
  character(len=256) :: fin, fout, arg3, arg4
  logical :: cold, mean, sss, floats, tides, harm
  integer :: hevery, ios

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  n2 = im_local*jm_local
  n3 = n2*kb
  nbd = 8*jm_local + 8*im_local + (12+12+6+6)*0   ! filled below
  nbd = 20*jm_local + 20*im_local + 18*jm_local*kb + 18*im_local*kb   ! bdry: 20 J, 20 I... see pom_layout.h
  cold = trim(fin) == '--cold' .or. trim(fin) == '--cold-z'
  mean = .false.; sss = .false.; ntrac = 0; floats = .false.; tides = .false.; harm = .false.; hevery = 1
  if (trim(fin) == '--cold-z') then         ! the init and the clim file are on z levels (initialize.f:410-422)
    pom_init_on_z = .true.; pom_clim_on_z = .true.
  end if
  if (cold) then                             ! one tile, the whole grid; read_input's constants (initialize.f:80-168)
    call get_command_argument(3, arg3)
    read(arg3, *) nsteps
    n = 4                                    ! --lbry-z, --lbry-sides <n> and --mean, in any order
    do while (n <= command_argument_count())
      call get_command_argument(n, arg3)
      if (trim(arg3) == '--lbry-z') pom_lbry_on_z = .true.
      if (trim(arg3) == '--mean') mean = .true.
      if (trim(arg3) == '--sss') sss = .true.
      if (trim(arg3) == '--floats') floats = .true.
      if (trim(arg3) == '--tides') tides = .true.
      if (trim(arg3) == '--harmonics') then
        harm = .true.
        if (n < command_argument_count()) then     ! an optional number behind it
          call get_command_argument(n + 1, arg4)
          read(arg4, *, iostat=ios) hevery
          if (ios == 0) then
            n = n + 1
          else
            hevery = 1
          end if
        end if
      end if
      if (trim(arg3) == '--lbry-sides') then
        n = n + 1
        call get_command_argument(n, arg3)
        read(arg3, *) pom_lbry_sides
      end if
      if (trim(arg3) == '--tracers') then
        n = n + 1
        call get_command_argument(n, arg3)
        read(arg3, *) ntrac
      end if
      n = n + 1
    end do
    im = im_local; jm = jm_local; nrec = 0
    n_west = -1; n_east = -1; n_south = -1; n_north = -1
    rhoref=1025.d0; tbias=0.d0; sbias=0.d0; grav=9.806d0; kappa=0.4d0; z0b=.01d0; cbcmin=.0025d0; cbcmax=1.d0
    horcon=0.1d0; tprni=.1d0; umol=1.d-6; vmaxl=100.d0; slmax=2.d0; ntp=2; nbct=1; nbcs=1; ispadv=1; smoth=0.10d0
    alpha=0.d0; aam_init=0.d0
  else
    open(71, file=trim(fin), form='unformatted', access='stream', status='old')
    read(71) im, jm, n_west, n_east, n_south, n_north, nsteps, nrec, nbd
    call blk_read(71, dz, 4*kb)                ! COMMON members are contiguous: read each block whole
    call blk_read(71, aam2d, 73*n2)
    call blk_read(71, aam, 40*n3)
    call blk_read(71, ele, nbd)
    call blk_read(71, alpha, 47)               ! blkcon: 376 bytes
  end if
  imm1=im-1; imm2=im-2; jmm1=jm-1; jmm2=jm-2; kbm1=kb-1; kbm2=kb-2
  allocate(tr(im,jm,kb,max(nrec,1)), sr(im,jm,kb,max(nrec,1)))
  if (.not. cold) then
    do n = 1, nrec
      read(71) tr(:,:,:,n), sr(:,:,:,n)
    end do
    close(71)
  end if
  lramp = .false.
  open(73, file='pom.nml', status='old')
  read(73, nml=pom_nml)
  close(73)
  dti=dte*float(isplit); dte2=dte*2; dti2=dti*2
  ispi=1.d0/float(isplit); isp2i=1.d0/(2.d0*float(isplit))
  if (cold) then                             ! the rest of read_input (initialize.f:178-198)
    small=1.d-9; pi=atan(1.d0)*4.d0
    iend=max0(nint(days*24.d0*3600.d0/dti),2)
    iprint=nint(prtd1*24.d0*3600.d0/dti)
    iswtch=nint(swtch*24.d0*3600.d0/dti)
    irestart=nint(write_rst*24.d0*3600.d0/dti)
    time0=0.d0; time=0.d0
    if (nread_rst == 0) cont_bry = 0
  end if

  call pomgpu_host_init(0)
  call pomgpu_upload_state
  my_task = 0; master_task = 0
  i_global(1) = 1; j_global(1) = 1           ! one tile: the patch starts at the grid's first cell
  if (cold) call cold_start_files            ! initialize.f:24-36
  if (nread_rst /= 0) call read_restart_pnetcdf   ! initialize.f:39, for a host without PnetCDF: <wrk_pth>in/<read_rst_file>
  call pomgpu_open_forcing_files(pom_frc_sfrc, pom_frc_lbry, pom_frc_clim)
  if (.not. pom_frc_clim) then                   ! (with a clim file restore_interior's records are the file's)
    do n = 1, nrec
      rc = pomgpu_set_restore_record(pom_ctx, int(n, c_int), c_loc(tr(1,1,1,n)), c_loc(sr(1,1,1,n)))
    end do
  end if
  if (ntrac > 0) then                        ! before the mean is switched on: its accumulators are made for the tracers registered then
    call pom_tracers(ntrac)
    call read_tracers_pnetcdf                ! <wrk_pth>in/<netcdf_file>.tracer.nc, where it exists
  end if
  if (floats) call read_floats_pnetcdf       ! <wrk_pth>in/<netcdf_file>.floats.nc, where it exists
  if (tides .or. harm) call read_tides_pnetcdf   ! <wrk_pth>in/<netcdf_file>.tide.nc, where it exists
  if (harm) call pom_harmonics(.true., hevery)
  if (mean) call pom_output_mean(.true.)
  if (sss) call pom_surface_sss(.true.)
  do n = 1, nsteps                          ! pom.f:17-19
    iint = iint + 1
    call advance_hot
    if (pom_mean_on .and. iprint > 0) then   ! advance.f:35-38: the mean file in the snapshot's place (Fortran does not short-circuit: iprint is tested first)
      if (mod(iint, iprint) == 0) then
        call write_output_pnetcdf
        if (ntrac > 0) call write_tracers_pnetcdf(2)   ! the tracers' means, beside the nine fields'
        if (floats) call write_floats_pnetcdf(1)       ! the floats as they are now, beside it
      end if
    end if
  end do
  if (ntrac > 0) call write_tracers_pnetcdf(0)   ! <wrk_pth>out/<netcdf_file>.tracer.rst.nc: trb, tr and the work array trf
  if (floats) call write_floats_pnetcdf(0)       ! <wrk_pth>out/<netcdf_file>.floats.rst.nc: output and checkpoint in one
  if (harm) call write_harmonics_pnetcdf         ! <wrk_pth>out/<netcdf_file>.harmonics.nc
  if (pom_mean_on) call pom_output_mean(.false.)
  my_task = 0; master_task = 0
  call domain_stats(vtot, atot, mtot, stot, tavg, savg, eavg, ekin)   ! print_section's sums, no state download needed
  write(6,'(a,8es25.16e3)') 'domain_stats:', vtot, atot, mtot, stot, tavg, savg, eavg, ekin
  call pomgpu_download_state
  open(72, file=trim(fout), form='unformatted', access='stream', status='replace')
  call blk_write(72, aam2d, 73*n2)
  call blk_write(72, aam, 40*n3)
  call blk_write(72, alpha, 47)
  close(72)
  write(6,'(a,i6,a,i3)') 'pom_gpu_main: steps ', nsteps, '  error_status ', error_status
  call pomgpu_destroy(pom_ctx)
end program

! advance.f:6-59 without print_section and output; surface_forcing (advance.f:77-93) / lateral_bc where the library has the file
subroutine advance_hot
  use pomgpu_iface, only: pom_frc_sfrc, pom_frc_lbry
  implicit none
  include 'pom.h'
  time=dti*float(iint)/86400.d0+time0        ! get_time, advance.f:62-75
  if(iint.ge.iswtch) iprint=nint(prtd2*24.d0*3600.d0/dti)
  if(lramp) then
    ramp=time/period
    if(ramp.gt.1.d0) ramp=1.d0
  else
    ramp=1.d0
  endif
  if (pom_frc_sfrc) then
    call wind
    call heat
    call water                               ! advance.f:89 (commented there); nothing unless <netcdf_file>.water.0000.nc was found
    call surface
  else
    call water
  end if
  if (pom_frc_lbry) call lateral_bc
  call lateral_viscosity
  call mode_interaction
  do iext=1,isplit
    call mode_external
  end do
  call mode_internal
  call mean_accumulate                       ! the time-mean output, where advance.f:38 writes (nothing while it is off)
  call float_step                            ! the Lagrangian floats (nothing without them)
  call harmonic_step                         ! the harmonic analysis (nothing while it is off)
  call check_velocity
end subroutine

! this driver runs ONE task: the rank reductions of the reference's parallel_mpi.f:125-151 are identities
subroutine sum0d_mpi(work, to)
  implicit none
  double precision work
  integer to
end subroutine
subroutine bcast0d_mpi(work, from)
  implicit none
  double precision work
  integer from
end subroutine
subroutine pomgpu_minmax0d_mpi(mn, mx, to)
  implicit none
  double precision mn, mx
  integer to
end subroutine
subroutine pomgpu_barrier_mpi               ! pom_gpu_io.f90's barrier between ranks: one task, nothing to wait for
end subroutine
