!------------------------------------------------------------------------------
! contour_gpu_driver -- the exchange post-processing up to the pair recursion (the call sequence of calculation.f90:816-940, on an
! ordinary bulk Hamiltonian: the contour routines do not depend on where `ee` came from), then the Gauss-Legendre contour routines of
! post_processing_exchange_p2rs (calculation.f90:803-813) and post_processing_paoflow2rs (:718), which the reference ships no input for:
!   green%calculate_intersite_gf_eta, exchange%calculate_exchange_gauss_legendre        on the chains of the pair recursion,
!   bands%calculate_moments_gauss_legendre, bands%calculate_occupation_gauss_legendre   after an on-site recursion of the same cell.
!
! Built by fortran/build_dropin.sh on the object set of the zero-edit drop-in: every `type(x)` below is the GPU type behind the
! reference's module name (fortran/shadow/); `exchange_plain` and `bands_plain` are the reference's own types, compiled unchanged under
! the module names exchange_ref_mod / bands_ref_mod.  Run inside a scratch copy of a case directory; reads input.nml.
!
! CONTOUR_DRIVER_MODE (environment):
!   contour        (default) the routines on type(exchange_gpu) / type(bands_gpu): one library call each
!   contour_plain  the reference's own type(exchange) / type(bands) over the same GPU objects: the inherited per-point loops
! Prints `eta_arrays_allocated=` and `eta_arrays_max=` (the largest |element| of gij_eta, 0 where it does not exist) after the exchange.
!------------------------------------------------------------------------------
program contour_gpu_driver
   use mpi_mod
   use control_mod
   use lattice_mod
   use charge_mod
   use mix_mod
   use energy_mod
   use hamiltonian_mod
   use recursion_mod
   use density_of_states_mod
   use green_mod
   use bands_mod
   use exchange_mod
   use exchange_ref_mod, only: exchange_plain => exchange
   use bands_ref_mod, only: bands_plain => bands
   use math_mod, only: ang2au
   use precision_mod, only: rp
   use timer_mod, only: g_timer, timer
   implicit none

   type(control), target :: control_obj
   type(lattice), target :: lattice_obj
   type(energy), target :: energy_obj
   type(charge), target :: charge_obj
   type(hamiltonian), target :: hamiltonian_obj
   type(recursion), target :: recursion_obj
   type(green), target :: green_obj
   type(dos), target :: dos_obj
   type(bands), target :: bands_obj
   type(mix), target :: mix_obj
   type(exchange), target :: exchange_obj
   type(exchange_plain), target :: plain_obj
   type(bands_plain), target :: bands_plain_obj
   real(rp) :: sumocc, etamax
   character(len=32) :: mode
   integer :: i, elen, estat, n

   rank = 0
   numprocs = 1
   g_timer = timer()
   call g_timer%start('Calculation')
   call get_environment_variable('CONTOUR_DRIVER_MODE', mode, elen, estat)
   if (estat /= 0 .or. elen == 0) mode = 'contour'

   control_obj = control('input.nml')
   lattice_obj = lattice(control_obj)
   call lattice_obj%build_data()
   call lattice_obj%bravais()
   select case (control_obj%calctype)
   case ('B')
      call lattice_obj%structb(.true.)
   case ('S')
      call lattice_obj%build_surf_full()
      call lattice_obj%structb(.true.)
   case ('I')
      call lattice_obj%newclu()
      call lattice_obj%structb(.true.)
   end select
   call lattice_obj%atomlist()
   call get_mpi_variables(rank, lattice_obj%njij)
   charge_obj = charge(lattice_obj)
   select case (control_obj%calctype)
   case ('B')
      call charge_obj%bulkmat()
   case ('S')
      call charge_obj%build_alelay
      call charge_obj%surfmat
   case ('I')
      call charge_obj%impmad()
   end select
   mix_obj = mix(lattice_obj, charge_obj)
   energy_obj = energy(lattice_obj)
   call energy_obj%e_mesh()
   hamiltonian_obj = hamiltonian(charge_obj)
   n = lattice_obj%ntype
   if (control_obj%calctype == 'B') n = lattice_obj%nrec
   do i = 1, n
      call lattice_obj%symbolic_atoms(i)%build_pot()
   end do
   if (control_obj%nsp == 2 .or. control_obj%nsp == 4) call hamiltonian_obj%build_lsham
   call hamiltonian_obj%build_bulkham()
   if (control_obj%calctype == 'I') call hamiltonian_obj%build_locham()
   recursion_obj = recursion(hamiltonian_obj, energy_obj)
   dos_obj = dos(recursion_obj, energy_obj)
   green_obj = green(dos_obj)
   bands_obj = bands(green_obj)
   if (trim(mode) == 'contour_plain') then
      plain_obj = exchange_plain(bands_obj)
   else
      exchange_obj = exchange(bands_obj)
   end if
   do i = 1, lattice_obj%ntype
      call lattice_obj%symbolic_atoms(i)%predls(lattice_obj%wav*ang2au)
   end do
   select case (control_obj%recur)
   case ('block')
      call recursion_obj%recur_b_ij()
   case ('chebyshev')
      call recursion_obj%chebyshev_recur_ij()
   end select
   call green_obj%calculate_intersite_gf_eta()
   if (trim(mode) == 'contour_plain') then
      call plain_obj%calculate_exchange_gauss_legendre()
   else if (trim(mode) == 'contour') then
      call exchange_obj%calculate_exchange_gauss_legendre()
   else
      stop 'contour_gpu_driver: unknown CONTOUR_DRIVER_MODE'
   end if
   etamax = 0.0_rp
   if (allocated(green_obj%gij_eta)) etamax = maxval(abs(green_obj%gij_eta))
   write (*, '(a,l1)') 'eta_arrays_allocated=', allocated(green_obj%gij_eta)
   write (*, '(a,es12.4)') 'eta_arrays_max=', etamax

   ! the occupations: an on-site recursion of the same cell (no pairs from here on), zsqr as the callers of block_green_eta run it
   lattice_obj%njij = 0
   call get_mpi_variables(rank, lattice_obj%nrec)
   select case (control_obj%recur)
   case ('block')
      call recursion_obj%recur_b()
      call recursion_obj%zsqr()
   case ('chebyshev')
      call recursion_obj%chebyshev_recur()
   end select
   if (trim(mode) == 'contour_plain') then
      bands_plain_obj = bands_plain(green_obj)
      call bands_plain_obj%calculate_moments_gauss_legendre()
      if (control_obj%recur == 'block') call bands_plain_obj%calculate_occupation_gauss_legendre(energy_obj%fermi, sumocc)
   else
      call bands_obj%calculate_moments_gauss_legendre()
      if (control_obj%recur == 'block') call bands_obj%calculate_occupation_gauss_legendre(energy_obj%fermi, sumocc)
   end if
   call g_timer%stop('Calculation')
   call g_timer%print_report()
end program contour_gpu_driver
