!------------------------------------------------------------------------------
! jijk_gpu_driver -- the exchange post-processing up to the pair recursion and the intersite stage (the call sequence of
! calculation.f90:816-940) on an input with njijk trios, then exchange%calculate_jijk, which the reference's main program leaves
! commented out.
!
! Built by fortran/build_dropin.sh on the object set of the zero-edit drop-in, as damping_gpu_driver.f90: every `type(x)` below is the
! GPU type behind the reference's module name, and `exchange_plain` is the reference's own type(exchange).  Run inside a scratch copy of
! a case directory; reads input.nml.
!
! JIJK_DRIVER_MODE (environment):
!   gpu    (default) calculate_jijk on a type(exchange_gpu): one rsrec_spin_lattice call (timer region jijk-gpu)
!   plain  calculate_jijk on the reference's type(exchange) over the same GPU objects (the host intersite stage runs; timer region
!          jijk-plain around the routine)
! Both print `host_intersite_allocated=` afterwards.
!------------------------------------------------------------------------------
program jijk_gpu_driver
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
   character(len=32) :: mode
   integer :: i, elen, estat, n

   rank = 0
   numprocs = 1
   g_timer = timer()
   call g_timer%start('Calculation')
   call get_environment_variable('JIJK_DRIVER_MODE', mode, elen, estat)
   if (estat /= 0 .or. elen == 0) mode = 'gpu'

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
   if (trim(mode) == 'plain') then
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
   call green_obj%calculate_intersite_gf()
   call green_obj%calculate_intersite_gf_twoindex()

   select case (trim(mode))
   case ('gpu')
      call exchange_obj%calculate_jijk()
      write (*, '(a,l1)') 'host_intersite_allocated=', allocated(green_obj%gij)
   case ('plain')
      call g_timer%start('jijk-plain')
      call plain_obj%calculate_jijk()
      call g_timer%stop('jijk-plain')
      write (*, '(a,l1)') 'host_intersite_allocated=', allocated(green_obj%gij)
   case default
      stop 'jijk_gpu_driver: unknown JIJK_DRIVER_MODE'
   end select
   call g_timer%stop('Calculation')
   call g_timer%print_report()
end program jijk_gpu_driver
