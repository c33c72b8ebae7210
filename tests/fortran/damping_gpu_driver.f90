!------------------------------------------------------------------------------
! damping_gpu_driver -- the exchange post-processing up to the pair recursion (the call sequence of calculation.f90:816-940), then the
! routines of type(exchange) that the reference's main program leaves commented out (:945-947).
!
! Built by fortran/build_dropin.sh on the object set of the zero-edit drop-in: every `type(x)` below is the GPU type behind the
! reference's module name (fortran/shadow/), and `exchange_plain` is the reference's own type(exchange), compiled unchanged under the
! module name exchange_ref_mod.  Run inside a scratch copy of a case directory; reads input.nml.
!
! DAMPING_DRIVER_MODE (environment):
!   damping         (default) calculate_gilbert_damping on a type(exchange_gpu); prints `host_intersite_allocated=`, then dumps what a
!                   restatement needs to damping_dump.bin (stream, native): nen, npairs, ntype, ene, fermi, ijpair, iz and lmax of both
!                   atoms and ql(1, 0:2, 1:2) of atom i per pair, tmat, and g0(18,18,nen,4) of every pair from green%block_green_ij
!   auxgreen        calculate_jij_auxgreen on the type(exchange_gpu)
!   auxgreen_plain  calculate_jij_auxgreen on the reference's type(exchange) over the same GPU objects (the host intersite stage runs)
!------------------------------------------------------------------------------
program damping_gpu_driver
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
   integer :: i, p, elen, estat, n, at, side
   real(rp) :: ql(3, 2)

   rank = 0
   numprocs = 1
   g_timer = timer()
   call g_timer%start('Calculation')
   call get_environment_variable('DAMPING_DRIVER_MODE', mode, elen, estat)
   if (estat /= 0 .or. elen == 0) mode = 'damping'

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
   if (trim(mode) == 'auxgreen_plain') then
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
   case ('damping')
      call exchange_obj%calculate_gilbert_damping()
      write (*, '(a,l1)') 'host_intersite_allocated=', allocated(green_obj%gij)
      open (unit=77, file='damping_dump.bin', access='stream', form='unformatted', status='replace')
      write (77) int(size(green_obj%g0, 3)), int(lattice_obj%njij), int(lattice_obj%ntype)
      write (77) energy_obj%ene(1:size(green_obj%g0, 3)), energy_obj%fermi
      do p = 1, lattice_obj%njij
         write (77) int(lattice_obj%ijpair(p, 1)), int(lattice_obj%ijpair(p, 2))
         do side = 1, 2
            at = lattice_obj%iz(lattice_obj%ijpair(p, side))
            write (77) int(at), int(lattice_obj%symbolic_atoms(at)%potential%lmax)
         end do
         at = lattice_obj%iz(lattice_obj%ijpair(p, 1))
         ql = 0.0_rp
         do i = 0, min(2, lattice_obj%symbolic_atoms(at)%potential%lmax)
            ql(i + 1, :) = lattice_obj%symbolic_atoms(at)%potential%ql(1, i, 1:2)
         end do
         write (77) ql
      end do
      write (77) hamiltonian_obj%tmat(:, :, :, 1:lattice_obj%ntype)
      do p = 1, lattice_obj%njij
         if (control_obj%recur == 'block') then
            call green_obj%block_green_ij(4*(p - 1) + 1)
         else
            call green_obj%chebyshev_green_ij(4*(p - 1) + 1)
         end if
         write (77) green_obj%g0(:, :, :, 1:4)
      end do
      close (77)
   case ('auxgreen')
      call exchange_obj%calculate_jij_auxgreen()
      write (*, '(a,l1)') 'host_intersite_allocated=', allocated(green_obj%gij)
   case ('auxgreen_plain')
      call plain_obj%calculate_jij_auxgreen()
      write (*, '(a,l1)') 'host_intersite_allocated=', allocated(green_obj%gij)
   case default
      stop 'damping_gpu_driver: unknown DAMPING_DRIVER_MODE'
   end select
   call g_timer%stop('Calculation')
   call g_timer%print_report()
end program damping_gpu_driver
