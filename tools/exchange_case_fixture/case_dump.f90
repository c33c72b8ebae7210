! Fixture dump for the drop-in exchange cases (tools/exchange_case_fixture/make_fixture.py): links the compiled reference
! (oracle/_ref/librslmto_ref.a + its .mod files) and replays post_processing_exchange (calculation.f90:816-941) up to the reference's
! own pair recursion -- recur_b_ij (then zsqr, as calculate_intersite_gf does first, green.f90:434) or chebyshev_recur_ij -- on the
! input.nml of the working directory.  Writes case.bin (stream, little endian):
!   int32 kk, nncols, ntype, nslots, njij, lld, nsp, hoh, kind (0 block, 1 Chebyshev), channels_ldos, nv1
!   real(8) fermi, energy_min, energy_max;  real(8) ene(channels_ldos + 10)
!   int32 iz(kk), nn(kk, nncols), ijpair(njij, 2);  real(8) cr(3, kk)
!   complex(8) ee(18,18,nslots,ntype), lsham(18,18,ntype), eeo(18,18,nslots,ntype), enim(18,18,ntype)
!   real(8) per type: c(0:2, 2), dele(0:2, 2), vmad   (after predls, the values d_matrix reads)
!   block: complex(8) a_b(18,18,lld,4 njij), b2_b(18,18,lld,4 njij) after zsqr;  Chebyshev: mu_n(18,18,2 lld + 2,4 njij)
program case_dump
   use mpi_mod
   use control_mod
   use lattice_mod
   use charge_mod
   use energy_mod
   use hamiltonian_mod
   use recursion_mod
   use precision_mod, only: rp
   use math_mod, only: ang2au
   implicit none
   type(control), target :: control_obj
   type(lattice), target :: lattice_obj
   type(energy), target :: energy_obj
   type(charge), target :: charge_obj
   type(hamiltonian), target :: hamiltonian_obj
   type(recursion), target :: recursion_obj
   integer :: i, u, kind_rec, hoh_i

   control_obj = control('input.nml')
   lattice_obj = lattice(control_obj)
   call lattice_obj%build_data()
   call lattice_obj%bravais()
   call lattice_obj%structb(.true.)
   call lattice_obj%atomlist()
   call get_mpi_variables(rank, lattice_obj%njij)
   charge_obj = charge(lattice_obj)
   call charge_obj%bulkmat()
   energy_obj = energy(lattice_obj)
   call energy_obj%e_mesh()
   hamiltonian_obj = hamiltonian(charge_obj)
   do i = 1, lattice_obj%nrec
      call lattice_obj%symbolic_atoms(i)%build_pot()
   end do
   if (control_obj%nsp == 2 .or. control_obj%nsp == 4) call hamiltonian_obj%build_lsham
   call hamiltonian_obj%build_bulkham()
   recursion_obj = recursion(hamiltonian_obj, energy_obj)
   do i = 1, lattice_obj%ntype
      call lattice_obj%symbolic_atoms(i)%predls(lattice_obj%wav*ang2au)
   end do
   select case (control_obj%recur)
   case ('block')
      kind_rec = 0
      call recursion_obj%recur_b_ij()
      call recursion_obj%zsqr()
   case ('chebyshev')
      kind_rec = 1
      call recursion_obj%chebyshev_recur_ij()
   case default
      stop 'case_dump: recur must be block or chebyshev'
   end select
   hoh_i = 0
   if (hamiltonian_obj%hoh) hoh_i = 1

   open (newunit=u, file='case.bin', access='stream', form='unformatted', status='replace')
   write (u) lattice_obj%kk, size(lattice_obj%nn, 2), lattice_obj%ntype, size(hamiltonian_obj%ee, 3), lattice_obj%njij, &
      control_obj%lld, control_obj%nsp, hoh_i, kind_rec, energy_obj%channels_ldos, energy_obj%nv1
   write (u) energy_obj%fermi, energy_obj%energy_min, energy_obj%energy_max
   write (u) energy_obj%ene(1:energy_obj%channels_ldos + 10)
   write (u) lattice_obj%iz(1:lattice_obj%kk)
   write (u) lattice_obj%nn
   write (u) lattice_obj%ijpair
   write (u) lattice_obj%cr(1:3, 1:lattice_obj%kk)
   write (u) hamiltonian_obj%ee, hamiltonian_obj%lsham, hamiltonian_obj%eeo, hamiltonian_obj%enim
   do i = 1, lattice_obj%ntype
      write (u) lattice_obj%symbolic_atoms(i)%potential%c(0:2, 1:2), lattice_obj%symbolic_atoms(i)%potential%dele(0:2, 1:2), &
         lattice_obj%symbolic_atoms(i)%potential%vmad
   end do
   if (kind_rec == 0) then
      write (u) recursion_obj%a_b(:, :, 1:control_obj%lld, 1:4*lattice_obj%njij), recursion_obj%b2_b(:, :, 1:control_obj%lld, 1:4*lattice_obj%njij)
   else
      write (u) recursion_obj%mu_n(:, :, 1:2*control_obj%lld + 2, 1:4*lattice_obj%njij)
   end if
   close (u)
end program case_dump
