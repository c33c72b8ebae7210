! Fixture driver for rsrec_exchange (tools/exchange_fixture/make_fixture.py): links the compiled reference
! (oracle/_ref/librslmto_ref.a + its .mod files) and runs ITS green%calculate_intersite_gf, calculate_intersite_gf_twoindex,
! exchange%calculate_exchange and calculate_exchange_twoindex (green.f90:386-469, exchange.f90:1032-1615) for ONE pair, on inputs
! read from xc_in.bin:
!   int32 nch, same;  real(8) fermi;  real(8) ene(nch + 10);  real(8) c(0:2, 2, 2), dele(0:2, 2, 2), vmad(2), cr(3, 2);
!   complex(8) g0(18, 18, nch + 10, 4)
! (atom 1 = i, atom 2 = j of types 1 and 2; same = 1: the pair is (1, 1)).  control%recur is set to neither 'block' nor 'chebyshev', so
! calculate_intersite_gf takes green%g0 as given -- the g0 block_green_ij / chebyshev_green_ij would leave -- and skips zsqr.
! energy%ene has two more points, far above every Fermi level, so the element simpson_f reads past nch + 10 has Fermi weight 0.
! Writes xc_out.bin: real(8) jij, dmi(3), aij(3,3) after calculate_exchange; jij, dmi, aij (= the first-order values the printing loop
! leaves), jijcd, jijsd, jijcc, jijsc, dmicc(3), dmisc(3), aijsd(3,3), aijsc(3,3) after calculate_exchange_twoindex.  The reference's own
! files (jij.out ... aijparts.out, fort.150, fort.99) are written into the working directory.
program exchange_driver
   use control_mod
   use lattice_mod
   use energy_mod
   use green_mod
   use exchange_mod
   use mpi_mod, only: start_atom, end_atom, g2l_map
   use precision_mod, only: rp
   implicit none
   type(control), target :: ctl
   type(lattice), target :: lat
   type(energy), target :: en
   type(green), target :: gr
   type(exchange) :: ex
   integer :: u, nch, same, ne, t
   real(rp) :: c(0:2, 2, 2), dele(0:2, 2, 2), vmad(2), cr(3, 2)

   open (newunit=u, file='xc_in.bin', access='stream', form='unformatted', status='old')
   read (u) nch, same
   ne = nch + 10
   en%channels_ldos = nch
   en%nv1 = nch + 1
   read (u) en%fermi
   allocate (en%ene(ne + 2))
   read (u) en%ene(1:ne)
   en%ene(ne + 1:ne + 2) = 1.0e6_rp
   read (u) c, dele, vmad, cr
   ctl%recur = 'given'
   lat%control => ctl
   lat%njij = 1
   lat%ntype = 2
   allocate (lat%ijpair(1, 2), lat%iz(2), lat%cr(3, 2))
   lat%ijpair(1, 1) = 1
   lat%ijpair(1, 2) = 2
   if (same == 1) lat%ijpair(1, 2) = 1
   lat%iz = [1, 2]
   lat%cr = cr
   allocate (lat%symbolic_atoms(2))
   do t = 1, 2
      allocate (lat%symbolic_atoms(t)%potential%c(0:2, 2), lat%symbolic_atoms(t)%potential%dele(0:2, 2))
      lat%symbolic_atoms(t)%potential%c = c(:, :, t)
      lat%symbolic_atoms(t)%potential%dele = dele(:, :, t)
      lat%symbolic_atoms(t)%potential%vmad = vmad(t)
   end do
   start_atom = 1
   end_atom = 1
   allocate (g2l_map(1))
   g2l_map(1) = 1
   allocate (gr%g0(18, 18, ne, 4), gr%gij(18, 18, ne, 1), gr%gji(18, 18, ne, 1))
   read (u) gr%g0
   close (u)
   allocate (gr%ginmag(9, 9, ne, 1), gr%gjnmag(9, 9, ne, 1), gr%gix(9, 9, ne, 1), gr%giy(9, 9, ne, 1), gr%giz(9, 9, ne, 1), &
             gr%gjx(9, 9, ne, 1), gr%gjy(9, 9, ne, 1), gr%gjz(9, 9, ne, 1))
   allocate (gr%g00ij(9, 9, ne, 1), gr%g01ij(9, 9, ne, 1), gr%g00ji(9, 9, ne, 1), gr%g01ji(9, 9, ne, 1), &
             gr%gx1ij(9, 9, ne, 1), gr%gy1ij(9, 9, ne, 1), gr%gz1ij(9, 9, ne, 1), gr%gx0ij(9, 9, ne, 1), gr%gy0ij(9, 9, ne, 1), &
             gr%gz0ij(9, 9, ne, 1), gr%gx1ji(9, 9, ne, 1), gr%gy1ji(9, 9, ne, 1), gr%gz1ji(9, 9, ne, 1), gr%gx0ji(9, 9, ne, 1), &
             gr%gy0ji(9, 9, ne, 1), gr%gz0ji(9, 9, ne, 1))
   gr%control => ctl
   gr%lattice => lat
   gr%en => en
   gr%symbolic_atom => lat%symbolic_atoms
   call gr%calculate_intersite_gf()
   call gr%calculate_intersite_gf_twoindex()
   ex%green => gr
   ex%lattice => lat
   ex%en => en
   ex%control => ctl
   ex%symbolic_atom => lat%symbolic_atoms
   open (newunit=u, file='xc_out.bin', access='stream', form='unformatted', status='replace')
   call ex%calculate_exchange()
   write (u) ex%jij, ex%dmi, ex%aij
   call ex%calculate_exchange_twoindex()
   write (u) ex%jij, ex%dmi, ex%aij, ex%jijcd, ex%jijsd, ex%jijcc, ex%jijsc, ex%dmicc, ex%dmisc, ex%aijsd, ex%aijsc
   close (u)
end program exchange_driver
