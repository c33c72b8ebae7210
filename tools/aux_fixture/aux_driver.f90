! Fixture driver for rsrec_exchange_aux / rsrec_spin_lattice (tools/aux_fixture/make_fixture.py): links the compiled reference
! (oracle/_ref/librslmto_ref.a + its .mod files) and runs ITS green%calculate_intersite_gf (per pair), exchange%calculate_jij_auxgreen and
! exchange%calculate_jijk (exchange.f90:171-601, green.f90:758-885, symbolic_atom.f90:274-472) on inputs read from aux_in.bin:
!   int32 nch, npairs, ntrio (0 or 1);  int32 pairs(npairs, 2);  real(8) fermi, wav, disp(3);  real(8) ene(nch + 10);
!   real(8) c(0:2, 2, 3), dele(0:2, 2, 3), qpar(0:2, 2, 3), vmad(3);  complex(8) g0(18, 18, nch + 10, 4 npairs)
! Atoms 1, 2, 3 are of types 1, 2, 3.  ntrio = 1: the pairs are the trio's (i,j), (i,k), (j,k) and calculate_jijk runs; ntrio = 0:
! calculate_jij_auxgreen runs on the pairs (its members keep the last i /= j and the last i == j pair's values).
! control%recur is neither 'block' nor 'chebyshev', so calculate_intersite_gf takes green%g0 as given; it is called once per pair with
! that pair's four chains in g0.  energy%ene has two more points far above every Fermi level (the Green functions there are zero), so
! the element simpson_f reads past nch + 10 has Fermi weight 0.
! Writes aux_out.bin: real(8) jij_aux(9), jij00_aux, jijk(9);  complex(8) dmat(18, 18) = disp_matrix for disp.
program aux_driver
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
   integer :: u, nch, npairs, ntrio, ne, t, p
   integer, allocatable :: pairs(:, :)
   real(rp) :: c(0:2, 2, 3), dele(0:2, 2, 3), qpar(0:2, 2, 3), vmad(3), disp(3), wav
   complex(rp), allocatable :: g0(:, :, :, :), sij(:, :, :, :), sji(:, :, :, :), dmat(:, :)

   open (newunit=u, file='aux_in.bin', access='stream', form='unformatted', status='old')
   read (u) nch, npairs, ntrio
   allocate (pairs(npairs, 2))
   read (u) pairs
   ne = nch + 10
   en%channels_ldos = nch
   en%nv1 = nch + 1
   read (u) en%fermi, wav, disp
   allocate (en%ene(ne + 2))
   read (u) en%ene(1:ne)
   en%ene(ne + 1:ne + 2) = 1.0e6_rp
   read (u) c, dele, qpar, vmad
   allocate (g0(18, 18, ne, 4*npairs))
   read (u) g0
   close (u)
   ctl%recur = 'given'
   lat%control => ctl
   lat%njij = npairs
   lat%njijk = ntrio
   lat%ntype = 3
   lat%wav = wav
   allocate (lat%ijpair(npairs, 2), lat%iz(3), lat%ijktrio(max(ntrio, 1), 6))
   lat%ijpair = pairs
   lat%iz = [1, 2, 3]
   lat%ijktrio(1, 1:3) = 1.0_rp
   if (ntrio == 1) lat%ijktrio(1, 1:3) = [real(pairs(1, 1), rp), real(pairs(1, 2), rp), real(pairs(2, 2), rp)]
   lat%ijktrio(1, 4:6) = disp
   allocate (lat%symbolic_atoms(3))
   do t = 1, 3
      allocate (lat%symbolic_atoms(t)%potential%c(0:2, 2), lat%symbolic_atoms(t)%potential%dele(0:2, 2), &
                lat%symbolic_atoms(t)%potential%qpar(0:2, 2))
      lat%symbolic_atoms(t)%potential%lmax = 2
      lat%symbolic_atoms(t)%potential%c = c(:, :, t)
      lat%symbolic_atoms(t)%potential%dele = dele(:, :, t)
      lat%symbolic_atoms(t)%potential%qpar = qpar(:, :, t)
      lat%symbolic_atoms(t)%potential%vmad = vmad(t)
   end do
   allocate (g2l_map(npairs))
   allocate (gr%g0(18, 18, ne + 2, 4), gr%gij(18, 18, ne + 2, npairs), gr%gji(18, 18, ne + 2, npairs))
   allocate (sij(18, 18, ne + 2, npairs), sji(18, 18, ne + 2, npairs))
   allocate (gr%ginmag(9, 9, ne + 2, npairs), gr%gjnmag(9, 9, ne + 2, npairs), gr%gix(9, 9, ne + 2, npairs), gr%giy(9, 9, ne + 2, npairs), &
             gr%giz(9, 9, ne + 2, npairs), gr%gjx(9, 9, ne + 2, npairs), gr%gjy(9, 9, ne + 2, npairs), gr%gjz(9, 9, ne + 2, npairs))
   gr%control => ctl
   gr%lattice => lat
   gr%en => en
   gr%symbolic_atom => lat%symbolic_atoms
   do p = 1, npairs
      g2l_map(p) = p
      start_atom = p
      end_atom = p
      gr%g0 = (0.0_rp, 0.0_rp)
      gr%g0(:, :, 1:ne, :) = g0(:, :, :, 4*p - 3:4*p)
      call gr%calculate_intersite_gf()
      sij(:, :, :, p) = gr%gij(:, :, :, p)
      sji(:, :, :, p) = gr%gji(:, :, :, p)
   end do
   gr%gij = sij
   gr%gji = sji
   ex%green => gr
   ex%lattice => lat
   ex%en => en
   ex%control => ctl
   ex%symbolic_atom => lat%symbolic_atoms
   ex%jij_aux = 0.0_rp
   ex%jij00_aux = 0.0_rp
   ex%jijk = 0.0_rp
   if (ntrio == 1) then
      call ex%calculate_jijk()
   else
      call ex%calculate_jij_auxgreen()
   end if
   allocate (dmat(18, 18))
   dmat = (0.0_rp, 0.0_rp)
   call lat%symbolic_atoms(3)%disp_matrix(dmat, disp, 2, wav)
   open (newunit=u, file='aux_out.bin', access='stream', form='unformatted', status='replace')
   write (u) ex%jij_aux, ex%jij00_aux, ex%jijk
   write (u) dmat
   close (u)
end program aux_driver
