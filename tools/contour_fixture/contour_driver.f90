! Fixture driver for rsrec_exchange_contour / rsrec_contour_occupation (tools/contour_fixture/make_fixture.py): links the compiled
! reference (oracle/_ref/librslmto_ref.a + its .mod files) and runs ITS green%calculate_intersite_gf_eta (green.f90:471-536),
! exchange%calculate_exchange_gauss_legendre (exchange.f90:1756-1919), recursion%get_terminf and green%block_green_eta /
! chebyshev_green_eta (green.f90:544-581, :1116-1184) for ONE pair, on inputs read from ct_in.bin:
!   int32 kind (0 block, 1 Chebyshev), lld, channels_ldos, sym_term;  real(8) fermi, energy_min, energy_max;
!   complex(8) ee(18, 18, 1, 2);  real(8) cr(3, 2);
!   block: complex(8) a_b(18, 18, lld, 4), b2_b(18, 18, lld, 4) BEFORE zsqr (calculate_intersite_gf_eta calls zsqr itself);
!   Chebyshev: complex(8) mu_n(18, 18, 2 lld + 2, 4)
! (atom 1 = i of type 1, atom 2 = j of type 2).  control%fname names an empty file, so energy%e_mesh keeps the members set here.
! Writes ct_out.bin: real(8) x(64), w(64); int32 nen, fermi_point; real(8) ene(nen); complex(8) gij_eta(64,18,18), gji_eta(64,18,18);
! real(8) jij, dmi(3), aij(3,3) (the scaled values the routine leaves in its members after its one pair = T_comm_xc);
! block: complex(8) b_sqrt(18,18,lld,4); real(8) a_inf(18,18,4), b_inf(18,18,4);
! complex(8) gdiag(18, 64, 4): the diagonal of block_green_eta / chebyshev_green_eta of the four chains taken as four sites.
program contour_driver
   use control_mod
   use lattice_mod
   use energy_mod
   use hamiltonian_mod
   use recursion_mod
   use green_mod
   use exchange_mod
   use math_mod, only: gauss_legendre
   use mpi_mod, only: start_atom, end_atom, g2l_map, atoms_per_process
   use precision_mod, only: rp
   implicit none
   type(control), target :: ctl
   type(lattice), target :: lat
   type(energy), target :: en
   type(hamiltonian), target :: ham
   type(recursion), target :: rec
   type(green), target :: gr
   type(exchange) :: ex
   integer :: u, kind, lld, nch, isym, i, k, fermi_point, nm
   real(rp) :: cr(3, 2), x(64), w(64), a_inf(18, 18, 4), b_inf(18, 18, 4), a0(4), b0(4)
   complex(rp) :: eta, g_ef(18, 18, 4), gd(18, 64, 4)
   integer :: nw

   open (newunit=u, file='ct_in.bin', access='stream', form='unformatted', status='old')
   read (u) kind, lld, nch, isym
   read (u) en%fermi, en%energy_min, en%energy_max
   en%channels_ldos = nch
   allocate (ham%ee(18, 18, 1, 2))
   read (u) ham%ee, cr
   ctl%lld = lld
   ctl%sym_term = isym /= 0
   ctl%fname = 'input.nml'
   ctl%recur = 'block'
   if (kind == 1) ctl%recur = 'chebyshev'
   nm = 2*lld + 2
   if (kind == 0) then
      allocate (rec%a_b(18, 18, lld, 4), rec%b2_b(18, 18, lld, 4))
      read (u) rec%a_b, rec%b2_b
   else
      allocate (rec%mu_n(18, 18, nm, 4), rec%mu_ng(18, 18, nm, 4))
      read (u) rec%mu_n
      rec%mu_ng = (0.0_rp, 0.0_rp)
   end if
   close (u)
   lat%control => ctl
   lat%njij = 1
   lat%ntype = 2
   lat%nrec = 1
   allocate (lat%ijpair(1, 2), lat%iz(2), lat%cr(3, 2))
   lat%ijpair(1, 1) = 1
   lat%ijpair(1, 2) = 2
   lat%iz = [1, 2]
   lat%cr = cr
   en%lattice => lat
   rec%lattice => lat
   start_atom = 1
   end_atom = 1
   atoms_per_process = 1
   allocate (g2l_map(4))
   g2l_map = [1, 2, 3, 4]
   gr%control => ctl
   gr%lattice => lat
   gr%en => en
   gr%recursion => rec
   allocate (gr%gij_eta(64, 18, 18, 1), gr%gji_eta(64, 18, 18, 1), gr%ginmag_eta(64, 9, 9, 1), gr%gjnmag_eta(64, 9, 9, 1), &
             gr%gix_eta(64, 9, 9, 1), gr%giy_eta(64, 9, 9, 1), gr%giz_eta(64, 9, 9, 1), gr%gjx_eta(64, 9, 9, 1), &
             gr%gjy_eta(64, 9, 9, 1), gr%gjz_eta(64, 9, 9, 1))
   call gr%calculate_intersite_gf_eta()
   ex%green => gr
   ex%lattice => lat
   ex%en => en
   ex%control => ctl
   ex%hamiltonian => ham
   call gauss_legendre(64, 0.0_rp, 1.0_rp, x, w)
   do i = 1, en%channels_ldos + 10
      if ((en%ene(i) - en%fermi) .le. 0.000001d0) fermi_point = i
   end do
   open (newunit=u, file='ct_out.bin', access='stream', form='unformatted', status='replace')
   write (u) x, w, size(en%ene), fermi_point
   write (u) en%ene
   write (u) gr%gij_eta(:, :, :, 1), gr%gji_eta(:, :, :, 1)
   call ex%calculate_exchange_gauss_legendre()
   write (u) ex%jij, ex%dmi, ex%aij
   ! the four chains as four sites (b2_b is square-rooted by now: block_green_eta's callers run zsqr before it)
   atoms_per_process = 4
   end_atom = 4
   lat%nrec = 4
   if (kind == 0) then
      nw = 10*lld
      call rec%get_terminf(rec%a_b, rec%b2_b, 4, lld, 18, nw, a_inf, b_inf, a0, b0)
      write (u) rec%b2_b, a_inf, b_inf
   end if
   do k = 1, 64
      eta = cmplx(0.0_rp, (1 - x(k))/x(k))          ! no KIND, as bands.f90:563 writes it: default (single-precision) complex
      g_ef = (0.0_rp, 0.0_rp)
      if (kind == 0) then
         call gr%block_green_eta(eta, fermi_point, g_ef)
      else
         call gr%chebyshev_green_eta(eta, fermi_point, g_ef)
      end if
      do i = 1, 18
         gd(i, k, :) = g_ef(i, i, :)
      end do
   end do
   write (u) gd
   close (u)
end program contour_driver
