! Fixture driver for the conductivity integrand (tools/cond_fixture/make_fixture.py): links the compiled reference
! (oracle/_ref/librslmto_ref.a + its .mod files) and runs ITS calculate_gamma_nm and calculate_conductivity_tensor
! (conductivity.f90:158-376) on synthetic inputs read from cond_in.bin:
!   int32 cond_ll, nvec, channels_ldos, calctype (1 = 'per_type', 2 = 'random_vec');  real(8) energy_min, energy_max, fermi;
!   real(8) ene(channels_ldos + 10);  complex(8) mu_nm_stochastic(18, 18, cond_ll, cond_ll, nvec)
! and writes gamma_nm (channels_ldos + 10, cond_ll, cond_ll) to cond_gamma.bin.  calculate_conductivity_tensor writes fort.123 and the
! cond_*.out files into the working directory.  No object is built from an input file: the pointers of type(conductivity) are set to
! objects that carry just what those two routines read.
program cond_driver
   use control_mod
   use lattice_mod
   use energy_mod
   use recursion_mod
   use conductivity_mod
   use precision_mod, only: rp
   implicit none
   type(control), target :: ctl
   type(lattice), target :: lat
   type(energy), target :: en
   type(recursion), target :: rec
   type(conductivity) :: cond
   integer :: u, ll, nvec, nch, ctype, i
   real(rp) :: emin, emax, ef

   open (newunit=u, file='cond_in.bin', access='stream', form='unformatted', status='old')
   read (u) ll, nvec, nch, ctype
   read (u) emin, emax, ef
   ctl%cond_ll = ll
   ctl%random_vec_num = nvec
   if (ctype == 1) then
      ctl%cond_calctype = 'per_type'
   else
      ctl%cond_calctype = 'random_vec'
   end if
   lat%control => ctl
   lat%ntype = nvec
   lat%a = 0.0_rp
   lat%a(1, 1) = 1.0_rp; lat%a(2, 2) = 1.0_rp; lat%a(3, 3) = 1.0_rp
   allocate (lat%symbolic_atoms(nvec))
   do i = 1, nvec
      write (lat%symbolic_atoms(i)%element%symbol, '(a,i0)') 'T', i
   end do
   en%channels_ldos = nch
   en%nv1 = nch + 1
   en%energy_min = emin
   en%energy_max = emax
   en%fermi = ef
   allocate (en%ene(nch + 10))
   read (u) en%ene
   allocate (rec%mu_nm_stochastic(18, 18, ll, ll, nvec))
   read (u) rec%mu_nm_stochastic
   close (u)
   cond%control => ctl
   cond%lattice => lat
   cond%en => en
   cond%recursion => rec
   call cond%calculate_gamma_nm()
   open (newunit=u, file='cond_gamma.bin', access='stream', form='unformatted', status='replace')
   write (u) cond%gamma_nm
   close (u)
   call cond%calculate_conductivity_tensor()
end program cond_driver
