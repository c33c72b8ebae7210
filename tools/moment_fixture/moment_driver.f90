! Fixture driver for rsrec_spectra_integrals (tools/moment_fixture/make_fixture.py): links the compiled reference
! (oracle/_ref/librslmto_ref.a + its .mod files) and calls ITS math_mod::simpson_f (math.f90:1600-1632, fermi = .true., T = 0) for every
! series and every limit EF = ene(i), and ITS math_mod::simpson_m (math.f90:1579-1598) for every series, every Fermi-level case and
! nexp = 0, 1, 2, on inputs read from moment_in.bin:
!   int32 nen, nv1, nser, ncase;  real(8) edel;  real(8) ene(nen);  real(8) y(nen, nser);
!   per case: int32 npts;  real(8) e1, fermi
! simpson_f's loop I = 2, nv1 + 9, 2 reads Y(I + 1) and Ene(I + 1) up to element nv1 + 10.  Both arrays are held with
! max(nen, nv1 + 10) elements here, the padding zero, so the compiled reference reads nothing undefined; simpson_m reads up to
! element npts + 2 <= nen.
! Writes moment_out.bin: real(8) cum(nen, nser), cum(i, s) = simpson_f(.., EF = ene(i), nv1, y(:, s), .true., .false., 0);
!                        real(8) mom(3, nser, ncase), mom(p + 1, s, c) = simpson_m(.., edel, fermi_c, npts_c, y(:, s), e1_c, p, ene).
program moment_driver
   use math_mod, only: simpson_f, simpson_m
   use precision_mod, only: rp
   implicit none
   integer :: u, nen, nv1, nser, ncase, npad, i, s, c, p
   real(rp) :: edel
   integer, allocatable :: npts(:)
   real(rp), allocatable :: ene(:), y(:, :), cum(:, :), mom(:, :, :), e1(:), fermi(:)

   open (newunit=u, file='moment_in.bin', access='stream', form='unformatted', status='old')
   read (u) nen, nv1, nser, ncase
   read (u) edel
   npad = max(nen, nv1 + 10)
   allocate (ene(npad), y(npad, nser), cum(nen, nser), mom(3, nser, ncase), npts(ncase), e1(ncase), fermi(ncase))
   ene = 0.0_rp
   y = 0.0_rp
   read (u) ene(1:nen)
   do s = 1, nser
      read (u) y(1:nen, s)
   end do
   do c = 1, ncase
      read (u) npts(c)
      read (u) e1(c), fermi(c)
   end do
   close (u)
   do s = 1, nser
      do i = 1, nen
         call simpson_f(cum(i, s), ene, ene(i), nv1, y(:, s), .true., .false., 0.0_rp)
      end do
   end do
   do c = 1, ncase
      do s = 1, nser
         do p = 0, 2
            call simpson_m(mom(p + 1, s, c), edel, fermi(c), npts(c), y(:, s), e1(c), p, ene)
         end do
      end do
   end do
   open (newunit=u, file='moment_out.bin', access='stream', form='unformatted', status='replace')
   write (u) cum
   write (u) mom
   close (u)
end program moment_driver
