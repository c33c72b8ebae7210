! Fixture driver for rsrec_kubo_conductivity (tools/cond_tensor_fixture/make_fixture.py): links the compiled reference
! (oracle/_ref/librslmto_ref.a + its .mod files) and calls ITS math_mod::simpson_f (math.f90:1600-1632) with fermi = .true. for every
! series and every limit EF = x(i), on inputs read from simpson_in.bin:
!   int32 nen, nv1, nser;  real(8) T;  real(8) x(nen);  real(8) y(nen, nser)
! simpson_f's loop I = 2, nv1 + 9, 2 reads Y(I + 1) and Ene(I + 1) up to element nv1 + 10.  Both arrays are held with
! max(nen, nv1 + 10) elements here, the padding zero, so the compiled reference reads nothing undefined.
! Writes simpson_out.bin: real(8) aint(nen, nser), aint(i, s) = simpson_f(.., EF = x(i), .., y(:, s), .true., .false., T).
program simpson_driver
   use math_mod, only: simpson_f
   use precision_mod, only: rp
   implicit none
   integer :: u, nen, nv1, nser, npad, i, s
   real(rp) :: T
   real(rp), allocatable :: x(:), y(:, :), aint(:, :)

   open (newunit=u, file='simpson_in.bin', access='stream', form='unformatted', status='old')
   read (u) nen, nv1, nser
   read (u) T
   npad = max(nen, nv1 + 10)
   allocate (x(npad), y(npad, nser), aint(nen, nser))
   x = 0.0_rp
   y = 0.0_rp
   read (u) x(1:nen)
   do s = 1, nser
      read (u) y(1:nen, s)
   end do
   close (u)
   do s = 1, nser
      do i = 1, nen
         call simpson_f(aint(i, s), x, x(i), nv1, y(:, s), .true., .false., T)
      end do
   end do
   open (newunit=u, file='simpson_out.bin', access='stream', form='unformatted', status='replace')
   write (u) aint
   close (u)
end program simpson_driver
