!------------------------------------------------------------------------------
! conductivity_gpu_mod -- GPU drop-in for type(conductivity) (conductivity.f90:47-72).
!
! The energy-resolved Kubo-Bastin integrand that calculate_gamma_nm (:158-225) + the loops of calculate_conductivity_tensor
! (:259-281) form on the host through the complex (channels_ldos + 10, cond_ll, cond_ll) array gamma_nm (10 GB at cond_ll = 500) is
! one call of librsrec, rsrec_kubo_integrand, on the per-process device context (rsrec_context_mod); the sum factorises and no
! array of that size exists anywhere (rslmtoasa_amd/csrc/kernels_cond.hpp).  So:
!   calculate_gamma_nm            : allocates nothing (the tables it would fill are built on the device per call)
!   calculate_conductivity_tensor : the device integrand, then the reference's tail (:283-372): the sums over the vectors and the
!                                   orbitals and the 38 (1 + ntype) nE Fermi-weighted Simpson integrals are one more call,
!                                   rsrec_kubo_conductivity (region conductivity-tensor-gpu); the host writes the same files in the same
!                                   formats (fort.123, cond_total*.out, <symbol>_cond*.out with 'per_type').  The device rule takes the
!                                   element simpson_f reads past its arrays as zero (include/rsrec.h).
!                                   RSREC_HOST_COND_TAIL set in the environment: the tail restated line for line on the host instead, with
!                                   simpson_f of math_mod as it is, the stray read included (region conductivity-tensor-host).
!                                   RSREC_KUBO_RESPONSES (recursion_gpu): the recursion formed the moments of further responses to the
!                                   same field; the integrand of all of them is one call, and the tail runs once per response -- the
!                                   namelist's response writes the files above, further response <op> the same files as <op>_fort.123,
!                                   <op>_cond_total*.out, <op>_<symbol>_cond*.out.
!                                   RSREC_KUBO_FIELDS (recursion_gpu): likewise for further applied-field directions -- every (response,
!                                   field) pair is one more set of the same integrand call and one more pass of the tail; the files of
!                                   further field f carry 'E<f>_' before whatever the set is called otherwise (Ey_fort.123,
!                                   Ey_cond_total.out, Ey_spin_cond_total.out, Ey_<symbol>_cond.out).
!                                   RSREC_KUBO_OPTICAL=<nw>: after the DC tensor, the optical conductivity sigma(omega_k), omega_k = k edel,
!                                   k = 1 .. nw, at energy%fermi and T = 0 from the orbital diagonals of mu_nm_stochastic
!                                   (rsrec_kubo_optical, region conductivity-optical-gpu) -> optical_cond.out: omega_k, then Re and Im of
!                                   the sum over orbitals and vectors divided by loop_over, in cond_total.out's format.  Unset: nothing
!                                   of this runs.  RSREC_KUBO_OPTICAL_MOMENTS=<file> beside it: the diagonals that call was given,
!                                   complex (18, cond_ll, cond_ll, loop_over), as a stream of raw bytes (for checking the file).
! Errors of the library become g_logger%fatal, the reference's error behaviour on this path.
!------------------------------------------------------------------------------
module conductivity_gpu_mod
   use, intrinsic :: iso_c_binding
   use conductivity_mod
   use self_mod, only: self
   use precision_mod, only: rp
   use string_mod, only: sl
   use math_mod, only: pi, cross_product, simpson_f
   use logger_mod, only: g_logger
   use timer_mod, only: g_timer
   use rsrec_binding
   use rsrec_context_mod, only: rsrec_gpu_context, rsrec_env_flag
   use recursion_gpu_mod, only: rsrec_gpu_kubo_diag_resident, rsrec_gpu_kubo_responses, rsrec_gpu_kubo_response_name, rsrec_gpu_kubo_response_diag
   implicit none

   private

   type, public, extends(conductivity) :: conductivity_gpu
   contains
      procedure :: calculate_gamma_nm => gpu_calculate_gamma_nm
      procedure :: calculate_conductivity_tensor => gpu_calculate_conductivity_tensor
   end type conductivity_gpu

   interface conductivity_gpu
      procedure :: gpu_constructor
   end interface conductivity_gpu

contains

   !> constructor (:87-100)
   function gpu_constructor(self_obj) result(obj)
      type(conductivity_gpu) :: obj
      class(self), target, intent(in) :: self_obj

      obj%self => self_obj
      obj%control => self_obj%control
      obj%lattice => self_obj%lattice
      obj%en => self_obj%en
      obj%recursion => self_obj%recursion

      call obj%restore_to_default()
      call obj%build_from_file()
   end function gpu_constructor

   !> calculate_gamma_nm (:158-225): nothing to do -- gamma_nm is never formed (calculate_conductivity_tensor below)
   subroutine gpu_calculate_gamma_nm(this)
      class(conductivity_gpu), intent(inout) :: this
      if (allocated(this%gamma_nm)) deallocate (this%gamma_nm)
   end subroutine gpu_calculate_gamma_nm

   subroutine gpu_calculate_conductivity_tensor(this)
      class(conductivity_gpu), intent(inout) :: this
      integer :: loop_over, nen, nresp, j, nw_opt
      integer(c_int) :: rc
      type(c_ptr) :: ctx
      complex(rp), dimension(:, :, :), allocatable, target :: integ           ! (18, nen, loop_over): integrand_at(l2, l2, :, v), factor applied;
                                                                              ! further responses: loop_over more vectors each
      character(len=sl) :: prefix
      real(rp), dimension(:), allocatable :: wscale
      real(rp), dimension(:), allocatable, target :: ene
      real(rp) :: a, b, factor, volume, de

      nen = this%en%channels_ldos + 10
      ! :238-241, :249-252
      a = (this%en%energy_max - this%en%energy_min)/(2 - 0.3)
      b = (this%en%energy_max + this%en%energy_min)/2
      de = this%en%energy_max - this%en%energy_min
      allocate (wscale(nen), ene(nen))
      ene(:) = this%en%ene(1:nen)
      wscale(:) = (this%en%ene(:) - b)/a

      ! :254-259
      select case (this%control%cond_calctype)
      case ('per_type')
         loop_over = this%lattice%ntype
      case ('random_vec')
         loop_over = this%control%random_vec_num
      case default
         call g_logger%fatal('conductivity_gpu: unknown cond_calctype '//trim(this%control%cond_calctype), __FILE__, __LINE__)
      end select
      if (.not. allocated(this%recursion%mu_nm_stochastic)) &
         call g_logger%fatal('conductivity_gpu: recursion%mu_nm_stochastic is not allocated', __FILE__, __LINE__)
      if (size(this%recursion%mu_nm_stochastic, 3) /= this%control%cond_ll .or. size(this%recursion%mu_nm_stochastic, 5) < loop_over) &
         call g_logger%fatal('conductivity_gpu: mu_nm_stochastic does not match cond_ll / the vectors', __FILE__, __LINE__)

      ! :261-267
      volume = dot_product(this%lattice%a(:, 1), (cross_product(this%lattice%a(:, 2), this%lattice%a(:, 3))))
      factor = 16/(pi*(de**2))
      write (*, *) factor, volume, de

      ! :268-281 (and calculate_gamma_nm :158-225): integrand_at(l2, l2, i, ntype) for every vector, on the device
      nresp = rsrec_gpu_kubo_responses()
      allocate (integ(18, nen, loop_over*(1 + nresp)))
      ctx = rsrec_gpu_context()
      rc = 1
      if (rsrec_gpu_kubo_diag_resident(this%control%cond_ll) == loop_over*(1 + nresp)) then
         ! the recursion (RSREC_KUBO_DIAG) left the orbital-diagonal moments of these vectors on the device: nothing is uploaded.  If the
         ! library did not keep them (they did not fit beside the call's buffers) it says so, and the host array is used as always.
         call g_timer%start('conductivity-integrand-gpu-resident')
         rc = rsrec_kubo_integrand_diag(ctx, int(loop_over*(1 + nresp), c_int), int(this%control%cond_ll, c_int), c_null_ptr, int(nen, c_int), &
                                        c_loc(ene), real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), c_loc(integ))
         call g_timer%stop('conductivity-integrand-gpu-resident')
      end if
      call g_timer%start('conductivity-integrand-gpu')
      if (rc /= 0) then
         rc = rsrec_kubo_integrand(ctx, int(loop_over, c_int), int(this%control%cond_ll, c_int), c_loc(this%recursion%mu_nm_stochastic), &
                                   int(nen, c_int), c_loc(ene), real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), &
                                   c_loc(integ))
         do j = 1, nresp                                         ! (the further responses: their diagonals as the recursion kept them)
            if (rc /= 0) exit
            rc = rsrec_kubo_integrand_diag(ctx, int(loop_over, c_int), int(this%control%cond_ll, c_int), rsrec_gpu_kubo_response_diag(j), &
                                           int(nen, c_int), c_loc(ene), real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), &
                                           c_loc(integ(1, 1, j*loop_over + 1)))
         end do
      end if
      if (rc /= 0) call g_logger%fatal('conductivity_gpu%calculate_conductivity_tensor: '//rsrec_error_string(ctx), __FILE__, __LINE__)
      call g_timer%stop('conductivity-integrand-gpu')

      ! :283-372, once per response: the namelist's first, under the reference's file names
      do j = 0, nresp
         prefix = ''
         if (j > 0) prefix = trim(rsrec_gpu_kubo_response_name(j))//'_'
         if (rsrec_env_flag('RSREC_HOST_COND_TAIL')) then
            call g_timer%start('conductivity-tensor-host')
            call host_tail(this, integ(:, :, j*loop_over + 1:(j + 1)*loop_over), wscale, a, b, loop_over, nen, trim(prefix))
            call g_timer%stop('conductivity-tensor-host')
         else
            call g_timer%start('conductivity-tensor-gpu')
            call device_tail(this, ctx, integ(:, :, j*loop_over + 1:(j + 1)*loop_over), ene, wscale, a, b, loop_over, nen, trim(prefix))
            call g_timer%stop('conductivity-tensor-gpu')
         end if
      end do

      ! RSREC_KUBO_OPTICAL=<nw>: sigma(omega) of the namelist's pair
      nw_opt = optical_frequencies()
      if (nw_opt > 0) call optical_tail(this, ctx, ene, loop_over, nen, nw_opt)

      deallocate (integ, wscale, ene)
   end subroutine gpu_calculate_conductivity_tensor

   !> RSREC_KUBO_OPTICAL as a number of frequencies; 0: unset or empty
   function optical_frequencies() result(nw)
      integer :: nw
      character(len=16) :: val
      integer :: n, stat, ios
      nw = 0
      call get_environment_variable('RSREC_KUBO_OPTICAL', val, n, stat)
      if (stat > 0 .or. n == 0) return
      ios = 1
      if (stat == 0) read (val, *, iostat=ios) nw
      if (ios /= 0 .or. nw < 1) call g_logger%fatal('conductivity_gpu: RSREC_KUBO_OPTICAL must be a number of frequencies >= 1', __FILE__, __LINE__)
   end function optical_frequencies

   !> sigma(omega_k), k = 1 .. nw, at energy%fermi from the orbital diagonals of mu_nm_stochastic -> optical_cond.out
   subroutine optical_tail(this, ctx, ene, loop_over, nen, nw)
      class(conductivity_gpu), intent(inout) :: this
      type(c_ptr), intent(in) :: ctx
      real(rp), dimension(:), intent(in), target :: ene
      integer, intent(in) :: loop_over, nen, nw
      complex(rp), dimension(:, :, :, :), allocatable, target :: dg, opt       ! (18, cond_ll, cond_ll, loop_over), (18, nw, 1, loop_over)
      real(rp), target :: fermi(1)
      complex(rp) :: tot
      integer :: l, n, m, v, k, ll, nchar, stat, u
      integer(c_int) :: rc
      character(len=sl) :: fname

      ll = this%control%cond_ll
      allocate (dg(18, ll, ll, loop_over), opt(18, nw, 1, loop_over))
      do v = 1, loop_over
         do m = 1, ll
            do n = 1, ll
               do l = 1, 18
                  dg(l, n, m, v) = this%recursion%mu_nm_stochastic(l, l, n, m, v)
               end do
            end do
         end do
      end do
      call get_environment_variable('RSREC_KUBO_OPTICAL_MOMENTS', fname, nchar, stat)
      if (stat == 0 .and. nchar > 0) then
         open (newunit=u, file=trim(fname), access='stream', form='unformatted', status='replace', action='write')
         write (u) dg
         close (u)
      end if
      fermi(1) = this%en%fermi
      call g_timer%start('conductivity-optical-gpu')
      rc = rsrec_kubo_optical(ctx, int(loop_over, c_int), int(ll, c_int), c_loc(dg), int(nen, c_int), c_loc(ene), &
                              real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), int(nw, c_int), 1_c_int, c_loc(fermi), &
                              0.0_c_double, c_loc(opt))
      if (rc /= 0) call g_logger%fatal('conductivity_gpu%optical_tail: '//rsrec_error_string(ctx), __FILE__, __LINE__)
      call g_timer%stop('conductivity-optical-gpu')

      open (unit=34, file='optical_cond.out', status='replace', action='write')
      do k = 1, nw
         tot = sum(opt(:, k, 1, :))
         write (34, '(3es16.6)') k*(ene(2) - ene(1)), real(tot)/real(loop_over), aimag(tot)/real(loop_over)
      end do
      close (34)
      deallocate (dg, opt)
   end subroutine optical_tail

   !> The tail on the device: series and sigma (38, nen, nsets) from one rsrec_kubo_conductivity call -- rows 1-2 Re / Im of the total,
   !> 3-20 / 21-38 Re / Im of the orbitals; set 1 the sum over the vectors, set 1 + ntype that type alone ('per_type') -- then the
   !> reference's files, formats, divisions and unit numbers (:293-367).  `prefix` goes before every file name (a further response's
   !> '<op>_'; empty: the reference's names, fort.123 the unit's own file).
   subroutine device_tail(this, ctx, integ, ene, wscale, a, b, loop_over, nen, prefix)
      class(conductivity_gpu), intent(inout) :: this
      type(c_ptr), intent(in) :: ctx
      complex(rp), dimension(:, :, :), intent(in), target, contiguous :: integ
      character(len=*), intent(in) :: prefix
      real(rp), dimension(:), intent(in), target :: ene
      real(rp), dimension(:), intent(in) :: wscale
      real(rp), intent(in) :: a, b
      integer, intent(in) :: loop_over, nen
      integer :: i, ntype, nsets, per_vector, u123
      integer(c_int) :: rc
      real(rp), dimension(:, :, :), allocatable, target :: sigma, series
      character(len=*), parameter :: fname_cond_total = "cond_total.out"
      character(len=*), parameter :: fname_cond_orb_real = "cond_total_orb_real.out"
      character(len=*), parameter :: fname_cond_orb_im = "cond_total_orb_im.out"
      character(len=sl) :: fname_r, fname_orb_r, fname_orb_i

      per_vector = 0
      if (this%control%cond_calctype == 'per_type') per_vector = 1
      nsets = 1 + per_vector*loop_over
      allocate (sigma(38, nen, nsets), series(38, nen, nsets))
      rc = rsrec_kubo_conductivity(ctx, int(loop_over, c_int), int(per_vector, c_int), int(nen, c_int), int(this%en%nv1, c_int), c_loc(ene), &
                                   real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), 0.0_c_double, c_loc(integ), &
                                   c_loc(sigma), c_loc(series))
      if (rc /= 0) call g_logger%fatal('conductivity_gpu%calculate_conductivity_tensor: '//rsrec_error_string(ctx), __FILE__, __LINE__)

      ! :293-313
      open (unit=3, file=prefix//fname_cond_total, status='replace', action='write')
      open (unit=32, file=prefix//fname_cond_orb_real, status='replace', action='write')
      open (unit=33, file=prefix//fname_cond_orb_im, status='replace', action='write')
      u123 = 123                                               ! (the reference writes the unit unopened: fort.123)
      if (len(prefix) > 0) then
         u123 = 1123
         open (unit=u123, file=prefix//'fort.123', status='replace', action='write')
      end if
      do i = 1, nen
         write (u123, '(3es16.6)') (a*wscale(i) + b) - this%en%fermi, series(1, i, 1), series(2, i, 1)
         write (3, '(3es16.6)') (a*wscale(i) + b) - this%en%fermi, sigma(1, i, 1)/real(loop_over), sigma(2, i, 1)/real(loop_over)
         write (32, '(19es16.6)') (a*wscale(i) + b) - this%en%fermi, sigma(3:20, i, 1)/real(loop_over)
         write (33, '(19es16.6)') (a*wscale(i) + b) - this%en%fermi, sigma(21:38, i, 1)/real(loop_over)
      end do
      if (u123 /= 123) close (u123)

      ! :316-367
      if (per_vector == 1) then
         do ntype = 1, loop_over
            fname_r = prefix//trim(this%lattice%symbolic_atoms(ntype)%element%symbol)//"_cond.out"
            fname_orb_r = prefix//trim(this%lattice%symbolic_atoms(ntype)%element%symbol)//"_cond_orb_real.out"
            fname_orb_i = prefix//trim(this%lattice%symbolic_atoms(ntype)%element%symbol)//"_cond_orb_im.out"

            open (unit=100 + ntype, file=fname_r, status='replace', action='write')
            open (unit=300 + ntype, file=fname_orb_r, status='replace', action='write')
            open (unit=400 + ntype, file=fname_orb_i, status='replace', action='write')
            do i = 1, nen
               write (100 + ntype, '(3es16.6)') (a*wscale(i) + b) - this%en%fermi, sigma(1, i, 1 + ntype), sigma(2, i, 1 + ntype)
               write (300 + ntype, '(19es16.6)') (a*wscale(i) + b) - this%en%fermi, sigma(3:20, i, 1 + ntype)
               write (400 + ntype, '(19es16.6)') (a*wscale(i) + b) - this%en%fermi, sigma(21:38, i, 1 + ntype)
            end do
            close (100 + ntype)
            close (300 + ntype)
            close (400 + ntype)
         end do
      end if
      deallocate (sigma, series)
   end subroutine device_tail

   !> The tail on the host (RSREC_HOST_COND_TAIL): the reference's lines (:283-372) restated, simpson_f of math_mod kept as it is -- its
   !> loop reads Y(nv1 + 10) and Ene(nv1 + 10), one element past both arrays.
   subroutine host_tail(this, integ, wscale, a, b, loop_over, nen, prefix)
      class(conductivity_gpu), intent(inout) :: this
      complex(rp), dimension(:, :, :), intent(in) :: integ
      character(len=*), intent(in) :: prefix
      real(rp), dimension(:), intent(in) :: wscale
      real(rp), intent(in) :: a, b
      integer, intent(in) :: loop_over, nen
      integer :: i, l2, ntype, u123
      real(rp), dimension(:, :), allocatable :: integrand_l_im, integrand_l_real
      real(rp), dimension(:), allocatable :: integrand_tot_real, integrand_tot_im, real_part_l, im_part_l
      real(rp) :: real_part, im_part
      character(len=*), parameter :: fname_cond_total = "cond_total.out"
      character(len=*), parameter :: fname_cond_orb_real = "cond_total_orb_real.out"
      character(len=*), parameter :: fname_cond_orb_im = "cond_total_orb_im.out"
      character(len=sl) :: fname_r, fname_orb_r, fname_orb_i

      allocate (real_part_l(18), im_part_l(18), integrand_tot_real(nen), integrand_tot_im(nen))
      allocate (integrand_l_real(18, nen), integrand_l_im(18, nen))

      ! :283-291: integrand(l2, l2, :) is the sum of integrand_at over the vectors
      integrand_tot_real(:) = 0.0d0
      integrand_tot_im(:) = 0.0d0
      do l2 = 1, 18
         integrand_l_real(l2, :) = 0.0d0
         integrand_l_im(l2, :) = 0.0d0
         do ntype = 1, loop_over
            integrand_l_real(l2, :) = integrand_l_real(l2, :) + real(integ(l2, :, ntype))
            integrand_l_im(l2, :) = integrand_l_im(l2, :) + aimag(integ(l2, :, ntype))
         end do
         integrand_tot_real(:) = integrand_tot_real(:) + integrand_l_real(l2, :)
         integrand_tot_im(:) = integrand_tot_im(:) + integrand_l_im(l2, :)
      end do

      ! :293-313
      open (unit=3, file=prefix//fname_cond_total, status='replace', action='write')
      open (unit=32, file=prefix//fname_cond_orb_real, status='replace', action='write')
      open (unit=33, file=prefix//fname_cond_orb_im, status='replace', action='write')
      u123 = 123                                               ! (the reference writes the unit unopened: fort.123)
      if (len(prefix) > 0) then
         u123 = 1123
         open (unit=u123, file=prefix//'fort.123', status='replace', action='write')
      end if
      do i = 1, nen
         real_part = 0.0d0; im_part = 0.0d0; real_part_l(:) = 0.0d0; im_part_l(:) = 0.0d0
         write (u123, '(3es16.6)') (a*wscale(i) + b) - this%en%fermi, integrand_tot_real(i), integrand_tot_im(i)
         call simpson_f(real_part, wscale, wscale(i), this%en%nv1, integrand_tot_real(:), .true., .false., 0.0d0)
         call simpson_f(im_part, wscale, wscale(i), this%en%nv1, integrand_tot_im(:), .true., .false., 0.0d0)
         write (3, '(3es16.6)') (a*wscale(i) + b) - this%en%fermi, real_part/real(loop_over), im_part/real(loop_over)
         do l2 = 1, 18
            call simpson_f(real_part_l(l2), wscale, wscale(i), this%en%nv1, integrand_l_real(l2, :), .true., .false., 0.0d0)
            call simpson_f(im_part_l(l2), wscale, wscale(i), this%en%nv1, integrand_l_im(l2, :), .true., .false., 0.0d0)
         end do
         write (32, '(19es16.6)') (a*wscale(i) + b) - this%en%fermi, real_part_l(1:18)/real(loop_over)
         write (33, '(19es16.6)') (a*wscale(i) + b) - this%en%fermi, im_part_l(1:18)/real(loop_over)
      end do
      if (u123 /= 123) close (u123)

      ! :316-367
      if (this%control%cond_calctype == 'per_type') then
         do ntype = 1, loop_over
            integrand_tot_real(:) = 0.0d0
            integrand_tot_im(:) = 0.0d0
            do l2 = 1, 18
               integrand_l_real(l2, :) = real(integ(l2, :, ntype))
               integrand_l_im(l2, :) = aimag(integ(l2, :, ntype))
               integrand_tot_real(:) = integrand_tot_real(:) + integrand_l_real(l2, :)
               integrand_tot_im(:) = integrand_tot_im(:) + integrand_l_im(l2, :)
            end do

            fname_r = prefix//trim(this%lattice%symbolic_atoms(ntype)%element%symbol)//"_cond.out"
            fname_orb_r = prefix//trim(this%lattice%symbolic_atoms(ntype)%element%symbol)//"_cond_orb_real.out"
            fname_orb_i = prefix//trim(this%lattice%symbolic_atoms(ntype)%element%symbol)//"_cond_orb_im.out"

            open (unit=100 + ntype, file=fname_r, status='replace', action='write')
            open (unit=300 + ntype, file=fname_orb_r, status='replace', action='write')
            open (unit=400 + ntype, file=fname_orb_i, status='replace', action='write')

            do i = 1, nen
               real_part = 0.0d0; im_part = 0.0d0; real_part_l(:) = 0.0d0; im_part_l(:) = 0.0d0
               call simpson_f(real_part, wscale, wscale(i), this%en%nv1, integrand_tot_real(:), .true., .false., 0.0d0)
               call simpson_f(im_part, wscale, wscale(i), this%en%nv1, integrand_tot_im(:), .true., .false., 0.0d0)
               write (100 + ntype, '(3es16.6)') (a*wscale(i) + b) - this%en%fermi, real_part, im_part
               do l2 = 1, 18
                  call simpson_f(real_part_l(l2), wscale, wscale(i), this%en%nv1, integrand_l_real(l2, :), .true., .false., 0.0d0)
                  call simpson_f(im_part_l(l2), wscale, wscale(i), this%en%nv1, integrand_l_im(l2, :), .true., .false., 0.0d0)
               end do
               write (300 + ntype, '(19es16.6)') (a*wscale(i) + b) - this%en%fermi, real_part_l(1:18)
               write (400 + ntype, '(19es16.6)') (a*wscale(i) + b) - this%en%fermi, im_part_l(1:18)
            end do
            close (100 + ntype)
            close (300 + ntype)
            close (400 + ntype)
         end do
      end if

      deallocate (integrand_tot_real, integrand_tot_im, real_part_l, im_part_l, integrand_l_real, integrand_l_im)
   end subroutine host_tail

end module conductivity_gpu_mod
