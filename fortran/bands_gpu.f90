!------------------------------------------------------------------------------
! RS-LMTO-ASA drop-in, third stage: the density-of-states reduction of `bands%calculate_fermi` on the GPU.
!------------------------------------------------------------------------------
!
! MODULE: bands_gpu_mod
!
! DESCRIPTION:
!> `type, extends(bands) :: bands_gpu` overrides `calculate_fermi` (bands.f90:227-346).  The reference forms
!>    dtot(i), dosia(site, i), dosial(site, 1:18, i) = -Im g0(j, j, i, site) / pi        (bands.f90:258-268)
!> from the full `g0(18,18,nE,site)` -- 13 MB per site that a GPU Green function first has to send over PCIe.  With a
!> `recursion_gpu` behind the class pointer the block coefficients of the rank's sites are still on the device after `recur_b`
!> (`rsrec_gpu_block_resident`), and `rsrec_block_ldos` (include/rsrec.h) runs zsqr -> get_terminf -> bgreen -> this reduction
!> there: 18 doubles per site and energy come back instead of 648, summed in the reference's loop order.
!> The Chebyshev recursion has the same stage: after `chebyshev_recur` the moments of the rank's sites are on the device
!> (`rsrec_gpu_cheb_resident`), and `rsrec_chebyshev_ldos` forms the diagonal of `green%chebyshev_green` and the same reduction there.
!> The two recursions differ in that one library call; everything after it is one code path.  Everything after the
!> reduction -- the MPI_ALLREDUCE of the zero-padded arrays (:271-274), the three output files (:279-324), the Fermi level
!> (:326-343) -- is the reference's, restated here because `calculate_fermi` is one routine.
!>
!> The moment stage of an SCF iteration (self.f90:837-852: `calculate_magnetic_moments`, `calculate_moments` with
!> `calculate_orbital_moments`) reads `g0` only through linear functionals Im Tr(O g0): the spin-resolved s / p / d brackets of
!> bands.f90:449-452 (whose sums are dx, dy, dz of :1175-1177) and Im Tr(L_a g0) of :1124-1126.  While `g0` is still pending in
!> `green_gpu` (`defer_g0`) and `device_moments` is set, ONE `rsrec_block_spectra` / `rsrec_chebyshev_spectra` call per recursion result
!> evaluates those 15 functionals on the resident chains (timer region `spectra-gpu`), the image is kept in the type, and the three
!> routines take their energy-resolved arrays from it; their tails (Simpson integrals, `<sym>_orbene.out`, log lines, `gravity_center`,
!> `ql`, `calculate_pl`, the exchange of the potentials between ranks) are the reference's lines restated.  No `g0` is produced in such
!> an iteration.  Deviation: `g0_x, g0_y, g0_z, d_orb` stay zero on this route (no routine of the reference reads them);
!> RSREC_HOST_MOMENTS restores them with the host route.
!>
!> The integrals of those tails run on the device as well (`device_tail`, the default of the spectra route): right after the spectra call,
!> while its image is still on the handle, ONE `rsrec_spectra_integrals` call (timer region `moment-integrals-gpu`) integrates the 15 rows
!> as they are -- `simpson_m` of orders 0, 1, 2 up to the Fermi level and the cumulative `simpson_f` up to every mesh energy, the latter in
!> O(nE) instead of the O(nE^2) loops behind `<sym>_spinene.out` / `<sym>_orbene.out`.  The integrals are linear, so the three routines
!> form dx / dy / dz (sums of three rows) and the dspd rows (which need the moment direction calculate_magnetic_moments has just updated:
!> no table built before that call could hold it) from the rows' integrals; the file formats, the `-1/pi` and `0.5/pi` factors, `ql`,
!> `gravity_center`, `mtot`, `mom` and the log lines stay here.  RSREC_HOST_MOMENT_TAIL keeps the reference's host loops (region
!> `moment-integrals-host`).  `calculate_orbital_quadrupoles` takes the same route while the chains are resident and g0 is pending: one
!> six-operator spectra call, one integrals call, no g0.
!>
!> `g0` on demand: the remaining consumers of `g0` (orbital quadrupoles, projected Green function, orbital DOS) and every case the
!> device route does not take are inherited; the overrides below only make sure `g0` exists first (`green_gpu%fetch_g0`, a no-op unless
!> `green_gpu%defer_g0` postponed it).
!>
!> Falls back to the inherited routine whenever the device does not hold this call's coefficients or moments (scalar recursion,
!> local-axis runs without RSREC_LOCAL_AXIS_DEVICE, a `green` that is not `green_gpu`).  With that switch `recursion_gpu` announces the
!> chains of a local-axis run, resident in each site's local frame, and every stage here takes them as it takes a collinear run's.
!------------------------------------------------------------------------------
module bands_gpu_mod
   use, intrinsic :: iso_c_binding
   use mpi_mod
   use bands_mod
   use green_mod
   use green_gpu_mod
   use precision_mod, only: rp
   use math_mod, only: pi, gauss_legendre, simpson_m, simpson_f, L_x, L_y, L_z, hcpx, i_unit, updatrotmom_single
   use logger_mod, only: g_logger
   use timer_mod, only: g_timer
   use string_mod, only: fmt
   use rsrec_binding
   use rsrec_context_mod, only: rsrec_gpu_context, rsrec_env_flag
   use recursion_gpu_mod, only: rsrec_gpu_block_resident, rsrec_gpu_cheb_resident
#ifdef USE_MPI
   use mpi
#endif
   implicit none

   private

   type, public, extends(bands) :: bands_gpu
      !> .false.: always the inherited host reduction (a g0 is then needed)
      logical :: device_ldos = .true.
      !> number of calculate_fermi calls served by the device stage (diagnostics / tests)
      integer :: n_device_ldos = 0
      !> .false.: the moment stage always reads a g0 on the host (the inherited routines)
      logical :: device_moments = .true.
      !> number of spectra calls made (diagnostics / tests)
      integer :: n_device_spectra = 0
      !> Im Tr(O_k g0) of the 15 SCF operators, (15, nE, nrec), this rank's sites filled; valid until calculate_fermi runs again
      real(rp), dimension(:, :, :), allocatable :: spec
      logical :: spec_valid = .false.
      integer :: spec_resident = -1       ! residency count the image was made for
      !> the operators, built once: 1-12 = P(c, l), c = 0, x, y, z outer, l = s, p, d inner; 13-15 = Lx, Ly, Lz
      complex(rp), dimension(:, :, :), allocatable :: spec_ops
      !> .false.: the Simpson tails of the spectra route stay the reference's host loops (RSREC_HOST_MOMENT_TAIL)
      logical :: device_tail = .true.
      !> number of rsrec_spectra_integrals calls made (diagnostics / tests)
      integer :: n_device_tail = 0
      !> the integrals of the 15 rows of `spec`: tail_mom(p + 1, k, site) = simpson_m(nexp = p), tail_cum(k, ie, site) = simpson_f up to ene(ie);
      !> valid for the Fermi-level arguments they were made with
      real(rp), dimension(:, :, :), allocatable :: tail_mom, tail_cum
      logical :: tail_valid = .false.
      integer :: tail_nv1 = -1
      real(rp) :: tail_e1 = 0.0_rp, tail_fermi = 0.0_rp
   contains
      procedure :: calculate_fermi => gpu_calculate_fermi
      procedure :: calculate_magnetic_moments => gpu_calculate_magnetic_moments
      procedure :: calculate_orbital_moments => gpu_calculate_orbital_moments
      procedure :: calculate_orbital_quadrupoles => gpu_calculate_orbital_quadrupoles
      procedure :: calculate_moments => gpu_calculate_moments
      procedure :: calculate_moments_gauss_legendre => gpu_calculate_moments_gauss_legendre
      procedure :: calculate_occupation_gauss_legendre => gpu_calculate_occupation_gauss_legendre
      procedure :: calculate_projected_green => gpu_calculate_projected_green
      procedure :: calculate_projected_dos => gpu_calculate_projected_dos
      procedure :: calculate_orbital_dos => gpu_calculate_orbital_dos
      procedure :: restore_to_default => gpu_restore_to_default
   end type bands_gpu

   interface bands_gpu
      procedure :: gpu_constructor
   end interface bands_gpu

contains

   !> Same construction as bands.f90:119-133; the dummy is polymorphic, which is what the reference's constructor needs to become
   !> (INTEGRATION.md) for `green_gpu` to survive it.
   function gpu_constructor(green_obj) result(obj)
      type(bands_gpu) :: obj
      class(green), target, intent(in) :: green_obj

      obj%green => green_obj
      obj%lattice => green_obj%dos%recursion%lattice
      obj%symbolic_atom => green_obj%dos%recursion%hamiltonian%charge%lattice%symbolic_atoms
      obj%dos => green_obj%dos
      obj%en => green_obj%dos%en
      obj%control => green_obj%dos%recursion%lattice%control
      obj%recursion => green_obj%dos%recursion
      call obj%restore_to_default()
      if (rsrec_env_flag('RSREC_HOST_LDOS')) obj%device_ldos = .false.   ! (hosts that cannot reach the member: fortran/shadow/)
      if (rsrec_env_flag('RSREC_HOST_MOMENTS')) obj%device_moments = .false.
      if (rsrec_env_flag('RSREC_HOST_MOMENT_TAIL')) obj%device_tail = .false.
   end function gpu_constructor

   !> bands.f90:178-217.  In a pair run (lattice%njij /= 0: the exchange post-processing, calculation.f90:816-950) atoms_per_process
   !> counts pairs, and the per-site energy arrays dx ... d_orb (20 MB per pair at 2500 energies) are read by no routine of the flow:
   !> there they are allocated with no site columns.  Otherwise the reference's routine.
   subroutine gpu_restore_to_default(this)
      class(bands_gpu) :: this
      integer :: nv
      if (this%lattice%njij == 0) then
         call this%bands%restore_to_default()
         return
      end if
      nv = this%en%channels_ldos + 10
      allocate (this%dtot(nv), this%dtotcheb(nv), this%dx(nv, 0), this%dy(nv, 0), this%dz(nv, 0), this%g0_x(9, 9, nv, 0), &
                this%g0_y(9, 9, nv, 0), this%g0_z(9, 9, nv, 0), this%dspd(6, nv, 0), this%d_orb(9, 9, 3, nv, 0), this%mag_for(3, 0))
      this%dtot(:) = 0.0d0
      this%dtotcheb(:) = 0.0d0
   end subroutine gpu_restore_to_default

   !> `g0` must exist before an inherited routine reads it
   subroutine ensure_g0(this)
      class(bands_gpu), intent(inout) :: this
      select type (g => this%green)
      class is (green_gpu)
         call g%fetch_g0()
      end select
   end subroutine ensure_g0

   !> .true. if the device holds what this call's densities of states are made of: the block coefficients (recur = 'block') or the
   !> Chebyshev moments (recur = 'chebyshev') of the rank's sites
   function device_stage_usable(this) result(ok)
      class(bands_gpu), intent(in) :: this
      logical :: ok
      ok = this%device_ldos .and. end_atom >= start_atom
      if (ok) then
         select case (trim(this%control%recur))
         case ('block')
            ok = rsrec_gpu_block_resident() == end_atom - start_atom + 1
         case ('chebyshev')
            ok = rsrec_gpu_cheb_resident() == end_atom - start_atom + 1
         case default
            ok = .false.
         end select
      end if
      if (ok) then
         select type (g => this%green)
         class is (green_gpu)
            ok = .true.
         class default
            ok = .false.
         end select
      end if
   end function device_stage_usable

   !---------------------------------------------------------------------------
   !> Total / site / orbital densities of states and the Fermi level (replaces bands.f90:227-346)
   !---------------------------------------------------------------------------
   subroutine gpu_calculate_fermi(this)
      class(bands_gpu) :: this
      integer :: nv, nrec, ia, ik1, ik1_mag, ifail
      integer(c_int) :: rc, sym_i, crank, cranks
      type(c_ptr) :: handle
      real(rp) :: e1, e1_mag, ef_mag
      real(rp), allocatable, target :: ene(:), dtot(:), dosia(:, :), dosial(:, :, :)

      this%spec_valid = .false.           ! a new Green function: the moment stage after it forms its own image
      this%tail_valid = .false.
      if (.not. device_stage_usable(this)) then
         call ensure_g0(this)
         call this%bands%calculate_fermi()
         return
      end if

      nv = this%en%channels_ldos + 10
      nrec = this%lattice%nrec
      allocate (ene(nv), dtot(nv), dosia(nrec, nv), dosial(nrec, 18, nv))
      ene = this%en%ene(1:nv)
      sym_i = 0
      if (this%control%sym_term) sym_i = 1
      handle = rsrec_gpu_context()
      ! zero-padded images over all nrec sites, this rank's sites start_atom .. end_atom filled (what bands.f90:258-268 leaves
      ! in dtot / dosia / dosial before the all-reduce); sums in the reference's loop order
      call g_timer%start('ldos-gpu')
      if (trim(this%control%recur) == 'chebyshev') then
         rc = rsrec_chebyshev_ldos(handle, int(nv, c_int), c_loc(ene), real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), &
                                   int(start_atom - 1, c_int), int(nrec, c_int), c_loc(dtot), c_loc(dosia), c_loc(dosial))
      else
         rc = rsrec_block_ldos(handle, int(nv, c_int), c_loc(ene), 0.0_c_double, 0.0_c_double, sym_i, int(start_atom - 1, c_int), int(nrec, c_int), &
                               c_loc(dtot), c_loc(dosia), c_loc(dosial), c_null_ptr, c_null_ptr)
      end if
      call g_timer%stop('ldos-gpu')
      if (rc /= 0) call g_logger%fatal('rsrec_'//trim(this%control%recur)//'_ldos: '//rsrec_error_string(handle), __FILE__, __LINE__)
      this%n_device_ldos = this%n_device_ldos + 1
      this%dtot(1:nv) = dtot

      this%qqv = real(sum(this%symbolic_atom(1:this%lattice%nbulk_bulk)%element%valence))      ! bands.f90:251
      if (rank == 0) call g_logger%info('Valence is:'//fmt('f16.6', this%qqv), __FILE__, __LINE__)
      ! the all-reduce of bands.f90:271-274: over the library's own communicator if the host set one up (rsrec_comm_init[_file]: RCCL
      ! over xGMI, no MPI needed), else the reference's MPI calls
      rc = rsrec_comm_size(handle, crank, cranks)
      if (cranks > 1) then
         dtot = this%dtot(1:nv)
         rc = rsrec_allreduce_sum(handle, c_loc(dtot), int(nv, c_size_t))
         if (rc == 0) rc = rsrec_allreduce_sum(handle, c_loc(dosia), int(size(dosia), c_size_t))
         if (rc == 0) rc = rsrec_allreduce_sum(handle, c_loc(dosial), int(size(dosial), c_size_t))
         if (rc /= 0) call g_logger%fatal('rsrec_allreduce_sum: '//rsrec_error_string(handle), __FILE__, __LINE__)
         this%dtot(1:nv) = dtot
      else
#ifdef USE_MPI
      call MPI_ALLREDUCE(MPI_IN_PLACE, this%dtot, nv, MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)       ! bands.f90:271-274
      call MPI_ALLREDUCE(MPI_IN_PLACE, dosia, size(dosia), MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)
      call MPI_ALLREDUCE(MPI_IN_PLACE, dosial, size(dosial), MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)
#endif
      end if
      ! output files of bands.f90:279-324 (same names, units, formats; every rank replaces totaldos.out, rank 0 fills the files)
      call write_columns(125, 'totaldos.out', nv, this%en%ene(1:nv) - this%en%fermi, reshape(this%dtot(1:nv), [1, nv]), rank == 0, .true.)
      do ia = 1, nrec
         call write_columns(250 + ia, trim(this%symbolic_atom(this%lattice%nbulk + ia)%element%symbol)//'_dos.out', nv, &
                            this%en%ene(1:nv) - this%en%fermi, reshape(dosia(ia, :), [1, nv]), rank == 0, rank == 0)
         call write_columns(450 + ia, trim(this%symbolic_atom(this%lattice%nbulk + ia)%element%symbol)//'_orbital_dos.out', nv, &
                            this%en%ene(1:nv) - this%en%fermi, dosial(ia, :, :), rank == 0, rank == 0)
      end do

      ! Fermi level (bands.f90:326-343)
      ik1 = this%en%ik1
      ik1_mag = 0
      ef_mag = this%en%fermi
      this%en%chebfermi = this%en%fermi
      if (.not. (this%en%fix_fermi) .and. this%control%calctype == 'B') then
         e1_mag = ef_mag
         call this%fermi(ef_mag, this%en%edel, ik1_mag, this%en%energy_min, nv, this%dtot, ifail, this%qqv, e1_mag)
         e1 = this%en%fermi
         call this%fermi(this%en%fermi, this%en%edel, ik1, this%en%energy_min, nv, this%dtot, ifail, this%qqv, e1_mag)
         this%nv1 = ik1
         this%e1 = e1_mag
         if (rank == 0) call g_logger%info('Free Fermi energy:'//fmt('f10.6', this%en%fermi), __FILE__, __LINE__)
      else if (this%en%fix_fermi) then
         ik1 = nint((this%en%fermi - this%en%energy_min)/this%en%edel)
         e1 = this%en%energy_min + (ik1 - 1)*this%en%edel
         this%nv1 = ik1
         this%e1 = e1
         if (rank == 0) call g_logger%info('Fixed Fermi energy:'//fmt('f10.6', this%en%fermi), __FILE__, __LINE__)
      end if
   end subroutine gpu_calculate_fermi

   !> One of the reference's DOS files: column 1 = x(i), then y(:, i), format (<1 + rows>f16.5), opened with status 'replace'.
   subroutine write_columns(unitnum, fname, n, x, y, fill, opened)
      integer, intent(in) :: unitnum, n
      character(len=*), intent(in) :: fname
      real(rp), intent(in) :: x(n), y(:, :)
      logical, intent(in) :: fill, opened
      integer :: i
      character(len=16) :: form

      if (.not. opened) return
      write (form, '(a,i0,a)') '(', size(y, 1) + 1, 'f16.5)'
      open (unit=unitnum, file=fname, status='replace', action='write')
      if (fill) then
         do i = 1, n
            write (unitnum, form) x(i), y(:, i)
         end do
         rewind (unitnum)
      end if
      close (unitnum)
   end subroutine write_columns

   ! ---- the moment stage: from the spectra image where g0 is still pending on the device, else g0 and the reference's routine ------
   !> .true. if this call is served from the resident chains: the device holds them, device_moments, and g0 is pending in green_gpu
   function spectra_route(this) result(ok)
      class(bands_gpu), intent(in) :: this
      logical :: ok
      ok = this%device_moments
      if (ok) ok = device_stage_usable(this)
      if (ok) then
         select type (g => this%green)
         class is (green_gpu)
            ok = g%defer_g0 .and. g%g0_stale
         class default
            ok = .false.
         end select
      end if
   end function spectra_route

   !> The 15 operators: P(c, l) such that Im Tr(P g) is the bracket of bands.f90:449-452 with spin component c over the orbitals of l,
   !> and the cartesian L matrices through cart2sph, the same block in both spins (bands.f90:1094-1111).  Tr(P g) = sum P(j, i) g(i, j).
   subroutine build_spectra_ops(this)
      class(bands_gpu), intent(inout) :: this
      integer :: l, m, o, k
      complex(rp), dimension(9, 9) :: mL

      allocate (this%spec_ops(18, 18, 15))
      this%spec_ops = (0.0_rp, 0.0_rp)
      do l = 1, 3
         do m = 1, 2*l - 1
            o = (l - 1)**2 + m
            this%spec_ops(o, o, l) = 1.0_rp;          this%spec_ops(o + 9, o + 9, l) = 1.0_rp          ! g(o,o) + g(o+9,o+9)
            this%spec_ops(o + 9, o, 3 + l) = 1.0_rp;  this%spec_ops(o, o + 9, 3 + l) = 1.0_rp          ! g(o,o+9) + g(o+9,o)
            this%spec_ops(o + 9, o, 6 + l) = i_unit;  this%spec_ops(o, o + 9, 6 + l) = -i_unit         ! i g(o,o+9) - i g(o+9,o)
            this%spec_ops(o, o, 9 + l) = 1.0_rp;      this%spec_ops(o + 9, o + 9, 9 + l) = -1.0_rp     ! g(o,o) - g(o+9,o+9)
         end do
      end do
      do k = 1, 3
         select case (k)
         case (1); mL = L_x
         case (2); mL = L_y
         case (3); mL = L_z
         end select
         call hcpx(mL, 'cart2sph')
         this%spec_ops(1:9, 1:9, 12 + k) = mL
         this%spec_ops(10:18, 10:18, 12 + k) = mL
      end do
   end subroutine build_spectra_ops

   !> One library call per recursion result: the image of the 15 functionals for the rank's sites
   subroutine ensure_spectra(this)
      class(bands_gpu), intent(inout), target :: this
      integer :: nv, nrec, nres
      integer(c_int) :: rc, sym_i
      type(c_ptr) :: handle
      real(rp), allocatable, target :: ene(:)
      real(rp), dimension(:, :, :), pointer :: sp
      complex(rp), dimension(:, :, :), pointer :: op

      nv = this%en%channels_ldos + 10
      nrec = this%lattice%nrec
      nres = rsrec_gpu_block_resident() + rsrec_gpu_cheb_resident()
      if (this%spec_valid .and. allocated(this%spec) .and. nres == this%spec_resident) then
         if (size(this%spec, 2) == nv .and. size(this%spec, 3) == nrec) return
      end if
      if (.not. allocated(this%spec_ops)) call build_spectra_ops(this)
      if (allocated(this%spec)) then
         if (size(this%spec, 2) /= nv .or. size(this%spec, 3) /= nrec) deallocate (this%spec)
      end if
      if (.not. allocated(this%spec)) allocate (this%spec(15, nv, nrec))
      allocate (ene(nv))
      ene = this%en%ene(1:nv)
      sym_i = 0
      if (this%control%sym_term) sym_i = 1
      handle = rsrec_gpu_context()
      sp => this%spec
      op => this%spec_ops
      call g_timer%start('spectra-gpu')
      if (trim(this%control%recur) == 'chebyshev') then
         rc = rsrec_chebyshev_spectra(handle, 15_c_int, c_loc(op), int(nv, c_int), c_loc(ene), real(this%en%energy_min, c_double), &
                                      real(this%en%energy_max, c_double), int(start_atom - 1, c_int), int(nrec, c_int), c_loc(sp))
      else
         rc = rsrec_block_spectra(handle, 15_c_int, c_loc(op), int(nv, c_int), c_loc(ene), 0.0_c_double, 0.0_c_double, sym_i, &
                                  int(start_atom - 1, c_int), int(nrec, c_int), c_loc(sp))
      end if
      call g_timer%stop('spectra-gpu')
      if (rc /= 0) call g_logger%fatal('rsrec_'//trim(this%control%recur)//'_spectra: '//rsrec_error_string(handle), __FILE__, __LINE__)
      this%n_device_spectra = this%n_device_spectra + 1
      this%spec_valid = .true.
      this%spec_resident = nres
      this%tail_valid = .false.
      if (this%device_tail) call spectra_tail(this, .true.)       ! the image is on the handle now: nothing is uploaded
   end subroutine ensure_spectra

   !> mom and cum of the 15 rows of the image, one library call.  resident: the image is the one the spectra call has just left on the
   !> handle; else the type's copy is passed.
   subroutine spectra_tail(this, resident)
      class(bands_gpu), intent(inout), target :: this
      logical, intent(in) :: resident
      integer :: nv, nrec
      integer(c_int) :: rc
      type(c_ptr) :: handle, sptr
      real(rp), allocatable, target :: ene(:)
      real(rp), dimension(:, :, :), pointer :: sp, pm, pc

      nv = this%en%channels_ldos + 10
      nrec = this%lattice%nrec
      if (allocated(this%tail_cum)) then
         if (size(this%tail_cum, 2) /= nv .or. size(this%tail_cum, 3) /= nrec) deallocate (this%tail_cum, this%tail_mom)
      end if
      if (.not. allocated(this%tail_cum)) allocate (this%tail_mom(3, 15, nrec), this%tail_cum(15, nv, nrec))
      allocate (ene(nv))
      ene = this%en%ene(1:nv)
      handle = rsrec_gpu_context()
      sp => this%spec
      pm => this%tail_mom
      pc => this%tail_cum
      sptr = c_null_ptr
      if (.not. resident) sptr = c_loc(sp)
      call g_timer%start('moment-integrals-gpu')
      rc = rsrec_spectra_integrals(handle, 15_c_int, sptr, 15_c_int, c_null_ptr, int(nv, c_int), c_loc(ene), int(this%en%nv1, c_int), &
                                   int(this%nv1, c_int), real(this%en%edel, c_double), real(this%e1, c_double), real(this%en%fermi, c_double), &
                                   int(end_atom - start_atom + 1, c_int), int(start_atom - 1, c_int), int(nrec, c_int), c_loc(pm), c_loc(pc))
      call g_timer%stop('moment-integrals-gpu')
      if (rc /= 0) call g_logger%fatal('rsrec_spectra_integrals: '//rsrec_error_string(handle), __FILE__, __LINE__)
      this%n_device_tail = this%n_device_tail + 1
      this%tail_valid = .true.
      this%tail_nv1 = this%nv1
      this%tail_e1 = this%e1
      this%tail_fermi = this%en%fermi
   end subroutine spectra_tail

   !> The image and, on the device tail, its integrals for the Fermi-level arguments as they are NOW (a routine that moved them since the
   !> spectra call gets a second call on the type's copy of the image)
   subroutine ensure_tail(this)
      class(bands_gpu), intent(inout) :: this
      call ensure_spectra(this)
      if (.not. this%device_tail) return
      if (this%tail_valid) then
         if (this%tail_nv1 == this%nv1 .and. this%tail_e1 == this%e1 .and. this%tail_fermi == this%en%fermi) return
      end if
      call spectra_tail(this, .false.)
   end subroutine ensure_tail

   !> calculate_magnetic_moments (bands.f90:791-855) reads nothing of g0 itself: it integrates the dx, dy, dz of calculate_projected_dos.
   !> A call through the parent component would bind that inner call to the reference's routine (the parent component's dynamic type is
   !> `bands`), so on the device route the routine is restated here around this type's calculate_projected_dos.
   subroutine gpu_calculate_magnetic_moments(this)
      class(bands_gpu) :: this
      real(rp) :: mx, my, mz, mxe, mye, mze
      integer :: na, ie, na_loc, unitmag, pb
      character(len=256) :: fnamemag

      if (.not. spectra_route(this)) then
         call ensure_g0(this)
         call this%bands%calculate_magnetic_moments()
         return
      end if

      call this%calculate_projected_dos()
      call ensure_tail(this)

      do na = start_atom, end_atom
         na_loc = g2l_map(na)
         pb = this%lattice%nbulk + na
         if (this%device_tail) then
            ! dx, dy, dz are -(row + row + row)/pi of the x, y, z brackets (rows 4-6, 7-9, 10-12), and so are their integrals
            this%symbolic_atom(pb)%potential%mx = bracket_sum(this%tail_mom(1, 4:6, na))
            this%symbolic_atom(pb)%potential%my = bracket_sum(this%tail_mom(1, 7:9, na))
            this%symbolic_atom(pb)%potential%mz = bracket_sum(this%tail_mom(1, 10:12, na))
         else
            call g_timer%start('moment-integrals-host')
            call simpson_m(this%symbolic_atom(pb)%potential%mx, this%en%edel, this%en%fermi, this%nv1, this%dx(:, na_loc), this%e1, 0, this%en%ene)
            call simpson_m(this%symbolic_atom(pb)%potential%my, this%en%edel, this%en%fermi, this%nv1, this%dy(:, na_loc), this%e1, 0, this%en%ene)
            call simpson_m(this%symbolic_atom(pb)%potential%mz, this%en%edel, this%en%fermi, this%nv1, this%dz(:, na_loc), this%e1, 0, this%en%ene)
            call g_timer%stop('moment-integrals-host')
         end if

         fnamemag = trim(this%symbolic_atom(pb)%element%symbol)//"_spinene.out"
         unitmag = 1000
         open (unit=unitmag, file=fnamemag, status='replace', action='write')
         if (.not. this%device_tail) call g_timer%start('moment-integrals-host')
         do ie = 1, this%en%channels_ldos + 10
            if (this%device_tail) then
               mxe = bracket_sum(this%tail_cum(4:6, ie, na))
               mye = bracket_sum(this%tail_cum(7:9, ie, na))
               mze = bracket_sum(this%tail_cum(10:12, ie, na))
            else
               mxe = 0.0d0; mye = 0.d00; mze = 0.0d0
               call simpson_f(mxe, this%en%ene, this%en%ene(ie), this%en%nv1, this%dx(:, na_loc), .true., .false., 0.0d0)
               call simpson_f(mye, this%en%ene, this%en%ene(ie), this%en%nv1, this%dy(:, na_loc), .true., .false., 0.0d0)
               call simpson_f(mze, this%en%ene, this%en%ene(ie), this%en%nv1, this%dz(:, na_loc), .true., .false., 0.0d0)
            end if
            write (unitmag, '(4es16.6)') this%en%ene(ie) - this%en%fermi, mxe, mye, mze
         end do
         if (.not. this%device_tail) call g_timer%stop('moment-integrals-host')
         rewind (unitmag)
         close (unitmag)

         this%symbolic_atom(pb)%potential%mom0(1) = this%symbolic_atom(pb)%potential%mx
         this%symbolic_atom(pb)%potential%mom0(2) = this%symbolic_atom(pb)%potential%my
         this%symbolic_atom(pb)%potential%mom0(3) = this%symbolic_atom(pb)%potential%mz

         if (this%device_tail) then
            this%symbolic_atom(pb)%potential%mom1(1) = bracket_sum(this%tail_mom(2, 4:6, na))
            this%symbolic_atom(pb)%potential%mom1(2) = bracket_sum(this%tail_mom(2, 7:9, na))
            this%symbolic_atom(pb)%potential%mom1(3) = bracket_sum(this%tail_mom(2, 10:12, na))
         else
            call g_timer%start('moment-integrals-host')
            call simpson_m(this%symbolic_atom(pb)%potential%mom1(1), this%en%edel, this%en%fermi, this%nv1, this%dx(:, na_loc), this%e1, 1, this%en%ene)
            call simpson_m(this%symbolic_atom(pb)%potential%mom1(2), this%en%edel, this%en%fermi, this%nv1, this%dy(:, na_loc), this%e1, 1, this%en%ene)
            call simpson_m(this%symbolic_atom(pb)%potential%mom1(3), this%en%edel, this%en%fermi, this%nv1, this%dz(:, na_loc), this%e1, 1, this%en%ene)
            call g_timer%stop('moment-integrals-host')
         end if

         this%symbolic_atom(pb)%potential%mtot = sqrt((this%symbolic_atom(pb)%potential%mx**2) + (this%symbolic_atom(pb)%potential%my**2) + &
                                                      (this%symbolic_atom(pb)%potential%mz**2)) + 1.0d-15

         this%symbolic_atom(pb)%potential%mom(1) = this%symbolic_atom(pb)%potential%mx/this%symbolic_atom(pb)%potential%mtot
         this%symbolic_atom(pb)%potential%mom(2) = this%symbolic_atom(pb)%potential%my/this%symbolic_atom(pb)%potential%mtot
         this%symbolic_atom(pb)%potential%mom(3) = this%symbolic_atom(pb)%potential%mz/this%symbolic_atom(pb)%potential%mtot

         call g_logger%info('Spin moment of atom'//fmt('i4', na)//' is '//fmt('f10.6', this%symbolic_atom(pb)%potential%mtot), __FILE__, __LINE__)
         mx = this%symbolic_atom(pb)%potential%mx
         my = this%symbolic_atom(pb)%potential%my
         mz = this%symbolic_atom(pb)%potential%mz

         if (this%control%nsp < 3) this%symbolic_atom(pb)%potential%mom(:) = [0.0d0, 0.0d0, 1.00d0]

         if (this%recursion%hamiltonian%local_axis) then            ! bands.f90:849-853
            call g_logger%info('Local spin moment projections of atom'//fmt('i4', na)//' is '//fmt('f10.6', mx)//' '//fmt('f10.6', my)//' '//fmt('f10.6', mz), __FILE__, __LINE__)
         else
            call g_logger%info('Spin moment projections of atom'//fmt('i4', na)//' is '//fmt('f10.6', mx)//' '//fmt('f10.6', my)//' '//fmt('f10.6', mz), __FILE__, __LINE__)
         end if
      end do
   end subroutine gpu_calculate_magnetic_moments

   !> -(a + b + c)/pi of three rows' integrals, the expression calculate_projected_dos applies to the rows themselves
   pure function bracket_sum(v) result(r)
      real(rp), intent(in) :: v(3)
      real(rp) :: r
      r = -(v(1) + v(2) + v(3))/pi
   end function bracket_sum

   !> calculate_orbital_moments (bands.f90:1075-1156): lxi, lyi, lzi from the image, the tail restated
   subroutine gpu_calculate_orbital_moments(this)
      class(bands_gpu) :: this
      real(rp) :: lx, ly, lz, lxe, lye, lze
      ! one element longer than the reference's, and zero there: with nv1 = channels_ldos + 1 simpson_f reads Y(nv1 + 10)
      real(rp), dimension(this%en%channels_ldos + 11) :: lxi, lyi, lzi
      integer :: na, ie, unitorb, nv
      character(len=256) :: fnameorb

      if (.not. spectra_route(this)) then
         call ensure_g0(this)
         call this%bands%calculate_orbital_moments()
         return
      end if
      call ensure_tail(this)
      nv = this%en%channels_ldos + 10
      do na = start_atom, end_atom
         lx = 0.0d0; ly = 0.0d0; lz = 0.d0
         if (this%device_tail) then
            lx = this%tail_mom(1, 13, na)
            ly = this%tail_mom(1, 14, na)
            lz = this%tail_mom(1, 15, na)
         else
            lxi = 0.0d0; lyi = 0.0d0; lzi = 0.0d0
            lxi(1:nv) = this%spec(13, :, na)
            lyi(1:nv) = this%spec(14, :, na)
            lzi(1:nv) = this%spec(15, :, na)

            call g_timer%start('moment-integrals-host')
            call simpson_m(lx, this%en%edel, this%en%fermi, this%nv1, lxi, this%e1, 0, this%en%ene)
            call simpson_m(ly, this%en%edel, this%en%fermi, this%nv1, lyi, this%e1, 0, this%en%ene)
            call simpson_m(lz, this%en%edel, this%en%fermi, this%nv1, lzi, this%e1, 0, this%en%ene)
            call g_timer%stop('moment-integrals-host')
         end if

         fnameorb = trim(this%symbolic_atom(this%lattice%nbulk + na)%element%symbol)//"_orbene.out"
         unitorb = (rank + 1)*132 + na
         open (unit=unitorb, file=fnameorb, status='replace', action='write')
         if (.not. this%device_tail) call g_timer%start('moment-integrals-host')
         do ie = 1, this%en%channels_ldos + 10
            if (this%device_tail) then
               lxe = this%tail_cum(13, ie, na)
               lye = this%tail_cum(14, ie, na)
               lze = this%tail_cum(15, ie, na)
            else
               call simpson_f(lxe, this%en%ene, this%en%ene(ie), this%en%nv1, lxi, .true., .false., 0.0d0)
               call simpson_f(lye, this%en%ene, this%en%ene(ie), this%en%nv1, lyi, .true., .false., 0.0d0)
               call simpson_f(lze, this%en%ene, this%en%ene(ie), this%en%nv1, lzi, .true., .false., 0.0d0)
            end if
            write (unitorb, '(4es16.6)') this%en%ene(ie) - this%en%fermi, -(lxe/pi), -(lye/pi), -(lze/pi)
         end do
         if (.not. this%device_tail) call g_timer%stop('moment-integrals-host')
         rewind (unitorb)
         close (unitorb)

         lz = -(lz/pi)
         lx = -(lx/pi)
         ly = -(ly/pi)

         call g_logger%info('Orbital moment of atom'//fmt('i4', na)//' is '//fmt('f10.6', lx)//' '//fmt('f10.6', ly)//' '//fmt('f10.6', lz), __FILE__, __LINE__)
         this%symbolic_atom(this%lattice%nbulk + na)%potential%lmom(1) = lx
         this%symbolic_atom(this%lattice%nbulk + na)%potential%lmom(2) = ly
         this%symbolic_atom(this%lattice%nbulk + na)%potential%lmom(3) = lz
      end do
   end subroutine gpu_calculate_orbital_moments

   !> calculate_orbital_quadrupoles (bands.f90:878-1067).  On the spectra route with the device tail -- the chains still resident, g0 still
   !> pending -- the six Q operators (:906-955) go through one spectra call and one integrals call: Im Tr(Q g0) of :985-993, simpson_m of
   !> :998-1004 and the cumulative simpson_f of :1019-1025 without a g0; the file and the two log lines are the reference's.  (The
   !> reference first calls calculate_orbital_dos, which reads g0; the quadrupoles read nothing of what it leaves.)  In every other case: g0
   !> and the reference's routine.
   subroutine gpu_calculate_orbital_quadrupoles(this)
      class(bands_gpu) :: this
      real(rp) :: q(6), qe(6), qx2y2, q3z2r2
      integer :: na, ie, k, nv, nrec, unitquad
      integer(c_int) :: rc, sym_i
      type(c_ptr) :: handle
      character(len=256) :: fnamequad
      complex(rp), dimension(9, 9) :: mL
      complex(rp), dimension(18, 18, 3) :: mL_ext
      complex(rp), dimension(:, :, :), allocatable, target :: ops
      real(rp), dimension(:, :, :), allocatable, target :: qspec, qmom, qcum
      real(rp), allocatable, target :: ene(:)

      if (.not. (spectra_route(this) .and. this%device_tail)) then
         call ensure_g0(this)
         call this%bands%calculate_orbital_quadrupoles()
         return
      end if

      mL_ext = (0.0_rp, 0.0_rp)
      do k = 1, 3
         select case (k)
         case (1); mL = L_x
         case (2); mL = L_y
         case (3); mL = L_z
         end select
         call hcpx(mL, 'cart2sph')
         mL_ext(1:9, 1:9, k) = mL
         mL_ext(10:18, 10:18, k) = mL
      end do
      allocate (ops(18, 18, 6))
      ops(:, :, 1) = matmul(mL_ext(:, :, 1), mL_ext(:, :, 1))                                                             ! Qxx, Qyy, Qzz
      ops(:, :, 2) = matmul(mL_ext(:, :, 2), mL_ext(:, :, 2))
      ops(:, :, 3) = matmul(mL_ext(:, :, 3), mL_ext(:, :, 3))
      ops(:, :, 4) = 0.5_rp*(matmul(mL_ext(:, :, 1), mL_ext(:, :, 2)) + matmul(mL_ext(:, :, 2), mL_ext(:, :, 1)))         ! Qxy, Qyz, Qzx
      ops(:, :, 5) = 0.5_rp*(matmul(mL_ext(:, :, 2), mL_ext(:, :, 3)) + matmul(mL_ext(:, :, 3), mL_ext(:, :, 2)))
      ops(:, :, 6) = 0.5_rp*(matmul(mL_ext(:, :, 3), mL_ext(:, :, 1)) + matmul(mL_ext(:, :, 1), mL_ext(:, :, 3)))

      nv = this%en%channels_ldos + 10
      nrec = this%lattice%nrec
      allocate (ene(nv), qspec(6, nv, nrec), qmom(3, 6, nrec), qcum(6, nv, nrec))
      ene = this%en%ene(1:nv)
      sym_i = 0
      if (this%control%sym_term) sym_i = 1
      handle = rsrec_gpu_context()
      call g_timer%start('spectra-gpu')
      if (trim(this%control%recur) == 'chebyshev') then
         rc = rsrec_chebyshev_spectra(handle, 6_c_int, c_loc(ops), int(nv, c_int), c_loc(ene), real(this%en%energy_min, c_double), &
                                      real(this%en%energy_max, c_double), int(start_atom - 1, c_int), int(nrec, c_int), c_loc(qspec))
      else
         rc = rsrec_block_spectra(handle, 6_c_int, c_loc(ops), int(nv, c_int), c_loc(ene), 0.0_c_double, 0.0_c_double, sym_i, &
                                  int(start_atom - 1, c_int), int(nrec, c_int), c_loc(qspec))
      end if
      call g_timer%stop('spectra-gpu')
      if (rc /= 0) call g_logger%fatal('rsrec_'//trim(this%control%recur)//'_spectra: '//rsrec_error_string(handle), __FILE__, __LINE__)
      this%n_device_spectra = this%n_device_spectra + 1
      ! (the handle's resident image is now the six-row one, not the 15 rows of ensure_spectra: spectra_tail(resident = .true.) is only ever
      ! called from ensure_spectra, right behind its own spectra call; every later repeat (ensure_tail) passes the type's copy this%spec)
      call g_timer%start('moment-integrals-gpu')
      rc = rsrec_spectra_integrals(handle, 6_c_int, c_null_ptr, 6_c_int, c_null_ptr, int(nv, c_int), c_loc(ene), int(this%en%nv1, c_int), &
                                   int(this%nv1, c_int), real(this%en%edel, c_double), real(this%e1, c_double), real(this%en%fermi, c_double), &
                                   int(end_atom - start_atom + 1, c_int), int(start_atom - 1, c_int), int(nrec, c_int), c_loc(qmom), c_loc(qcum))
      call g_timer%stop('moment-integrals-gpu')
      if (rc /= 0) call g_logger%fatal('rsrec_spectra_integrals: '//rsrec_error_string(handle), __FILE__, __LINE__)
      this%n_device_tail = this%n_device_tail + 1

      do na = start_atom, end_atom
         fnamequad = trim(this%symbolic_atom(this%lattice%nbulk + na)%element%symbol)//"_orbquadene.out"
         unitquad = (rank + 1)*132 + na
         open (unit=unitquad, file=fnamequad, status='replace', action='write')
         do ie = 1, nv
            qe = qcum(:, ie, na)
            write (unitquad, '(9es16.6)') this%en%ene(ie) - this%en%fermi, &
               -(qe(1)/pi), -(qe(2)/pi), -(qe(3)/pi), &
               -(qe(4)/pi), -(qe(5)/pi), -(qe(6)/pi), &
               -((qe(1) - qe(2))/pi), &
               -((2.0_rp*qe(3) - qe(1) - qe(2))/pi)
         end do
         rewind (unitquad)
         close (unitquad)

         q = -(qmom(1, :, na)/pi)
         qx2y2 = q(1) - q(2)
         q3z2r2 = 2.0_rp*q(3) - q(1) - q(2)

         call g_logger%info('Orbital quadrupoles of atom'//fmt('i4', na)// &
                            ' Qxx Qyy Qzz Qxy Qyz Qzx = '// &
                            fmt('f10.6', q(1))//' '//fmt('f10.6', q(2))//' '//fmt('f10.6', q(3))//' '// &
                            fmt('f10.6', q(4))//' '//fmt('f10.6', q(5))//' '//fmt('f10.6', q(6)), &
                            __FILE__, __LINE__)
         call g_logger%info('Traceless orbital quadrupoles of atom'//fmt('i4', na)// &
                            ' Qx2y2 Q3z2r2 = '// &
                            fmt('f10.6', qx2y2)//' '//fmt('f10.6', q3z2r2), &
                            __FILE__, __LINE__)
      end do
   end subroutine gpu_calculate_orbital_quadrupoles

   !> calculate_moments (bands.f90:409-524): dspd from the image and the (mixed) moment directions, the tail restated.  Local-axis runs
   !> (chains resident in each site's frame, RSREC_LOCAL_AXIS_DEVICE) rotate every site's direction back to the global frame inside the
   !> atom loop, as :427-432 and :458-467 do.
   subroutine gpu_calculate_moments(this)
      class(bands_gpu) :: this
      integer :: i, l, ie, na, na_glob, isp, soff, nsp, plusbulk
      real(rp) :: sgef, pmef, smef, isgn, mnorm
      real(rp), dimension(3) :: mom
      real(rp), dimension(this%en%channels_ldos + 10) :: y
      real(rp), dimension(3, atoms_per_process) :: mom_prev, mom_used
      real(rp), dimension(3) :: band_int
#ifdef USE_MPI
      integer :: pot_size
      real(rp), dimension(:, :), allocatable :: T_comm
#endif

      if (.not. spectra_route(this)) then
         call ensure_g0(this)
         call this%bands%calculate_moments()
         return
      end if

      do na_glob = start_atom, end_atom                             ! bands.f90:427-432
         na = g2l_map(na_glob)
         plusbulk = this%lattice%nbulk + na_glob
         mom_prev(:, na) = this%symbolic_atom(plusbulk)%potential%mom
      end do

      call this%calculate_orbital_moments()
      call ensure_tail(this)

      this%dspd(:, :, :) = 0.0d0
      do na_glob = start_atom, end_atom
         na = g2l_map(na_glob)
         plusbulk = this%lattice%nbulk + na_glob
         mom = this%symbolic_atom(plusbulk)%potential%mom
         mom_used(:, na) = mom
         do isp = 1, 2
            isgn = (-1.0d0)**(isp - 1)
            soff = 3*(isp - 1)
            do l = 1, 3
               do ie = 1, this%en%channels_ldos
                  this%dspd(l + soff, ie, na) = -this%spec(l, ie, na_glob) - isgn*mom(3)*this%spec(9 + l, ie, na_glob) &
                                                - isgn*mom(2)*this%spec(6 + l, ie, na_glob) - isgn*mom(1)*this%spec(3 + l, ie, na_glob)
               end do
            end do
         end do
         if (this%recursion%hamiltonian%local_axis) then            ! bands.f90:458-467
            call updatrotmom_single(this%symbolic_atom(plusbulk)%potential%mom, mom_prev(:, na))
            call this%symbolic_atom(plusbulk)%potential%copy_mom_to_scal()

            mnorm = this%symbolic_atom(plusbulk)%potential%mtot
            call g_logger%info('Global spin moment projections of atom'//fmt('i4', na)//' is '// &
                               fmt('f10.6', this%symbolic_atom(plusbulk)%potential%mom(1)*mnorm)//' '// &
                               fmt('f10.6', this%symbolic_atom(plusbulk)%potential%mom(2)*mnorm)//' '// &
                               fmt('f10.6', this%symbolic_atom(plusbulk)%potential%mom(3)*mnorm), __FILE__, __LINE__)
         end if
      end do
      this%dspd(:, :, :) = this%dspd(:, :, :)*0.5d0/pi

      do na_glob = start_atom, end_atom
         na = g2l_map(na_glob)
         plusbulk = this%lattice%nbulk + na_glob
         do i = 1, 6
            if (i > 3) then
               nsp = 2
            else
               nsp = 1
            end if
            soff = 3*(nsp - 1)
            sgef = 0.0d0; pmef = 0.0d0; smef = 0.0d0
            if (this%device_tail) then
               ! the dspd row is a combination of four rows of the image (see above), and so are its integrals
               l = i - soff
               isgn = (-1.0d0)**(nsp - 1)
               mom = mom_used(:, na)
               band_int(:) = (-this%tail_mom(:, l, na_glob) - isgn*mom(3)*this%tail_mom(:, 9 + l, na_glob) &
                              - isgn*mom(2)*this%tail_mom(:, 6 + l, na_glob) - isgn*mom(1)*this%tail_mom(:, 3 + l, na_glob))*0.5d0/pi
               sgef = band_int(1); pmef = band_int(2); smef = band_int(3)
            else
               y(:) = this%dspd(i, :, na)
               call g_timer%start('moment-integrals-host')
               call simpson_m(sgef, this%en%edel, this%en%fermi, this%nv1, y, this%e1, 0, this%en%ene)
               call simpson_m(pmef, this%en%edel, this%en%fermi, this%nv1, y, this%e1, 1, this%en%ene)
               call simpson_m(smef, this%en%edel, this%en%fermi, this%nv1, y, this%e1, 2, this%en%ene)
               call g_timer%stop('moment-integrals-host')
            end if
            this%symbolic_atom(plusbulk)%potential%gravity_center(i - soff, nsp) = (pmef/sgef) - this%symbolic_atom(plusbulk)%potential%vmad
            this%symbolic_atom(plusbulk)%potential%ql(1, i - soff - 1, nsp) = sgef
            this%symbolic_atom(plusbulk)%potential%ql(2, i - soff - 1, nsp) = 0.0d0
            this%symbolic_atom(plusbulk)%potential%ql(3, i - soff - 1, nsp) = smef - 2.0d0*(pmef/sgef)*pmef + ((pmef/sgef)**2)*sgef
         end do
      end do

      call this%calculate_pl()

#ifdef USE_MPI
      pot_size = this%symbolic_atom(start_atom)%potential%sizeof_potential_lite()
      allocate (T_comm(pot_size, this%lattice%nrec))
      T_comm = 0.0_rp
      do na_glob = start_atom, end_atom
         call this%symbolic_atom(this%lattice%nbulk + na_glob)%potential%flatten_potential_lite(T_comm(:, na_glob))
      end do
      call MPI_ALLREDUCE(MPI_IN_PLACE, T_comm, product(shape(T_comm)), MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)
      do na_glob = 1, this%lattice%nrec
         call this%symbolic_atom(this%lattice%nbulk + na_glob)%potential%expand_potential_lite(T_comm(:, na_glob))
      end do
      deallocate (T_comm)
#endif
   end subroutine gpu_calculate_moments

   !> occ(site, orbital) of the rank's sites on the 64-point Gauss-Legendre contour at ene(fermi_point), from the on-site chains the
   !> recursion left on the device: one rsrec_contour_occupation call (the loop of bands.f90:559-586 / :631-650: block_green_eta or
   !> chebyshev_green_eta at 64 points, the terminator once per chain instead of once per point)
   subroutine occupation_on_device(this, fermi_point, occ)
      class(bands_gpu), intent(inout) :: this
      integer, intent(in) :: fermi_point
      real(rp), dimension(this%lattice%nrec, 18), intent(out) :: occ
      real(rp), dimension(64), target :: x, w
      real(rp), dimension(:, :), allocatable, target :: img
      integer(c_int) :: rc, sym_i, ikind
      type(c_ptr) :: ctx

      call gauss_legendre(64, 0.0_rp, 1.0_rp, x, w)
      allocate (img(18, this%lattice%nrec))
      img = 0.0_rp
      ikind = 0
      if (trim(this%control%recur) == 'chebyshev') ikind = 1
      sym_i = 0
      if (this%control%sym_term) sym_i = 1
      ctx = rsrec_gpu_context()
      call g_timer%start('contour-occupation-gpu')
      rc = rsrec_contour_occupation(ctx, ikind, int(end_atom - start_atom + 1, c_int), int(this%control%lld, c_int), 64_c_int, c_loc(x), &
                                    c_loc(w), real(this%en%ene(fermi_point), c_double), sym_i, real(this%en%energy_min, c_double), &
                                    real(this%en%energy_max, c_double), c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                                    int(start_atom - 1, c_int), int(this%lattice%nrec, c_int), c_loc(img), c_null_ptr)
      call g_timer%stop('contour-occupation-gpu')
      if (rc /= 0) call g_logger%fatal('bands_gpu: rsrec_contour_occupation: '//rsrec_error_string(ctx), __FILE__, __LINE__)
      occ = transpose(img)
   end subroutine occupation_on_device

   !> calculate_moments_gauss_legendre (bands.f90:526-604): occ from the device, the rest the reference's lines
   subroutine gpu_calculate_moments_gauss_legendre(this)
      class(bands_gpu) :: this
      integer :: i, m, fermi_point
      real(rp) :: sumocc
      real(rp), dimension(this%lattice%nrec, 18) :: occ

      if (.not. device_stage_usable(this)) then
         call this%bands%calculate_moments_gauss_legendre()
         return
      end if

      call this%en%e_mesh()

      fermi_point = 0
      do i = 1, this%en%channels_ldos + 10
         if ((this%en%ene(i) - this%en%fermi) .le. 0.0001d0) fermi_point = i
      end do
      if (rank == 0) write (*, *) this%en%fermi, fermi_point

      call occupation_on_device(this, fermi_point, occ)

      ! Transfer calculated occupations across MPI
#ifdef USE_MPI
      call MPI_ALLREDUCE(MPI_IN_PLACE, occ, product(shape(occ)), MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)
#endif

      sumocc = 0.0d0
      do m = 1, this%lattice%nrec
         if (rank == 0) call g_logger%info('Spin moment of atom'//fmt('i4', m)//' is '//fmt('f10.6', sum(occ(m, 1:9)) - sum(occ(m, 10:18))), __FILE__, __LINE__)
         if (rank == 0) call g_logger%info('Total charge for atom'//fmt('i4', m)//' is '// &
                                           'total= '//fmt('f10.6', sum(occ(m, 1:18)))// &
                                           ' s= '//fmt('f10.6', occ(m, 1) + occ(m, 10))// &
                                           ' p= '//fmt('f10.6', sum(occ(m, 2:4)) + sum(occ(m, 11:13)))// &
                                           ' d= '//fmt('f10.6', sum(occ(m, 5:9)) + sum(occ(m, 14:18))), __FILE__, __LINE__)
         sumocc = sumocc + sum(occ(m, :))
      end do
      if (rank == 0) call g_logger%info('Total number of electrons is '//fmt('f16.6', sumocc), __FILE__, __LINE__)
   end subroutine gpu_calculate_moments_gauss_legendre

   !> calculate_occupation_gauss_legendre (bands.f90:606-656), which calculate_fermi_gauss bisects on.  The reference uses block_green_eta
   !> whatever control%recur is and sizes its arrays for one rank: the device path is taken for block chains on a single rank only.
   subroutine gpu_calculate_occupation_gauss_legendre(this, fermi_energy, sumocc_out)
      class(bands_gpu) :: this
      real(rp), intent(in)  :: fermi_energy
      real(rp), intent(out) :: sumocc_out
      integer :: i, m, fermi_point
      real(rp), dimension(this%lattice%nrec, 18) :: occ

      if (.not. (device_stage_usable(this) .and. trim(this%control%recur) == 'block' .and. numprocs == 1)) then
         call this%bands%calculate_occupation_gauss_legendre(fermi_energy, sumocc_out)
         return
      end if

      fermi_point = 0
      do i = 1, this%en%channels_ldos + 10
         if ((this%en%ene(i) - fermi_energy) .le. 0.001d0) fermi_point = i
      end do
      write (*, *) fermi_energy, fermi_point

      call occupation_on_device(this, fermi_point, occ)

      sumocc_out = 0.0d0
      do m = 1, this%lattice%nrec
         sumocc_out = sumocc_out + sum(occ(m, :))
      end do
      write (*, *) 'Total electrons:', sumocc_out
   end subroutine gpu_calculate_occupation_gauss_legendre

   subroutine gpu_calculate_projected_green(this)
      class(bands_gpu) :: this
      call ensure_g0(this)
      call this%bands%calculate_projected_green()
   end subroutine gpu_calculate_projected_green

   !> calculate_projected_dos (bands.f90:1158-1181): dx, dy, dz are the s + p + d sums of the x, y, z brackets of the image
   subroutine gpu_calculate_projected_dos(this)
      class(bands_gpu) :: this
      integer :: na, na_glob, ie
      if (.not. spectra_route(this)) then
         call ensure_g0(this)
         call this%bands%calculate_projected_dos()
         return
      end if
      call ensure_spectra(this)
      this%dz = 0.0d0; this%dy = 0.0d0; this%dx = 0.0d0
      do na_glob = start_atom, end_atom
         na = g2l_map(na_glob)
         do ie = 1, this%en%channels_ldos + 10
            this%dz(ie, na) = -(this%spec(10, ie, na_glob) + this%spec(11, ie, na_glob) + this%spec(12, ie, na_glob))/pi
            this%dy(ie, na) = -(this%spec(7, ie, na_glob) + this%spec(8, ie, na_glob) + this%spec(9, ie, na_glob))/pi
            this%dx(ie, na) = -(this%spec(4, ie, na_glob) + this%spec(5, ie, na_glob) + this%spec(6, ie, na_glob))/pi
         end do
      end do
   end subroutine gpu_calculate_projected_dos

   subroutine gpu_calculate_orbital_dos(this)
      class(bands_gpu) :: this
      call ensure_g0(this)
      call this%bands%calculate_orbital_dos()
   end subroutine gpu_calculate_orbital_dos

end module bands_gpu_mod
