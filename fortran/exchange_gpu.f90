!------------------------------------------------------------------------------
! exchange_gpu_mod -- GPU drop-in for type(exchange) (exchange.f90:46-96).
!
! green%calculate_intersite_gf / _twoindex (green.f90:386-469) and the integrands and Fermi-weighted Simpson integrals of
! calculate_exchange / _twoindex (exchange.f90:1032-1615) are one call of librsrec, rsrec_exchange, on the chains the pair recursion
! (recursion_gpu%recur_b_ij / chebyshev_recur_ij) left on the device; the 24 intersite arrays (0.1 GB per pair at 2500 energies) are
! never formed (rslmtoasa_amd/csrc/kernels_exchange.hpp).  So:
!   constructor                 : the reference's, then green_gpu is told that the intersite stage is done here (its
!                                 calculate_intersite_gf / _twoindex then allocate and fill nothing)
!   calculate_exchange          : the call for the rank's pairs, then the reference's tail (:1543-1612) restated line for line: the
!                                 MPI_ALLREDUCE, the rank-0 stdout lines, jij.out / dij.out / aij.out / jtens.out and unit 99
!   calculate_exchange_twoindex : the values of that call (or the call, if calculate_exchange did not run), then the eleven files of
!                                 :1061-1131 and fort.150 in the reference's formats and order
! What stays on the host is O(pairs): the T_comm images and the formatting, plus fort.150's cumulative J of the rank's pairs (one real
! per pair and energy, 20 KB per pair at 2500 energies) between the two routines.
!   calculate_gilbert_damping   : (:613-743) the nsp == 2 guard and hamiltonian%torque_operator_collinear on the host, then one
!                                 rsrec_damping call on the same resident chains for the rank's pairs (the traces of :674-694 without
!                                 gij / gji or the seven temporaries), the reduction of its images over the ranks, and the reference's
!                                 tail (:695-733): the nearest-energy search, the stdout lines, alldampings.out and damping-energy.out
!                                 in its formats, written by rank 0.
!                                 One deliberate deviation: the reference never initialises spin_i in this routine, so it starts
!                                 undefined and accumulates across the pairs; here it starts at zero for every pair.
!                                 damping-energy.out uses the last pair's factor, as the reference's code does.
!   calculate_jijk              : (:338-601) one rsrec_spin_lattice call for all trios on the resident chains (timer region jijk-gpu):
!                                 apar = (c + vmad, dele, qpar) of atoms i, j, k from potential, dmat = one spin block of the
!                                 reference's own disp_matrix of atom k for uni_disp, then the reference's three stdout lines per trio
!                                 (:558-560), format for format.  Neither green%gij / gji nor the 18 work arrays per trio are formed.
!                                 Falls back to the host route below when an atom has lmax /= 2, when the pairs are not exactly the
!                                 trios' pairs, or when the rank does not hold every pair (more than one rank).
!   calculate_moment_of_inertia, calculate_jij_auxgreen : these read green%gij / gji ..., which the constructor released.  Each is a
!                                 wrapper: green_gpu%fetch_intersite first (the host arrays, allocated and filled by the inherited
!                                 calculate_intersite_gf / _twoindex from the recursion's host coefficients), then the inherited
!                                 routine.  The moment of inertia defines no result to match (its final loop indexes with nv after
!                                 the energy loop has ended, :869-882).  Jij_aux is on the device through the library
!                                 (rsrec_exchange_aux) and Exchange.aux only: this type keeps the host route for it.
!   calculate_exchange_gauss_legendre : (:1756-1919) one rsrec_exchange_contour call for the rank's pairs on the resident chains
!                                 (green%calculate_intersite_gf_eta + the 64-point loop of :1811-1867: the terminator once per chain
!                                 instead of once per point, no _eta array, no gij_eta_to_gij), x and w from the reference's own
!                                 gauss_legendre, e0 = ene(fermi_point) with the `.le. 1.0d-6` rule of green.f90:489-491; then the
!                                 reference's tail (:1869-1918) restated line for line.
!                                 One deliberate deviation, i == j pairs: recur_b_ij runs one chain for such a pair and never writes
!                                 slots 2..4 (recursion.f90:1702-1707), and the reference's contour routine combines chain 1 with
!                                 those unwritten slots; here gij = gji = g(chain 1), as calculate_intersite_gf takes it
!                                 (green.f90:446-448).
! Errors of the library become g_logger%fatal, the reference's error behaviour on this path.
!------------------------------------------------------------------------------
module exchange_gpu_mod
   use, intrinsic :: iso_c_binding
   use exchange_mod
   use bands_mod, only: bands
   use green_gpu_mod, only: green_gpu
   use mpi_mod
   use precision_mod, only: rp
   use math_mod, only: pi, gauss_legendre
   use logger_mod, only: g_logger
   use timer_mod, only: g_timer
   use rsrec_binding
   use rsrec_context_mod, only: rsrec_gpu_context
#ifdef USE_MPI
   use mpi
#endif
   implicit none

   private

   type, public, extends(exchange) :: exchange_gpu
      !> T_comm_xc, T_comm_xcso, T_comm_xcfo (13, njij) and T_comm_xcparts (28, njij) of the last call, reduced over the ranks
      real(rp), dimension(:, :), allocatable :: xc, so, fo, parts
      !> fort.150's second column for the rank's pairs (channels_ldos + 10, end_atom - start_atom + 1)
      real(rp), dimension(:, :), allocatable :: jcum
   contains
      procedure :: calculate_exchange => gpu_calculate_exchange
      procedure :: calculate_exchange_twoindex => gpu_calculate_exchange_twoindex
      procedure :: calculate_gilbert_damping => gpu_calculate_gilbert_damping
      procedure :: calculate_exchange_gauss_legendre => gpu_calculate_exchange_gauss_legendre
      procedure :: calculate_moment_of_inertia => gpu_calculate_moment_of_inertia
      procedure :: calculate_jij_auxgreen => gpu_calculate_jij_auxgreen
      procedure :: calculate_jijk => gpu_calculate_jijk
   end type exchange_gpu

   interface exchange_gpu
      procedure :: gpu_constructor
   end interface exchange_gpu

contains

   !> constructor (:101-115)
   function gpu_constructor(bands_obj) result(obj)
      type(exchange_gpu) :: obj
      type(bands), target, intent(in) :: bands_obj

      obj%bands => bands_obj
      obj%green => bands_obj%green
      obj%lattice => bands_obj%lattice
      obj%symbolic_atom => bands_obj%symbolic_atom
      obj%en => bands_obj%en
      obj%control => bands_obj%lattice%control
      obj%recursion => bands_obj%recursion
      obj%hamiltonian => bands_obj%recursion%hamiltonian

      call obj%restore_to_default()
      ! the intersite stage is ours: green's arrays go, its calculate_intersite_gf / _twoindex only keep their side effect (green_gpu.f90)
      select type (g => obj%green)
      class is (green_gpu)
         call g%release_intersite()
      end select
   end function gpu_constructor

   !> What the device routines take alike for the pairs first .. last of lattice%ijpair: the kind of the pair recursion (a control%recur
   !> without one is fatal), control%sym_term as the library takes it, and same(p) = 1 where pair first + p - 1 is an i == j pair
   subroutine pair_front(this, first, last, ikind, sym_i, same)
      class(exchange_gpu), intent(in) :: this
      integer, intent(in) :: first, last
      integer(c_int), intent(out) :: ikind, sym_i
      integer(c_int), dimension(:), allocatable, target, intent(out) :: same
      integer :: ij

      select case (this%control%recur)
      case ('block')
         ikind = 0
      case ('chebyshev')
         ikind = 1
      case default
         call g_logger%fatal('exchange_gpu: control%recur '//trim(this%control%recur)//' has no pair recursion', __FILE__, __LINE__)
      end select
      sym_i = merge(1_c_int, 0_c_int, this%control%sym_term)
      allocate (same(max(last - first + 1, 0)))
      do ij = first, last
         same(ij - first + 1) = merge(1_c_int, 0_c_int, this%lattice%ijpair(ij, 1) == this%lattice%ijpair(ij, 2))
      end do
   end subroutine pair_front

   !> rsrec_exchange for the pairs start_atom .. end_atom of this rank (get_mpi_variables over njij), on the resident chains of the
   !> pair recursion; the images are reduced over the ranks as :1543-1546 / :1375-1382 reduce theirs.
   subroutine exchange_on_device(this)
      class(exchange_gpu), intent(inout) :: this
      integer :: nloc, nen, njij, p, ij, side, l, at
      integer(c_int) :: rc, ikind, sym_i
      type(c_ptr) :: ctx
      integer(c_int), dimension(:), allocatable, target :: same
      real(rp), dimension(:), allocatable, target :: ene
      real(rp), dimension(:, :, :, :), allocatable, target :: dpar
      real(rp), dimension(:, :), allocatable, target :: xc, so, fo, parts, jcum

      nen = this%en%channels_ldos + 10
      njij = this%lattice%njij
      nloc = end_atom - start_atom + 1
      call pair_front(this, start_atom, end_atom, ikind, sym_i, same)
      allocate (xc(13, njij), so(13, njij), fo(13, njij), parts(28, njij), jcum(nen, max(nloc, 0)))
      xc = 0.0_rp; so = 0.0_rp; fo = 0.0_rp; parts = 0.0_rp; jcum = 0.0_rp
      if (nloc > 0) then
         allocate (ene(nen), dpar(4, 3, 2, nloc))
         ene(:) = this%en%ene(1:nen)
         ! d_matrix's parameters of atoms i and j (symbolic_atom.f90:250-255): (c_up + vmad, c_dn + vmad, dele_up, dele_dn) per l
         do ij = start_atom, end_atom
            p = ij - start_atom + 1
            do side = 1, 2
               at = this%lattice%iz(this%lattice%ijpair(ij, side))
               associate (pot => this%symbolic_atom(at)%potential)
                  do l = 0, 2
                     dpar(1, l + 1, side, p) = pot%c(l, 1) + pot%vmad
                     dpar(2, l + 1, side, p) = pot%c(l, 2) + pot%vmad
                     dpar(3, l + 1, side, p) = pot%dele(l, 1)
                     dpar(4, l + 1, side, p) = pot%dele(l, 2)
                  end do
               end associate
            end do
         end do
         ctx = rsrec_gpu_context()
         call g_timer%start('exchange-gpu')
         ! coefficients and terminators NULL: the chains recur_b_ij / chebyshev_recur_ij left on the device (i == j pairs: one chain)
         rc = rsrec_exchange(ctx, ikind, int(nloc, c_int), c_loc(same), int(this%control%lld, c_int), int(nen, c_int), &
                             c_loc(ene), int(this%en%nv1, c_int), real(this%en%fermi, c_double), sym_i, &
                             real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), c_null_ptr, c_null_ptr, &
                             c_null_ptr, c_null_ptr, c_loc(dpar), int(start_atom - 1, c_int), int(njij, c_int), c_loc(xc), c_loc(so), &
                             c_loc(fo), c_loc(parts), c_loc(jcum), c_null_ptr)
         call g_timer%stop('exchange-gpu')
         if (rc /= 0) call g_logger%fatal('exchange_gpu: rsrec_exchange: '//rsrec_error_string(ctx), __FILE__, __LINE__)
      end if
#ifdef USE_MPI
      call MPI_ALLREDUCE(MPI_IN_PLACE, xc, product(shape(xc)), MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)
      call MPI_ALLREDUCE(MPI_IN_PLACE, so, product(shape(so)), MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)
      call MPI_ALLREDUCE(MPI_IN_PLACE, fo, product(shape(fo)), MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)
      call MPI_ALLREDUCE(MPI_IN_PLACE, parts, product(shape(parts)), MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)
#endif
      call move_alloc(xc, this%xc)
      call move_alloc(so, this%so)
      call move_alloc(fo, this%fo)
      call move_alloc(parts, this%parts)
      call move_alloc(jcum, this%jcum)
   end subroutine exchange_on_device

   !> open `fname` on `funit` as :1467-1490 / :1061-1131 do (a unit already open is fatal)
   subroutine open_unit(funit, fname, what)
      integer, intent(in) :: funit
      character(len=*), intent(in) :: fname, what
      logical :: isopen
      inquire (unit=funit, opened=isopen)
      if (isopen) then
         call g_logger%fatal('exchange%calculate_exchange, file '//what, __FILE__, __LINE__)
      else
         open (unit=funit, file=fname)
      end if
   end subroutine open_unit

   !> the records of the pair (i, j) in jij.out, dij.out and aij.out (units 20, 30, 40) and its line on unit 99 (:1589-1596, :1905-1912),
   !> from its column of T_comm_xc: Jij | Dij | Iij
   subroutine write_pair_records(this, i, j, col)
      class(exchange_gpu), intent(in) :: this
      integer, intent(in) :: i, j
      real(rp), dimension(13), intent(in) :: col

      associate (iz => this%lattice%iz, cr => this%lattice%cr)
         write (20, '(2i8,2x,3f12.6,2x,1f12.6,1x,f12.6)') iz(i), iz(j), cr(:, j) - cr(:, i), col(1), norm2(cr(:, i) - cr(:, j))
         write (30, '(2i8,2x,3f12.6,2x,3f12.6,1x,f12.6)') iz(i), iz(j), cr(:, j) - cr(:, i), col(2:4), norm2(cr(:, i) - cr(:, j))
         write (40, '(2i8,2x,3f12.6,2x,9f12.6,1x,f12.6)') iz(i), iz(j), cr(:, j) - cr(:, i), col(5:13), norm2(cr(:, i) - cr(:, j))
         write (99, *) 'null', (cr(:, j) + cr(:, i))/2, col(2:4)/norm2(col(2:4))
      end associate
   end subroutine write_pair_records

   !> calculate_exchange (:1437-1615)
   subroutine gpu_calculate_exchange(this)
      class(exchange_gpu) :: this
      real(rp), dimension(3, 3) :: jtens
      integer :: i, j, njij_glob

      call exchange_on_device(this)

      call open_unit(20, 'jij.out', 'jij.out: Unit 20 is already open')
      call open_unit(30, 'dij.out', 'dij.out: Unit 30 is already open')
      call open_unit(40, 'aij.out', 'aij.out: Unit 40 is already open')
      call open_unit(60, 'jtens.out', 'jtens.out: Unit 40 is already open')

      ! :1549-1603
      if (rank == 0) then
         do njij_glob = 1, this%lattice%njij
            i = this%lattice%ijpair(njij_glob, 1)
            j = this%lattice%ijpair(njij_glob, 2)

            write (*, *) 'Atom', i, 'coordinates:', this%lattice%cr(:, i)
            write (*, *) 'Atom', j, 'coordinates:', this%lattice%cr(:, j)

            this%jij = this%xc(1, njij_glob)
            write (*, *) 'Jij between pair', i, 'and ', j, 'is ', this%jij
            this%dmi = this%xc(2:4, njij_glob)
            write (*, *) 'Dij between pair', i, 'and ', j, 'is ', this%dmi
            this%aij = reshape(this%xc(5:13, njij_glob), [3, 3])
            write (*, *) 'Iij between pair', i, 'and ', j, 'is'
            print '(3f12.6)', this%aij(1, :)
            print '(3f12.6)', this%aij(2, :)
            print '(3f12.6)', this%aij(3, :)

            call write_pair_records(this, i, j, this%xc(:, njij_glob))
            jtens = 0.0d0
            jtens(1, 1) = this%jij
            jtens(2, 2) = jtens(1, 1)
            jtens(3, 3) = jtens(1, 1)
            jtens(1, 2) = this%dmi(3)
            jtens(2, 1) = -jtens(1, 2)
            jtens(1, 3) = -this%dmi(2)
            jtens(3, 1) = -jtens(1, 3)
            jtens(2, 3) = this%dmi(1)
            jtens(3, 2) = -jtens(2, 3)
            jtens(:, :) = jtens(:, :) + this%aij(:, :)
            write (*, *) 'J tensor between pair', i, 'and ', j, 'is'
            print '(3f12.6)', jtens(1, :)
            print '(3f12.6)', jtens(2, :)
            print '(3f12.6)', jtens(3, :)
         end do
      end if

      close (20)
      close (30)
      close (40)
      close (60)

#ifdef USE_MPI
      call MPI_BARRIER(MPI_COMM_WORLD, ierr)
#endif
   end subroutine gpu_calculate_exchange

   !> calculate_exchange_twoindex (:1032-1435)
   subroutine gpu_calculate_exchange_twoindex(this)
      class(exchange_gpu) :: this
      integer :: i, j, nv, njij_glob

      if (.not. allocated(this%jcum)) call exchange_on_device(this)

      call open_unit(20, 'jijso.out', 'jijso.out: Unit 20 is already open')
      call open_unit(25, 'jijfo.out', 'jijfo.out: Unit 25 is already open')
      call open_unit(30, 'dijso.out', 'dijso.out: Unit 30 is already open')
      call open_unit(35, 'dijfo.out', 'dijfo.out: Unit 30 is already open')
      call open_unit(40, 'aijso.out', 'aijso.out: Unit 40 is already open')
      call open_unit(45, 'aijfo.out', 'aijfo.out: Unit 45 is already open')
      call open_unit(60, 'jtensfo.out', 'jtensso.out: Unit 60 is already open')
      call open_unit(65, 'jtensso.out', 'jtensfo.out: Unit 65 is already open')
      call open_unit(70, 'jijparts.out', 'jijparts.out: Unit 70 is already open')
      call open_unit(75, 'dijparts.out', 'dijparts.out: Unit 75 is already open')
      call open_unit(80, 'aijparts.out', 'aijparts.out: Unit 80 is already open')

      ! :1281-1285: fort.150, per pair of this rank in order, written before the reduction
      do njij_glob = start_atom, end_atom
         do nv = 1, this%en%channels_ldos + 10
            write (150, *) this%en%ene(nv) - this%en%fermi, this%jcum(nv, njij_glob - start_atom + 1)
         end do
      end do

      ! :1385-1414
      if (rank == 0) then
         do njij_glob = 1, this%lattice%njij
            i = this%lattice%ijpair(njij_glob, 1)
            j = this%lattice%ijpair(njij_glob, 2)

            this%jij = this%so(1, njij_glob)
            write (20, '(2i8,2x,3e20.11,2x,1es16.6,1x,f12.6)') &
               this%lattice%iz(i), this%lattice%iz(j), this%lattice%cr(:, j) - this%lattice%cr(:, i), this%jij, norm2(this%lattice%cr(:, i) - this%lattice%cr(:, j))
            this%jij = this%fo(1, njij_glob)
            write (25, '(2i8,2x,3e20.11,2x,1es16.6,1x,f12.6)') &
               this%lattice%iz(i), this%lattice%iz(j), this%lattice%cr(:, j) - this%lattice%cr(:, i), this%jij, norm2(this%lattice%cr(:, i) - this%lattice%cr(:, j))
            this%jijcd = this%parts(1, njij_glob); this%jijsd = this%parts(2, njij_glob)
            this%jijcc = this%parts(3, njij_glob); this%jijsc = this%parts(4, njij_glob)
            write (70, '(2i8,2x,3e20.11,2x,4es16.6,1x,f12.6)') &
               this%lattice%iz(i), this%lattice%iz(j), this%lattice%cr(:, j) - this%lattice%cr(:, i), this%jijcd, this%jijsd, this%jijcc, this%jijsc, &
               norm2(this%lattice%cr(:, i) - this%lattice%cr(:, j))
            this%dmi = this%so(2:4, njij_glob)
            write (30, '(2i8,2x,3e20.11,2x,3es16.6,1x,f12.6)') &
               this%lattice%iz(i), this%lattice%iz(j), this%lattice%cr(:, j) - this%lattice%cr(:, i), this%dmi, norm2(this%lattice%cr(:, i) - this%lattice%cr(:, j))
            this%dmi = this%fo(2:4, njij_glob)
            write (35, '(2i8,2x,3e20.11,2x,3es16.6,1x,f12.6)') &
               this%lattice%iz(i), this%lattice%iz(j), this%lattice%cr(:, j) - this%lattice%cr(:, i), this%dmi, norm2(this%lattice%cr(:, i) - this%lattice%cr(:, j))
            this%dmicc = this%parts(5:7, njij_glob); this%dmisc = this%parts(8:10, njij_glob)
            write (75, '(2i8,2x,3e20.11,2x,6es16.6,1x,f12.6)') &
               this%lattice%iz(i), this%lattice%iz(j), this%lattice%cr(:, j) - this%lattice%cr(:, i), this%dmicc, this%dmisc, norm2(this%lattice%cr(:, i) - this%lattice%cr(:, j))
            this%aij = reshape(this%so(5:13, njij_glob), [3, 3])
            write (40, '(2i8,2x,3e20.11,2x,9es16.6,1x,f12.6)') &
               this%lattice%iz(i), this%lattice%iz(j), this%lattice%cr(:, j) - this%lattice%cr(:, i), this%aij, norm2(this%lattice%cr(:, i) - this%lattice%cr(:, j))
            this%aij = reshape(this%fo(5:13, njij_glob), [3, 3])
            write (45, '(2i8,2x,3e20.11,2x,9es16.6,1x,f12.6)') &
               this%lattice%iz(i), this%lattice%iz(j), this%lattice%cr(:, j) - this%lattice%cr(:, i), this%aij, norm2(this%lattice%cr(:, i) - this%lattice%cr(:, j))
            this%aijsd = reshape(this%parts(11:19, njij_glob), [3, 3]); this%aijsc = reshape(this%parts(20:28, njij_glob), [3, 3])
            write (80, '(2i8,2x,3e20.11,2x,18es16.6,1x,f12.6)') &
               this%lattice%iz(i), this%lattice%iz(j), this%lattice%cr(:, j) - this%lattice%cr(:, i), this%aijsd, this%aijsc, norm2(this%lattice%cr(:, i) - this%lattice%cr(:, j))
         end do
      end if

      close (20)
      close (25)
      close (30)
      close (35)
      close (40)
      close (45)
      close (60)
      close (65)
      close (70)
      close (75)
      close (80)

      deallocate (this%jcum)
#ifdef USE_MPI
      call MPI_BARRIER(MPI_COMM_WORLD, ierr)
#endif
   end subroutine gpu_calculate_exchange_twoindex

   !> calculate_gilbert_damping (:613-743)
   subroutine gpu_calculate_gilbert_damping(this)
      class(exchange_gpu) :: this
      integer :: nloc, nen, njij, p, ij, side, i, j, k, nv, ief, lmaxi
      integer(c_int) :: rc, ikind, sym_i
      type(c_ptr) :: ctx
      real(rp) :: spin_i, diff, factor, distance_alat
      integer(c_int), dimension(:), allocatable, target :: same
      real(rp), dimension(:), allocatable, target :: ene
      complex(rp), dimension(:, :, :, :, :), allocatable, target :: tmat
      real(rp), dimension(:, :), allocatable, target :: at_ef, total

      if (this%control%nsp .ne. 2) return ! check if spin-orbit (l.s) is enabled

      call this%hamiltonian%torque_operator_collinear() ! the torque operators for all NTYPE
      nen = size(this%en%ene)
      njij = this%lattice%njij
      nloc = end_atom - start_atom + 1
      call pair_front(this, start_atom, end_atom, ikind, sym_i, same)
      ! :695-702, the closest energy point of the Fermi level (the same for every pair)
      ief = 0; diff = 1000.0_rp
      do nv = 1, nen
         if (abs(this%en%ene(nv) - this%en%fermi) .lt. diff) then
            diff = abs(this%en%ene(nv) - this%en%fermi)
            ief = nv
         end if
      end do
      allocate (at_ef(18, njij), total(9, nen))
      at_ef = 0.0_rp; total = 0.0_rp
      if (nloc > 0) then
         allocate (ene(nen), tmat(18, 18, 3, 2, nloc))
         ene(:) = this%en%ene(1:nen)
         do ij = start_atom, end_atom
            p = ij - start_atom + 1
            do side = 1, 2
               tmat(:, :, :, side, p) = this%hamiltonian%tmat(:, :, :, this%lattice%iz(this%lattice%ijpair(ij, side)))
            end do
         end do
         ctx = rsrec_gpu_context()
         call g_timer%start('damping-gpu')
         ! coefficients and terminators NULL: the chains recur_b_ij / chebyshev_recur_ij left on the device (i == j pairs: one chain)
         rc = rsrec_damping(ctx, ikind, int(nloc, c_int), c_loc(same), int(this%control%lld, c_int), int(nen, c_int), &
                            c_loc(ene), int(ief, c_int), sym_i, real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), &
                            c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_loc(tmat), int(start_atom - 1, c_int), int(njij, c_int), &
                            c_loc(at_ef), c_loc(total), c_null_ptr)
         call g_timer%stop('damping-gpu')
         if (rc /= 0) call g_logger%fatal('exchange_gpu: rsrec_damping: '//rsrec_error_string(ctx), __FILE__, __LINE__)
      end if
#ifdef USE_MPI
      call MPI_ALLREDUCE(MPI_IN_PLACE, at_ef, product(shape(at_ef)), MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)
      call MPI_ALLREDUCE(MPI_IN_PLACE, total, product(shape(total)), MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)
#endif

      if (rank == 0) then
         open (UNIT=103, FILE='damping-energy.out', STATUS='replace', ACTION='write')
         open (UNIT=104, FILE='alldampings.out', STATUS='replace', ACTION='write')
         write (104, *) '    #i     #j   #xx          #xy           #xz           '// &
            '#yx           #yy           #yz           #zx           #zy           '// &
            '#zz          #0.5*(xx + yy)     #Dist           #rij = (ri - rj)'
         factor = 0.0_rp
         do ij = 1, njij
            i = this%lattice%ijpair(ij, 1)
            j = this%lattice%ijpair(ij, 2)
            distance_alat = norm2(this%lattice%cr(:, i) - this%lattice%cr(:, j))
            lmaxi = this%symbolic_atom(this%lattice%iz(i))%potential%lmax
            ! the spin magnetic moment of the i-th atom, from zero for every pair (see the file header)
            spin_i = 0.0_rp
            do k = 0, lmaxi
               spin_i = spin_i + this%symbolic_atom(this%lattice%iz(i))%potential%ql(1, k, 1) - &
                        this%symbolic_atom(this%lattice%iz(i))%potential%ql(1, k, 2)
            end do
            factor = (-0.25_rp)*(2.0_rp/(pi*spin_i))
            write (*, '(A,I6,A,I6,A)') 'Damping tensor between pair', i, ' and ', j, ' is'
            write (*, '(3F14.9)') factor*at_ef(1:9, ij)
            write (*, '(A,I6,A,I6,A)') 'Imaginary part of the tensor between pair', i, ' and ', j, ' is'
            write (*, '(3F14.9)') factor*at_ef(10:18, ij)
            write (*, *) '----------------------'
            write (104, '(2I7,11F14.9,3F10.6)') i, j, factor*at_ef(1:9, ij), 0.5*factor*(at_ef(1, ij) + at_ef(5, ij)), &
               distance_alat, this%lattice%cr(:, i) - this%lattice%cr(:, j)
            write (*, *) 'ief = ', this%en%ene(ief), 'fermi = ', this%en%fermi
         end do
         write (103, *) '#Energy (E-Ef)         #xx         #xy           #xz           '// &
            '#yx           #yy           #yz           #zx           #zy           #zz'
         do nv = 1, nen
            write (103, '(10F14.9)') this%en%ene(nv) - this%en%fermi, factor*total(:, nv)
         end do
         close (103)
         close (104)
      end if
#ifdef USE_MPI
      call MPI_BARRIER(MPI_COMM_WORLD, ierr)
#endif
   end subroutine gpu_calculate_gilbert_damping

   !> calculate_exchange_gauss_legendre (:1756-1919)
   subroutine gpu_calculate_exchange_gauss_legendre(this)
      class(exchange_gpu) :: this
      integer :: nloc, njij, p, ij, side, i, j, fermi_point, njij_glob, at
      integer(c_int) :: rc, ikind, sym_i
      type(c_ptr) :: ctx
      integer(c_int), dimension(:), allocatable, target :: same
      real(rp), dimension(64), target :: x, w
      real(rp), dimension(:, :, :, :), allocatable, target :: dmat
      real(rp), dimension(:, :), allocatable, target :: T_comm_xc

      njij = this%lattice%njij
      nloc = end_atom - start_atom + 1
      call pair_front(this, start_atom, end_atom, ikind, sym_i, same)
      allocate (T_comm_xc(13, njij))
      T_comm_xc = 0.0_rp

      call open_unit(20, 'jij.out', 'jij.outt: Unit 20 is already open')
      call open_unit(30, 'dij.out', 'dij.outt: Unit 30 is already open')
      call open_unit(40, 'aij.out', 'aij.out: Unit 40 is already open')
      call open_unit(60, 'jtens.out', 'jtens.out: Unit 40 is already open')

      ! Find the Gauss Legendre roots and weights
      call gauss_legendre(64, 0.00_rp, 1.0_rp, x, w)
      ! the point of the mesh the Green functions were taken at (green.f90:489-491)
      fermi_point = 0
      do i = 1, this%en%channels_ldos + 10
         if ((this%en%ene(i) - this%en%fermi) .le. 0.000001d0) fermi_point = i
      end do

      if (nloc > 0) then
         allocate (dmat(9, 9, 2, nloc))
         do ij = start_atom, end_atom
            p = ij - start_atom + 1
            do side = 1, 2
               at = this%lattice%iz(this%lattice%ijpair(ij, side))
               dmat(:, :, side, p) = real(this%hamiltonian%ee(1:9, 1:9, 1, at) - this%hamiltonian%ee(10:18, 10:18, 1, at))
            end do
         end do
         ctx = rsrec_gpu_context()
         call g_timer%start('exchange-contour-gpu')
         ! coefficients and terminators NULL: the chains recur_b_ij / chebyshev_recur_ij left on the device (i == j pairs: one chain)
         rc = rsrec_exchange_contour(ctx, ikind, int(nloc, c_int), c_loc(same), int(this%control%lld, c_int), 64_c_int, &
                                     c_loc(x), c_loc(w), real(this%en%ene(fermi_point), c_double), sym_i, &
                                     real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), c_null_ptr, c_null_ptr, &
                                     c_null_ptr, c_null_ptr, c_loc(dmat), int(start_atom - 1, c_int), int(njij, c_int), &
                                     c_loc(T_comm_xc), c_null_ptr)
         call g_timer%stop('exchange-contour-gpu')
         if (rc /= 0) call g_logger%fatal('exchange_gpu: rsrec_exchange_contour: '//rsrec_error_string(ctx), __FILE__, __LINE__)
      end if

#ifdef USE_MPI
      call MPI_ALLREDUCE(MPI_IN_PLACE, T_comm_xc, product(shape(T_comm_xc)), &
                         MPI_DOUBLE_PRECISION, MPI_SUM, MPI_COMM_WORLD, ierr)
#endif

      if (rank == 0) then
         do njij_glob = 1, this%lattice%njij
            i = this%lattice%ijpair(njij_glob, 1) ! Atom number in the clust file, atom i
            j = this%lattice%ijpair(njij_glob, 2) ! Atom number in the clust file, atom j

            write (*, *) 'Atom', i, 'coordinates:', this%lattice%cr(:, i), 'Atom Type', this%lattice%iz(i)
            write (*, *) 'Atom', j, 'coordinates:', this%lattice%cr(:, j), 'Atom Type', this%lattice%iz(j)
            write (*, *) 'Distance = ', norm2(this%lattice%cr(:, i) - this%lattice%cr(:, j))

            ! Jij
            this%jij = T_comm_xc(1, njij_glob)
            write (*, *) 'Jij between pair', i, 'and ', j, 'is ', this%jij

            ! Dij
            this%dmi = T_comm_xc(2:4, njij_glob)
            write (*, *) 'Dij between pair', i, 'and ', j, 'is ', this%dmi

            ! Aij
            this%aij = reshape(T_comm_xc(5:13, njij_glob), [3, 3])
            write (*, *) 'Iij between pair', i, 'and ', j, 'is'
            print '(3f12.6)', this%aij(1, :)
            print '(3f12.6)', this%aij(2, :)
            print '(3f12.6)', this%aij(3, :)
            !
            call write_pair_records(this, i, j, T_comm_xc(:, njij_glob))
         end do
      end if
      close (20)
      close (30)
      close (40)
      deallocate (T_comm_xc)
#ifdef USE_MPI
      call MPI_BARRIER(MPI_COMM_WORLD, ierr)
#endif
   end subroutine gpu_calculate_exchange_gauss_legendre

   !> the host intersite arrays for an inherited routine that reads them (green_gpu%fetch_intersite)
   subroutine host_intersite(this)
      class(exchange_gpu), intent(inout) :: this
      select type (g => this%green)
      class is (green_gpu)
         call g%fetch_intersite()
      end select
   end subroutine host_intersite

   subroutine gpu_calculate_moment_of_inertia(this)
      class(exchange_gpu) :: this
      call host_intersite(this)
      call this%exchange%calculate_moment_of_inertia()
   end subroutine gpu_calculate_moment_of_inertia

   subroutine gpu_calculate_jij_auxgreen(this)
      class(exchange_gpu) :: this
      call host_intersite(this)
      call this%exchange%calculate_jij_auxgreen()
   end subroutine gpu_calculate_jij_auxgreen

   !> calculate_jijk (:338-601) as one rsrec_spin_lattice call for all trios on the resident chains of the pair recursion: the pairs are
   !> the trios' (i,j), (i,k), (j,k) (lattice.f90:644-651).  apar: (c + vmad, dele, qpar) per l, spin and atom, as p_matrix, auxiliary_gij
   !> and transform_pmatrix read them; dmat: one spin block of the reference's own disp_matrix of atom k for uni_disp (:489-495, :507).
   !> Then the reference's three stdout lines per trio (:558-560).  Host route (fetch_intersite + the inherited routine) when an atom has
   !> lmax /= 2, when the pairs are not exactly the trios' pairs, or when this rank does not hold every pair (more than one rank).
   subroutine gpu_calculate_jijk(this)
      class(exchange_gpu) :: this
      integer :: ntrio, njij, nen, t, a, l, s, at
      integer :: atoms(3)
      logical :: device
      integer(c_int) :: rc, ikind, sym_i
      type(c_ptr) :: ctx
      integer(c_int), dimension(:), allocatable, target :: same
      real(rp), dimension(:), allocatable, target :: ene
      real(rp), dimension(:, :, :, :, :), allocatable, target :: apar
      real(rp), dimension(:, :), allocatable, target :: jijk
      real(rp), dimension(:, :), allocatable :: uni
      complex(rp), dimension(:, :, :), allocatable, target :: dmat
      complex(rp), dimension(:, :), allocatable :: d18
      real(rp) :: disp(3)

      ntrio = this%lattice%njijk
      njij = this%lattice%njij
      device = ntrio > 0 .and. njij == 3*ntrio .and. start_atom == 1 .and. end_atom == njij .and. &
               (this%control%recur == 'block' .or. this%control%recur == 'chebyshev')
      if (device) then
         do t = 1, ntrio
            do a = 1, 3
               at = this%lattice%iz(int(this%lattice%ijktrio(t, a)))
               if (this%symbolic_atom(at)%potential%lmax /= 2) device = .false.
            end do
         end do
      end if
      if (.not. device) then
         call host_intersite(this)
         call this%exchange%calculate_jijk()
         return
      end if

      nen = this%en%channels_ldos + 10
      allocate (ene(nen), apar(3, 3, 2, 3, ntrio), dmat(9, 9, ntrio), jijk(9, ntrio), uni(3, ntrio), d18(18, 18))
      ene(:) = this%en%ene(1:nen)
      jijk = 0.0_rp
      do t = 1, ntrio
         atoms(:) = int(this%lattice%ijktrio(t, 1:3))
         do a = 1, 3
            at = this%lattice%iz(atoms(a))
            associate (pot => this%symbolic_atom(at)%potential)
               do s = 1, 2
                  do l = 0, 2
                     apar(1, l + 1, s, a, t) = pot%c(l, s) + pot%vmad
                     apar(2, l + 1, s, a, t) = pot%dele(l, s)
                     apar(3, l + 1, s, a, t) = pot%qpar(l, s)
                  end do
               end do
            end associate
         end do
         disp(:) = 1.0_rp*this%lattice%ijktrio(t, 4:6)
         uni(1, t) = disp(1)/norm2(disp)
         uni(2, t) = disp(2)/norm2(disp)
         uni(3, t) = disp(3)/norm2(disp)
         d18 = (0.0_rp, 0.0_rp)
         call this%symbolic_atom(this%lattice%iz(atoms(3)))%disp_matrix(d18, uni(:, t), 2, this%lattice%wav)
         dmat(:, :, t) = d18(1:9, 1:9)
      end do
      call pair_front(this, 1, njij, ikind, sym_i, same)
      ctx = rsrec_gpu_context()
      call g_timer%start('jijk-gpu')
      ! coefficients and terminators NULL: the chains recur_b_ij / chebyshev_recur_ij left on the device (i == j pairs: one chain)
      rc = rsrec_spin_lattice(ctx, ikind, int(njij, c_int), c_loc(same), int(this%control%lld, c_int), int(nen, c_int), &
                              c_loc(ene), int(this%en%nv1, c_int), real(this%en%fermi, c_double), sym_i, &
                              real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), c_null_ptr, c_null_ptr, &
                              c_null_ptr, c_null_ptr, c_loc(apar), c_loc(dmat), 0_c_int, int(ntrio, c_int), c_loc(jijk), c_null_ptr)
      call g_timer%stop('jijk-gpu')
      if (rc /= 0) call g_logger%fatal('exchange_gpu: rsrec_spin_lattice: '//rsrec_error_string(ctx), __FILE__, __LINE__)
      do t = 1, ntrio
         atoms(:) = int(this%lattice%ijktrio(t, 1:3))
         this%jijk(:) = jijk(:, t)
         write (*, *) 'Jijk tensor between trio ', atoms(1), ',', atoms(2), ' and ', atoms(3), 'is (in meV/a.u.)'
         write (*, '(A, "(", F7.4, ", ", F7.4, ", ", F7.4, ")")') ' Displacement vector: ', uni(1, t), uni(2, t), uni(3, t)
         write (*, '(3F14.9)') this%jijk*(1.0d3/8.0d0/pi)*(13.605693122994d0/1.8897261246d0)
      end do
   end subroutine gpu_calculate_jijk

end module exchange_gpu_mod
