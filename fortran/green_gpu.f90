!------------------------------------------------------------------------------
! RS-LMTO-ASA drop-in, second stage: the Green function of the block recursion on the GPU.
!------------------------------------------------------------------------------
!
! MODULE: green_gpu_mod
!
! DESCRIPTION:
!> `type, extends(green) :: green_gpu` overrides the continued fraction of the reference's `green` type, `bgreen` (and its all-sites driver `block_green`, to batch the sites)
!> (green.f90:1191-1339), the continued fraction  coefficients -> g(E)  that `block_green` (:588), `block_green_eta`
!> (:541) and the inter-site variants call per site.  Everything else -- the terminator (`recursion%get_terminf`),
!> the result arrays `g0, gij, ...`, `sgreen`, `chebyshev_green` -- is inherited.  The GPU side is `rsrec_block_green`
!> (include/rsrec.h): one wave per energy point, register-resident 18x18 complex inverse with LAPACK's pivot rule (LDS carries only pivot rows / columns).
!>
!> `bands`, `self` and `exchange` hold `class(green), pointer` (bands.f90:49, self.f90:76, exchange.f90:48); the only
!> non-polymorphic spot is the dummy of the `bands` constructor (bands.f90:121, `type(green), target`), which a maintainer
!> changes to `class(green), target` (INTEGRATION.md).
!>
!> Intersite stage (green.f90:386-469): the 24 arrays `gij, gji, ginmag ... gz1ji` are (9|18, 9|18, channels_ldos + 10, pairs), about
!> 0.1 GB per pair at 2500 energies.  The reference's `restore_to_default` allocates and zeroes them at construction; here they are
!> allocated (and zeroed) only when a host routine that fills them runs (`intersite_arrays`).  When `exchange_gpu` (exchange_gpu.f90)
!> has taken the stage over -- `rsrec_exchange` forms Jij / Dij / Iij straight from the recursion's chains -- `calculate_intersite_gf`
!> and `_twoindex` allocate and fill nothing; the first keeps only the reference's side effect on the recursion (zsqr, :434).
!> The inherited routines of `exchange` that still read the host arrays (calculate_moment_of_inertia, calculate_jij_auxgreen, and
!> calculate_jijk only where its device route does not apply: lmax /= 2, or more than one rank) get them through `fetch_intersite`,
!> which `exchange_gpu` calls before each of them: it allocates the arrays and runs
!> the inherited `calculate_intersite_gf` / `_twoindex` on the recursion's host coefficients (the idea of bands_gpu's `fetch_g0`).
!------------------------------------------------------------------------------
module green_gpu_mod
   use, intrinsic :: iso_c_binding
   use green_mod
   use density_of_states_mod, only: dos
   use precision_mod, only: rp
   use logger_mod, only: g_logger
   use timer_mod, only: g_timer
   use rsrec_binding
   use rsrec_context_mod, only: rsrec_gpu_context, rsrec_env_flag
   implicit none

   private

   type, public, extends(green) :: green_gpu
      !> `g0` on demand: with defer_g0 = .true. `block_green` only notes that `g0` is out of date; the continued fraction and the
      !> 13 MB per site it brings over PCIe happen in `fetch_g0`, which the consumers of `g0` call (bands_gpu does before every
      !> inherited routine that reads it).  A flow that only needs densities of states (`bands_gpu%calculate_fermi`, served by the
      !> device LDOS stage from the coefficients the recursion left on the GPU) then never produces `g0` at all.
      logical :: defer_g0 = .false.
      logical :: g0_stale = .false.
      logical :: fetching = .false.   ! set by fetch_g0 around its own Green call: the one caller that makes a deferred g0
      logical :: stale_is_chebyshev = .false.   ! which routine postponed it: chebyshev_green (else block_green)
      !> .true. once exchange_gpu owns the intersite stage (its constructor, `release_intersite`)
      logical :: intersite_on_device = .false.
      !> .true. once fetch_intersite has filled the host arrays from the present coefficients
      logical :: intersite_fetched = .false.
      !> recursion%b2_b as it was before the first zsqr of the on-device branch (B^2; 0.4 MB per pair at lld 20): fetch_intersite puts it
      !> back before the inherited calculate_intersite_gf, which takes the root itself (:434)
      complex(rp), dimension(:, :, :, :), allocatable :: b2_unrooted
   contains
      procedure :: restore_to_default => gpu_restore_to_default
      procedure :: calculate_intersite_gf => gpu_calculate_intersite_gf
      procedure :: calculate_intersite_gf_twoindex => gpu_calculate_intersite_gf_twoindex
      procedure :: calculate_intersite_gf_eta => gpu_calculate_intersite_gf_eta
      procedure :: release_intersite => gpu_release_intersite
      procedure :: fetch_intersite => gpu_fetch_intersite
      procedure :: bgreen => gpu_bgreen
      procedure :: block_green => gpu_block_green
      procedure :: chebyshev_green => gpu_chebyshev_green
      procedure :: fetch_g0 => gpu_fetch_g0
   end type green_gpu

   interface green_gpu
      procedure :: gpu_constructor
   end interface green_gpu

contains

   !> Same construction as green.f90:101-113.
   function gpu_constructor(dos_obj) result(obj)
      type(green_gpu) :: obj
      type(dos), target, intent(in) :: dos_obj

      obj%dos => dos_obj
      obj%recursion => dos_obj%recursion
      obj%en => dos_obj%en
      obj%symbolic_atom => dos_obj%recursion%hamiltonian%charge%lattice%symbolic_atoms
      obj%lattice => dos_obj%recursion%lattice
      obj%control => dos_obj%recursion%lattice%control
      call obj%restore_to_default()
      if (rsrec_env_flag('RSREC_DEFER_G0')) obj%defer_g0 = .true.    ! (hosts that cannot reach the member: fortran/shadow/)
   end function gpu_constructor

   !> Replaces green.f90:1191-1339 (same interface; `g_out` is zeroed and the energy range ie_start .. ie_start+ie_len-1 filled).
   subroutine gpu_bgreen(this, g_out, i_site, ie_start, ie_len, a_inf, b_inf, eta)
      class(green_gpu), intent(inout) :: this
      integer, intent(in) :: i_site
      integer, intent(in) :: ie_start
      integer, intent(in) :: ie_len
      complex(rp), dimension(18, 18, this%en%channels_ldos + 10), intent(inout) :: g_out
      real(rp), dimension(18, 18), intent(in) :: a_inf
      real(rp), dimension(18, 18), intent(in) :: b_inf
      complex(rp), intent(in) :: eta
      !
      integer :: ll
      integer(c_int) :: rc, sym_i
      type(c_ptr) :: handle
      real(rp), allocatable, target :: ene(:), ai(:, :), bi(:, :)
      complex(rp), allocatable, target :: ab(:, :, :), bs(:, :, :), gt(:, :, :)

      g_out = (0.0d0, 0.0d0)
      if (ie_len <= 0) return
      ll = this%control%lld
      allocate (ene(ie_len), ai(18, 18), bi(18, 18), ab(18, 18, ll), bs(18, 18, ll), gt(18, 18, ie_len))
      ene = this%en%ene(ie_start:ie_start + ie_len - 1)
      ai = a_inf
      bi = b_inf
      ab = this%recursion%a_b(:, :, 1:ll, i_site)
      bs = this%recursion%b2_b(:, :, 1:ll, i_site)          ! sqrt(B^2): zsqr ran before (self.f90:829)
      sym_i = 0
      if (this%control%sym_term) sym_i = 1
      handle = rsrec_gpu_context()
      call g_timer%start('bgreen-gpu')
      rc = rsrec_block_green(handle, 1_c_int, int(ll, c_int), int(ie_len, c_int), c_loc(ene), real(eta, c_double), aimag(eta), sym_i, &
                             c_loc(ai), c_loc(bi), c_loc(ab), c_loc(bs), gt)
      call g_timer%stop('bgreen-gpu')
      if (rc /= 0) call g_logger%fatal('rsrec_block_green: '//rsrec_error_string(handle), __FILE__, __LINE__)
      g_out(:, :, ie_start:ie_start + ie_len - 1) = gt
   end subroutine gpu_bgreen

   !> Replaces green.f90:588-621: the per-site loop over `bgreen` becomes ONE library call for all sites of this rank, so the
   !> kernel of one chunk of sites overlaps the download of the previous one (rsrec.hip green_pipeline) instead of a
   !> launch + 13 MB copy per site.  The terminator comes from recursion%get_terminf (GPU kernel behind recursion_gpu).
   subroutine gpu_block_green(this)
      use mpi_mod, only: start_atom, end_atom, g2l_map, atoms_per_process
      class(green_gpu), intent(inout) :: this
      integer :: nw, ll, ldim, nv, nloc, n1, n, nw_site
      integer(c_int) :: rc, sym_i
      type(c_ptr) :: handle
      real(rp), dimension(this%lattice%nrec) :: a_inf0, b_inf0
      real(rp), dimension(18, 18, this%lattice%nrec) :: a_inf, b_inf
      real(rp), allocatable, target :: ene(:), ai(:, :, :), bi(:, :, :)
      complex(rp), allocatable, target :: ab(:, :, :, :), bs(:, :, :, :), gt(:, :, :, :)

      if (this%defer_g0 .and. .not. this%fetching) then
         this%g0_stale = .true.                               ! produced by fetch_g0 when somebody reads g0; repeated calls without a
         this%stale_is_chebyshev = .false.                    ! reader in between (block_green + calculate_fermi, DOS-only flows) stay free
         return
      end if
      this%g0_stale = .false.
      ll = this%control%lld
      ldim = 18
      nw = 10*ll
      nloc = end_atom - start_atom + 1
      if (nloc <= 0) return
      n1 = g2l_map(start_atom)                               ! local indices of the rank's sites are contiguous (mpi.f90:72-78)
      ! Terminator: ONE get_terminf call for all sites of the rank (recursion.f90:2092).  With a recursion_gpu behind the class
      ! pointer this dispatches to the terminator kernel (one thread per site and matrix element, rsrec_terminator); with the
      ! reference's own type it is the reference's serial loop over the sites.
      a_inf = 0.0_rp; b_inf = 0.0_rp
      nw_site = nw
      call this%recursion%get_terminf(this%recursion%a_b(:, :, :, n1:n1 + nloc - 1), this%recursion%b2_b(:, :, :, n1:n1 + nloc - 1), nloc, &
                                      ll, ldim, nw_site, a_inf(:, :, n1:n1 + nloc - 1), b_inf(:, :, n1:n1 + nloc - 1), &
                                      a_inf0(n1:n1 + nloc - 1), b_inf0(n1:n1 + nloc - 1))
      nv = this%en%channels_ldos + 10
      allocate (ene(nv), ai(18, 18, nloc), bi(18, 18, nloc), ab(18, 18, ll, nloc), bs(18, 18, ll, nloc))
      ene = this%en%ene(1:nv)
      ai = a_inf(:, :, n1:n1 + nloc - 1)
      bi = b_inf(:, :, n1:n1 + nloc - 1)
      ab = this%recursion%a_b(:, :, 1:ll, n1:n1 + nloc - 1)
      bs = this%recursion%b2_b(:, :, 1:ll, n1:n1 + nloc - 1)  ! sqrt(B^2): zsqr ran before (self.f90:829)
      sym_i = 0
      if (this%control%sym_term) sym_i = 1
      handle = rsrec_gpu_context()
      call g_timer%start('bgreen-gpu')
      if (n1 == 1 .and. size(this%g0, 3) == nv .and. size(this%g0, 4) >= nloc) then
         ! green%g0(18,18,nv,atoms_per_process) (green.f90:192) is the library's output buffer itself: no staging copy of 13 MB per site
         rc = rsrec_block_green(handle, int(nloc, c_int), int(ll, c_int), int(nv, c_int), c_loc(ene), 0.0_c_double, 0.0_c_double, sym_i, &
                                c_loc(ai), c_loc(bi), c_loc(ab), c_loc(bs), this%g0)
      else
         allocate (gt(18, 18, nv, nloc))
         rc = rsrec_block_green(handle, int(nloc, c_int), int(ll, c_int), int(nv, c_int), c_loc(ene), 0.0_c_double, 0.0_c_double, sym_i, &
                                c_loc(ai), c_loc(bi), c_loc(ab), c_loc(bs), gt)
         if (rc == 0) this%g0(:, :, 1:nv, n1:n1 + nloc - 1) = gt
      end if
      call g_timer%stop('bgreen-gpu')
      if (rc /= 0) call g_logger%fatal('rsrec_block_green: '//rsrec_error_string(handle), __FILE__, __LINE__)
   end subroutine gpu_block_green

   !> `g0` of the last (deferred) `block_green` / `chebyshev_green` call, now.  A no-op when `g0` is up to date.
   subroutine gpu_fetch_g0(this)
      class(green_gpu), intent(inout) :: this
      if (.not. this%g0_stale) return
      this%fetching = .true.
      if (this%stale_is_chebyshev) then                      ! the one call that does the work
         call this%chebyshev_green()
      else
         call this%block_green()
      end if
      this%fetching = .false.
   end subroutine gpu_fetch_g0

   !> Replaces green.f90:1030-1108: g0 of the sites of this rank from the Chebyshev moments.  The side effect of the reference
   !> routine -- recursion%mu_ng = mu_n * Jackson kernel (* 2 beyond the first moment), read later by bands.f90:762 -- is kept, and is
   !> made at once even when `defer_g0` postpones the library call and the download of `g0` to `fetch_g0` (it is cheap host work).
   subroutine gpu_chebyshev_green(this)
      use mpi_mod, only: start_atom, end_atom, g2l_map
      use math_mod, only: jackson_kernel
      class(green_gpu), intent(inout) :: this
      integer :: n, n_glob, nv, nm, l, m, nloc, n1
      integer(c_int) :: rc
      type(c_ptr) :: handle
      real(rp), dimension(this%control%lld*2 + 2) :: kernel
      real(rp), allocatable, target :: ene(:)
      complex(rp), allocatable, target :: mu(:, :, :, :), gt(:, :, :, :)

      nv = this%en%channels_ldos + 10
      nm = this%control%lld*2 + 2
      nloc = end_atom - start_atom + 1
      if (.not. this%fetching) then                          ! (fetch_g0 repeats a call whose side effect is already made)
         if (.not. this%defer_g0) this%g0 = 0.0d0
         if (nloc <= 0) return
         call jackson_kernel(nm, kernel)
         do n_glob = start_atom, end_atom
            n = g2l_map(n_glob)
            do l = 1, 18
               do m = 1, 18
                  this%recursion%mu_ng(l, m, :, n) = this%recursion%mu_n(l, m, :, n)*kernel(:)
               end do
            end do
            this%recursion%mu_ng(:, :, 2:nm, n) = this%recursion%mu_ng(:, :, 2:nm, n)*2.0_rp
         end do
         if (this%defer_g0) then
            this%g0_stale = .true.
            this%stale_is_chebyshev = .true.
            return
         end if
      else
         this%g0 = 0.0d0
      end if
      this%g0_stale = .false.
      n1 = g2l_map(start_atom)
      allocate (ene(nv), mu(18, 18, nm, nloc))
      ene = this%en%ene(1:nv)
      mu = this%recursion%mu_n(:, :, 1:nm, n1:n1 + nloc - 1)
      handle = rsrec_gpu_context()
      call g_timer%start('chebyshev-green-gpu')
      if (n1 == 1 .and. size(this%g0, 3) == nv .and. size(this%g0, 4) >= nloc) then
         rc = rsrec_chebyshev_green(handle, int(nloc, c_int), int(this%control%lld, c_int), int(nv, c_int), c_loc(ene), &
                                    real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), c_loc(mu), this%g0)
      else
         allocate (gt(18, 18, nv, nloc))
         rc = rsrec_chebyshev_green(handle, int(nloc, c_int), int(this%control%lld, c_int), int(nv, c_int), c_loc(ene), &
                                    real(this%en%energy_min, c_double), real(this%en%energy_max, c_double), c_loc(mu), gt)
         if (rc == 0) this%g0(:, :, 1:nv, n1:n1 + nloc - 1) = gt
      end if
      call g_timer%stop('chebyshev-green-gpu')
      if (rc /= 0) call g_logger%fatal('rsrec_chebyshev_green: '//rsrec_error_string(handle), __FILE__, __LINE__)
   end subroutine gpu_chebyshev_green

   !> green.f90:186-313 without the pair x energy arrays `gij ... gz1ji`: `g0` and the `_eta` set as the reference allocates and zeroes
   !> them; the others come with the first host routine that fills them (`intersite_arrays`).
   subroutine gpu_restore_to_default(this)
      use mpi_mod, only: atoms_per_process
      class(green_gpu) :: this
      integer :: nv, n
      nv = this%en%channels_ldos + 10
      n = atoms_per_process
      if (this%lattice%njij == 0) then
         allocate (this%g0(18, 18, nv, this%lattice%nrec))
      else
         allocate (this%g0(18, 18, nv, 4))
      end if
      allocate (this%gij_eta(64, 18, 18, n), this%gji_eta(64, 18, 18, n))
      allocate (this%ginmag_eta(64, 9, 9, n), this%gjnmag_eta(64, 9, 9, n), this%gix_eta(64, 9, 9, n), this%giy_eta(64, 9, 9, n), &
                this%giz_eta(64, 9, 9, n), this%gjx_eta(64, 9, 9, n), this%gjy_eta(64, 9, 9, n), this%gjz_eta(64, 9, 9, n))
      this%g0(:, :, :, :) = (0.0d0, 0.0d0)
      this%gij_eta(:, :, :, :) = (0.0d0, 0.0d0)
      this%gji_eta(:, :, :, :) = (0.0d0, 0.0d0)
      this%ginmag_eta(:, :, :, :) = (0.0d0, 0.0d0)
      this%gjnmag_eta(:, :, :, :) = (0.0d0, 0.0d0)
      this%gix_eta(:, :, :, :) = (0.0d0, 0.0d0)
      this%giy_eta(:, :, :, :) = (0.0d0, 0.0d0)
      this%giz_eta(:, :, :, :) = (0.0d0, 0.0d0)
      this%gjx_eta(:, :, :, :) = (0.0d0, 0.0d0)
      this%gjy_eta(:, :, :, :) = (0.0d0, 0.0d0)
      this%gjz_eta(:, :, :, :) = (0.0d0, 0.0d0)
   end subroutine gpu_restore_to_default

   !> The pair x energy arrays of green.f90:208-263, allocated and zeroed as restore_to_default (:276-300) leaves them; a no-op once
   !> they exist.
   subroutine intersite_arrays(this)
      use mpi_mod, only: atoms_per_process
      class(green_gpu), intent(inout) :: this
      integer :: nv, n
      if (allocated(this%gij)) return
      nv = this%en%channels_ldos + 10
      n = atoms_per_process
      allocate (this%gij(18, 18, nv, n), this%gji(18, 18, nv, n))
      allocate (this%ginmag(9, 9, nv, n), this%gjnmag(9, 9, nv, n), this%gix(9, 9, nv, n), this%giy(9, 9, nv, n), this%giz(9, 9, nv, n), &
                this%gjx(9, 9, nv, n), this%gjy(9, 9, nv, n), this%gjz(9, 9, nv, n))
      allocate (this%g00ij(9, 9, nv, n), this%g00ji(9, 9, nv, n), this%g01ij(9, 9, nv, n), this%g01ji(9, 9, nv, n), &
                this%gx0ij(9, 9, nv, n), this%gy0ij(9, 9, nv, n), this%gz0ij(9, 9, nv, n), this%gx1ij(9, 9, nv, n), &
                this%gy1ij(9, 9, nv, n), this%gz1ij(9, 9, nv, n), this%gx0ji(9, 9, nv, n), this%gy0ji(9, 9, nv, n), &
                this%gz0ji(9, 9, nv, n), this%gx1ji(9, 9, nv, n), this%gy1ji(9, 9, nv, n), this%gz1ji(9, 9, nv, n))
      this%gij = 0.0d0; this%gji = 0.0d0
      this%ginmag = 0.0d0; this%gjnmag = 0.0d0; this%gix = 0.0d0; this%giy = 0.0d0; this%giz = 0.0d0
      this%gjx = 0.0d0; this%gjy = 0.0d0; this%gjz = 0.0d0
      this%g00ij = 0.0d0; this%g00ji = 0.0d0; this%g01ij = 0.0d0; this%g01ji = 0.0d0
      this%gx0ij = 0.0d0; this%gy0ij = 0.0d0; this%gz0ij = 0.0d0; this%gx1ij = 0.0d0; this%gy1ij = 0.0d0; this%gz1ij = 0.0d0
      this%gx0ji = 0.0d0; this%gy0ji = 0.0d0; this%gz0ji = 0.0d0; this%gx1ji = 0.0d0; this%gy1ji = 0.0d0; this%gz1ji = 0.0d0
   end subroutine intersite_arrays

   !> Called by exchange_gpu's constructor: the intersite stage is done on the device from now on, and the host arrays go (if any).
   subroutine gpu_release_intersite(this)
      class(green_gpu), intent(inout) :: this
      this%intersite_on_device = .true.
      this%intersite_fetched = .false.
      if (allocated(this%b2_unrooted)) deallocate (this%b2_unrooted)
      if (allocated(this%gij)) deallocate (this%gij, this%gji, this%ginmag, this%gjnmag, this%gix, this%giy, this%giz, this%gjx, &
                                           this%gjy, this%gjz, this%g00ij, this%g00ji, this%g01ij, this%g01ji, this%gx0ij, this%gy0ij, &
                                           this%gz0ij, this%gx1ij, this%gy1ij, this%gz1ij, this%gx0ji, this%gy0ji, this%gz0ji, &
                                           this%gx1ji, this%gy1ji, this%gz1ji)
      ! the Gauss-Legendre images of the same stage (64 x 18 x 18 per pair and array): exchange_gpu's contour routine forms none of them
      if (allocated(this%gij_eta)) deallocate (this%gij_eta, this%gji_eta, this%ginmag_eta, this%gjnmag_eta, this%gix_eta, this%giy_eta, &
                                               this%giz_eta, this%gjx_eta, this%gjy_eta, this%gjz_eta)
   end subroutine gpu_release_intersite

   !> green.f90:425-469.  With exchange_gpu behind the stage only its side effect on the recursion stays: b2_b <- sqrt(b2_b) for
   !> block (:434), on the host arrays.  (rsrec_exchange reads the B^2 chains resident on the device and roots a copy of its own;
   !> rsrec_zsqr works in a buffer of its own, so the resident chains are rooted once.)
   subroutine gpu_calculate_intersite_gf(this)
      class(green_gpu), intent(inout) :: this
      if (this%intersite_on_device) then
         if (this%control%recur == 'block') then
            if (.not. allocated(this%b2_unrooted)) this%b2_unrooted = this%recursion%b2_b
            call this%recursion%zsqr()
         end if
         this%intersite_fetched = .false.
         return
      end if
      call intersite_arrays(this)
      call this%green%calculate_intersite_gf()
   end subroutine gpu_calculate_intersite_gf

   !> The host intersite arrays, now: for the inherited routines of `exchange` that read `gij / gji / ginmag ...` after exchange_gpu
   !> released them.  Allocates the 24 arrays and runs the inherited calculate_intersite_gf and _twoindex on the recursion's host
   !> coefficients.  The inherited routine roots b2_b itself (block, :434): where the on-device branch above has rooted it already, B^2
   !> is put back first, so the arrays carry the bits of a run with the plain types and b2_b is left rooted once, as before.
   !> A no-op while the arrays are up to date; a new pair recursion is followed by a new calculate_intersite_gf, which marks them stale.
   subroutine gpu_fetch_intersite(this)
      class(green_gpu), intent(inout) :: this
      if (.not. this%intersite_on_device) return              ! the host stage is the reference's own: its arrays are the caller's business
      if (this%intersite_fetched .and. allocated(this%gij)) return
      call intersite_arrays(this)
      if (this%control%recur == 'block') then
         if (allocated(this%b2_unrooted)) then
            this%recursion%b2_b = this%b2_unrooted
         else
            this%b2_unrooted = this%recursion%b2_b
         end if
      end if
      call g_timer%start('fetch-intersite')
      call this%green%calculate_intersite_gf()
      call this%green%calculate_intersite_gf_twoindex()
      call g_timer%stop('fetch-intersite')
      this%intersite_fetched = .true.
   end subroutine gpu_fetch_intersite

   !> green.f90:386-423: nothing to do when exchange_gpu owns the stage.
   subroutine gpu_calculate_intersite_gf_twoindex(this)
      class(green_gpu), intent(inout) :: this
      if (this%intersite_on_device) return
      call intersite_arrays(this)
      call this%green%calculate_intersite_gf_twoindex()
   end subroutine gpu_calculate_intersite_gf_twoindex

   !> green.f90:471-536.  With exchange_gpu behind the stage (rsrec_exchange_contour forms T_comm_xc from the resident chains, the
   !> terminator once per chain) only the side effects stay: e_mesh, the `fermi, fermi_point` line (:487-493), and zsqr on the host
   !> arrays exactly as gpu_calculate_intersite_gf does it.  The ten _eta arrays are neither allocated (release_intersite let them go)
   !> nor filled.  Otherwise the inherited routine, as before.
   subroutine gpu_calculate_intersite_gf_eta(this)
      class(green_gpu), intent(inout) :: this
      integer :: i, fermi_point
      if (this%intersite_on_device) then
         call this%en%e_mesh()
         fermi_point = 0
         do i = 1, this%en%channels_ldos + 10
            if ((this%en%ene(i) - this%en%fermi) .le. 0.000001d0) fermi_point = i
         end do
         write (*, *) this%en%fermi, fermi_point
         if (this%control%recur == 'block') then
            if (.not. allocated(this%b2_unrooted)) this%b2_unrooted = this%recursion%b2_b
            call this%recursion%zsqr()
         end if
         this%intersite_fetched = .false.
         return
      end if
      call intersite_arrays(this)
      call this%green%calculate_intersite_gf_eta()
   end subroutine gpu_calculate_intersite_gf_eta

end module green_gpu_mod
