!------------------------------------------------------------------------------
! rsrec_binding -- iso_c_binding interface of librsrec (include/rsrec.h).
!
! The reference is 100 % Fortran and has no FFI today; these are the bind(C)
! interfaces the GPU recursion type (recursion_gpu.f90) calls.  Every array is
! passed exactly as the reference stores it (column-major, complex(rp) =
! interleaved re/im, 1-based atom numbers), so no host-side reshuffling.
!------------------------------------------------------------------------------
module rsrec_binding
   use, intrinsic :: iso_c_binding
   implicit none
   public

   interface
      function rsrec_version() bind(C, name='rsrec_version') result(v)
         import :: c_int
         integer(c_int) :: v
      end function

      function rsrec_device_count() bind(C, name='rsrec_device_count') result(n)
         import :: c_int
         integer(c_int) :: n
      end function

      function rsrec_create(handle, device) bind(C, name='rsrec_create') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), intent(out) :: handle
         integer(c_int), value :: device
         integer(c_int) :: rc
      end function

      function rsrec_destroy(handle) bind(C, name='rsrec_destroy') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function

      function rsrec_set_lattice(handle, kk, nncols, nn, iz, nmax, ntype) bind(C, name='rsrec_set_lattice') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: kk, nncols, nmax, ntype
         type(c_ptr), value :: nn, iz
         integer(c_int) :: rc
      end function

      function rsrec_block_green(handle, nsites, lld, nen, ene, eta_re, eta_im, sym_term, a_inf, b_inf, a_b, b_sqrt, g0) &
         bind(C, name='rsrec_block_green') result(rc)
         import :: c_int, c_ptr, c_double, c_double_complex
         type(c_ptr), value :: handle
         integer(c_int), value :: nsites, lld, nen, sym_term
         real(c_double), value :: eta_re, eta_im
         type(c_ptr), value :: ene, a_inf, b_inf, a_b, b_sqrt
         complex(c_double_complex), dimension(*), intent(inout) :: g0   ! by address: green%g0 itself can be the target (833 MB for 64 sites: no staging copy)
         integer(c_int) :: rc
      end function

      function rsrec_chebyshev_green(handle, nsites, lld, nen, ene, energy_min, energy_max, mu_n, g0) &
         bind(C, name='rsrec_chebyshev_green') result(rc)
         import :: c_int, c_ptr, c_double, c_double_complex
         type(c_ptr), value :: handle
         integer(c_int), value :: nsites, lld, nen
         real(c_double), value :: energy_min, energy_max
         type(c_ptr), value :: ene, mu_n
         complex(c_double_complex), dimension(*), intent(inout) :: g0   ! by address (see rsrec_block_green)
         integer(c_int) :: rc
      end function

      function rsrec_set_positions(handle, cr) bind(C, name='rsrec_set_positions') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         type(c_ptr), value :: cr
         integer(c_int) :: rc
      end function

      function rsrec_set_hamiltonian(handle, nslots, hoh, nsp, ee, lsham, eeo, enim, hall, hallo) &
         bind(C, name='rsrec_set_hamiltonian') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: nslots, hoh, nsp
         type(c_ptr), value :: ee, lsham, eeo, enim, hall, hallo
         integer(c_int) :: rc
      end function

      function rsrec_assemble_blocks(handle, part, ncls, nslots, hoh, hmag, nbr_type, obarm, ntype, blocks, blocks_o) &
         bind(C, name='rsrec_assemble_blocks') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: part, ncls, nslots, hoh, ntype
         type(c_ptr), value :: hmag, nbr_type, obarm, blocks, blocks_o
         integer(c_int) :: rc
      end function

      function rsrec_block_lanczos(handle, nsites, seed_atoms, lld, a_b, b2_b) bind(C, name='rsrec_block_lanczos') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: nsites, lld
         type(c_ptr), value :: seed_atoms, a_b, b2_b
         integer(c_int) :: rc
      end function

      function rsrec_block_lanczos_seeded(handle, nchains, nseed, seed_atoms, seed_coef, lld, a_b, b2_b) &
         bind(C, name='rsrec_block_lanczos_seeded') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: nchains, nseed, lld
         type(c_ptr), value :: seed_atoms, seed_coef, a_b, b2_b
         integer(c_int) :: rc
      end function

      function rsrec_block_lanczos_local_axis(handle, nsites, seed_atoms, rot, lld, a_b, b2_b) &
         bind(C, name='rsrec_block_lanczos_local_axis') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: nsites, lld
         type(c_ptr), value :: seed_atoms, rot, a_b, b2_b
         integer(c_int) :: rc
      end function

      function rsrec_pack_diag(handle, site_offset, nsites_total, a_img, b2_img) bind(C, name='rsrec_pack_diag') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: site_offset, nsites_total
         type(c_ptr), value :: a_img, b2_img
         integer(c_int) :: rc
      end function

      function rsrec_terminator(handle, nsites, lld, a_b, b_sqrt, a_inf, b_inf, a_inf0, b_inf0) bind(C, name='rsrec_terminator') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: nsites, lld
         type(c_ptr), value :: a_b, b_sqrt, a_inf, b_inf, a_inf0, b_inf0
         integer(c_int) :: rc
      end function

      function rsrec_scalar_density(handle, nsites, nmdir, llmax, lld, a, b2, npts, ene, dw_l, cshi, tdens) bind(C, name='rsrec_scalar_density') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: nsites, nmdir, llmax, lld, npts
         type(c_ptr), value :: a, b2, ene, dw_l, cshi, tdens
         integer(c_int) :: rc
      end function

      function rsrec_block_ldos(handle, nen, ene, eta_re, eta_im, sym_term, site_offset, nsites_total, dtot, dosia, dosial, a_inf, b_inf) &
         bind(C, name='rsrec_block_ldos') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nen, sym_term, site_offset, nsites_total
         real(c_double), value :: eta_re, eta_im
         type(c_ptr), value :: ene, dtot, dosia, dosial, a_inf, b_inf
         integer(c_int) :: rc
      end function

      ! the LDOS stage on the Chebyshev moments resident on the device: the images of rsrec_block_ldos
      function rsrec_chebyshev_ldos(handle, nen, ene, energy_min, energy_max, site_offset, nsites_total, dtot, dosia, dosial) &
         bind(C, name='rsrec_chebyshev_ldos') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nen, site_offset, nsites_total
         real(c_double), value :: energy_min, energy_max
         type(c_ptr), value :: ene, dtot, dosia, dosial
         integer(c_int) :: rc
      end function

      ! spec(k, ie, site) = Im Tr(O_k g0) on the chains resident on the device (no g0 is formed): ops complex (18,18,nop), spec real
      ! (nop, nen, nsites_total), this rank's sites at site_offset+1 ..
      function rsrec_block_spectra(handle, nop, ops, nen, ene, eta_re, eta_im, sym_term, site_offset, nsites_total, spec) &
         bind(C, name='rsrec_block_spectra') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nop, nen, sym_term, site_offset, nsites_total
         real(c_double), value :: eta_re, eta_im
         type(c_ptr), value :: ops, ene, spec
         integer(c_int) :: rc
      end function

      function rsrec_chebyshev_spectra(handle, nop, ops, nen, ene, energy_min, energy_max, site_offset, nsites_total, spec) &
         bind(C, name='rsrec_chebyshev_spectra') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nop, nen, site_offset, nsites_total
         real(c_double), value :: energy_min, energy_max
         type(c_ptr), value :: ops, ene, spec
         integer(c_int) :: rc
      end function

      ! the integrals behind the spectra: mom(p+1, s, site) = simpson_m(.., nexp = p) and cum(s, ie, site) = simpson_f(.., EF = ene(ie), T = 0) of
      ! the series y = comb . spec (comb = NULL: the rows themselves); spec = NULL: the image the last spectra call left on the device
      function rsrec_spectra_integrals(handle, nop, spec, nser, comb, nen, ene, nv1, nv1_fermi, edel, e1, fermi, nsites, site_offset, &
                                       nsites_total, mom, cum) bind(C, name='rsrec_spectra_integrals') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nop, nser, nen, nv1, nv1_fermi, nsites, site_offset, nsites_total
         real(c_double), value :: edel, e1, fermi
         type(c_ptr), value :: spec, comb, ene, mom, cum
         integer(c_int) :: rc
      end function

      ! the Kubo-Bastin conductivity integrand integrand_at(l,l,:,v), factor applied, without gamma_nm (conductivity.f90:158-281)
      function rsrec_kubo_integrand(handle, nvec, cond_ll, mu_nm, nen, ene, energy_min, energy_max, integrand) &
         bind(C, name='rsrec_kubo_integrand') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nvec, cond_ll, nen
         type(c_ptr), value :: mu_nm, ene, integrand
         real(c_double), value :: energy_min, energy_max
         integer(c_int) :: rc
      end function

      ! the same from the orbital-diagonal moments (18,cond_ll,cond_ll,nvec); mu_diag = c_null_ptr: the moments rsrec_kubo_moments_diag left
      ! resident on the handle (an error if there are none, or nvec / cond_ll differ)
      function rsrec_kubo_integrand_diag(handle, nvec, cond_ll, mu_diag, nen, ene, energy_min, energy_max, integrand) &
         bind(C, name='rsrec_kubo_integrand_diag') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nvec, cond_ll, nen
         type(c_ptr), value :: mu_diag, ene, integrand
         real(c_double), value :: energy_min, energy_max
         integer(c_int) :: rc
      end function

      ! the conductivity from the integrand: the 38 series of every set (the sum over the vectors; with per_vector /= 0 every vector too)
      ! and their Fermi-weighted Simpson integrals up to every energy (conductivity.f90:283-372); sigma, series: real (38, nen, nsets)
      function rsrec_kubo_conductivity(handle, nvec, per_vector, nen, nv1, ene, energy_min, energy_max, temperature, integrand, sigma, series) &
         bind(C, name='rsrec_kubo_conductivity') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nvec, per_vector, nen, nv1
         type(c_ptr), value :: ene, integrand, sigma, series
         real(c_double), value :: energy_min, energy_max, temperature
         integer(c_int) :: rc
      end function

      ! the optical conductivity from the orbital-diagonal moments (NULL: the resident ones) on a uniform mesh: opt complex (18, nw, nfermi, nset),
      ! opt(l, k, f, s) at omega_k = k (ene(2) - ene(1)) and Fermi level fermi(f); J(E, E') is never formed (kernels_optical.hpp)
      function rsrec_kubo_optical(handle, nset, cond_ll, mu_diag, nen, ene, energy_min, energy_max, nw, nfermi, fermi, temperature, opt) &
         bind(C, name='rsrec_kubo_optical') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nset, cond_ll, nen, nw, nfermi
         type(c_ptr), value :: mu_diag, ene, fermi, opt
         real(c_double), value :: energy_min, energy_max, temperature
         integer(c_int) :: rc
      end function

      ! exchange couplings of the rank's pairs: intersite g + Jij / Dij / Iij integrands + Simpson integrals (exchange.f90:1032-1615)
      function rsrec_exchange(handle, kind, npairs, same, lld, nen, ene, nv1, fermi, sym_term, energy_min, energy_max, a_inf, b_inf, &
                              coef_a, coef_b, dpar, pair_offset, npairs_total, xc, so, fo, parts, jcum, integrand) &
         bind(C, name='rsrec_exchange') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: kind, npairs, lld, nen, nv1, sym_term, pair_offset, npairs_total
         real(c_double), value :: fermi, energy_min, energy_max
         type(c_ptr), value :: same, ene, a_inf, b_inf, coef_a, coef_b, dpar, xc, so, fo, parts, jcum, integrand
         integer(c_int) :: rc
      end function

      ! torque-correlation damping traces of the rank's pairs on the same chains (exchange.f90:674-694); the prefactor stays the caller's
      function rsrec_damping(handle, kind, npairs, same, lld, nen, ene, ief, sym_term, energy_min, energy_max, a_inf, b_inf, &
                             coef_a, coef_b, tmat, pair_offset, npairs_total, at_ef, total, rows) &
         bind(C, name='rsrec_damping') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: kind, npairs, lld, nen, ief, sym_term, pair_offset, npairs_total
         real(c_double), value :: energy_min, energy_max
         type(c_ptr), value :: same, ene, a_inf, b_inf, coef_a, coef_b, tmat, at_ef, total, rows
         integer(c_int) :: rc
      end function

      ! auxiliary-GF exchange tensor of the rank's pairs on the same chains (exchange.f90:171-335); jaux unscaled (caller: * 1.0d3/4/pi)
      function rsrec_exchange_aux(handle, kind, npairs, same, lld, nen, ene, nv1, fermi, sym_term, energy_min, energy_max, a_inf, b_inf, &
                                  coef_a, coef_b, apar, pair_offset, npairs_total, jaux, rows) &
         bind(C, name='rsrec_exchange_aux') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: kind, npairs, lld, nen, nv1, sym_term, pair_offset, npairs_total
         real(c_double), value :: fermi, energy_min, energy_max
         type(c_ptr), value :: same, ene, a_inf, b_inf, coef_a, coef_b, apar, jaux, rows
         integer(c_int) :: rc
      end function

      ! spin-lattice coupling of the rank's trios, three pairs (i,j), (i,k), (j,k) each (exchange.f90:338-601); jijk unscaled
      function rsrec_spin_lattice(handle, kind, npairs, same, lld, nen, ene, nv1, fermi, sym_term, energy_min, energy_max, a_inf, b_inf, &
                                  coef_a, coef_b, apar, dmat, trio_offset, ntrios_total, jijk, rows) &
         bind(C, name='rsrec_spin_lattice') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: kind, npairs, lld, nen, nv1, sym_term, trio_offset, ntrios_total
         real(c_double), value :: fermi, energy_min, energy_max
         type(c_ptr), value :: same, ene, a_inf, b_inf, coef_a, coef_b, apar, dmat, jijk, rows
         integer(c_int) :: rc
      end function

      ! T_comm_xc of the rank's pairs on the Gauss-Legendre contour at e0 (green.f90:471-536 + exchange.f90:1804-1865); x, w host arrays
      function rsrec_exchange_contour(handle, kind, npairs, same, lld, npts, x, w, e0, sym_term, energy_min, energy_max, a_inf, b_inf, &
                                      coef_a, coef_b, dmat, pair_offset, npairs_total, xc, rows) &
         bind(C, name='rsrec_exchange_contour') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: kind, npairs, lld, npts, sym_term, pair_offset, npairs_total
         real(c_double), value :: e0, energy_min, energy_max
         type(c_ptr), value :: same, x, w, a_inf, b_inf, coef_a, coef_b, dmat, xc, rows
         integer(c_int) :: rc
      end function

      ! orbital occupations of the rank's on-site chains on the same contour (bands.f90:559-586, :631-650); occ is (18, nsites_total)
      function rsrec_contour_occupation(handle, kind, nsites, lld, npts, x, w, e0, sym_term, energy_min, energy_max, a_inf, b_inf, &
                                        coef_a, coef_b, site_offset, nsites_total, occ, gdiag) &
         bind(C, name='rsrec_contour_occupation') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: kind, nsites, lld, npts, sym_term, site_offset, nsites_total
         real(c_double), value :: e0, energy_min, energy_max
         type(c_ptr), value :: x, w, a_inf, b_inf, coef_a, coef_b, occ, gdiag
         integer(c_int) :: rc
      end function

      function rsrec_kubo_moments(handle, nvec, nseed, seed_atoms, seed_coef, cond_ll, a, b, v_a, vo_a, v_b, vo_b, mu_nm) &
         bind(C, name='rsrec_kubo_moments') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nvec, nseed, cond_ll
         real(c_double), value :: a, b
         type(c_ptr), value :: seed_atoms, seed_coef, v_a, vo_a, v_b, vo_b, mu_nm
         integer(c_int) :: rc
      end function

      ! only the orbital-diagonal moments mu_nm(l,l,n,m,v) -- conductivity.f90:289, :292 read nothing else: mu_diag (18,cond_ll,cond_ll,nvec),
      ! or c_null_ptr; they also stay resident on the handle for rsrec_kubo_integrand_diag
      function rsrec_kubo_moments_diag(handle, nvec, nseed, seed_atoms, seed_coef, cond_ll, a, b, v_a, vo_a, v_b, vo_b, mu_diag) &
         bind(C, name='rsrec_kubo_moments_diag') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nvec, nseed, cond_ll
         real(c_double), value :: a, b
         type(c_ptr), value :: seed_atoms, seed_coef, v_a, vo_a, v_b, vo_b, mu_diag
         integer(c_int) :: rc
      end function

      ! the same for nout output operators v_out / vo_out (18,18,nslots,ntype,nout) on one input operator: mu_diag
      ! (18,cond_ll,cond_ll,nvec,nout), set j = rsrec_kubo_moments_diag with v_a = v_out(:,:,:,:,j); resident as nvec*nout vectors
      function rsrec_kubo_moments_diag_multi(handle, nout, nvec, nseed, seed_atoms, seed_coef, cond_ll, a, b, v_out, vo_out, v_b, vo_b, mu_diag) &
         bind(C, name='rsrec_kubo_moments_diag_multi') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nout, nvec, nseed, cond_ll
         real(c_double), value :: a, b
         type(c_ptr), value :: seed_atoms, seed_coef, v_out, vo_out, v_b, vo_b, mu_diag
         integer(c_int) :: rc
      end function

      ! the double sum over those moments at ne weight columns without the moments: wl, wr complex (cond_ll,ne), row n for order n - 1;
      ! s_full (18,18,ne,nvec,nout) and s_diag (18,ne,nvec,nout) = sum_{n,m} wl(m,e) wr(n,e) mu_j(:,:,n,m,v), either may be c_null_ptr.
      ! Nothing is normalised, nothing stays resident.  The reference writes no file this could fill: there is no drop-in switch.
      function rsrec_kubo_single_shot(handle, nout, nvec, nseed, seed_atoms, seed_coef, cond_ll, a, b, v_out, vo_out, v_b, vo_b, ne, wl, wr, &
                                      s_full, s_diag) bind(C, name='rsrec_kubo_single_shot') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nout, nvec, nseed, cond_ll, ne
         real(c_double), value :: a, b
         type(c_ptr), value :: seed_atoms, seed_coef, v_out, vo_out, v_b, vo_b, wl, wr, s_full, s_diag
         integer(c_int) :: rc
      end function

      ! the same for nout output operators and nin input operators v_in / vo_in (18,18,nslots,ntype,nin): mu_diag
      ! (18,cond_ll,cond_ll,nvec,nout,nin), set (j, i) = rsrec_kubo_moments_diag with (v_a, v_b) = (v_out(:,:,:,:,j), v_in(:,:,:,:,i));
      ! resident as nvec*nout*nin vectors, the input outermost
      function rsrec_kubo_moments_diag_tensor(handle, nin, nout, nvec, nseed, seed_atoms, seed_coef, cond_ll, a, b, v_out, vo_out, v_in, vo_in, &
                                              mu_diag) bind(C, name='rsrec_kubo_moments_diag_tensor') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nin, nout, nvec, nseed, cond_ll
         real(c_double), value :: a, b
         type(c_ptr), value :: seed_atoms, seed_coef, v_out, vo_out, v_in, vo_in, mu_diag
         integer(c_int) :: rc
      end function

      function rsrec_apply_operator(handle, vel, v_op, vo_op, psi_in, psi_out, a, b) bind(C, name='rsrec_apply_operator') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: vel
         real(c_double), value :: a, b
         type(c_ptr), value :: v_op, vo_op, psi_in, psi_out
         integer(c_int) :: rc
      end function

      function rsrec_zsqr(handle, nmat, b2_b) bind(C, name='rsrec_zsqr') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: nmat
         type(c_ptr), value :: b2_b
         integer(c_int) :: rc
      end function

      function rsrec_chebyshev(handle, nsites, seed_atoms, lld, a, b, mu_n) bind(C, name='rsrec_chebyshev') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nsites, lld
         real(c_double), value :: a, b
         type(c_ptr), value :: seed_atoms, mu_n
         integer(c_int) :: rc
      end function

      function rsrec_chebyshev_seeded(handle, nchains, nseed, seed_atoms, seed_coef, lld, a, b, mu_n) &
         bind(C, name='rsrec_chebyshev_seeded') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nchains, nseed, lld
         real(c_double), value :: a, b
         type(c_ptr), value :: seed_atoms, seed_coef, mu_n
         integer(c_int) :: rc
      end function

      !> ijpair: int32 (2, npairs); mu_n: complex (18,18,2*lld+2,4*npairs); m_pair: complex (18,18,2*lld+2,2,npairs) or c_null_ptr
      function rsrec_chebyshev_pairs_direct(handle, npairs, ijpair, lld, a, b, both_ends, mu_n, m_pair) &
         bind(C, name='rsrec_chebyshev_pairs_direct') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: npairs, lld, both_ends
         real(c_double), value :: a, b
         type(c_ptr), value :: ijpair, mu_n, m_pair
         integer(c_int) :: rc
      end function

      !> sources: int32 (nsrc); cr: real (3,kk); cell: real (3,3) or c_null_ptr; kpt: real (3,nk); group: int32 (kk) or c_null_ptr;
      !> s_k: complex (18,18,2*lld+2,nk,ngroup,nsrc) or c_null_ptr
      function rsrec_chebyshev_bloch(handle, nsrc, sources, lld, a, b, cr, cell, nk, kpt, ngroup, group, s_k) &
         bind(C, name='rsrec_chebyshev_bloch') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nsrc, lld, nk, ngroup
         real(c_double), value :: a, b
         type(c_ptr), value :: sources, cr, cell, kpt, group, s_k
         integer(c_int) :: rc
      end function

      !> as rsrec_chebyshev_bloch; w: complex (2*lld+2,ne); g_k: complex (18,18,ne,nk,ngroup,nsrc), a_k: real (18,ne,nk,ngroup,nsrc),
      !> host or device memory, either one c_null_ptr
      function rsrec_chebyshev_bloch_map(handle, nsrc, sources, lld, a, b, cr, cell, nk, kpt, ngroup, group, ne, w, g_k, a_k) &
         bind(C, name='rsrec_chebyshev_bloch_map') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nsrc, lld, nk, ngroup, ne
         real(c_double), value :: a, b
         type(c_ptr), value :: sources, cr, cell, kpt, group, w, g_k, a_k
         integer(c_int) :: rc
      end function

      !> seed_atoms: int32 (nseed,nchains), 0 = unused entry; seed_coef: complex (nseed,nchains); group: int32 (kk) or c_null_ptr;
      !> m_g: complex (18,18,2*lld+2,ngroup,nchains), host or device memory, or c_null_ptr
      function rsrec_chebyshev_lattice(handle, nchains, nseed, seed_atoms, seed_coef, lld, a, b, ngroup, group, m_g) &
         bind(C, name='rsrec_chebyshev_lattice') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nchains, nseed, lld, ngroup
         real(c_double), value :: a, b
         type(c_ptr), value :: seed_atoms, seed_coef, group, m_g
         integer(c_int) :: rc
      end function

      !> the 18 x 18 block of ne functions of H on every atom from the same seeds: w complex (2*lld+2,ne), host; d_full complex
      !> (18,18,ne,kk), d_diag complex (18,ne,kk), host or device memory, either may be c_null_ptr; cnorm real (kk) or c_null_ptr.
      !> Nothing is normalised, nothing stays resident.  The reference has no counterpart: there is no drop-in switch.
      function rsrec_chebyshev_site_map(handle, nvec, nseed, seed_atoms, seed_coef, lld, a, b, ne, w, d_full, d_diag, cnorm) &
         bind(C, name='rsrec_chebyshev_site_map') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nvec, nseed, lld, ne
         real(c_double), value :: a, b
         type(c_ptr), value :: seed_atoms, seed_coef, w, d_full, d_diag, cnorm
         integer(c_int) :: rc
      end function

      !> wave-packet propagation: nt * stride steps of the Chebyshev table w complex (korder), host, from psi(0) = r, chi(0) = 0 with
      !> D = d_op / do_op (18,18,nslots,ntype), applied as v_b / vo_b are; a record after every stride steps: ret complex (18,18,nt,nvec),
      !> m0_full (18,18,mom,nvec), m0_diag (18,mom,nvec), m_full (18,18,mom,nt,nvec), m_diag (18,mom,nt,nvec), host or device memory, each
      !> may be c_null_ptr (mom = 0: ret only).  Nothing is normalised, nothing stays resident.  The reference has no counterpart: there
      !> is no drop-in switch.
      function rsrec_chebyshev_evolve(handle, nvec, nseed, seed_atoms, seed_coef, a, b, d_op, do_op, korder, w, nt, stride, mom, &
                                      ret, m0_full, m0_diag, m_full, m_diag) bind(C, name='rsrec_chebyshev_evolve') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nvec, nseed, korder, nt, stride, mom
         real(c_double), value :: a, b
         type(c_ptr), value :: seed_atoms, seed_coef, d_op, do_op, w, ret, m0_full, m0_diag, m_full, m_diag
         integer(c_int) :: rc
      end function

      function rsrec_scalar_lanczos(handle, nsites, seed_atoms, lld, llmax, a, b2) bind(C, name='rsrec_scalar_lanczos') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: nsites, lld, llmax
         type(c_ptr), value :: seed_atoms, a, b2
         integer(c_int) :: rc
      end function

      subroutine rsrec_site_partition(rank, nprocs, nsites, start_atom, end_atom) bind(C, name='rsrec_site_partition')
         import :: c_int
         integer(c_int), value :: rank, nprocs, nsites
         integer(c_int), intent(out) :: start_atom, end_atom
      end subroutine

      function rsrec_orbital_moments(handle, nseeds, seed_atoms, lld, a, b, cr, alat, mu_orb, mu_seed) bind(C, name='rsrec_orbital_moments') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: nseeds, lld
         real(c_double), value :: a, b, alat
         type(c_ptr), value :: seed_atoms, cr, mu_orb, mu_seed
         integer(c_int) :: rc
      end function

      function rsrec_pack_moments(handle, site_offset, nsites_total, mu_img) bind(C, name='rsrec_pack_moments') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), value :: site_offset, nsites_total
         type(c_ptr), value :: mu_img
         integer(c_int) :: rc
      end function

      ! library-level communicator (RCCL inside librsrec; include/rsrec.h): the MPI_ALLREDUCE(MPI_IN_PLACE, ..., MPI_SUM) of
      ! bands.f90:271-274 without MPI on the host
      function rsrec_comm_unique_id(id) bind(C, name='rsrec_comm_unique_id') result(rc)
         import :: c_int, c_char
         character(kind=c_char), intent(out) :: id(*)          ! 128 bytes
         integer(c_int) :: rc
      end function

      function rsrec_comm_init(handle, rank, nranks, id) bind(C, name='rsrec_comm_init') result(rc)
         import :: c_int, c_ptr, c_char
         type(c_ptr), value :: handle
         integer(c_int), value :: rank, nranks
         character(kind=c_char), intent(in) :: id(*)
         integer(c_int) :: rc
      end function

      function rsrec_comm_init_file(handle, rank, nranks, path, timeout_s) bind(C, name='rsrec_comm_init_file') result(rc)
         import :: c_int, c_ptr, c_char, c_double
         type(c_ptr), value :: handle
         integer(c_int), value :: rank, nranks
         character(kind=c_char), intent(in) :: path(*)         ! NUL-terminated
         real(c_double), value :: timeout_s
         integer(c_int) :: rc
      end function

      function rsrec_allreduce_sum(handle, buf, n) bind(C, name='rsrec_allreduce_sum') result(rc)
         import :: c_int, c_ptr, c_size_t
         type(c_ptr), value :: handle, buf
         integer(c_size_t), value :: n
         integer(c_int) :: rc
      end function

      function rsrec_comm_size(handle, rank, nranks) bind(C, name='rsrec_comm_size') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int), intent(out) :: rank, nranks
         integer(c_int) :: rc
      end function

      function rsrec_comm_destroy(handle) bind(C, name='rsrec_comm_destroy') result(rc)
         import :: c_int, c_ptr
         type(c_ptr), value :: handle
         integer(c_int) :: rc
      end function

      function rsrec_last_error(handle, buf, n) bind(C, name='rsrec_last_error') result(rc)
         import :: c_int, c_ptr, c_char, c_size_t
         type(c_ptr), value :: handle
         character(kind=c_char), intent(out) :: buf(*)
         integer(c_size_t), value :: n
         integer(c_int) :: rc
      end function

      function rsrec_set_option(handle, key, val) bind(C, name='rsrec_set_option') result(rc)
         import :: c_int, c_ptr, c_char, c_long
         type(c_ptr), value :: handle
         character(kind=c_char), intent(in) :: key(*)
         integer(c_long), value :: val
         integer(c_int) :: rc
      end function

      function rsrec_get_timing(handle, out, n) bind(C, name='rsrec_get_timing') result(rc)
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: handle
         real(c_double), intent(out) :: out(*)
         integer(c_int), value :: n
         integer(c_int) :: rc
      end function
   end interface

contains

   !> Error text of a handle as a Fortran string
   function rsrec_error_string(handle) result(msg)
      type(c_ptr), intent(in) :: handle
      character(len=:), allocatable :: msg
      character(kind=c_char) :: buf(512)
      integer :: i, rc
      rc = rsrec_last_error(handle, buf, int(512, c_size_t))
      msg = ''
      do i = 1, 512
         if (buf(i) == c_null_char) exit
         msg = msg//buf(i)
      end do
   end function rsrec_error_string

end module rsrec_binding
