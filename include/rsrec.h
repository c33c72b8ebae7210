/* rsrec.h -- C ABI of librsrec: the MI355X (gfx950) recursion engine for RS-LMTO-ASA.
 *
 * Drop-in boundary for ONE hot path of rslmtoasa/rslmtoasa: the Haydock / block-Lanczos /
 * Chebyshev recursion of source/recursion.f90.  The reference has no FFI today (it is 100 %
 * Fortran); these entry points are what a `bind(C)` interface block in a replacement
 * `recursion_mod` binds (see fortran/rsrec_binding.f90 and INTEGRATION.md).  Each entry point
 * cites the reference procedure it replaces.
 *
 * Conventions (all follow the reference so Fortran arrays are passed as they are):
 *   - every array is caller-allocated HOST memory in Fortran (column-major) order;
 *   - complex(8) data are passed as `const double*` pointing at interleaved (re,im) pairs,
 *     i.e. exactly Fortran `complex(rp)` / C `double _Complex` storage;
 *   - atom numbers are 1-based, 0 = "no neighbour" (lattice.f90:1854, nn(kk, nnmax+1));
 *   - every function returns 0 on success, non-zero on error; the message is read with
 *     rsrec_last_error().  The Fortran shim turns non-zero into g_logger%fatal, which is the
 *     reference's only error behaviour on this path (recursion.f90:1942, :2595).
 *   - one handle per process/GPU; not re-entrant (like the reference's `this%` scratch).
 *   - there is NO CPU fallback: rsrec_create fails if no gfx950 device is usable.
 */
#ifndef RSREC_H
#define RSREC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsrec_handle rsrec_t;

#define RSREC_OK 0
#define RSREC_ERR_ARG 1        /* bad argument / call order */
#define RSREC_ERR_DEVICE 2     /* HIP runtime error (no device, out of memory, launch failure) */
#define RSREC_ERR_DIVERGED 3   /* Chebyshev moments blew up: recursion.f90:2594-2596 (fatal in the reference) */
#define RSREC_ERR_EIG 4        /* 18x18 eigen-solve did not converge: recursion.f90:1942 (zheev info /= 0) */

/* Library/ABI version (major*100 + minor). */
int rsrec_version(void);

/* Number of usable HIP devices (0 if none): the Fortran host maps MPI rank -> device with it (mpi.f90 rank). */
int rsrec_device_count(void);

/* Create / destroy the per-GPU context.  `device` = HIP device ordinal (the rank's local GPU).
 * Replaces nothing in the reference (its recursion type owns host arrays only, recursion.f90:41-116,
 * allocated in restore_to_default :3713-3790); the drop-in module creates the context lazily on the
 * first recur* call (finalizer trap: SURVEY.md section 8b). */
int rsrec_create(rsrec_t **out, int device);
int rsrec_destroy(rsrec_t *h);

/* Geometry tables read by the recursion: lattice%kk, %nn, %iz, %nmax, %ntype
 * (lattice.f90:138-239; read at recursion.f90:1577-1580, :1603-1606).
 *   nn  : int32 (kk, nncols) column-major; nn(i,1) = number of slots incl. on-site, nn(i,j>=2) = atom or 0
 *   iz  : int32 (kk) atom type, 1..ntype
 *   nmax: the first nmax atoms carry per-atom blocks `hall` (impurity region), 0 for bulk/surface */
int rsrec_set_lattice(rsrec_t *h, int kk, int nncols, const int32_t *nn, const int32_t *iz, int nmax, int ntype);

/* OPTIONAL locality hint: Cartesian atom positions, lattice%cr(3,kk) (lattice.f90:138-239), any unit.  The recursion's
 * arithmetic never reads them; they only decide the ORDER in which atoms are processed so that neighbouring atoms share
 * their psi-block gathers in L2.  Without the hint an ordering is derived from graph distances.  Results do not depend on it
 * beyond summation order of the reductions. */
int rsrec_set_positions(rsrec_t *h, const double *cr);

/* Operator blocks read by the recursion: hamiltonian%ee, %lsham, %eeo, %enim, %hall, %hallo
 * (hamiltonian.f90:51-64, shapes :290-301).  Must be called again whenever the caller rebuilt them
 * (self.f90:777-797 rebuilds before every recur* call).
 *   ee, eeo    : complex (18,18,nslots,ntype)      hall, hallo : complex (18,18,nslots,nmax) (NULL if nmax = 0)
 *   lsham, enim: complex (18,18,ntype)
 *   hoh != 0 selects H = h - h*o*h + e_nu + l.s (hop_b_hoh, recursion.f90:1411); eeo/enim/hallo may be NULL otherwise.
 *   nsp: control%nsp (1..4); only the scalar recursion reads it (hop is a no-op unless nsp = 1, recursion.f90:3326). */
int rsrec_set_hamiltonian(rsrec_t *h, int nslots, int hoh, int nsp, const double *ee, const double *lsham,
                          const double *eeo, const double *enim, const double *hall, const double *hallo);

/* The raw blocks themselves, assembled on the device: what build_bulkham (hamiltonian.f90:1553-1616; part = 0: one class per atom type,
 * result ee / eeo) and build_locham (:1618-1667; part = 1: one class per impurity atom, result hall / hallo) do after chbar_nc:
 *   blocks(:,:,m,c)   = [[H0 + Hz, Hx - i Hy], [Hx + i Hy, H0 - Hz]]  with (Hx, Hy, Hz, H0) = hmag(:,:,m,1..4) of class c   (:1565-1570, :1631-1636)
 *   blocks_o(:,:,m,c) = blocks(:,:,m,c) * obarm(:,:,nbr_type(m,c)),  zero where nbr_type(m,c) = 0                          (:1599, :1654; hoh only)
 *   hmag     : complex (9,9,nslots,4,ncls) -- the scratch array chbar_nc fills, collected per class by the caller
 *   nbr_type : int32 (nslots,ncls), atom type (1..ntype) behind slot m of the class atom (slot 1: the atom itself), 0 = no atom (:1586-1597)
 *   obarm    : complex (18,18,ntype) (build_obarm, hamiltonian.f90:1486-1506);  nbr_type / obarm / blocks_o may be NULL when hoh = 0
 *   blocks, blocks_o : complex (18,18,nslots,ncls) out -- the caller's ee / eeo or hall / hallo (the reference's host routines read them too).
 * The device copies stay behind: a following rsrec_set_hamiltonian that is handed exactly these arrays (compared bit for bit) takes them
 * from there instead of uploading; arrays that were edited on the host in between are uploaded as always.  Needs no lattice. */
int rsrec_assemble_blocks(rsrec_t *h, int part, int ncls, int nslots, int hoh, const double *hmag, const int32_t *nbr_type,
                          const double *obarm, int ntype, double *blocks, double *blocks_o);

/* Block Lanczos recursion for `nsites` independent chains seeded with psi(:,:,seed) = I18.
 * Replaces recur_b (recursion.f90:1807-1866) + crecal_b (:1873-1973) + hop_b/hop_b_hoh (:1560/:1411).
 *   seed_atoms : int32 (nsites), 1-based cluster atom numbers (lattice%irec(start_atom:end_atom))
 *   a_b, b2_b  : complex (18,18,lld,nsites) out; a_b(:,:,lld,:) = 0 and b2_b(:,:,1,:) = I as in :1836-1837.
 * b2_b holds B^2 (NOT its square root: the reference takes the root later in zsqr). */
int rsrec_block_lanczos(rsrec_t *h, int nsites, const int32_t *seed_atoms, int lld, double *a_b, double *b2_b);

/* Same with general seeds: chain c starts from coef(k,c) * I18 placed on atom seed(k,c), k = 1..nseed.
 * Replaces the four-chain seeds of recur_b_ij (recursion.f90:1655-1800: (psi_i +- psi_j)/sqrt2, (psi_i +- i psi_j)/sqrt2).
 * Seeds are ASSIGNED in order, psi(l,l,seed(k,c)) = coef(k,c): a later seed on the same atom overwrites (as :1709-1714 do).
 *   seed_atoms : int32 (nseed, nchains);  seed_coef : complex (nseed, nchains) */
int rsrec_block_lanczos_seeded(rsrec_t *h, int nchains, int nseed, const int32_t *seed_atoms, const double *seed_coef,
                               int lld, double *a_b, double *b2_b);

/* recur_b with hamiltonian%local_axis = T (non-collinear runs, recursion.f90:1830-1832), every site in ONE batched call.
 * The reference rotates all blocks into the spin frame of site i's moment before that site's chain (rotate_to_local_axis,
 * hamiltonian.f90:2442-2465: ee, hall, eeo, hallo, enim -- NOT lsham) and runs the sites one after the other.  Here the
 * operator is set ONCE in the GLOBAL frame (rsrec_set_hamiltonian with ee_glob, hall_glob, eeo_glob, hallo_glob, enim_glob and
 * lsham) and every chain carries its rotation:
 *   rot : complex (18,18,nsites), R_i = ROTMAT(alpha_i, beta_i, 0) of site i's moment direction (math.f90:2026, car2sph :2155)
 * The chain of the rotated operator equals the chain of the global operator with the on-site term R_i l.s R_i^H, conjugated:
 * a_b(:,:,:,i) = R_i^H A R_i, b2_b likewise -- the library does both, the conjugation on the device (sums in a fixed order, no FMA
 * contraction); a_b(:,:,lld,:) = 0 and b2_b(:,:,1,:) = I stay exact.  Outputs are in the local frame of each site like the reference's.
 *   a_b, b2_b : complex (18,18,lld,nsites) out.
 * The chains are LEFT RESIDENT in each site's local frame, the same bits as the returned arrays: rsrec_pack_diag, rsrec_block_ldos,
 * rsrec_block_spectra and rsrec_contour_occupation (resident) follow this call as they follow rsrec_block_lanczos (the continued fraction,
 * zsqr, get_terminf and their epilogues are covariant under the unitary transform).  rsrec_get_timing: out[12] ms of the conjugation. */
int rsrec_block_lanczos_local_axis(rsrec_t *h, int nsites, const int32_t *seed_atoms, const double *rot, int lld, double *a_b, double *b2_b);

/* The per-site result the ranks exchange after the recursion, packed ON THE DEVICE from the coefficients the last
 * rsrec_block_lanczos / rsrec_block_lanczos_local_axis call left there: a(ll,l,site) = Re a_b(l,l,ll,site), b2 likewise (recursion.f90:1850-1851).
 * The reference gathers per-site arrays with MPI_ALLREDUCE(MPI_IN_PLACE, ..., MPI_SUM) on zero-padded images
 * (bands.f90:271-274); this writes such an image for this rank: sites site_offset+1 .. site_offset+nsites (the rank's
 * start_atom-1 from rsrec_site_partition) are filled, every other site is zero, so one RCCL all-reduce(sum) over the
 * ranks' images is the gather.
 *   a_img, b2_img : real (lld, 18, nsites_total) out -- HOST or DEVICE memory (detected): a device buffer (e.g. the
 *   tensor handed to the collective) is written in place, no host round trip. */
int rsrec_pack_diag(rsrec_t *h, int site_offset, int nsites_total, double *a_img, double *b2_img);

/* In-place principal square root of `nmat` Hermitian 18x18 matrices: b2_b <- sqrt(b2_b).
 * Replaces zsqr (recursion.f90:1980-2023).
 *   Both triangles of every matrix are read and must agree to rounding (zheev('U') of the reference reads the upper one only): the
 *   root returned is the one of the Hermitian matrix both stand for.  Any finite scale is fine -- the solver works on the matrix
 *   times a power of two that brings max|entry| into [1, 2), and sqrt(S 2^k) = sqrt(S) 2^(k/2) holds bit for bit for even k.  A
 *   matrix with a NaN or Inf entry comes back all NaN and the call still returns RSREC_OK (the reference prints zheev's info and
 *   goes on, :2013); RSREC_ERR_EIG only if the Jacobi sweeps of a finite matrix do not converge. */
int rsrec_zsqr(rsrec_t *h, int nmat, double *b2_b);

/* Green function from the block coefficients -- the stage right after the recursion.
 * Replaces green%block_green (green.f90:588-621) + green%bgreen (:1191-1339) for the sites of this rank:
 *   g0(:,:,ie,site) = B_1^H [ E - A_1 - B_2^H [ ... ]^-1 B_2 ]^-1 B_1 , levels lld-1 .. 1, closed by the square-root terminator.
 *   ene    : real (nen) energy mesh, energy%ene(1:channels_ldos+10) (energy.f90:205-207)
 *   eta    : complex broadening added to E on the diagonal (block_green: 0; block_green_eta: the caller's eta)
 *   sym_term: control%sym_term (orbital-independent terminator, green.f90:1268-1277)
 *   a_inf, b_inf : real (18,18,nsites) from recursion%get_terminf (recursion.f90:2092) or rsrec_terminator
 *   a_b    : complex (18,18,lld,nsites) as returned by rsrec_block_lanczos
 *   b_sqrt : complex (18,18,lld,nsites) = b2_b AFTER rsrec_zsqr (self.f90:829 calls zsqr before block_green)
 *   g0     : complex (18,18,nen,nsites) out */
int rsrec_block_green(rsrec_t *h, int nsites, int lld, int nen, const double *ene, double eta_re, double eta_im, int sym_term,
                      const double *a_inf, const double *b_inf, const double *a_b, const double *b_sqrt, double *g0);

/* Band-dependent terminator coefficients of the block recursion.  Replaces recursion%get_terminf (recursion.f90:2092-2135) with
 * get_cinf (:2030-2086), bpopt (:3540-3580: Beer-Pettifor iteration) and emami (:3589-3700: extreme eigenvalues of the tridiagonal
 * chain by Sturm bisection): one GPU thread per matrix element and site, the reference's operations in the reference's order.
 *   a_b    : complex (18,18,lld,nsites);  b_sqrt : complex (18,18,lld,nsites) = b2_b after zsqr (self.f90:829)
 *   a_inf, b_inf : real (18,18,nsites) out;  a_inf0, b_inf0 : real (nsites) out (mean diagonals; may be NULL) */
int rsrec_terminator(rsrec_t *h, int nsites, int lld, const double *a_b, const double *b_sqrt, double *a_inf, double *b_inf,
                     double *a_inf0, double *b_inf0);

/* The stage behind the SCALAR recursion (control%recur = 'lanczos'): replaces dos%density (density_of_states.f90:248-363) with its
 * continued fraction bprldos (:370-404), which green%sgreen (green.f90:628-705) calls for every site and direction and turns into g0.
 * Per chain (orbital, site, direction): the Beer-Pettifor band edges (bpOPT on sqrt(b2), recursion.f90:3540; x 1.01 on orbitals 1 and 10),
 * then one scalar continued fraction per energy, closed by the square-root terminator of that band -- one GPU thread each, the reference's
 * operations in the reference's order.
 *   a, b2  : real (llmax,18,nsites,nmdir) = recursion%a, %b2 (recursion.f90:3485 recur);  lld = control%lld <= llmax
 *   ene    : real (npts) = energy%ene(1:channels_ldos+10);  dw_l, cshi : real (18,nsites) = potential%dw_l, %cshi of the sites' atoms
 *   tdens  : real (18,npts,nsites,nmdir) out = density's `tdens` for every (site, direction) */
int rsrec_scalar_density(rsrec_t *h, int nsites, int nmdir, int llmax, int lld, const double *a, const double *b2, int npts, const double *ene,
                         const double *dw_l, const double *cshi, double *tdens);

/* The whole LDOS stage for the sites of the LAST rsrec_block_lanczos call, from the coefficients that call left on the device
 * (nothing is uploaded but the energy mesh): zsqr (recursion.f90:1980) -> get_terminf (:2092) -> green%bgreen (green.f90:1191,
 * eta / sym_term as in rsrec_block_green) -> the reduction of bands%calculate_fermi (bands.f90:258-268),
 *   dosial(ia,j,i) = -Im g0(j,j,i,ia)/pi,  dosia(ia,i) = sum_j dosial,  dtot(i) = sum_ia dosia   (summed in the reference's order).
 * Outputs are the zero-padded images the reference all-reduces over the ranks (bands.f90:271-274): this rank's sites are
 * site_offset+1 .. site_offset+nsites of nsites_total, every other site is zero.
 *   dtot : real (nen);  dosia : real (nsites_total, nen);  dosial : real (nsites_total, 18, nen)  -- HOST or DEVICE memory (all three
 *   alike, detected): device buffers are written in place and can be handed to the collective without a host round trip.
 *   a_inf, b_inf : real (18,18,nsites) host out, the terminators used (may be NULL).
 * 18 doubles per site and energy leave the GPU instead of the 648 of g0. */
int rsrec_block_ldos(rsrec_t *h, int nen, const double *ene, double eta_re, double eta_im, int sym_term, int site_offset, int nsites_total,
                     double *dtot, double *dosia, double *dosial, double *a_inf, double *b_inf);

/* Green function from the Chebyshev moments.  Replaces green%chebyshev_green (green.f90:1030-1108) for the sites of this rank:
 *   g0(:,:,ie,site) = sum_i mu_n(:,:,i,site) k_i (-i) exp(-i (i-1) acos w_ie) / sqrt(a^2 - (e_ie - b)^2),  w = (e - b)/a,
 *   k = Jackson kernel (math.f90:1641) times 2 for i > 1; a, b from energy_min/max as in rsrec_chebyshev.
 *   mu_n : complex (18,18,2*lld+2,nsites) as returned by rsrec_chebyshev;  g0 : complex (18,18,nen,nsites) out */
int rsrec_chebyshev_green(rsrec_t *h, int nsites, int lld, int nen, const double *ene, double energy_min, double energy_max,
                          const double *mu_n, double *g0);

/* The LDOS stage for the sites of the LAST rsrec_chebyshev call, from the moments that call left on the device (nothing is uploaded
 * but the energy mesh and the 2*lld+2 kernel weights): the diagonal of green%chebyshev_green (green.f90:1030-1108; a, b and the
 * Jackson kernel as in rsrec_chebyshev_green, the sum over the moments in the reference's order) -> the reduction of
 * bands%calculate_fermi (bands.f90:258-268), the one rsrec_block_ldos ends with.  Only the 18 diagonal elements of every moment are
 * read and no g0 is formed.  The moments stay resident and unchanged (rsrec_pack_moments, rsrec_exchange kind = 1 and a second call
 * still find them); two calls with the same input give the same bits.
 *   dtot : real (nen);  dosia : real (nsites_total, nen);  dosial : real (nsites_total, 18, nen)  -- the zero-padded images of
 *   rsrec_block_ldos (this rank's sites at site_offset+1 ..), HOST or DEVICE memory (all three alike, detected).
 * Energies on or outside b -+ a give NaN, as in the reference (acos and the square root of a negative number).
 * RSREC_ERR_ARG unless the moments of rsrec_chebyshev are what the device holds.
 * rsrec_get_timing: out[0] device ms of the call, out[1] ms of the diagonal kernel alone. */
int rsrec_chebyshev_ldos(rsrec_t *h, int nen, const double *ene, double energy_min, double energy_max, int site_offset, int nsites_total,
                         double *dtot, double *dosia, double *dosial);

/* Operator spectra of the on-site Green function for the sites of the LAST rsrec_block_lanczos / rsrec_chebyshev call, from the chains
 * that call left on the device:
 *   spec(k, ie, s) = Im Tr(O_k g0(:,:,ie,s))          (no -1/pi applied)
 * with g0 exactly what green%bgreen (block: zsqr -> get_terminf -> the continued fraction, eta / sym_term as in rsrec_block_green) or
 * green%chebyshev_green (a, b and the Jackson kernel as in rsrec_chebyshev_green) gives for that site and energy.  No g0 is formed in
 * memory: the block kernel contracts it where it lies after the last level, the Chebyshev route forms Tr(O_k mu_i) once per site and
 * sums those over the moments.  Everything bands%calculate_magnetic_moments, calculate_orbital_moments, calculate_moments and
 * calculate_orbital_quadrupoles read of g0 is such a functional (bands.f90:437-456, :985-993, :1123-1127, :1168-1180).
 *   ops  : complex (18,18,nop), column-major, interleaved re/im, 1 <= nop <= 32 -- HOST or DEVICE memory (detected)
 *   spec : real (nop, nen, nsites_total) out, HOST or DEVICE memory (detected): the zero-padded image, this rank's sites at
 *          site_offset+1 .. site_offset+nsites, every other site zero.
 * The sums over the 324 elements run in a fixed order: repeated calls, host and device `spec`, and calls that differ in site_offset give
 * the same bits.  The resident chains stay as they are (b2_b stays B^2).
 * RSREC_ERR_ARG unless the chains of the matching recursion are what the device holds; rsrec_chebyshev_spectra also refuses an lld whose
 * nop (2 lld + 2) traces do not fit the LDS staging.  RSREC_ERR_EIG as rsrec_block_ldos.
 * rsrec_get_timing: out[0] device ms of the call, out[1] ms of the Green kernel (block) / the energy sum (Chebyshev) alone. */
int rsrec_block_spectra(rsrec_t *h, int nop, const double *ops, int nen, const double *ene, double eta_re, double eta_im,
                        int sym_term, int site_offset, int nsites_total, double *spec);
int rsrec_chebyshev_spectra(rsrec_t *h, int nop, const double *ops, int nen, const double *ene, double energy_min, double energy_max,
                        int site_offset, int nsites_total, double *spec);

/* The integrals that follow the spectra in an SCF iteration (bands.f90:476-496, :807-832, :1129-1143, :1040-1060), on the device.
 * A series is a fixed-order real combination of the spectra rows of one site,
 *   y(s, i, site) = 0.0 + sum_k comb(k, s, site) spec(k, i, site),  k ascending, no FMA contraction
 * (dx / dy / dz, the six dspd rows with the site's moment direction, the L and Q rows), and every series gets
 *   cum(s, i, site) = simpson_f(ene, EF = ene(i), nv1, y(s, :, site), fermi = .true., .false., T = 0)   for every i of the mesh
 *   mom(p+1, s, site) = simpson_m(.., H = edel, EF = fermi, NPTS = nv1_fermi, y(s, :, site), EA = e1, nexp = p, ene),  p = 0, 1, 2
 * (math.f90:1600-1632, :1579-1598, the end term (EF - EA)/6 included when e1 /= fermi).  cum costs O(nen) per series: at T = 0 the Fermi
 * weights are exactly 1, 0.5, 0, the triples below a limit are a running sum shared by all limits, and only the one or two triples that
 * hold the limit differ (kernels_moments.hpp).  For finite input cum carries the bits of the rule evaluated limit by limit; every index
 * above nen contributes zero (the convention of kernels_simpson.hpp).  No atomics, fixed order: results are identical run to run.
 *   spec : real (nop, nen, nsites_total), HOST or DEVICE memory (detected), the zero-padded image of the spectra calls; the sites
 *          site_offset+1 .. site_offset+nsites are read.  NULL: the image the last rsrec_block_spectra / rsrec_chebyshev_spectra call on
 *          this handle produced -- those calls keep it on the handle (nop nen nsites doubles) until the resident chains are dropped; nop,
 *          nen, nsites, site_offset and nsites_total must then be that call's.  With spec given neither lattice nor Hamiltonian is needed.
 *   comb : real (nop, nser, nsites), HOST or DEVICE memory, or NULL: the series are the rows themselves (nser = nop).
 *          1 <= nop <= 32, 1 <= nser <= RSREC_MOMENT_NSER_MAX.
 *   ene  : real (nen), host; ascending by more than 1e-12 per point (what makes the weights exact).  nv1: the mesh's nv1 of the cumulative
 *          rule, nen >= nv1 + 9.  nv1_fermi, edel, e1, fermi: bands%nv1, energy%edel, bands%e1, energy%fermi; 1 <= nv1_fermi <= nen - 2.
 *   mom  : real (3, nser, nsites_total) out;  cum : real (nser, nen, nsites_total) out -- zero-padded images like spec, each HOST or DEVICE
 *          memory (detected); either may be NULL, not both.
 * RSREC_ERR_ARG with a message (the handle stays usable) for: no resident image or one of another shape; nen < nv1 + 9; nv1_fermi out of
 * range; non-finite edel, e1 or fermi; nop or nser out of range; a mesh that does not ascend.
 * rsrec_get_timing: out[0] device ms of the call. */
#define RSREC_MOMENT_NSER_MAX 64
int rsrec_spectra_integrals(rsrec_t *h, int nop, const double *spec, int nser, const double *comb, int nen, const double *ene, int nv1,
                            int nv1_fermi, double edel, double e1, double fermi, int nsites, int site_offset, int nsites_total,
                            double *mom, double *cum);

/* Chebyshev (KPM, moment doubling) recursion.  Replaces chebyshev_recur (recursion.f90:3057-3130) with
 * cheb_0th_mom (:2145), cheb_1st_mom[_hoh] (:2169/:2245), chebyshev_recur_ll[_hoh] (:2495/:2605).
 *   a, b : scale and shift, a = (energy_max-energy_min)/(2-0.3), b = (energy_max+energy_min)/2 (:3078-3079)
 *   mu_n : complex (18,18,2*lld+2,nsites) out
 * Returns RSREC_ERR_DIVERGED if sum(real(mu_n(:,:,2ll+2))) > 1000 at any step (:2594). */
int rsrec_chebyshev(rsrec_t *h, int nsites, const int32_t *seed_atoms, int lld, double a, double b, double *mu_n);

/* Same with general seeds, psi0(l,l,seed(k,c)) = coef(k,c) in order.  Replaces chebyshev_recur_ij (recursion.f90:2376-2487),
 * whose four chains per pair start from (psi_i +- psi_j)/sqrt2 and (psi_i +- i psi_j)/sqrt2; both new moments are tested
 * against the 1000 bound (:2484).  seed_atoms int32 (nseed, nchains), seed_coef complex (nseed, nchains), nseed <= 8. */
int rsrec_chebyshev_seeded(rsrec_t *h, int nchains, int nseed, const int32_t *seed_atoms, const double *seed_coef,
                           int lld, double a, double b, double *mu_n);

/* The pair moments of chebyshev_recur_ij from ONE chain per atom instead of four per pair.  Everything that reads the four moment sets of
 * a pair only recombines them (green.f90:446-453; chebyshev_green_ij is linear in the moments) into
 *   M_ij(n) = <i| T_{n-1}(H~) |j>,  M_ji(n) = <j| T_{n-1}(H~) |i>,   n = 1 .. 2*lld+2,
 * and M_ji(n) is the 18x18 block at atom j of the Chebyshev vector psi_{n-1} started from the identity at atom i: one chain from i, run
 * for 2*lld+1 applications of H~ (three-term recurrence, no moment doubling, no Gram pass), gives M_ji for every j at once.
 *   ijpair    : int32 (2,npairs), 1-based: pair p is (ijpair(1,p), ijpair(2,p)) = (i, j)
 *   both_ends : 0: the sources are the distinct FIRST atoms of the pairs and M_ij := M_ji^H.  THE CALLER ASSERTS THAT H IS HERMITIAN (the
 *               reference's own doubling identities, mu_{2n+1} = 2 psi_n^H psi_n - mu_1, already require it); nothing checks it.
 *               1: the sources are the distinct atoms of both columns and nothing is conjugated: M_ij comes from source j, M_ji from
 *               source i, M_ii and M_jj from their own sources.
 *   mu_n      : complex (18,18,2*lld+2,4*npairs) out, slot order ij_loc*4 - 4 + reci as rsrec_chebyshev_seeded fills it for the reference's
 *               seeds.  With o = (M_ij + M_ji)/2, q = i (M_ij - M_ji)/2, d = (M_ii + M_jj)/2:
 *                 i /= j, both_ends = 1: d + o, d - o, d + q, d - q -- the reference's own slot values;
 *                 i /= j, both_ends = 0: o, -o, q, -q -- THE REFERENCE'S SLOTS WITHOUT d, which every consumer cancels (gij and gji are
 *                 differences of slots 1, 2 and of slots 3, 4); slots 2 and 4 are the exact negatives of slots 1 and 3;
 *                 i == j: M_ii / 2 in all four slots (the reference's second seed coefficient overwrites the first).
 *   m_pair    : complex (18,18,2*lld+2,2,npairs) out or NULL: M_ij and M_ji themselves.
 * A moment of an order at which the chain's growing region has not reached the target atom is an exact zero.
 * The packed image stays resident exactly as a rsrec_chebyshev_seeded call of 4*npairs chains of depth lld leaves its moments: rsrec_exchange,
 * rsrec_damping, rsrec_exchange_aux, rsrec_spin_lattice and rsrec_exchange_contour with NULL coefficient arrays, and rsrec_pack_moments,
 * follow it unchanged.  Cost of P pairs around one atom: 2*lld+1 chain applications instead of 4*P*(lld+1).
 * Every sum runs in a fixed order without atomics: the same inputs give the same bits, and a pair's moments depend neither on the other
 * pairs of the call nor on option batch.  Both kernel sets (option kernels), hoh and per-atom operator blocks are served.
 * RSREC_ERR_DIVERGED if sum(real(M_ii(n))) > 1000 for any source and order -- the reference's test (recursion.f90:2479) on the one moment
 * that is a chain moment.  RSREC_ERR_ARG for an atom outside 1..kk, lld < 1, a == 0 or a NULL ijpair / mu_n with npairs > 0; the handle
 * stays usable.  npairs = 0 returns RSREC_OK.  rsrec_get_timing as rsrec_chebyshev_seeded: out[0] device ms, out[1] ms in the H|psi>
 * launches, out[2] their number. */
int rsrec_chebyshev_pairs_direct(rsrec_t *h, int npairs, const int32_t *ijpair, int lld, double a, double b, int both_ends,
                                 double *mu_n, double *m_pair);

/* k-resolved Chebyshev moments from ONE chain per atom (no counterpart in the reference, which has no k-space routine).  The Chebyshev
 * vector psi_n started from the identity at atom i holds <j| T_n(H~) |i> at every atom j of its region; its lattice Fourier sum
 *   S_i(k, n) = sum_j exp(-i k.(r_j - r_i)) <j| T_n(H~) |i>
 * is the k-resolved moment: T_n(H~(k)) itself on a periodic one-atom cell, and with the kernel-weighted sum of rsrec_chebyshev_ldos /
 * rsrec_chebyshev_spectra / rsrec_chebyshev_green the Bloch spectral function A(k,E) = -Im Tr G(k,E) / pi (bands of bulk cells, unfolded
 * bands of supercells; with atoms grouped by layer and k in the surface plane the k-parallel resolved spectral function of a slab).
 *   sources : int32 (nsrc), 1-based atoms: chain s starts from the identity at sources(s).  Duplicates are allowed and give equal bits.
 *   cr      : real (3,kk), the positions for THIS call (the rsrec_set_positions hint is neither read nor changed)
 *   cell    : real (3,3), columns = the supercell vectors, or NULL.  Given: every displacement d = cr(:,j) - cr(:,i) is reduced to its
 *             minimum image d - cell nint(cell^-1 d).  For k commensurate with the supercell the reduction does not matter (the phase
 *             of a supercell vector is 1); for any other k the sum only means something while the chain's region has not wrapped
 *             around the cell, and the minimum image is then the displacement the hopping path actually covered.
 *   kpt     : real (3,nk), Cartesian, 2 pi included: the phase is exp(-i k.d).  1 <= nk <= RSREC_BLOCH_NK_MAX.
 *   group   : int32 (kk), values 0..ngroup, 0 = the atom is left out; NULL with ngroup = 1: every atom in group 1.
 *             1 <= ngroup <= RSREC_BLOCH_NGROUP_MAX.
 *   s_k     : complex (18,18,2*lld+2,nk,ngroup,nsrc) out, or NULL (nothing is downloaded):
 *               s_k(:,:,n,q,g,s) = sum over the atoms j with group(j) == g inside the chain's region at order n-1
 *                                  of exp(-i k_q.d(j,i_s)) [psi_{n-1}]_j,    n = 1 .. 2*lld+2
 *             psi follows the three-term recurrence of rsrec_chebyshev_pairs_direct: 2*lld+1 applications of H~, no moment doubling.
 * An atom contributes from the order at which it joins the region; nothing outside the region is ever read.
 * The image stays resident exactly as a rsrec_chebyshev call of nsrc*ngroup*nk sites of depth lld leaves its moments, image index
 * q + nk*((g-1) + ngroup*(s-1)) (0-based q): rsrec_chebyshev_ldos, rsrec_chebyshev_spectra and rsrec_pack_moments follow unchanged, called
 * with nsites_total >= that count.
 * The phases are tabulated once per (source, k-point, atom) with FP64 sincos; the sums are FP64 matrix-core GEMMs (kernels_bloch.hpp).
 * Every sum runs in a fixed order without atomics: the bits of an image depend only on its own k-point, the atom set of its own group
 * and its own source -- not on the other k-points, groups or sources of the call, nor on option batch, nor on what earlier calls left in
 * the work buffers.  Both kernel sets (option kernels), hoh and per-atom operator blocks are served.
 * RSREC_ERR_DIVERGED if sum(real(M_ii(n))) > 1000 for the own block of any source at any order (as rsrec_chebyshev_pairs_direct).
 * RSREC_ERR_ARG with a message, the handle staying usable, for: nk or ngroup out of range; a group value outside 0..ngroup; NULL group
 * with ngroup > 1; a source outside 1..kk; NULL sources, cr or kpt; a singular cell; lld < 1; a == 0.  nsrc = 0 returns RSREC_OK.
 * rsrec_get_timing: out[0] device ms, out[1] ms in the H|psi> launches, out[2] their number, out[5] ms in the phase-table and Bloch-sum
 * kernels alone. */
#define RSREC_BLOCH_NK_MAX 4096
#define RSREC_BLOCH_NGROUP_MAX 16
int rsrec_chebyshev_bloch(rsrec_t *h, int nsrc, const int32_t *sources, int lld, double a, double b, const double *cr, const double *cell,
                          int nk, const double *kpt, int ngroup, const int32_t *group, double *s_k);

/* Functions of H at MANY k-points and a FEW energies from one chain per atom: constant-energy maps A(k, E_F) on dense 2-D grids, layer-resolved
 * cuts of slabs (no counterpart in the reference).  rsrec_chebyshev_bloch Bloch-sums the vector of every order and keeps every moment of every
 * k-point; here the sums are taken in the other order.  With psi_n = T_n(H~)|i> the vector the chain forms anyway,
 *   Y_e = sum_n w(n,e) psi_{n-1},      g_k(:,:,e,q,g,s) = sum_{j in group g, in the final region of source s} exp(-i k_q.d(j,i_s)) [Y_e]_j
 *                                                       = sum_n w(n,e) s_k(:,:,n,q,g,s)   of rsrec_chebyshev_bloch,
 * at the cost of ne complex axpys per order and ONE Bloch sum per energy behind the last order: nothing grows as orders x k-points.
 *   sources, lld, a, b, cr, cell, kpt, ngroup, group : exactly as rsrec_chebyshev_bloch -- the same chain (three-term recurrence, 2*lld+1
 *             applications, twice the launches with hoh), minimum-image rule and groups --, with 1 <= nk <= RSREC_BLOCH_MAP_NK_MAX.
 *   w       : complex (2*lld+2, ne), column-major, host memory: row n weights order n-1.  1 <= ne <= RSREC_BLOCH_MAP_NE_MAX.  The library does
 *             not interpret the weights: the kernel-weighted coefficients of rsrec_chebyshev_green,
 *               w(n,e) = jackson(n) (2 for n > 1) (-i exp(-i (n-1) acos x_e)) / sqrt(a^2 - (E_e - b)^2),   x_e = (E_e - b)/a,
 *             give G(k,E); others give other functions of H (a Fermi function: occupations n(k)).
 *   g_k     : complex (18,18,ne,nk,ngroup,nsrc) out, host or device memory (detected), or NULL: the layout of s_k with the energy in the
 *             moment's place.
 *   a_k     : real (18,ne,nk,ngroup,nsrc) out, host or device memory (detected), or NULL: -Im g_k(l,l,...)/pi, formed on the device from the
 *             same blocks -- bit for bit the diagonal of g_k; a dense map that only wants orbital weights downloads 144 B per point and
 *             energy instead of 5 184 B.  At least one of g_k and a_k is given.
 * Nothing is normalised, and only the sum over the groups has a non-negative spectral weight (a single group's image is not Hermitian).
 * An atom contributes to Y_e from the order at which it joins the source's region; nothing outside the region of the current level is read
 * or written, and the Y_e of a batch are cleared before the seed.  The accumulation is one streaming pass per two orders (option
 * "blochmap_orders" = 1: per order; the same bits), 1 + 2 ne block streams per atom (kernels_blochmap.hpp).  Behind the last order the
 * k-points are taken in chunks: phase table, per energy and group the GEMM and reduce kernels of rsrec_chebyshev_bloch on Y_e, the diagonal,
 * and the chunk's slice of the outputs.  The accumulators, ONE chunk's table and partials are charged per chain when the batch is planned:
 * a call with large ne runs a smaller batch.  The call leaves no resident image, and drops what an earlier call left.
 * Every sum runs in a fixed order without atomics: the bits of g_k(:,:,e,q,g,s) depend only on its own k-point, column e of w, the atom set
 * of its own group and its own source -- not on the other k-points, energies, groups or sources of the call, on ne or nk, on how the
 * k-points are cut into chunks, on options batch and blochmap_orders, or on what earlier calls left in the work buffers.  Both kernel sets
 * (option kernels), hoh and per-atom operator blocks are served.
 * RSREC_ERR_DIVERGED as rsrec_chebyshev_bloch (the source's own block at every order).  RSREC_ERR_ARG with a message, the handle staying
 * usable, for everything rsrec_chebyshev_bloch refuses (nk against RSREC_BLOCH_MAP_NK_MAX), ne out of range, NULL w, a non-finite weight,
 * g_k and a_k both NULL.  nsrc = 0 returns RSREC_OK.
 * rsrec_get_timing: out[0] device ms, out[1] ms in the H|psi> launches, out[2] their number, out[5] ms in the accumulation passes, the
 * phase tables and the final sums together, out[14], out[15], out[16] the three apart. */
#define RSREC_BLOCH_MAP_NE_MAX 16
#define RSREC_BLOCH_MAP_NK_MAX 1048576
int rsrec_chebyshev_bloch_map(rsrec_t *h, int nsrc, const int32_t *sources, int lld, double a, double b, const double *cr, const double *cell,
                              int nk, const double *kpt, int ngroup, const int32_t *group, int ne, const double *w, double *g_k, double *a_k);

/* Chebyshev moments from whole-lattice seeds (no counterpart in the reference).  rsrec_chebyshev_pairs_direct and rsrec_chebyshev_bloch start
 * every chain from ONE atom -- right for a perfect crystal, where every source gives the same answer.  Here the seed covers the lattice,
 * |x> = sum_j c_j |j> (x) 1_18, and the moment is the seed-weighted sum of the vector's own blocks, group by group:
 *   M_g(n) = sum_{j in group g} conj(c_j) [T_n(H~) x]_j = <x| P_g T_n(H~) |x>,   H~ = (H - b)/a.
 *   - plane-wave seeds c_j = exp(+i k.r_j)/sqrt(kk): sum_g M_g(n) is the average over ALL sources i of rsrec_chebyshev_bloch's S_i(k, n) -- the
 *     effective (unfolded) band structure of a disordered supercell, resolved by atom type or layer through `group`, from one chain per
 *     k-point instead of kk;
 *   - random-phase seeds (the vectors cond_calctype = 'random_vec' draws): M_g(n) is the stochastic trace over the atoms of g -- the DOS and
 *     the operator spectra of the whole cell by type, on the vectors a conductivity run uses;
 *   - a seed on one atom i with coefficient 1: M is the chain's own block M_ii(n) of rsrec_chebyshev_pairs_direct.
 *   seed_atoms : int32 (nseed,nchains), 1-based, 0 = unused entry;  seed_coef : complex (nseed,nchains).  1 <= nseed <= kk.  The seed is
 *                placed exactly as rsrec_kubo_moments places its vectors (entries in order: of several on one atom the last one stays), and
 *                the projection weight of an atom is the conjugate of the coefficient actually placed there.
 *   a, b, lld  : as rsrec_chebyshev_pairs_direct: the three-term recurrence, 2*lld+1 applications of H~, orders n = 1 .. 2*lld+2 (order 1 is
 *                the seed itself).  A projected moment has no doubling identity (P_g does not commute with H): one layout serves every use.
 *   group      : int32 (kk), values 0..ngroup, 0 = the atom is left out; NULL with ngroup = 1: every atom in group 1.
 *                1 <= ngroup <= RSREC_LATTICE_NGROUP_MAX.
 *   m_g        : complex (18,18,2*lld+2,ngroup,nchains) out, host or device memory (detected), or NULL (nothing is downloaded).
 * The image stays resident exactly as a rsrec_chebyshev call of nchains*ngroup sites of depth lld leaves its moments, image index
 * (g-1) + ngroup*(c-1): rsrec_chebyshev_ldos, rsrec_chebyshev_spectra, rsrec_pack_moments and rsrec_spectra_integrals follow unchanged, called
 * with nsites_total >= that count.  The LDOS stage reads the REAL PART OF THE DIAGONAL of an image: for a single group that is the
 * symmetrised group weight (P_g delta + delta P_g)/2 -- M_g itself is not Hermitian, only the sum over the groups is.
 * Normalisation: with |c_j|^2 = 1/kk the first moment has tr M_g(1) = 18 N_g/kk (N_g atoms in group g); the caller divides.
 * Every product runs over the WHOLE lattice from order 0 (one k_spmm5 launch per order, two with hoh; there is no growing region), so a
 * sparse seed pays for the whole lattice and gains nothing over the one-atom calls above.  Behind the seed and every product one projection
 * pass reads the blocks of the grouped seeded atoms once (kernels_lattice.hpp).  Up to 8 chains advance together as the chains of one
 * launch (option lattice_vbatch), fewer if the work vectors do not fit.  Both kernel sets (option kernels), hoh and per-atom operator
 * blocks are served.
 * Every sum runs in a fixed order without atomics: the bits of an image depend on its own chain and on the atom set of its own group alone
 * -- not on the other chains of the call or their order, on the other groups' membership, on lattice_vbatch, or on what earlier calls left
 * in the work buffers.
 * RSREC_ERR_DIVERGED if for any chain and order sum_g sum(real(M_g(n))) > 1000 max(1, sum_j |c_j|^2): the sums the call forms anyway (a
 * diverging recurrence grows wherever the vector is non-zero).  RSREC_ERR_ARG with a message, the handle staying usable, for: ngroup out
 * of range; a group value outside 0..ngroup; NULL group with ngroup > 1; a seed atom outside 0..kk; nseed out of range; a chain without
 * any seed; NULL seeds with nchains > 0; nchains < 0; lld < 1; a == 0.  nchains = 0 returns RSREC_OK.
 * rsrec_get_timing: out[0] device ms, out[1] ms in the H|psi> launches, out[2] their number, out[5] ms in the projection kernels alone. */
#define RSREC_LATTICE_NGROUP_MAX 16
int rsrec_chebyshev_lattice(rsrec_t *h, int nchains, int nseed, const int32_t *seed_atoms, const double *seed_coef, int lld, double a, double b,
                            int ngroup, const int32_t *group, double *m_g);

/* Per-atom blocks of ne functions of H for a whole cell, from whole-lattice seeds (kernels_sitemap.hpp).  With the seeds
 * |x^v> = sum_j c^v_j |j> (x) 1_18 of rsrec_chebyshev_lattice the vector the chain forms anyway holds, at atom j,
 *   conj(c^v_j) [f(H~) x^v]_j = |c^v_j|^2 f(H~)_jj + sum_{k != j} conj(c^v_j) c^v_k f(H~)_jk,
 * and the call sums it over the vectors while the orders stream by:
 *   z_n[j]     = sum_v conj(c^v_j) [T_{n-1}(H~) x^v]_j       (v ascending within a tile of vectors, fused multiply-adds)
 *   D(:,:,e,j) = sum_n w(n,e) z_n[j]                          (n ascending)
 *   - random-phase seeds: the second term averages out over the vectors -- the stochastic on-site density matrix of EVERY atom;
 *   - probing seeds (non-zero only on atoms far apart): the second term is small, and exactly zero when the degree 2*lld+1 is below the
 *     graph distance between seeded atoms;
 *   - one-atom seeds with coefficient 1: D(:,:,e,j) = sum_n w(n,e) M_jj(n) of rsrec_chebyshev_pairs_direct.
 * With the columns of the Green weights this is the LDOS of every atom at ne energies; with the Chebyshev coefficients of f, E f, E^2 f for a
 * Fermi function f the occupation matrices and band moments of every atom: 2*lld+1 whole-lattice products per vector, ne accumulators for
 * the whole call, nothing that grows as atoms x orders -- O(N) where one chain per atom is O(N^2).
 *   seed_atoms, seed_coef, nseed, lld, a, b : exactly as rsrec_chebyshev_lattice (placement: of several entries on one atom the last stays;
 *             three-term recurrence, 2*lld+1 applications of H~, orders n = 1 .. 2*lld+2; no growing region).
 *   w       : complex (2*lld+2, ne) column-major, host memory, not interpreted, as in rsrec_chebyshev_bloch_map.  1 <= ne <= RSREC_SITE_MAP_NE_MAX.
 *   d_full  : complex (18,18,ne,kk) out;  d_diag : complex (18,ne,kk) out, bit for bit the diagonal of d_full.  Each host or device memory
 *             (detected) or NULL; at least one is given.  The blocks are in the reference's column-major order.
 *   cnorm   : real (kk) out or NULL: sum_v |c^v_j|^2 of the coefficients actually placed.  The caller divides; nothing is normalised.
 * An atom on which no vector of the call has a coefficient gives an exact zero block.  Both kernel sets (option kernels: the products are
 * k_spmm5 launches on CI vectors either way), hoh and per-atom operator blocks are served.  The call leaves no resident image and drops what
 * an earlier call left.  Up to 8 vectors advance as the chains of one launch (option kubo_vbatch), fewer if the ring does not fit; per
 * vector in flight the call holds PT + 2 ring slots (one more with hoh), once per call ne accumulators of kk blocks and, for a host output,
 * a staging slice whose size does not depend on kk.  RSREC_ERR_DEVICE with the bytes needed if one vector at a time does not fit.
 * Reproducibility: fixed order, no float atomics; the same inputs and options give the same bits whatever earlier calls left in the buffers.
 * The bits of column e depend on neither ne nor the other columns; the bits of an atom's block do not depend on which outputs are asked for,
 * nor on host or device destination.  They DO depend on the order of the vectors, on sitemap_vtile, sitemap_orders and on the vector batch:
 * the accumulator is shared by all vectors, and the sequence of adds into it is (batch, pass, tile, order).
 * RSREC_ERR_DIVERGED if the real or imaginary part of any element of any z_n exceeds 1000 max(1, sum_v sum_j |c^v_j|^2) in magnitude, tested
 * by the accumulation pass on the values it holds; the outputs are then left alone.  RSREC_ERR_ARG with a message, the handle staying
 * usable, for everything rsrec_chebyshev_lattice refuses about seeds, lld and a, for ne out of range, NULL w, a non-finite weight, and
 * d_full and d_diag both NULL.  nvec = 0 returns RSREC_OK and writes nothing.
 * rsrec_get_timing: out[0] device ms, out[1] ms in the H|psi> launches, out[2] their number ((2 with hoh, else 1) (2*lld+1) per batch),
 * out[5] ms in the accumulation passes plus the output stage; out[21], out[22] the two apart. */
#define RSREC_SITE_MAP_NE_MAX 16
int rsrec_chebyshev_site_map(rsrec_t *h, int nvec, int nseed, const int32_t *seed_atoms, const double *seed_coef,
                             int lld, double a, double b, int ne, const double *w,
                             double *d_full, double *d_diag, double *cnorm);

/* Stochastic Kubo-Bastin double moments.  Replaces compute_moments_stochastic (recursion.f90:979-1234) together with the
 * whole-vector products it is built from: ham_vec_matmul (:913), ham_hoh_vec_matmul (:785), velo_vec_matmul (:587),
 * velo_hoh_vec_matmul (:656):
 *   mu(:,:,n,m,i) = sum_k [ T_{m-1}(H~) r_i ]_k^H  [ v_a T_{n-1}(H~) v_b r_i ]_k ,   H~ = (H - b)/a ,  n, m = 1..cond_ll
 * with H the operator set by rsrec_set_hamiltonian (hoh included), T the Chebyshev polynomials (three-term recurrence on whole
 * vectors) and the sum running over every atom k of the lattice.
 *   nvec vectors; vector i starts from psiref(l,l,seed(k,i)) = coef(k,i), k = 1..nseed (seed = 0: entry unused):
 *     cond_calctype = 'per_type'   : one seed, the type's atom lattice%atlist(i), coefficient 1            (:1093-1102)
 *     cond_calctype = 'random_vec' : nseed = kk, coefficient exp(2 pi i rng_k) / sqrt(kk) from the caller's generator (:1103-1114)
 *   seed_atoms : int32 (nseed, nvec);  seed_coef : complex (nseed, nvec)
 *   a, b : scale and shift as in rsrec_chebyshev (:1023-1024)
 *   v_a, v_b   : complex (18,18,nslots,ntype), hamiltonian%v_a / %v_b as setup_kubo_operators (:242) left them
 *   vo_a, vo_b : complex (18,18,nslots,ntype), hamiltonian%vo_a / %vo_b (hoh only, else NULL)
 *   mu_nm : complex (18,18,cond_ll,cond_ll,nvec) out = recursion%mu_nm_stochastic
 * The velocity operators act on the bulk (per-type) atoms only, as in the reference (:591, "not yet implemented" for the
 * per-atom region): rows of v psi on the first nmax atoms are zero. */
int rsrec_kubo_moments(rsrec_t *h, int nvec, int nseed, const int32_t *seed_atoms, const double *seed_coef, int cond_ll, double a, double b,
                       const double *v_a, const double *vo_a, const double *v_b, const double *vo_b, double *mu_nm);

/* The orbital-diagonal part of the same moments, mu_nm_stochastic(l, l, n, m, v): the reference reads the array in two places only,
 * conductivity.f90:289 and :292, and both take (l2, l2, n, m, ntype) -- only conductivity.f90:289, :292 read the moments, and neither
 * reads an off-diagonal element.  Same recurrences and arguments as rsrec_kubo_moments; the contraction forms the 18 diagonals alone
 * (k_kubo_gram_diag: 1/18 of the flops, 1/18 of the download).
 *   mu_diag : complex (18,cond_ll,cond_ll,nvec) out, host or device memory (detected), mu_diag(l,n,m,v) = mu_nm(l,l,n,m,v); NULL: nothing
 *             is copied out.  1 <= cond_ll <= RSREC_COND_LL_MAX.
 * The diagonal moments of all nvec vectors stay on the handle after the call (72 MB per vector at cond_ll = 500) for
 * rsrec_kubo_integrand_diag(mu_diag = NULL) -- unless they do not fit the device beside the call's buffers: the call still succeeds
 * and nothing stays.  They are dropped by the next rsrec_kubo_moments / rsrec_kubo_moments_diag call, by rsrec_set_hamiltonian, by a
 * rsrec_set_lattice that changes the lattice, and whenever another entry point takes the Kubo buffers' memory back.
 * Results are run-to-run bit-identical and do not depend on how many vectors advance together (options kubo_lchunk, kubo_vbatch apply
 * as in rsrec_kubo_moments).  rsrec_get_timing as rsrec_kubo_moments: out[0] device ms, out[5] ms in the contractions. */
int rsrec_kubo_moments_diag(rsrec_t *h, int nvec, int nseed, const int32_t *seed_atoms, const double *seed_coef, int cond_ll, double a, double b,
                            const double *v_a, const double *vo_a, const double *v_b, const double *vo_b, double *mu_diag);

/* The diagonal moments of several responses to one applied field (the reference's sigma_xy, sigma_xy_z-spin and sigma_xy_z-orb examples
 * are three runs that differ in linear_out alone): set j is what rsrec_kubo_moments_diag returns for v_a = v_out(:,:,:,:,j),
 * vo_a = vo_out(:,:,:,:,j) with the same other arguments, bit for bit.  The left vectors T_{m-1}(H~) r and the right recurrence
 * T_{n-1}(H~) v_b r do not depend on the output operator and are formed once: (2 + nout) cond_ll whole-lattice products instead of
 * 3 nout cond_ll, and with hoh the h_bulk pass of every V product is shared too ((5 + 2 nout) cond_ll - 1 launches instead of
 * nout (7 cond_ll - 1)).  With random vectors all responses are evaluated on the same vectors.
 *   nout    : 1 .. RSREC_KUBO_NOUT_MAX
 *   v_out, vo_out : complex (18,18,nslots,ntype,nout); vo_out: hoh only, else NULL
 *   mu_diag : complex (18,cond_ll,cond_ll,nvec,nout) out, host or device (detected) or NULL.  The set index is outermost: a set's slice is
 *             what rsrec_kubo_integrand_diag and rsrec_kubo_conductivity take.
 * The moments of all nvec * nout (vector, set) pairs stay on the handle in that layout when they fit (the rules of
 * rsrec_kubo_moments_diag): rsrec_kubo_integrand_diag(h, nvec * nout, cond_ll, NULL, ...) then returns the integrand (18,nen,nvec,nout).
 * Errors: RSREC_ERR_ARG with a message for nout out of range, a NULL v_out or v_b, hoh without vo_out or vo_b, and the argument errors of
 * rsrec_kubo_moments_diag; the handle stays usable.  Run-to-run bit-identical; a set's bits depend neither on kubo_vbatch nor on the other
 * sets of the call or their order.  rsrec_get_timing as rsrec_kubo_moments_diag. */
#define RSREC_KUBO_NOUT_MAX 8
int rsrec_kubo_moments_diag_multi(rsrec_t *h, int nout, int nvec, int nseed, const int32_t *seed_atoms, const double *seed_coef,
                                  int cond_ll, double a, double b, const double *v_out, const double *vo_out, const double *v_b,
                                  const double *vo_b, double *mu_diag);

/* The diagonal moments of several responses to several applied fields (sigma_xx beside sigma_xy, a Hall angle, the 3 x 3 tensor of a
 * response: the reference's example families in which v_alpha and v_beta take x, y and z in turn).  Set (j, i) is what
 * rsrec_kubo_moments_diag returns for (v_a, v_b) = (v_out(:,:,:,:,j), v_in(:,:,:,:,i)) and the matching vo operators, bit for bit:
 *   mu(l,n,m,v,j,i) = sum_k [T_{m-1}(H~) r_v]_k^H [v_out_j T_{n-1}(H~) v_in_i r_v]_k  on the diagonal.
 * The left vectors are formed once for all sets; the right recurrences of the nin inputs advance together as chains of one launch (chain
 * i nb + c: vector c of input i; at most 8 / nin vectors advance together); every output operator is applied once per order to all inputs'
 * chains.  Per order 1 + nin + nin nout whole-lattice products in 2 + nout launches (hoh: 5 + 2 nout), against nin (2 + nout) for nin multi
 * calls.  With kubo_lchunk = 0 and one batch the call makes 2 L - 2 + nin + nout L SpMM launches (hoh: 4 L - 3 + 2 nin + L (1 + 2 nout)).
 *   nin     : 1 .. RSREC_KUBO_NIN_MAX;  nout : 1 .. RSREC_KUBO_NOUT_MAX;  nin * nout <= RSREC_KUBO_NSET_MAX
 *   v_out, vo_out : complex (18,18,nslots,ntype,nout);  v_in, vo_in : complex (18,18,nslots,ntype,nin);  vo_*: hoh only, else NULL
 *   mu_diag : complex (18,cond_ll,cond_ll,nvec,nout,nin) out, host or device (detected) or NULL.  The input index is outermost: slice
 *             [..., i] is what rsrec_kubo_moments_diag_multi returns for v_b = v_in(:,:,:,:,i), and a single set's slice is what
 *             rsrec_kubo_integrand_diag and rsrec_kubo_conductivity take.
 * The moments of all nvec * nout * nin (vector, set) pairs stay on the handle in that layout when they fit (the rules of
 * rsrec_kubo_moments_diag): rsrec_kubo_integrand_diag(h, nvec * nout * nin, cond_ll, NULL, ...) then returns (18,nen,nvec,nout,nin).
 * Option kubo_setgroup (this call only): the contraction stages one tile of left vectors for up to that many sets of a vector
 * (k_kubo_gram_diag_sets) -- 1: every set by itself with k_kubo_gram_diag, 2 / 3: groups of at most that width (larger values: 3), 0: the
 * default (2: measured 0.75 of the per-set contraction at cond_ll = 500; groups of 3 measured no faster than 1).  A set's bits depend neither on it, nor on kubo_vbatch, nor on the other sets of the call or their order.
 * Errors: RSREC_ERR_ARG with a message for nin, nout or nin * nout out of range, a NULL v_out or v_in, hoh without vo_out or vo_in, and the
 * argument errors of rsrec_kubo_moments_diag; the handle stays usable.  Run-to-run bit-identical.  rsrec_get_timing as
 * rsrec_kubo_moments_diag_multi. */
#define RSREC_KUBO_NIN_MAX 4
#define RSREC_KUBO_NSET_MAX 16
int rsrec_kubo_moments_diag_tensor(rsrec_t *h, int nin, int nout, int nvec, int nseed, const int32_t *seed_atoms, const double *seed_coef,
                                   int cond_ll, double a, double b, const double *v_out, const double *vo_out, const double *v_in,
                                   const double *vo_in, double *mu_diag);

/* Single-shot Kubo sums: the double sum over the moments at a few weight columns, without the moments (kernels_shot.hpp).
 *   L_e = sum_m conj(wl(m,e)) T_{m-1}(H~) r,   R_e = sum_n wr(n,e) T_{n-1}(H~) v_b r,
 *   s(:,:,e,v,j) = sum_k [L_e]_k^H [v_out_j R_e]_k = sum_{n,m} wl(m,e) wr(n,e) mu_j(:,:,n,m,v)
 * with mu_j what rsrec_kubo_moments returns for (v_a, v_b) = (v_out(:,:,:,:,j), v_b).  No left matrix, no cond_ll x cond_ll contraction and
 * no moment array: 2 (cond_ll - 1) chain steps per vector whatever the cell size and about 2 ne + 2 P + 6 work vectors per vector in flight
 * (P: option "shot_orders"), so cond_ll in the thousands fits on a 10^5-atom cell.  The weights are not interpreted.  wl = wr = the damped
 * expansion of delta(E_e - H) gives the Kubo-Greenwood sigma(E_e); two columns per energy give the reference's Kubo-Bastin integrand at
 * chosen energies (Recursion.kubo_greenwood_weights / kubo_bastin_weights of the Python front end).  A Fermi-sea integral over a whole
 * energy mesh (sigma_xy) still needs the moments: rsrec_kubo_moments_diag and rsrec_kubo_conductivity.
 *   seeds, a, b, v_out / vo_out (18,18,nslots,ntype,nout), v_b / vo_b : exactly as rsrec_kubo_moments_diag_multi takes them.
 *             1 <= nout <= RSREC_KUBO_NOUT_MAX.  One applied field per call; several fields are several calls.
 *   wl, wr  : complex (cond_ll, ne) column-major, host; row n weights order n - 1.  1 <= ne <= RSREC_KUBO_SHOT_NE_MAX,
 *             1 <= cond_ll <= RSREC_KUBO_SHOT_LL_MAX.  wl enters bilinearly as written above: the library conjugates it when it
 *             accumulates the bra side.
 *   s_full  : complex (18,18,ne,nvec,nout) out;  s_diag : complex (18,ne,nvec,nout) out, bit for bit the diagonal of s_full.  Each host
 *             or device memory (detected) or NULL; at least one is given.
 * Nothing is normalised and nothing stays resident; resident diagonal moments of an earlier Kubo call are dropped, as any Kubo call drops
 * them.  The buffers are the handle's Kubo buffers, planned before anything is reserved; the vector batch (at most 4: the left and the
 * right recurrence of a vector advance as two chains of the same launches, option kubo_vbatch) shrinks with ne, and if not even one vector
 * fits the call returns RSREC_ERR_DEVICE with the bytes needed.  A diverging recurrence is not detected, as in rsrec_kubo_moments_diag.
 * SpMM launches per batch of nb vectors (rsrec_get_timing out[2] is their sum over the batches):
 *     cond_ll + nb nout ceil(ne / 8)           = 1 (v_b r) + cond_ll - 1 (both recurrences) + the final V products, 8 columns per launch
 *     2 cond_ll + 1 + nb (1 + 2 nout) ceil(ne / 8)   with hoh (every H product two launches, every V product two and a shared h_bulk pass).
 * Determinism: no atomics, every sum in a fixed order.  The bits of s(:,:,e,v,j) depend on their own column of wl / wr, their own vector
 * and their own output operator only -- not on ne or the other columns, the other vectors or kubo_vbatch, the other output operators or
 * their order, shot_orders, whether the outputs are host or device memory, or what earlier calls left in the buffers.  Both kernel sets
 * (option kernels: the Grams on the matrix cores or on plain FMAs) give the same values to rounding, not the same bits.
 * Errors: RSREC_ERR_ARG with a message that names the function for ne, cond_ll or nout out of range, a NULL wl, wr, v_out or v_b, a
 * non-finite weight, both outputs NULL, hoh without vo_out / vo_b, and every seed error of rsrec_kubo_moments_diag; the handle stays usable.
 * nvec = 0 returns RSREC_OK.  rsrec_get_timing: out[0], out[1], out[2], out[5] as rsrec_kubo_moments_diag; out[17] ms in the accumulation
 * passes, out[18] ms in the final stage (its V products, which out[1] counts as well, and the Grams); out[17] + out[18] = out[5]. */
#define RSREC_KUBO_SHOT_NE_MAX 16
#define RSREC_KUBO_SHOT_LL_MAX 65536
int rsrec_kubo_single_shot(rsrec_t *h, int nout, int nvec, int nseed, const int32_t *seed_atoms, const double *seed_coef,
                           int cond_ll, double a, double b, const double *v_out, const double *vo_out,
                           const double *v_b, const double *vo_b, int ne, const double *wl, const double *wr,
                           double *s_full, double *s_diag);

/* Wave-packet propagation: the energy-resolved spreading of a random state in time (kernels_evolve.hpp), the time-dependent route to
 * sigma(E) of large disordered cells (Roche-Mayou; LSQT).  With w the Chebyshev coefficients of exp(-i H tau) in H~ = (H - b)/a, one step is
 *   psi' = sum_n w(n) p_n,   p_n = T_n(H~) psi,
 *   chi' = sum_n w(n) g_n,   g_0 = chi,  g_1 = H~ g_0 + (1/a) D p_0,  g_{n+1} = 2 H~ g_n - g_{n-1} + (2/a) D p_n,      n = 0 .. korder - 1,
 * which gives psi' = U(tau) psi and chi' = [X, U(tau)] psi + U(tau) chi exactly when D = [X, H]; for any other D, chi' is the Frechet
 * derivative of exp(-i H tau) in direction D on psi, plus U(tau) chi.  Steps compose: from psi(0) = r (the placed seed) and chi(0) = 0,
 * chi(t) = [X, U(t)] r, and no position operator ever touches the periodic cell.  nt * stride steps are taken and a record is taken
 * after every `stride` of them, at t_s = s stride tau, s = 1 .. nt:
 *   ret(:,:,s,v)  = r^H psi(t_s) = sum_j conj(c_j) [psi(t_s)]_j                        (the seed projection of rsrec_chebyshev_lattice)
 *   m(:,:,n,s,v)  = chi(t_s)^H T_{n-1}(H~) chi(t_s),  n = 1 .. mom                     (a plain three-term chain from chi(t_s): mom - 1 products)
 *   m0(:,:,n,v)   = r^H T_{n-1}(H~) r                                                  (the same stage on r: the DOS moments DX^2 is divided by)
 *   seeds, a, b : exactly as rsrec_kubo_moments takes them.
 *   d_op, do_op : complex (18,18,nslots,ntype), applied exactly as the Kubo calls apply v_b / vo_b (bulk atoms only, unscaled); do_op is
 *             given with hoh only.  Not interpreted (Recursion.position_commutator of the Python front end builds [X, H]).
 *   w       : complex (korder), host memory: the step's coefficients of orders 0 .. korder - 1 with the phase exp(-i b tau) in them
 *             (evolution_weights of the Python front end).  Not interpreted.  2 <= korder <= RSREC_EVOLVE_KORDER_MAX.
 *   nt, stride, mom : 1 <= nt <= RSREC_EVOLVE_NT_MAX, 1 <= stride <= RSREC_EVOLVE_STRIDE_MAX, 0 <= mom <= RSREC_EVOLVE_MOM_MAX.
 *   ret     : complex (18,18,nt,nvec);  m0_full (18,18,mom,nvec), m0_diag (18,mom,nvec);  m_full (18,18,mom,nt,nvec), m_diag (18,mom,nt,nvec),
 *             the diag forms bit for bit the diagonals of the full ones.  Each host or device memory (detected) or NULL; at least one is
 *             given; with mom = 0 the four moment outputs must be NULL and only ret is formed.  A stage nobody asks for is not run.
 * Nothing is normalised and nothing stays resident; resident diagonal moments of an earlier Kubo call are dropped, as any Kubo call drops
 * them.  Per vector the p and the g recurrence advance as two chains of the same launches, one operator product D p_n is made per order,
 * and one pass per order adds the source term into g_{n+1}; the two sums ride in that pass (option "evolve_orders" = 1) or are added
 * from a ring every P orders (2 .. 16) -- the same bits either way.  Up to 4 vectors are in flight (option kubo_vbatch); the buffers are the
 * handle's Kubo buffers, planned before anything is reserved: per vector in flight 5 + 2 R work vectors (R = 3 fused, P + 2 batched: 41 by default; 4
 * more with hoh), whose ring also serves the moment stage.  RSREC_ERR_DEVICE with the bytes needed if one vector at a time does not fit.
 * Both kernel sets (option kernels: the Grams on the matrix cores or on plain FMAs), hoh and per-atom operator blocks are served.
 * Determinism: no atomics, every sum in a fixed order.  The bits of a vector's outputs depend on that vector, the operators, w, stride and
 * the records before them only -- not on nt, the other vectors, their order or kubo_vbatch, evolve_orders, which outputs are asked for,
 * host or device destination, or what earlier calls left in the buffers.
 * Errors: RSREC_ERR_ARG with a message that names the function, the handle staying usable, for korder, nt, stride or mom out of range, a
 * NULL w or d_op, a non-finite weight, hoh without do_op, every output NULL, a moment output with mom = 0, and every seed error of
 * rsrec_kubo_moments_diag.  nvec = 0 returns RSREC_OK.  RSREC_ERR_DIVERGED if any element of ret is not finite or exceeds
 * 1000 max(1, sum_j |c_j|^2) in magnitude (tested on the host behind the last record); the outputs are then left alone.
 * rsrec_get_timing: out[0] device ms, out[1] / out[2] ms in and number of the H|psi> and D launches, the moment stage's included; out[5]
 * everything else = out[23] ms in the step passes (source add and accumulation) + out[24] ms in the record stage (the seed projection and
 * the moment stage with its Grams; its H products are counted by out[1] as well).  The events behind these figures are folded into the
 * sums and reused whenever more than 8192 are pending behind a step or a record (one stream synchronisation each time), so a run of
 * thousands of steps holds a bounded number of them. */
#define RSREC_EVOLVE_KORDER_MAX 4096
#define RSREC_EVOLVE_NT_MAX 1024
#define RSREC_EVOLVE_STRIDE_MAX 65536
#define RSREC_EVOLVE_MOM_MAX 65536
int rsrec_chebyshev_evolve(rsrec_t *h, int nvec, int nseed, const int32_t *seed_atoms, const double *seed_coef,
                           double a, double b, const double *d_op, const double *do_op,
                           int korder, const double *w, int nt, int stride, int mom,
                           double *ret, double *m0_full, double *m0_diag, double *m_full, double *m_diag);

/* The Kubo-Bastin conductivity integrand of calculate_gamma_nm + calculate_conductivity_tensor (conductivity.f90:158-268), without the
 * (nen, cond_ll, cond_ll) array gamma_nm (the sum factorises into two tables of nen x cond_ll, kernels_cond.hpp):
 *   integrand(l, i, v) = factor sum_{n,m} gamma_nm(i, n, m) mu_nm(l, l, n, m, v),   factor = 16 / (pi (energy_max - energy_min)^2)
 *   mu_nm     : complex (18,18,cond_ll,cond_ll,nvec) in = recursion%mu_nm_stochastic; host or device memory (a device array must be
 *               complete when the call is made: it is read on the library's own stream)
 *   ene       : real (nen) host = energy%ene (the reference passes channels_ldos + 10 points)
 *   integrand : complex (18,nen,nvec) out, host or device = the reference's integrand_at(l,l,:,v); the caller sums over v to get its
 *               integrand(l,l,:).  1 <= cond_ll <= RSREC_COND_LL_MAX.
 * Two calls with the same inputs give the same bits (fixed summation order, no atomics).  rsrec_get_timing: out[0] device ms of the
 * call, out[5] ms in the contraction kernels. */
#define RSREC_COND_LL_MAX 4096
int rsrec_kubo_integrand(rsrec_t *h, int nvec, int cond_ll, const double *mu_nm, int nen, const double *ene, double energy_min,
                         double energy_max, double *integrand);
/* The same integrand from the orbital-diagonal moments (only conductivity.f90:289, :292 read the moments, both on the diagonal):
 *   mu_diag : complex (18,cond_ll,cond_ll,nvec), host or device, as rsrec_kubo_moments_diag returns it; NULL = the moments that call
 *             left resident on the handle.  RSREC_ERR_ARG (with a message; the handle stays usable) if nothing is resident or nvec /
 *             cond_ll differ from the resident call.
 * Everything else as rsrec_kubo_integrand, and the same bits as that call gives on a full array with these diagonals. */
int rsrec_kubo_integrand_diag(rsrec_t *h, int nvec, int cond_ll, const double *mu_diag, int nen, const double *ene, double energy_min,
                              double energy_max, double *integrand);

/* The conductivity itself: the tail of calculate_conductivity_tensor (conductivity.f90:283-372) -- the sums of the integrand over the
 * vectors and the orbitals, and their Fermi-weighted Simpson integrals up to every energy of the mesh (kernels_cond.hpp):
 *   sigma(r, i, s) = simpson_f(x, EF = x(i), nv1, S(r, :, s), fermi = .true., dfermi = .false., temperature)      (math.f90:1600-1632)
 * on the scaled axis x = (ene - b) / a of rsrec_kubo_integrand.  Rows r of a set: 1 Re total, 2 Im total, 3-20 Re orbital 1..18, 21-38 Im
 * orbital 1..18.  Rows, sets and vectors are numbered from 1 here (Fortran).  Set 1 is the sum over the vectors (v ascending; the total is the sum over the orbitals, l ascending: the reference's
 * order); with per_vector != 0 set 1 + v is vector v alone ('per_type'): nsets = 1 + (per_vector ? nvec : 0).
 *   integrand : complex (18,nen,nvec) in, as rsrec_kubo_integrand delivers it
 *   sigma     : real (38,nen,nsets) out.  NOT divided by nvec: the caller applies / real(loop_over) where the reference does (:321)
 *   series    : real (38,nen,nsets) out or NULL: the integrated series S themselves (rows 1-2 of set 1 are fort.123's columns)
 *   integrand, sigma, series: host or device memory, each detected by itself.  ene: real (nen) host.
 *   nv1       : energy%nv1; the rule's loop runs I = 2, nv1 + 9, 2, so nen >= nv1 + 9 (energy%e_mesh makes nen = nv1 + 9)
 *   temperature: simpson_f's argument T, applied on the scaled axis as the reference's call would apply it (kBT = 0.633362019e-5 T + 1e-15
 *               in units of x); 0 is what the reference passes
 * Deviation from the reference: simpson_f reads Y(nv1 + 10) and Ene(nv1 + 10), one element past its arrays when nen = nv1 + 9.  Here every
 * term with an index above nen is zero, as in the exchange entry points.
 * Needs no lattice and no Hamiltonian.  Resident diagonal moments (rsrec_kubo_moments_diag) survive the call.  Two calls with the same
 * inputs give the same bits, and a set's values do not depend on the other vectors of the call.  Errors: RSREC_ERR_ARG with a message
 * (nvec < 1, nen < 3, nv1 < 1, nen < nv1 + 9, an empty or non-finite window, a negative or non-finite temperature, a NULL ene, integrand
 * or sigma); the handle stays usable.  rsrec_get_timing: out[0] device ms of the call, out[5] ms in its two kernels. */
int rsrec_kubo_conductivity(rsrec_t *h, int nvec, int per_vector, int nen, int nv1, const double *ene, double energy_min, double energy_max,
                            double temperature, const double *integrand, double *sigma, double *series);

/* The frequency-dependent (optical) conductivity from the same orbital-diagonal moments (kernels_optical.hpp).  The moments are the
 * Chebyshev double expansion of the current-matrix-element density j(x, y) = <r| delta(y - H~) v_a delta(x - H~) v_b |r>; on the scaled
 * axis x_i = (ene_i - b) / a of rsrec_kubo_integrand (i = 0 .. nen - 1), which must be uniform with step Delta = ene(2) - ene(1) > 0
 * (|ene_i - ene_0 - i Delta| <= 1e-9 Delta),
 *   D(i,n)       = 2 w_n T_{n-1}(x_i) / (pi sqrt(1 - x_i^2)),  n = 1 .. cond_ll;  w_n = g_n weights_n, the table of rsrec_kubo_integrand
 *                  (Lorentz kernel, lambda = 6, weights_1 = 0.5); T from the three-term recurrence; a row with |x_i| >= 1 is zero
 *   J_{l,s}(i,j) = sum_{n,m} D(i,n) mu_diag(l,n,m,s) D(j,m)
 *   opt(l,k,f,s) = (pi / a^2) (1/k) sum_{i=0}^{nen-1-k} [F_f(x_i) - F_f(x_{i+k})] J_{l,s}(i, i+k),      omega_k = k Delta, k = 1 .. nw
 *   F_f(x)       = 1 / (exp((x - x_F,f) / kT) + 1),  x_F,f = (fermi_f - b) / a,  kT = 0.633362019e-5 temperature + 1e-15 on the scaled axis
 *                  (the convention of rsrec_kubo_conductivity; no T = 0 special case)
 * Complex throughout: no real part is taken, and e^2 hbar / Omega and the sign convention of the velocity operators stay with the caller.
 * The rectangle rule on the mesh: h / (k h) = 1 / k.  J is never formed in memory: two real x complex GEMMs per (orbital, set) on the
 * FP64 matrix cores, the second fused with the frequency sum over the tiles i < j <= i + nw.
 *   mu_diag : complex (18,cond_ll,cond_ll,nset), host or device (detected); NULL = the moments rsrec_kubo_moments_diag / _multi / _tensor left
 *             resident (nset = all their sets), with the rules and the error of rsrec_kubo_integrand_diag.  1 <= cond_ll <= RSREC_COND_LL_MAX.
 *   ene     : real (nen) host, nen >= 2;   fermi : real (nfermi) host, 1 <= nfermi <= RSREC_OPT_NFERMI_MAX;   1 <= nw <= nen - 1
 *   opt     : complex (18,nw,nfermi,nset) out, host or device
 * Needs no lattice and no Hamiltonian.  Resident diagonal moments survive the call.  The bits of opt(:,:,f,s) depend only on that set,
 * that Fermi level and the mesh: not on the other sets or levels of the call, their order, or earlier calls (fixed summation order, no
 * atomics).  Errors: RSREC_ERR_ARG with a message, the handle staying usable, for a mesh that is not uniform or does not increase,
 * nen < 2, nw or nfermi out of range, an empty or non-finite window, a negative or non-finite temperature, a non-finite Fermi level, a NULL
 * ene, fermi or opt.  rsrec_get_timing: out[0] device ms of the call, out[5] ms in its kernels. */
#define RSREC_OPT_NFERMI_MAX 16
int rsrec_kubo_optical(rsrec_t *h, int nset, int cond_ll, const double *mu_diag, int nen, const double *ene, double energy_min, double energy_max,
                       int nw, int nfermi, const double *fermi, double temperature, double *opt);

/* Exchange couplings of the pairs of one rank: green%calculate_intersite_gf / _twoindex (green.f90:386-469) and the integrands and
 * Fermi-weighted Simpson integrals of exchange%calculate_exchange / _twoindex (exchange.f90:1032-1615), without the intersite arrays
 * (kernels_exchange.hpp: g0 of a pair's chains stays in LDS; every quantity is a trace Tr(D_i A D_j B) of the diagonal d_matrix).
 *   kind        : 0 block (green%block_green_ij, eta = 0), 1 Chebyshev (chebyshev_green_ij)
 *   same        : int32 (npairs), 1 where ijpair(p,1) == ijpair(p,2): chain 1 alone is used (slots 2..4 are not read)
 *   lld, nen, ene, nv1, fermi : control%lld, channels_ldos + 10, energy%ene (host), energy%nv1, energy%fermi; nen >= nv1 + 9
 *   sym_term    : control%sym_term (block);  energy_min / energy_max: the Chebyshev scaling (kind 1)
 *   a_inf, b_inf: real (18,18,4*npairs) terminators of the chains (block), or both NULL: computed on the device (get_terminf).  With
 *               resident chains of a seeded call that skipped the repeats of i == j pairs they must be NULL (RSREC_ERR_ARG otherwise)
 *   coef_a, coef_b: block: a_b and b2_b AFTER zsqr, complex (18,18,lld,4*npairs); Chebyshev: coef_a = mu_n (18,18,2*lld+2,4*npairs),
 *               coef_b NULL.  Both NULL: the chains the last rsrec_*_seeded / rsrec_block_lanczos / rsrec_chebyshev call left on the device
 *               (block: b2_b, square-rooted here); it must have run 4*npairs chains of depth lld.  Slot order ij_loc*4 - 4 + reci.
 *   dpar        : real (4,3,2,npairs): per l = 0..2 and side i / j, (c_up + vmad, c_dn + vmad, dele_up, dele_dn) of the atom's type
 *   pair_offset, npairs_total : this rank's pairs are columns pair_offset+1 .. pair_offset+npairs of the zero-padded images
 *   xc, so, fo  : real (13,npairs_total) out = T_comm_xc / T_comm_xcso / T_comm_xcfo;  parts: real (28,npairs_total) = T_comm_xcparts
 *   jcum        : real (nen,npairs) out or NULL: the second-order J of fort.150 with Ef = ene(nv) (second column, scaled)
 *   integrand   : real (41,nen,npairs) out or NULL: the energy-resolved integrands (row order in kernels_exchange.hpp)
 * d_matrix's parameters are rounded to single precision as its cmplx() calls do.  Scalings as the reference: *1.0d3/4/pi, 2.0d3/4/pi
 * for the DMI parts.  simpson_f's read one element past its arrays is taken as 0.
 * Every array may be host or device memory.  Pairs run in chunks: the device memory that scales with energies (integrands, staged
 * coefficients) is bounded independent of npairs; only dpar, same and the output images (~0.8 KB per pair) grow with it.  Two calls with
 * the same inputs give the same bits.  rsrec_get_timing: out[0] device ms of the call, out[5] ms in the Green + trace kernels. */
int rsrec_exchange(rsrec_t *h, int kind, int npairs, const int32_t *same, int lld, int nen, const double *ene, int nv1, double fermi,
                   int sym_term, double energy_min, double energy_max, const double *a_inf, const double *b_inf, const double *coef_a,
                   const double *coef_b, const double *dpar, int pair_offset, int npairs_total, double *xc, double *so, double *fo,
                   double *parts, double *jcum, double *integrand);

/* Gilbert damping (torque correlation) of the pairs of one rank: the traces of exchange%calculate_gilbert_damping (exchange.f90:674-694)
 * on the chains rsrec_exchange reads, without gij / gji (kernels_exchange.hpp: a second epilogue on g0 of a pair's chains in LDS).  Per
 * pair and energy, with Aij = gij - gji^H and Aji = gji - gij^H:
 *   row m = 3 (k-1) + l, k, l = 1..3:  Tr( tmati(:,:,k) Aij  tmatj(:,:,l)^H Aji ),  rows 1..9 its real parts (dtott), 10..18 its imaginary
 *   parts (dtottim).  The prefactor -0.25 * 2 / (pi spin_i) is NOT applied: it is the caller's.
 *   kind, same, lld, nen, ene, sym_term, energy_min, energy_max, a_inf, b_inf, coef_a, coef_b, pair_offset, npairs_total: as rsrec_exchange
 *               (coef_a and coef_b NULL: the resident chains of the last seeded call; the same compaction and terminator rules)
 *   ief         : 1-based index into ene of the energy whose rows go to at_ef (the reference's point nearest the Fermi level)
 *   tmat        : complex (18,18,3,2,npairs): hamiltonian%tmat(:,:,:,iz) of atom i (side 1) and atom j (side 2) of every pair
 *   at_ef       : real (18,npairs_total) out: the 18 rows at ene(ief), this rank's pairs in their columns of the zero-padded image
 *   total       : real (9,nen) out: total_damping = the sum of dtott over THIS call's pairs, added in ascending pair order (:690-694)
 *   rows        : real (18,nen,npairs) out or NULL: every row at every energy
 * Every array may be host or device memory.  Pairs run in chunks: the device memory that scales with energies is bounded independent of
 * npairs; tmat is staged per chunk.  Every sum runs in a fixed order without atomics: two calls give the same bits, a pair's rows do not
 * depend on the other pairs of the call, and total does not depend on the chunking.  Errors as rsrec_exchange.  rsrec_get_timing: out[0]
 * device ms of the call, out[5] ms in the Green + trace + reduction kernels. */
int rsrec_damping(rsrec_t *h, int kind, int npairs, const int32_t *same, int lld, int nen, const double *ene, int ief, int sym_term,
                  double energy_min, double energy_max, const double *a_inf, const double *b_inf, const double *coef_a, const double *coef_b,
                  const double *tmat, int pair_offset, int npairs_total, double *at_ef, double *total, double *rows);

/* Exchange tensor in the auxiliary Green-function formalism for the pairs of one rank: exchange%calculate_jij_auxgreen
 * (exchange.f90:171-335) on the chains rsrec_exchange reads (kernels_auxgreen.hpp: a third epilogue on g0 of a pair's chains in LDS; gij and
 * gji are dressed with sqrt(Delta) and P_up - P_dn while their up-up and down-down blocks leave g0).  lmax = 2 only.
 *   kind, same, lld, nen, ene, nv1, fermi, sym_term, energy_min, energy_max, a_inf, b_inf, coef_a, coef_b, pair_offset, npairs_total: as
 *               rsrec_exchange (coef_a and coef_b NULL: the resident chains of the last seeded call; the same compaction and terminator rules)
 *   apar        : real (2,3,2,2,npairs): (c + vmad, dele) per l = 0..2, spin (up, down) and side (atom i, atom j).  The library rounds them
 *               and the energy to single precision where the reference's cmplx() without a KIND does (p_matrix, auxiliary_gij)
 *   jaux        : real (9,npairs_total) out: simpson_f of the rows, UNSCALED (the reference prints them * 1.0d3 / 4 / pi); an i == j pair
 *               carries J00 in row 1 and zeros in rows 2..9; this rank's pairs in their columns of the zero-padded image
 *   rows        : real (9,nen,npairs) out or NULL: jtot_aux(nv, 1:9) = xx, xy, xz, yx, .. zz (imtrace * 0.5), or jtot_00 (imtrace * -1) in row 1
 * Memory, repeatability, errors and timing as rsrec_damping; apar is staged per chunk. */
int rsrec_exchange_aux(rsrec_t *h, int kind, int npairs, const int32_t *same, int lld, int nen, const double *ene, int nv1, double fermi,
                       int sym_term, double energy_min, double energy_max, const double *a_inf, const double *b_inf, const double *coef_a,
                       const double *coef_b, const double *apar, int pair_offset, int npairs_total, double *jaux, double *rows);

/* Spin-lattice coupling Jijk of the atom trios of one rank: exchange%calculate_jijk (exchange.f90:338-601).  Trio t is the pairs 3t+1..3t+3
 * = (i,j), (i,k), (j,k) of the call (lattice.f90:644-651), 4 chains each; one workgroup per (trio, energy) runs their Green stages one after
 * another, keeps the canonical auxiliary blocks it needs (gij, gji, gki, gjk, gkj; gik is never read) in LDS and forms the 8 triple
 * products there.  lmax = 2 only.
 *   npairs      : 3 * ntrios.  kind .. coef_b as rsrec_exchange_aux; `same` per pair (a trio may repeat an atom)
 *   apar        : real (3,3,2,3,ntrios): (c + vmad, dele, qpar) per l, spin and atom (i, j, k), rounded as in rsrec_exchange_aux
 *   dmat        : complex (9,9,ntrios): one spin block of disp_matrix of atom k for the trio's unit displacement (symbolic_atom.f90:274-355)
 *   trio_offset, ntrios_total: this rank's columns of the zero-padded image
 *   jijk        : real (9,ntrios_total) out: simpson_f of the rows, UNSCALED (the reference prints them * (1.0d3 / 8 / pi) *
 *               (13.605693122994 / 1.8897261246))
 *   rows        : real (9,nen,ntrios) out or NULL: jijk_tot(nv, 1:9)
 * Every array may be host or device memory.  The call runs in chunks of whole trios: device memory is bounded independent of ntrios.
 * Fixed summation order, no atomics: two calls give the same bits and a trio's numbers do not depend on the other trios or on the
 * chunking.  Errors and timing as rsrec_damping; npairs that is no multiple of 3 is RSREC_ERR_ARG. */
int rsrec_spin_lattice(rsrec_t *h, int kind, int npairs, const int32_t *same, int lld, int nen, const double *ene, int nv1, double fermi,
                       int sym_term, double energy_min, double energy_max, const double *a_inf, const double *b_inf, const double *coef_a,
                       const double *coef_b, const double *apar, const double *dmat, int trio_offset, int ntrios_total, double *jijk,
                       double *rows);

/* Exchange couplings on the Gauss-Legendre contour at the Fermi level for the pairs of one rank: green%calculate_intersite_gf_eta
 * (green.f90:471-536) and exchange%calculate_exchange_gauss_legendre (exchange.f90:1804-1865) in one call, without the *_eta arrays
 * (kernels_contour.hpp: g of a pair's chains at a point stays in LDS).  Point k is the complex energy e0 + i (1 - x_k) / x_k and carries
 * the factor w_k / (x_k x_k), applied as the reference applies it: (value * w) / (x * x).  (1 - x_k) / x_k is rounded to single precision, as
 * the reference's eta = cmplx(0.0_rp, res) without a KIND does (green.f90:508, bands.f90:563).
 *   kind, same, lld, sym_term, energy_min, energy_max, a_inf, b_inf, coef_a, coef_b, pair_offset, npairs_total: as rsrec_exchange (kind 0:
 *               block_green_ij_eta, 1: chebyshev_green_ij_eta, all 324 elements; coef_a and coef_b NULL: the resident chains of the last
 *               seeded call, the same compaction and terminator rules).  Device terminators are computed once per chain, not once per point
 *   npts, x, w  : the contour: Gauss-Legendre nodes and weights on (0, 1), real (npts) HOST arrays; any npts >= 1 (the reference: 64)
 *   e0          : ene(fermi_point), the real part of every point
 *   dmat        : real (9,9,2,npairs): real(ee(1:9,1:9,1,iz) - ee(10:18,10:18,1,iz)) of atom i (side 1) and atom j (side 2), DENSE
 *   xc          : real (13,npairs_total) out = T_comm_xc: jij = -sum, dmi(1:3) = +sum, aij(3,3) = -sum over the points in ascending
 *               order, each * 1.0d3 / 4 / pi
 *   rows        : real (13,npts,npairs) out or NULL: the weighted per-point values jtot, jjtot(1:3), itot(3,3) before sign and scaling
 * Deviation from the reference, i == j pairs (same = 1): recur_b_ij runs one chain for such a pair and never writes slots 2..4
 * (recursion.f90:1702-1707), and the reference's contour routine combines chain 1 with those unwritten slots.  Here gij = gji = g(chain 1),
 * as calculate_intersite_gf takes it (green.f90:446-448).
 * coef_a, coef_b, a_inf, b_inf, dmat, xc, rows may be host or device memory.  Pairs run in chunks: the device memory that scales with
 * points is bounded independent of npairs.  Fixed summation order, no atomics: two calls give the same bits and a pair's numbers do not
 * depend on the other pairs of the call.  Errors: RSREC_ERR_ARG with a message; the handle stays usable.  rsrec_get_timing: out[0] device
 * ms of the call, out[5] ms in the Green + trace + point-sum kernels. */
int rsrec_exchange_contour(rsrec_t *h, int kind, int npairs, const int32_t *same, int lld, int npts, const double *x, const double *w, double e0,
                           int sym_term, double energy_min, double energy_max, const double *a_inf, const double *b_inf, const double *coef_a,
                           const double *coef_b, const double *dmat, int pair_offset, int npairs_total, double *xc, double *rows);

/* Orbital occupations on the same contour for the on-site chains of one rank: bands%calculate_moments_gauss_legendre (bands.f90:559-586)
 * and calculate_occupation_gauss_legendre (:631-650):  occ(i) = sum_k Re g_ii(z_k) w_k / x_k^2 / pi + 0.5, k ascending.
 *   kind        : 0 block_green_eta (green.f90:544-581: bgreen with the point's eta, honouring sym_term), 1 chebyshev_green_eta
 *               (:1116-1184).  For kind 1 only the diagonal of g is defined: the reference refreshes only mu_ng(i,i,..) there
 *   nsites, lld : chains (one per site) and their depth
 *   npts, x, w, e0, sym_term, energy_min, energy_max: as rsrec_exchange_contour
 *   a_inf, b_inf: real (18,18,nsites) or both NULL: the device terminator, once per chain
 *   coef_a, coef_b: block: a_b and b2_b AFTER zsqr (18,18,lld,nsites); Chebyshev: mu_n (18,18,2*lld+2,nsites) and NULL.  Both NULL: the
 *               chains rsrec_block_lanczos / rsrec_chebyshev left on the device (b2_b square-rooted in a private copy)
 *   site_offset, nsites_total: this rank's sites are columns site_offset+1 .. of the zero-padded image
 *   occ         : real (18,nsites_total) out;  gdiag: complex (18,npts,nsites) out or NULL: g_ii at every point
 * Memory, repeatability, errors and timing as rsrec_exchange_contour. */
int rsrec_contour_occupation(rsrec_t *h, int kind, int nsites, int lld, int npts, const double *x, const double *w, double e0, int sym_term,
                             double energy_min, double energy_max, const double *a_inf, const double *b_inf, const double *coef_a,
                             const double *coef_b, int site_offset, int nsites_total, double *occ, double *gdiag);

/* One whole-vector product on caller arrays psi(18,18,kk) (complex, the reference's layout):
 *   vel = 0 : psi_out = (H psi_in - b psi_in)/a      ham_vec_matmul (:913) / ham_hoh_vec_matmul (:785); v_op, vo_op ignored
 *   vel = 1 : psi_out = V psi_in                      velo_vec_matmul (:587, 'n') / velo_hoh_vec_matmul (:656) with v_op (and vo_op with hoh)
 * (The type-bound procedures of those names can be overridden with this; chebyshev_orbital_mod :2834 then runs its products on the GPU.) */
int rsrec_apply_operator(rsrec_t *h, int vel, const double *v_op, const double *vo_op, const double *psi_in, double *psi_out, double a, double b);

/* Scalar Haydock recursion, one chain per (site, orbital).  Replaces recur (recursion.f90:3485-3532),
 * crecal (:3423-3478), hop (:3310-3416).
 *   a, b2 : real (llmax,18,nsites) out (the (:,:,:,1) plane of the reference's a/b2); rows > lld are zeroed. */
int rsrec_scalar_lanczos(rsrec_t *h, int nsites, const int32_t *seed_atoms, int lld, int llmax, double *a, double *b2);

/* Site partition of get_mpi_variables (mpi.f90:32-58): 1-based inclusive range owned by `rank`. */
void rsrec_site_partition(int rank, int nprocs, int nsites, int *start_atom, int *end_atom);

/* Last error text of this handle (NUL-terminated, truncated to n). */
int rsrec_last_error(rsrec_t *h, char *buf, size_t n);

/* chebyshev_orbital_mod (recursion.f90:2834-3049; called at calculation.f90:1256), the moment part (:2893-3013), with the seeds advanced
 * together as chains and every vector resident on the device.  For seed atom s:  psiref = 1 on s;
 * left = i (Y H~ X - X H~ Y) psiref  with X, Y = alat cr(1,:), alat cr(2,:) and H~ = ham_vec_matmul (the plain operator also when hoh is
 * set);  v_1 = psiref, v_2 = H~' v_1, v_n = 2 H~' v_{n-1} - v_{n-2}  (H~' = ham_hoh_vec_matmul with hoh);  mu(:,:,n) = sum_k left_k^H v_n,k.
 *   cr      : lattice%cr(3,kk), units of alat;   a, b : scale and shift of H~ = (H - b)/a  (:2869-2870)
 *   mu_orb  : complex (18,18,lld): the SUM over the seeds of the call in seed order (the reference loops over all kk atoms and divides
 *             by kk afterwards, :3006; its own accumulator is never zeroed, :2907 -- here the sum starts from zero)
 *   mu_seed : optional complex (18,18,lld,nseeds): the contribution of every seed */
int rsrec_orbital_moments(rsrec_t *h, int nseeds, const int32_t *seed_atoms, int lld, double a, double b, const double *cr, double alat,
                          double *mu_orb, double *mu_seed);

/* The Chebyshev counterpart of rsrec_pack_diag: the moments mu_n(18,18,2 lld + 2,site) of the last rsrec_chebyshev call, as they lie on
 * the device, inside a zero image over all sites (shape (18,18,2 lld + 2,nsites_total) complex; device or host memory) -- the buffer a
 * sum all-reduce turns into the all-gather of recursion.f90:1790-1793 (commented-out MPI_Allgather of the coefficients). */
int rsrec_pack_moments(rsrec_t *h, int site_offset, int nsites_total, double *mu_img);

/* Library-level communicator: the one exchange of the path -- MPI_ALLREDUCE(MPI_IN_PLACE, ..., MPI_SUM) on zero-padded per-site arrays
 * (bands.f90:271-274; sites are dealt to the ranks by mpi.f90:32-58 = rsrec_site_partition) -- as ONE RCCL all-reduce over xGMI,
 * without MPI or torch on the host.  RCCL is bound with dlopen on first use.  One rank per GPU; the handle's device is the rank's GPU.
 *   rsrec_comm_unique_id : one rank creates the id (RSREC_COMM_ID_BYTES bytes) and hands it to the others (MPI_Bcast, a file, ...)
 *   rsrec_comm_init      : collective; same id on every rank
 *   rsrec_comm_init_file : the same with the id exchanged through `path` (rank 0 writes it, the others wait up to timeout_s seconds)
 *   rsrec_allreduce_sum  : in-place sum of n doubles over the ranks; buf = device memory (the images of rsrec_pack_diag /
 *                          rsrec_pack_moments / rsrec_block_ldos, reduced where they lie) or host memory (staged).  Identity without a
 *                          communicator, like the reference built without MPI.
 *   rsrec_comm_size      : rank and number of ranks of the handle's communicator (0, 1 without one) */
#define RSREC_COMM_ID_BYTES 128
int rsrec_comm_unique_id(char *id);
int rsrec_comm_init(rsrec_t *h, int rank, int nranks, const char *id);
int rsrec_comm_init_file(rsrec_t *h, int rank, int nranks, const char *path, double timeout_s);
int rsrec_allreduce_sum(rsrec_t *h, double *buf, size_t n);
int rsrec_comm_size(rsrec_t *h, int *rank, int *nranks);
int rsrec_comm_destroy(rsrec_t *h);

/* ---- tuning / measurement (not part of the reference interface) ---- */
/* key/value knobs (defaults in brackets; everything but "batch" and "kernels" exists for A/B measurements and tests):
 *   "batch"      chains advanced together per launch [0 = auto: up to 64, bounded by free device memory]
 *   "kernels"    0 = auto, 1 = FP64 VALU kernel set (the reference's layout and operation order; any stencil), 2 = matrix-core set [0]
 *   "spmm5"      SpMM of the matrix-core set: 0 = small-launch kernel k_spmm4<4> (LayoutRM vectors) whenever it applies, 1 = by launch size
 *                (k_spmm5 on CI vectors from 4096 groups per launch; always for hoh and local-axis runs), 2 = always k_spmm5 [2]
 *   "side_stream" reduction + eigen-solve of B_{n+1} on a second HIP stream, concurrent with the next H|u>; the chain-octet launch beside
 *                the main H|psi> launch [1]
 *   "graph"      the level loop of a block-Lanczos call as one HIP graph, replayed while lattice, seeds, depth, buffers and options stay
 *                the same: 0 = never, 1 = calls of up to 8 chains, 2 = every single-batch call [1]
 *   "nblk"       workgroups per chain / 2 of the reduction-bearing kernels [0 = by batch size]
 *   "orth3"      k_mfma_orth3: 1 = one 512-register wave per SIMD (tables in registers), 2 = two waves per SIMD (tables in LDS) [1]
 *   "cheb_fused" Chebyshev step inside the SpMM epilogue (H psi never written): 0 / 1 [1]
 *   "chain_fold" chains per k_spmm5 workgroup [1],  "s5_cap" cap on k_spmm5 workgroups per chain [0 = none],
 *   "s5_lds"     k_spmm5 with the operator fragments in LDS: 0 = never, 1 = operators with one class of atoms, whenever their stream fits,
 *                2 = also operators with several classes (one run of groups per class of the class-sorted atom list; slower) [1]
 *   "s5_queue"   the LDS form as persistent workgroups (one per CU) with per-(chain, XCD) group counters: 0 = never, 1 = launches of >= 256
 *                workgroups, 2 = always [1];  "s5_waves" waves per persistent workgroup, 8 or 4 [8];  "s5_split" 3 = a wave of the persistent form takes a
 *                third of a group's nine tiles (bitwise the same results, measured slower: DESIGN.md; s5_waves 8 / 12 then) [0];  "s5_run_min" smallest class run
 *                (groups) that gets LDS workgroups of its own under s5_lds = 2 [0 = by launch size]
 *   "s5_spin_xcd" persistent form on collinear operators: 1 = even XCDs serve output spin 0 and odd XCDs spin 1 (an XCD's L2 then holds one
 *                spin half of the neighbour blocks; the round-2 default), 0 = both spins on every XCD (2-4 % faster, round 3) [0]
 *   "s5_octet"   atoms with their own operator blocks (nmax) from which their groups are formed over 8 CHAINS of the batch (they then share
 *                the atom's operator fragments the way 8 atoms of a type do) once every chain's region covers the lattice; 0 = never [8]
 *   "s5_gram_min" the A_n Gram sum u^H (H u) formed in k_spmm5's epilogue instead of by a pass of its own over u and H u: a chain folds at a level
 *                when its region there has at least this many groups of 8 atoms; 0 = always.  Only block Lanczos on the matrix-core set with k_spmm5,
 *                on an operator with one class of atoms, without hoh, that rsrec_set_hamiltonian found Hermitian (opposite slots from nn, blocks
 *                compared to 1e-12 of the largest element); everything else keeps the separate pass [256: from there on the folded level measured faster, DESIGN.md]
 *   "s5_host_emit" 1 = swizzle k_spmm5's operator streams on the host instead of assembling them on the device (cross-check) [0]
 *   "orth_oop"   1 = the orthogonalisation pass writes u_{n+1} into a third u vector instead of over u_{n-1} (faster on the HBM, one more work vector) [1]
 *   "sat_pct"    a chain whose region holds at least this share (per cent) of the lattice runs on the list of ALL atoms instead of its own [100]
 *   "kubo_lchunk" rsrec_kubo_moments / _diag: left vectors held on the device at a time [0 = as many as fit];  "kubo_vbatch" vectors of a call advanced
 *                together as the chains of every launch [0 = up to 8, as many as fit beside a whole left matrix each]
 *   "lattice_vbatch" rsrec_chebyshev_lattice: chains of a call advanced together as the chains of every launch [0 = up to 8, as many as fit]
 *   "kubo_setgroup" rsrec_kubo_moments_diag_tensor: sets of a vector contracted against one staged tile of left vectors; 1 = every set by itself,
 *                2 / 3 = groups of at most that width [0 = 2]
 *   "shot_orders" rsrec_kubo_single_shot: orders P added to the accumulators per pass, 1..16 (larger values: 16); the ring holds P + 2 orders per
 *                chain and a pass moves (P + 2 ne) / P block streams per order and chain; the same bits for every value [0 = 16: the fastest of
 *                1, 2, 4, 8, 16 at ne = 2 and 16 on 8 000 and 97 336 atoms, 0.87-0.99 of the call's time at 8 and 0.33-0.83 of it at 1, DESIGN.md section 5]
 *   "sitemap_orders" rsrec_chebyshev_site_map: orders PT added to the accumulators per pass, 1, 2, 4, 8 or 16 (other values: the power of two below);
 *                the ring holds PT + 2 orders per vector [0 = 2]
 *   "sitemap_vtile" rsrec_chebyshev_site_map: vectors VT folded into z per pass, 1, 2, 4 or 8; a tile-pass moves (VT PT + 2 ne) 16 B per element.  VT PT <= 16:
 *                the value the caller did not set follows the other to VT PT = 16 (VT <= 8), of two set values VT gives way.  The bits depend on VT [0 = 8.  <8,2> is the fastest call of
 *                <1,16>, <2,8>, <4,4>, <8,2>, or within 0.02 % of it, in 7 of 9 measured configurations on 10 648 and 97 336 atoms, all four within 1.2 % of each other, and
 *                keeps the shallowest ring, DESIGN.md section 5]
 *   "evolve_orders" rsrec_chebyshev_evolve: 1 = the two sums ride in the per-order pass that adds the source term (fused); 2..16 = that pass adds the
 *                source alone and a ring collects that many orders per accumulation pass (batched; larger values: 16); the same bits for every value
 *                [0 = 16: the fastest step of 1, 4, 16 with 1 and 4 vectors on 10 648 and 97 336 atoms, 4.4-9.6 % below the fused one, DESIGN.md section 5] */
int rsrec_set_option(rsrec_t *h, const char *key, long value);
/* Timing of the last recursion call, measured with HIP events on the engine's own stream:
 *   out[0] total device ms, out[1] ms in the H|psi> kernels, out[2] number of H|psi> launches,
 *   out[3] atom-steps processed (sum over chains and steps of active atoms), out[4] block multiplies in H|psi>,
 *   out[5] ms in the remaining recursion kernels, out[6] host ms (region bookkeeping + transfers),
 *   out[7] 1 if the timed H|psi> kernel also forms the A_n partial (VALU set; k_spmm5 when every launch of the call folded the Gram), else 0,
 *   out[8] matrix flops EXECUTED by the timed k_spmm5 launches (padding of the MFMA tiles included, structural zeros of spin-diagonal
 *          blocks not: they are skipped), per operator class of the groups; 0 for the other kernels.
 *   out[9] flops of the H|psi> applications that the operator's BLOCK STRUCTURE requires: out[4] counts the reference's zgemm on full
 *          18x18 blocks (46 656 flop each, recursion.f90:1618); a spin-diagonal block (every hopping block of a collinear magnet,
 *          hamiltonian.f90:1553-1617) needs 23 328, a spin-mixing block 46 656 -- the unit roofline fractions are quoted in.
 *   out[10] block arrays (0..4: ee, eeo, hall, hallo) the last rsrec_set_hamiltonian took from rsrec_assemble_blocks' device copies.
 *   out[11] H|psi> launches of the last call in which the atoms with their own operator blocks were grouped over 8 chains (option "s5_octet").
 *   out[12] rsrec_block_lanczos_local_axis: ms in the conjugation of the resident coefficients with the sites' rotations (part of out[5]).
 *   out[13] H|psi> launches of the last call whose epilogue formed the A_n Gram of at least one chain (option "s5_gram_min").
 *   out[14..16] rsrec_chebyshev_bloch_map: ms in the accumulation passes, the phase tables and the final sums (together: out[5]).
 *   out[17..18] rsrec_kubo_single_shot: ms in the accumulation passes and in the final stage (together: out[5]).
 *   out[19..20] rsrec_kubo_moments and its _diag / _multi / _tensor forms: left chunks formed, summed over the vector batches of the call (one
 *           per batch when every left matrix fits), and the left vectors per chunk as planned (cond_ll then; option kubo_lchunk caps it).
 *   out[21..22] rsrec_chebyshev_site_map: ms in the accumulation passes and in the output stage (together: out[5]).
 *   out[23..24] rsrec_chebyshev_evolve: ms in the step passes (source add and accumulation) and in the record stage (seed projection, moment
 *           chains and their Grams); together: out[5].
 * After rsrec_block_green: out[0] = kernel + transfers, out[1] = the Green kernel alone. */
int rsrec_get_timing(rsrec_t *h, double *out, int n);

#ifdef __cplusplus
}
#endif
#endif /* RSREC_H */
