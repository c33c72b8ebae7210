// Kernels of the optical conductivity sigma(omega) from the orbital-diagonal Kubo moments (rsrec_kubo_optical).  With x_i = (ene_i - b)/a
// on a uniform mesh, D(i,n) = 2 w_n T_n(x_i) / (pi sqrt(1 - x_i^2)) (n = 0-based order, w_n the table of k_cond_basis; a row with
// |x_i| >= 1 is zero) and M = mu(l, :, :, s):
//   J(i,j)       = sum_{n,m} D(i,n) M(n,m) D(j,m)                                      the current-matrix-element density j(x_i, x_j)
//   opt(l,k,f,s) = pi / (a^2 k) sum_{i=0}^{nen-1-k} [F_f(x_i) - F_f(x_{i+k})] J(i, i+k),     k = 1..nw
// Two real x complex GEMMs per (orbital, set), J never in memory:
//   stage 1 (k_opt_project)  Pt(m,i) = sum_n M(n,m) D(i,n)          L x nen x L,  written transposed (energy fastest) for stage 2
//   stage 2 (k_opt_fused)    tiles of J(i,j) = sum_m Pt(m,i) D(j,m) with i < j <= i + nw only; in the epilogue the tile is turned so that
//                            a lane holds one diagonal k = j - i, multiplied by the weights of every Fermi level and summed along the
//                            diagonal -> per-tile partials;  k_opt_reduce adds a diagonal's tiles in ascending tile order.
// Every sum has a fixed order and nothing is atomic.  A Fermi level is weighted and summed by itself, and a term of weight exactly zero
// adds +-0 to a sum that starts at +0 -- the bits of a level depend neither on the other levels nor on which tiles were skipped.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_mfma.hpp"
#include "kernels_simpson.hpp"

namespace rsrec {

constexpr int KO_TI = 64;                     // stage 2: energies i (rows) of a wave's tile; the tables' energy dimension is padded to a multiple
constexpr int KO_TJ = 32;                     // stage 2: energies j (columns) of a wave's tile
constexpr int KO_TM = 32;                     // stage 1: moment orders m (rows) of a wave's tile; the order dimension is padded to a multiple
constexpr int KO_NDIAG = 96;                  // diagonal slots of a tile: slot q is k = j0 - i0 - 64 + q (slot 0 stays empty)
constexpr int KO_FB = 32;                     // energies per entry of the Fermi range table (k_opt_fermi_range)

// Basis and Fermi tables, one thread per energy:
//   td[n][i] = 2 w_n T_n(x_i) / (pi sqrt(1 - x_i^2))   n < lp   (zero for n >= L, i >= nen or |x_i| >= 1)
//   ft[f][i] = 1 / (exp((x_i - xf_f) / kbt) + 1)        f < nf   (zero for i >= nen)
__global__ __launch_bounds__(256) void k_opt_basis(int nen, int ep, int L, int lp, int nf, const double* __restrict__ ene, const double* __restrict__ w,
                                                   const double* __restrict__ fermi, double a, double b, double T, double* __restrict__ td,
                                                   double* __restrict__ ft) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ep) return;
    const bool live = i < nen;
    const double x = live ? (ene[i] - b) / a : 0.0;
    const double kbt = simpson_kbt(T);
    for (int f = 0; f < nf; ++f) ft[(size_t)f * ep + i] = live ? fermifun(x, (fermi[f] - b) / a, kbt) : 0.0;
    const bool inside = live && fabs(x) < 1.0;
    const double pre = inside ? 2.0 / (3.14159265358979323846 * sqrt(1.0 - x * x)) : 0.0;
    double t0 = 1.0, t1 = x;                  // T_n, T_{n+1}
    for (int n = 0; n < lp; ++n) {
        td[(size_t)n * ep + i] = inside && n < L ? pre * w[n] * t0 : 0.0;
        const double t2 = 2.0 * x * t1 - t0;
        t0 = t1; t1 = t2;
    }
}

// (min, max) of every Fermi level's weights over blocks of KO_FB mesh points: fr[f][i / KO_FB].  A tile whose row and column blocks all
// hold one single value has no non-zero weight F(x_i) - F(x_j) and is skipped (k_opt_tiles).
__global__ __launch_bounds__(256) void k_opt_fermi_range(int nen, int ep, int nf, const double* __restrict__ ft, double2* __restrict__ fr) {
    const int nb = ep / KO_FB, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nb * nf) return;
    const int f = e / nb, i0 = (e % nb) * KO_FB;
    double lo = 0.0, hi = 0.0;
    for (int i = i0; i < min(i0 + KO_FB, nen); ++i) {
        const double v = ft[(size_t)f * ep + i];
        lo = i == i0 ? v : fmin(lo, v);
        hi = i == i0 ? v : fmax(hi, v);
    }
    fr[e] = make_double2(lo, hi);
}

// live[it ntj + jt]: does the tile i0 .. i0 + 63 (rows) x j0 .. j0 + 31 (columns) hold a pair 1 <= j - i <= nw, j < nen, with a non-zero
// weight of some level?  Dead tiles are neither computed (k_opt_fused) nor read (k_opt_reduce).
__global__ __launch_bounds__(256) void k_opt_tiles(int nen, int ep, int nw, int nf, int nti, int ntj, const double2* __restrict__ fr, int* __restrict__ live) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nti * ntj) return;
    const int i0 = (e / ntj) * KO_TI, j0 = (e % ntj) * KO_TJ;
    int on = 0;
    if (j0 < nen && i0 < nen && min(j0 + KO_TJ, nen) - 1 > i0                  // (a pair above the diagonal)
        && j0 - min(i0 + KO_TI - 1, nen - 1) <= nw) {                         // (a pair within the last frequency)
        const int nb = ep / KO_FB, bi = i0 / KO_FB, bj = j0 / KO_FB;
        const bool two = i0 + KO_FB < nen;                                    // (the rows' second block holds mesh points)
        for (int f = 0; f < nf && !on; ++f) {
            const double2 r0 = fr[f * nb + bi], r1 = two ? fr[f * nb + bi + 1] : r0, c = fr[f * nb + bj];
            const double v = r0.x;
            on = !(r0.y == v && r1.x == v && r1.y == v && c.x == v && c.y == v);
        }
    }
    live[e] = on;
}

// The moments of the orbitals l0 .. l0 + nl - 1 of one set as the A-side planes of stage 1, from the compact diagonals mu(l, n, m) =
// mu[l + 18 (n + L m)]:  g[l - l0][n][m] = mu(l, n, m), n, m < lp, zero outside L x L.
__global__ __launch_bounds__(256) void k_opt_gather(const double2* __restrict__ mu, int l0, int nl, int L, int lp, double2* __restrict__ g) {
    const size_t per_l = (size_t)lp * lp, total = per_l * nl;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(e / per_l);
        const int n = (int)((e - (size_t)l * per_l) / lp), m = (int)(e % lp);
        g[e] = n < L && m < L ? mu[(size_t)(l0 + l) + (size_t)NB * ((size_t)n + (size_t)L * m)] : make_double2(0.0, 0.0);
    }
}

// Stage 1 on the FP64 matrix cores.  One wave = 32 orders m (rows) x 64 energies i (columns) of one orbital, re and im, over all of K = n.
// Per k-step lane (l15, l4) loads the 16-byte g[l][n0 + l4][m0 + 16 a + l15] of the two row tiles (A operand, re and im) and
// td[n0 + l4][i0 + 16 q + l15] of the four column tiles (B operand), one k-step ahead; 16 v_mfma_f64_16x16x4 per k-step.
// Accumulator row l4 + 4 rr, column l15 -> pt[l][m][i] (complex, energy fastest: 256 contiguous bytes per 16 lanes).
// Grid: x = energy blocks of 4 waves (256 energies), y = row tiles, z = orbitals of the chunk.  All tables are zero-padded: no clamping.
__global__ __launch_bounds__(256, 2) void k_opt_project(int ep, int lp, int lk, const double* __restrict__ td, const double2* __restrict__ g,
                                                        double2* __restrict__ pt) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int i0 = (blockIdx.x * 4 + wave) * 64;
    if (i0 >= ep) return;
    const int m0 = blockIdx.y * KO_TM, l = blockIdx.z;
    typedef double ko_d2 __attribute__((ext_vector_type(2)));
    const ko_d2* pa = reinterpret_cast<const ko_d2*>(g) + (size_t)l * lp * lp + (size_t)l4 * lp + m0 + l15;
    const double* pb = td + (size_t)l4 * ep + i0 + l15;
    const size_t sa = (size_t)4 * lp, sb = (size_t)4 * ep;
    double4_t acc[2][4][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[t][q][0] = acc[t][q][1] = (double4_t){0, 0, 0, 0};
    ko_d2 a0[2], a1[2];
    double b0[4], b1[4];
    auto fetch = [&](ko_d2 (&a)[2], double (&bb)[4]) {
        a[0] = pa[0]; a[1] = pa[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) bb[q] = pb[16 * q];
        pa += sa; pb += sb;
    };
    auto mac = [&](const ko_d2 (&a)[2], const double (&bb)[4]) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[t][q][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][0], bb[q], acc[t][q][0], 0, 0, 0);
                acc[t][q][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][1], bb[q], acc[t][q][1], 0, 0, 0);
            }
    };
    const int ks = lk >> 2;
    int s = 0;
    fetch(a0, b0);
#pragma unroll 1
    for (; s + 2 <= ks; s += 2) {
        fetch(a1, b1);
        mac(a0, b0);
        if (s + 2 < ks) fetch(a0, b0);
        mac(a1, b1);
    }
    if (s < ks) mac(a0, b0);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            double2* row = pt + ((size_t)l * lp + m0 + 16 * t + l4 + 4 * rr) * ep + i0 + l15;
#pragma unroll
            for (int q = 0; q < 4; ++q) row[16 * q] = make_double2(acc[t][q][0][rr], acc[t][q][1][rr]);
        }
}

// Stage 2, fused with the frequency sum.  One wave = 64 energies i (rows) x 32 energies j (columns) of one orbital, re and im, over all of
// K = m: per k-step lane (l15, l4) loads the 16-byte pt[l][m0 + l4][i0 + 16 q + l15] of the four row tiles (A operand) and
// td[m0 + l4][j0 + 16 c + l15] of the two column tiles (B operand), one k-step ahead; 16 v_mfma_f64_16x16x4 per k-step.
// Epilogue.  A 16 x 16 sub-tile (q, c) leaves J(ib + r, jb + l15), r = l4 + 4 rr, in register rr of lane (l15, l4).  One shuffle inside
// the lane's row of 16 turns it: lane (d, l4) then holds J(ib + r, jb + ((d + r) & 15)), an element of the diagonal
//   k = jb - ib + d        (d + r < 16)      or      k = jb - ib + d - 16      (d + r >= 16, "wrapped").
// With jb - ib = j0 - i0 + 16 (c - q) the tile's diagonals fall into six slabs of 16, slab u = c - q + 4 - wrapped, slot 16 u + d.  Per
// Fermi level the lane adds weight x J over (q, c, rr) in that order onto its six slab sums, the four rows l4 are added by a fixed xor
// butterfly, and row 0 writes part[tile][f][slot] (complex).  Weights of pairs outside 1 <= k <= nw, j < nen are zero.
// Grid: x = column blocks of 4 waves (128 energies j), y = row tiles, z = orbitals of the chunk; a wave whose tile is not live leaves at once.
__global__ __launch_bounds__(256, 2) void k_opt_fused(int nen, int ep, int lp, int lk, int nw, int nf, int nti, int ntj, const double* __restrict__ td,
                                                      const double2* __restrict__ pt, const double* __restrict__ ft, const int* __restrict__ live,
                                                      double2* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int it = blockIdx.y, jt = blockIdx.x * 4 + wave, l = blockIdx.z;
    if (jt >= ntj) return;
    if (!live[it * ntj + jt]) return;
    const int i0 = it * KO_TI, j0 = jt * KO_TJ;
    typedef double ko_d2 __attribute__((ext_vector_type(2)));
    const ko_d2* pa = reinterpret_cast<const ko_d2*>(pt) + ((size_t)l * lp + l4) * ep + i0 + l15;
    const double* pb = td + (size_t)l4 * ep + j0 + l15;
    const size_t sk = (size_t)4 * ep;
    double4_t acc[4][2][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[q][c][0] = acc[q][c][1] = (double4_t){0, 0, 0, 0};
    ko_d2 a0[4], a1[4];
    double b0[2], b1[2];
    auto fetch = [&](ko_d2 (&a)[4], double (&bb)[2]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = pa[16 * q];
        bb[0] = pb[0]; bb[1] = pb[16];
        pa += sk; pb += sk;
    };
    auto mac = [&](const ko_d2 (&a)[4], const double (&bb)[2]) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                acc[q][c][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q][0], bb[c], acc[q][c][0], 0, 0, 0);
                acc[q][c][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q][1], bb[c], acc[q][c][1], 0, 0, 0);
            }
    };
    const int ks = lk >> 2;
    int s = 0;
    fetch(a0, b0);
#pragma unroll 1
    for (; s + 2 <= ks; s += 2) {
        fetch(a1, b1);
        mac(a0, b0);
        if (s + 2 < ks) fetch(a0, b0);
        mac(a1, b1);
    }
    if (s < ks) mac(a0, b0);
    // turn every sub-tile: register rr of lane (d, l4) takes column (d + r) & 15 of its own row of 16 lanes
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int src = (lane & 48) | ((l15 + l4 + 4 * rr) & 15);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                acc[q][c][0][rr] = __shfl(acc[q][c][0][rr], src, 64);
                acc[q][c][1][rr] = __shfl(acc[q][c][1][rr], src, 64);
            }
    }
    const size_t tile = ((size_t)l * nti + it) * ntj + jt;
#pragma unroll 1
    for (int f = 0; f < nf; ++f) {
        const double* F = ft + (size_t)f * ep;
        double fi[4][4], fj[2][4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
            for (int q = 0; q < 4; ++q) fi[q][rr] = F[i0 + 16 * q + l4 + 4 * rr];
#pragma unroll
            for (int c = 0; c < 2; ++c) fj[c][rr] = F[j0 + 16 * c + ((l15 + l4 + 4 * rr) & 15)];
        }
        double sr[6], si[6];
#pragma unroll
        for (int u = 0; u < 6; ++u) sr[u] = si[u] = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int r = l4 + 4 * rr, cc = (l15 + r) & 15;
                    const bool wrapped = l15 + r >= 16;
                    const int j = j0 + 16 * c + cc, k = j - (i0 + 16 * q + r);
                    const double wgt = k >= 1 && k <= nw && j < nen ? fi[q][rr] - fj[c][rr] : 0.0;
                    const double vr = wgt * acc[q][c][0][rr], vi = wgt * acc[q][c][1][rr];
                    sr[c - q + 4] += wrapped ? 0.0 : vr; si[c - q + 4] += wrapped ? 0.0 : vi;
                    sr[c - q + 3] += wrapped ? vr : 0.0; si[c - q + 3] += wrapped ? vi : 0.0;
                }
        double2* P = part + (tile * nf + f) * KO_NDIAG;
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            double re = sr[u], im = si[u];
            re += __shfl_xor(re, 16, 64); im += __shfl_xor(im, 16, 64);
            re += __shfl_xor(re, 32, 64); im += __shfl_xor(im, 32, 64);
            if (l4 == 0) P[16 * u + l15] = make_double2(re, im);
        }
    }
}

// opt(l, k, f) of the chunk's orbitals: the tiles that hold diagonal k, row tiles ascending and within a row tile column tiles ascending,
// times pi / (a^2 k).  One thread per (l, k, f); out: this set's (18, nw, nf) complex slice, l0 the chunk's first orbital.
__global__ __launch_bounds__(256) void k_opt_reduce(int nw, int nf, int nti, int ntj, int l0, int nl, double pref,
                                                    const int* __restrict__ live, const double2* __restrict__ part, double2* __restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nl * nw * nf) return;
    const int k = e % nw + 1, l = (e / nw) % nl, f = e / (nw * nl);         // (k fastest: neighbouring threads read neighbouring slots)
    double sr = 0.0, si = 0.0;
    for (int it = 0; it < nti; ++it) {
        const int i0 = it * KO_TI;
        // slot = k - j0 + i0 + 64 in 1 .. 95  <=>  k + i0 - 31 <= j0 <= k + i0 + 63
        const int jlo = max(0, (k + i0 - 31 + KO_TJ - 1) / KO_TJ), jhi = min(ntj - 1, (k + i0 + 63) / KO_TJ);
        for (int jt = jlo; jt <= jhi; ++jt) {
            const int j0 = jt * KO_TJ;
            if (!live[it * ntj + jt]) continue;
            const double2 v = part[((((size_t)l * nti + it) * ntj + jt) * nf + f) * KO_NDIAG + (k - j0 + i0 + 64)];
            sr += v.x; si += v.y;
        }
    }
    const double sc = pref / (double)k;
    out[(size_t)(l0 + l) + (size_t)NB * ((size_t)(k - 1) + (size_t)nw * f)] = make_double2(sc * sr, sc * si);
}

}  // namespace rsrec
