// Kernels of the Kubo-Bastin conductivity integrand (conductivity_mod, conductivity.f90:158-268): the energy-resolved
//   integrand(l, i, v) = factor sum_{n,m} Gamma(i, n, m) mu(l, l, n, m, v)
// WITHOUT the nE x L x L array Gamma.  With x = (ene_i - b)/a, s = sqrt(1 - x^2), theta = acos x, w_n = g_n weights_n (Lorentz kernel x
// the half weight of n = 1, :190-194), A(i,n) = w_n (x - i n s) e^{i n theta}, B(i,n) = w_n T_n(x) (n = 0-based order):
//   Gamma(i,n,m) (1 - x^2)^2 = A(i,n) B(i,m) + B(i,n) conj(A(i,m))                                            (:213-218)
// and, with M = mu(l,l,:,:,v), S = M + M^T, D = M - M^T (complex),
//   sum_{n,m} Gamma M = [ sum_n Re A(i,n) (B S^T)(i,n) + i Im A(i,n) (B D^T)(i,n) ] / (1 - x^2)^2.
// So per (orbital, vector) the work is ONE real A-side operand (the table B, nE x L) against four real B-side planes (Re S, Im S,
// Re D, Im D; L x L): four real GEMMs of nE x L x L -- two thirds of the six the complex form A M^T, conj(A) M^T needs -- with a
// row-wise dot against A in the epilogue.  S and D come from the 18 orbital diagonals of mu alone (k_cond_gather).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_mfma.hpp"
#include "kernels_simpson.hpp"

namespace rsrec {

constexpr int KC_TI = 4;                      // 16-row tiles (energies) per wave
constexpr int KC_ROWS = 16 * KC_TI;           // 64 energies per wave; the tables' energy dimension is padded to a multiple of this

// Basis tables, one thread per energy (the Chebyshev recurrence runs along n, :203-207):
//   tb[n][i] = w_n T_n(x_i)                     n < lk   (the A-side operand, zero for n >= L or i >= nen)
//   ta[n][i] = w_n (x_i - i n s_i) e^{i n theta_i}   n < ln   (the epilogue factor, zero for n >= L or i >= nen)
//   pre[i]   = factor / (1 - x_i^2)^2
__global__ __launch_bounds__(256) void k_cond_basis(int nen, int ep, int L, int lk, int ln, const double* __restrict__ ene, const double* __restrict__ w,
                                                    double a, double b, double factor, double* __restrict__ tb, double2* __restrict__ ta,
                                                    double* __restrict__ pre) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ep) return;
    const bool live = i < nen;
    const double x = live ? (ene[i] - b) / a : 0.0;
    const double s = sqrt(1.0 - x * x), th = acos(x);
    if (live) { const double d = 1.0 - x * x; pre[i] = factor / (d * d); }
    double t0 = 1.0, t1 = x;                  // T_{n}, T_{n+1}
    const int nn = max(lk, ln);
    for (int n = 0; n < nn; ++n) {
        const bool on = live && n < L;
        const double wn = on ? w[n] : 0.0;
        if (n < lk) tb[(size_t)n * ep + i] = wn * t0;
        if (n < ln) {
            double sn, cs;
            sincos((double)n * th, &sn, &cs);
            const double cr = x, ci = -(double)n * s;      // (x - i n s) (cos + i sin)
            ta[(size_t)n * ep + i] = make_double2(wn * (cr * cs - ci * sn), wn * (cr * sn + ci * cs));
        }
        const double t2 = 2.0 * x * t1 - t0;
        t0 = t1; t1 = t2;
    }
}

// S = M + M^T and D = M - M^T of the orbital diagonals of one vector's moments, written as the B-side planes of k_cond_contract:
//   g[l][m][n] = (S(n,m), D(n,m)) as four doubles (Re S, Im S, Re D, Im D), m < lk rows, n < ln columns, zero outside L x L.
// M(n,m) = mu[l sl + sn (n + L m)] (complex): sl = 19, sn = 324 reads the reference's mu_nm(18,18,L,L) where it lies (the diagonal
// of every 18x18 block); sl = 1, sn = 18 a compact (18,L,L) copy of the diagonals.
__global__ __launch_bounds__(256) void k_cond_gather(const double2* __restrict__ mu, int sl, int sn, int L, int lk, int ln, double4_t* __restrict__ g) {
    const size_t per_l = (size_t)lk * ln, total = per_l * NB;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(e / per_l);
        const int m = (int)((e - (size_t)l * per_l) / ln), n = (int)(e % ln);
        double4_t v = {0.0, 0.0, 0.0, 0.0};
        if (n < L && m < L) {
            const double2 p = mu[(size_t)l * sl + (size_t)sn * ((size_t)n + (size_t)L * m)];
            const double2 q = mu[(size_t)l * sl + (size_t)sn * ((size_t)m + (size_t)L * n)];
            v = (double4_t){p.x + q.x, p.y + q.y, p.x - q.x, p.y - q.y};
        }
        g[e] = v;
    }
}

// The contraction on the FP64 matrix cores.  One wave = 64 energies x 16 columns n of one orbital, over all of K = m (no split:
// every partial is one wave's fixed-order sum).  Per k-step (4 values of m) lane (l15, l4) loads tb[m0 + l4][i0 + 16 q + l15] for the
// four row tiles (A operand) and the 32-byte (Re S, Im S, Re D, Im D) of g[l][m0 + l4][n0 + l15] (B operand), requested one k-step
// ahead; 16 v_mfma_f64_16x16x4 per k-step into four accumulator planes per row tile.
// Epilogue: accumulator row l4 + 4 rr, column l15 (the f64 C/D map) times ta(i, n) -> re = Re A Re(BS) - Im A Im(BD),
// im = Re A Im(BS) + Im A Re(BD), summed over the 16 columns by a fixed xor butterfly -> part[l][ntile][i].
// Grid: x = energy blocks of 4 waves (256 energies), y = column tiles, z = orbitals.  All tables are zero-padded: no clamping.
__global__ __launch_bounds__(256, 2) void k_cond_contract(int ep, int lk, int ln, const double* __restrict__ tb, const double2* __restrict__ ta,
                                                       const double4_t* __restrict__ g, double2* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int i0 = (blockIdx.x * 4 + wave) * KC_ROWS;
    if (i0 >= ep) return;
    const int nt = blockIdx.y, n0 = nt * 16, l = blockIdx.z;
    typedef double kc_d2 __attribute__((ext_vector_type(2)));
    const double* pa = tb + (size_t)l4 * ep + i0 + l15;
    const kc_d2* pb = reinterpret_cast<const kc_d2*>(g + (size_t)l * lk * ln + (size_t)l4 * ln + n0 + l15);
    const size_t sa = (size_t)4 * ep, sb = (size_t)4 * ln * 2;      // one k-step: 4 rows of tb, 4 rows of g (two kc_d2 per entry)
    double4_t acc[KC_TI][4];
#pragma unroll
    for (int q = 0; q < KC_TI; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[q][c] = (double4_t){0, 0, 0, 0};
    double a0[KC_TI], a1[KC_TI];
    kc_d2 s0, d0, s1, d1;
    auto fetch = [&](double (&a)[KC_TI], kc_d2& bs, kc_d2& bd) {
#pragma unroll
        for (int q = 0; q < KC_TI; ++q) a[q] = pa[16 * q];
        bs = pb[0]; bd = pb[1];
        pa += sa; pb += sb;
    };
    auto mac = [&](const double (&a)[KC_TI], const kc_d2& bs, const kc_d2& bd) {
#pragma unroll
        for (int q = 0; q < KC_TI; ++q) {
            acc[q][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], bs[0], acc[q][0], 0, 0, 0);
            acc[q][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], bs[1], acc[q][1], 0, 0, 0);
            acc[q][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], bd[0], acc[q][2], 0, 0, 0);
            acc[q][3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], bd[1], acc[q][3], 0, 0, 0);
        }
    };
    const int ks = lk >> 2;
    int s = 0;
    fetch(a0, s0, d0);
#pragma unroll 1
    for (; s + 2 <= ks; s += 2) {
        fetch(a1, s1, d1);
        mac(a0, s0, d0);
        if (s + 2 < ks) fetch(a0, s0, d0);
        mac(a1, s1, d1);
    }
    if (s < ks) mac(a0, s0, d0);
    double2* P = part + ((size_t)l * (ln >> 4) + nt) * ep;
#pragma unroll
    for (int q = 0; q < KC_TI; ++q)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int i = i0 + 16 * q + l4 + 4 * rr;
            const double2 w = ta[(size_t)(n0 + l15) * ep + i];
            double re = w.x * acc[q][0][rr] - w.y * acc[q][3][rr];
            double im = w.x * acc[q][1][rr] + w.y * acc[q][2][rr];
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) { re += __shfl_xor(re, o, 16); im += __shfl_xor(im, o, 16); }
            if (l15 == 0) P[i] = make_double2(re, im);
        }
}

// The column tiles' partials summed in tile order, times factor / (1 - x^2)^2 -> integrand(l, i) of this vector (complex (18, nen)).
__global__ __launch_bounds__(256) void k_cond_reduce(int nen, int ep, int ntiles, const double2* __restrict__ part, const double* __restrict__ pre,
                                                     double2* __restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nen * NB) return;
    const int l = e % NB, i = e / NB;
    double sr = 0.0, si = 0.0;
    for (int t = 0; t < ntiles; ++t) { const double2 v = part[((size_t)l * ntiles + t) * ep + i]; sr += v.x; si += v.y; }
    out[e] = make_double2(pre[i] * sr, pre[i] * si);
}

// ---- the conductivity itself: the tail of calculate_conductivity_tensor (conductivity.f90:283-372) ----
// sigma(r, i, s) = simpson_f(x, EF = x(i), nv1, S(r, :, s), fermi = .true., T) for the 38 series r of every set s: Re and Im of the total
// and of the 18 orbitals; sets and vectors 0-based in this file: set 0 the sum over the vectors, set 1 + v vector v alone ('per_type').
constexpr int CT_ROWS = 2 + 2 * NB;           // 38: Re total, Im total, Re orbital 1..18, Im orbital 1..18
constexpr int CT_TILE = 512;                  // Fermi weights staged in LDS at a time (CT_TILE + 1: neighbouring tiles share their end point)

// The series, in the order the reference forms them (:283-291, :316-326).  One thread per (energy k, set s).
//   set 0    : orbital row l = 0.0 + sum_v integ(l, k, v), v ascending;  total row = 0.0 + sum_l of the orbital rows, l ascending
//   set 1 + v: orbital row l = integ(l, k, v);  total row = the same sum over l
// sk: [k][row + 38 set], the layout k_cond_tensor reads (neighbouring threads, neighbouring addresses); series (optional): (38, nen, nsets).
__global__ __launch_bounds__(256) void k_cond_series(int nen, int nvec, int nsets, const double2* __restrict__ integ, double* __restrict__ sk,
                                                     double* __restrict__ series) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nen * nsets) return;
    const int k = e % nen, s = e / nen;
    double* o = sk + ((size_t)k * nsets + s) * CT_ROWS;
    double* p = series ? series + ((size_t)s * nen + k) * CT_ROWS : nullptr;
    double tr = 0.0, ti = 0.0;
    for (int l = 0; l < NB; ++l) {
        double re, im;
        if (s == 0) {
            re = 0.0; im = 0.0;
            for (int v = 0; v < nvec; ++v) { const double2 z = integ[((size_t)v * nen + k) * NB + l]; re += z.x; im += z.y; }
        } else {
            const double2 z = integ[((size_t)(s - 1) * nen + k) * NB + l];
            re = z.x; im = z.y;
        }
        tr += re; ti += im;
        o[2 + l] = re; o[2 + NB + l] = im;
        if (p) { p[2 + l] = re; p[2 + NB + l] = im; }
    }
    o[0] = tr; o[1] = ti;
    if (p) { p[0] = tr; p[1] = ti; }
}

// The integrals.  Workgroup (i, y): limit EF = x(i), columns c = y blockDim.x + thread of the ncol = 38 nsets (row, set) columns.
// The weight row f(k) = fermifun(x(k), x(i), kBT) of the limit is computed once per workgroup, CT_TILE + 1 values at a time, in LDS (its
// size does not depend on nen); every thread then runs its column's serial loop over that tile (simpson_fermi_terms: the bits of one pass
// over I = 2 .. nv1 + 9).  x(k) = (ene(k) - b) / a as k_cond_basis forms it; weights and integrand from index nen on are zero.
// No T = 0 special case: kBT = 1e-15 gives the weights 1, 0.5, 0 by itself.  sigma: (38, nen, nsets).
__global__ __launch_bounds__(1024) void k_cond_tensor(int nen, int nv1, int ncol, const double* __restrict__ ene, double a, double b, double T,
                                                      const double* __restrict__ sk, double* __restrict__ sigma) {
#pragma clang fp contract(off)
    __shared__ double fw[CT_TILE + 1];
    const int i = blockIdx.x, c = blockIdx.y * blockDim.x + threadIdx.x;
    const bool live = c < ncol;
    const double xi = (ene[i] - b) / a, kbt = simpson_kbt(T);
    const int itop = nv1 + 9;                                        // last I (1-based) of the loop
    auto y = [&](int k) -> double { return k < nen ? sk[(size_t)k * ncol + c] : 0.0; };
    double A = 0.0;
    for (int t0 = 0; t0 + 2 <= itop; t0 += CT_TILE) {                // this tile: I = t0 + 2 .. t0 + CT_TILE, 0-based indices t0 .. t0 + CT_TILE
        __syncthreads();
        for (int j = threadIdx.x; j <= CT_TILE; j += blockDim.x) {
            const int k = t0 + j;
            fw[j] = k < nen ? fermifun((ene[k] - b) / a, xi, kbt) : 0.0;
        }
        __syncthreads();
        if (live) A = simpson_fermi_terms(A, t0 + 2, min(t0 + CT_TILE, itop), nen, [&](int k) -> double { return fw[k - t0]; }, y);
    }
    if (live) {
        const double H = (ene[1] - b) / a - (ene[0] - b) / a;
        sigma[((size_t)(c / CT_ROWS) * nen + i) * CT_ROWS + c % CT_ROWS] = H * A / 3.0;
    }
}

}  // namespace rsrec
