// Operator spectra of the on-site Green function: spec(k, ie, site) = Im Tr(O_k g0(:,:,ie,site)) for a small set of 18 x 18 complex
// operators O_k, without g0 leaving the kernel that forms it.  Everything bands%calculate_magnetic_moments, calculate_orbital_moments,
// calculate_moments and calculate_orbital_quadrupoles take from g0 is such a functional (bands.f90:437-456, :985-993, :1123-1127,
// :1168-1180): 15 to 21 real numbers per (site, energy) instead of 648.
//
//  * k_block_spectra: k_block_green's shape (one wave per (site, energy), block_green_wave), then every lane of 0..53 contracts its
//    2 x 3 block of g with O_k(j, i), and the 64 partial sums of an operator are added in a fixed butterfly (no atomics: the same bits
//    whatever else the launch holds).  The operators (at most 32 x 5184 B) are read through the cache.
//  * k_chebyshev_optrace + k_chebyshev_spectra: Tr(O g0) is linear in the moments, so t(k, i) = Tr(O_k mu_i) is formed once per site and
//    the energy sum of k_chebyshev_ldos runs on t instead of on the diagonal of the moments.
//  * k_spectra_image: the zero-padded image over all sites, written where the caller's array is device memory.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_green.hpp"

namespace rsrec {

constexpr int SPECTRA_MAX_OPS = 32;

// sum over the 64 lanes, the same tree in every wave
__device__ __forceinline__ double wave_sum_fixed(double s) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
    return s;
}

// L.M holds g0 of the wave's (site, energy), column-major.  out[k] = Im Tr(O_k g) = sum_ij Im(O_k(j, i) g(i, j)), k = 0 .. nop - 1.
__device__ __forceinline__ void spectra_epilogue(const GreenLds& L, int lane, int ig, int jg, bool act, int nop, const double2* __restrict__ ops,
                                                 double* __restrict__ out) {
#pragma clang fp contract(off)
    double2 g[2][3];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
        for (int c = 0; c < 3; ++c) g[rr][c] = L.M[(2 * ig + rr) + NB * (3 * jg + c)];
#pragma unroll 1
    for (int k = 0; k < nop; ++k) {
        const double2* O = ops + (size_t)k * BLK;
        double s = 0.0;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double2 o = O[(3 * jg + c) + NB * (2 * ig + rr)];
                s = s + (o.x * g[rr][c].y + o.y * g[rr][c].x);
            }
        s = wave_sum_fixed(act ? s : 0.0);                       // lanes 54..63 shadow lane 53
        if (lane == 0) out[k] = s;
    }
}

// grid = (ceil(nen / GREEN_WAVES), nsites), as k_block_green.  ops: [nop][324] complex, column-major; spec: [site][nen][nop].
__global__ __launch_bounds__(GREEN_WAVES * 64, GREEN_WAVES_PER_SIMD) void k_block_spectra(int lld, int nen, const double* __restrict__ ene, double eta_re, double eta_im,
                                                                   int sym_term, const double* __restrict__ a_inf, const double* __restrict__ b_inf,
                                                                   const double2* __restrict__ a_b, const double2* __restrict__ b_sqrt, int nop,
                                                                   const double2* __restrict__ ops, double* __restrict__ spec) {
    __shared__ GreenLds lds[GREEN_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ei = blockIdx.x * GREEN_WAVES + wave, site = blockIdx.y;
    if (ei >= nen) return;                                       // wave-uniform; no workgroup barriers below
    GreenLds& L = lds[wave];
    const bool act = lane < 54;
    const int ig = act ? lane / 6 : 8, jg = act ? lane % 6 : 5;
    block_green_wave(L, lane, ig, jg, act, ene[ei], site, lld, eta_re, eta_im, sym_term, a_inf, b_inf, a_b, b_sqrt);
    spectra_epilogue(L, lane, ig, jg, act, nop, ops, spec + ((size_t)site * nen + ei) * nop);
}

// t[site][i][k] = Tr(O_k mu_i) (complex).  grid = (nm, nsites), one wave: lane l owns the elements l, l + 64, ... of the moment, the 64
// partial sums of an operator are added by the fixed butterfly.
__global__ __launch_bounds__(64) void k_chebyshev_optrace(int nm, int nop, const double2* __restrict__ ops, const double2* __restrict__ mu /*[site][nm][324]*/,
                                                         double2* __restrict__ t) {
#pragma clang fp contract(off)
    const int i = blockIdx.x, site = blockIdx.y, lane = threadIdx.x;
    const double2* m = mu + ((size_t)site * nm + i) * BLK;
    double2 mv[6];
    int oi[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const int el = lane + 64 * q;
        const bool in = el < BLK;
        mv[q] = in ? m[el] : make_double2(0.0, 0.0);
        oi[q] = in ? (el / NB) + NB * (el % NB) : 0;             // element (r, c) of the moment meets O(c, r)
    }
#pragma unroll 1
    for (int k = 0; k < nop; ++k) {
        const double2* O = ops + (size_t)k * BLK;
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double2 o = O[oi[q]];
            sr = sr + (o.x * mv[q].x - o.y * mv[q].y);
            si = si + (o.x * mv[q].y + o.y * mv[q].x);
        }
        sr = wave_sum_fixed(sr);
        si = wave_sum_fixed(si);
        if (lane == 0) t[((size_t)site * nm + i) * nop + k] = make_double2(sr, si);
    }
}

// spec[site][ie][k] = Im( sum_i t(k, i) (-i exp(-i i acos w_ie)) kern_i ) / sqrt(a^2 - (e_ie - b)^2): k_chebyshev_ldos with the operator
// traces in the place of the diagonal moments.  grid = (ceil(nen / CHEB_LDOS_TILE), nsites), dynamic LDS = nm nop complex; one thread owns
// one energy and keeps the nop sums in registers (i = 1 .. nm in the reference's order); all lanes read the same t: an LDS broadcast.
__global__ __launch_bounds__(CHEB_LDOS_TILE) void k_chebyshev_spectra(int nm, int nop, int nen, const double* __restrict__ ene, double a, double b,
                                                                     const double* __restrict__ kern /*[nm] jackson * {1,2,2,...}*/,
                                                                     const double2* __restrict__ t /*[site][nm][nop]*/, double* __restrict__ spec /*[site][nen][nop]*/) {
    extern __shared__ double2 dm[];
    const int site = blockIdx.y, ie = blockIdx.x * CHEB_LDOS_TILE + threadIdx.x;
    const double2* ts = t + (size_t)site * nm * nop;
    for (int k = threadIdx.x; k < nm * nop; k += CHEB_LDOS_TILE) dm[k] = ts[k];
    __syncthreads();
    if (ie >= nen) return;                                   // (no barrier below)
    const double e = ene[ie];
    const double th = acos((e - b) / a);
    double si[SPECTRA_MAX_OPS];
#pragma unroll
    for (int k = 0; k < SPECTRA_MAX_OPS; ++k) si[k] = 0.0;
    for (int i = 0; i < nm; ++i) {
        const double2 f = chebyshev_phase(i, th, kern[i]);
#pragma unroll
        for (int k = 0; k < SPECTRA_MAX_OPS; ++k)
            if (k < nop) {                                   // uniform
                const double2 v = dm[i * nop + k];
                si[k] += v.x * f.y + v.y * f.x;
            }
    }
    const double den = sqrt(a * a - (e - b) * (e - b));
    double* out = spec + ((size_t)site * nen + ie) * nop;
#pragma unroll
    for (int k = 0; k < SPECTRA_MAX_OPS; ++k)
        if (k < nop) out[k] = si[k] / den;
}

// The image over all sites, spec(nop, nen, nsites_total) in Fortran order: elements [lo, lo + nfill) are the rank's compact block, the rest zero.
__global__ void k_spectra_image(const double* __restrict__ compact, size_t lo, size_t nfill, size_t total, double* __restrict__ img) {
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (size_t)gridDim.x * blockDim.x)
        img[k] = (k >= lo && k - lo < nfill) ? compact[k - lo] : 0.0;
}

}  // namespace rsrec
