// The integrals that follow the SCF spectra Im Tr(O g0) (kernels_spectra.hpp): what bands%calculate_magnetic_moments, calculate_orbital_moments,
// calculate_moments and calculate_orbital_quadrupoles do with their energy-resolved arrays (bands.f90:476-496, :807-832, :1129-1143, :1040-1060).
//
// A series is a fixed-order real combination of the spectra rows of one site,
//   y(s, i, site) = 0.0 + sum_k comb(k, s, site) spec(k, i, site),  k ascending
// and every series gets
//   cum(s, i, site) = simpson_f(ene, EF = ene(i), nv1, y, fermi = .true., T = 0)       for EVERY mesh energy i   (math.f90:1600-1632)
//   mom(p, s, site) = simpson_m(.., H, EF, NPTS, y, EA, nexp = p, ene),  p = 0, 1, 2                            (math.f90:1579-1598)
//
// cum in O(nE) per series instead of O(nE^2).  With kBT = 1e-15 the Fermi weight f(k) of the limit ene(i) is exactly 1 for k < i, 0.5 at
// k = i and 0 for k > i on every mesh whose step exceeds 1e-12 (the entry point refuses other meshes): exp of a quotient below -37 vanishes
// beside 1, exp of one above 710 is inf and 1 / (inf + 1) = 0.  The rule (kernels_simpson.hpp) walks the triples t = 0, 1, ... of elements
// 2t, 2t + 1, 2t + 2 and adds ((A + y0 f0) + 4 y1 f1) + y2 f2.  Every triple that lies wholly below the limit (2t + 2 < i) has all three
// weights 1, and y * 1.0 is y: those triples form ONE running sum that is the same for all limits above them (k_moment_prefix: the value
// after every triple, formed once, serially, in the rule's association).  The limit itself lies in one triple (i odd: its middle) or two
// (i even: the end of one and the start of the next); k_moment_cum adds those with simpson_fermi_terms.  Every later triple adds
// ((A + y 0) + 4 y 0) + y 0 = A for finite y (A is never -0: it starts as +0, and +0 + -0 = +0), so it is left out.  The result carries
// the bits of simpson_fermi evaluated limit by limit.  Terms whose index lies above nen are zero, as there.
//
// Layout: everything is [site][energy][series], the layout of the spectra image (nop, nen, nsites) and of the cum image.
// No atomics; every sum is one thread's, in a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_simpson.hpp"

namespace rsrec {

constexpr int MI_WIDTH = 256;                 // workgroup width of the four kernels; k_moment_cum: (series, energy) pairs per workgroup
constexpr int MI_CHUNK = 16;                  // triples a serial thread loads (2 MI_CHUNK + 1 elements) before it adds them
constexpr int MOMENT_MAX_SERIES = 64;            // RSREC_MOMENT_NSER_MAX of rsrec.h

// y(s, i, site) of the n sites: spec [site][nen][nop] from the first of them, comb [site][nser][nop], y [site][nen][nser].
// Grid: x over the nen nser pairs, y = site.
__global__ __launch_bounds__(MI_WIDTH) void k_moment_series(int nop, int nser, int nen, const double* __restrict__ spec, const double* __restrict__ comb,
                                                            double* __restrict__ y) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * MI_WIDTH + threadIdx.x;
    if (e >= nen * nser) return;
    const int s = e % nser, i = e / nser;
    const size_t site = blockIdx.y;
    const double* row = spec + (site * nen + i) * nop;
    const double* c = comb + (site * nser + s) * nop;
    double v = 0.0;
    for (int k = 0; k < nop; ++k) v = v + c[k] * row[k];
    y[(site * nen + i) * nser + s] = v;
}

// P(t, s, site), t = 0 .. ntrip: the rule's sum after the first t triples with all weights 1, P(0) = 0.  One thread per (s, site), serial in t.
// y [site][nen][ld] (ld = nser, or nop where the series are the spectra rows themselves), P [site][ntrip + 1][nser].
// ((A + y0) + 4 y1) + y2 is ((A + y0 * 1.0) + 4.0 * y1 * 1.0) + y2 * 1.0 bit for bit; elements from nen on are zero (y 0 * f 0).
__global__ __launch_bounds__(MI_WIDTH) void k_moment_prefix(int nser, int ld, int nen, int ntrip, int n, const double* __restrict__ y, double* __restrict__ P) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * MI_WIDTH + threadIdx.x;
    if (e >= nser * n) return;
    const int s = e % nser;
    const size_t site = e / nser;
    const double* ys = y + site * nen * ld + s;
    double* Ps = P + site * (ntrip + 1) * nser + s;
    double A = 0.0;
    Ps[0] = A;
    for (int t0 = 0; t0 < ntrip; t0 += MI_CHUNK) {
        double b[2 * MI_CHUNK + 1];
#pragma unroll
        for (int j = 0; j <= 2 * MI_CHUNK; ++j) {
            const int k = 2 * t0 + j;
            b[j] = k < nen ? ys[(size_t)k * ld] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < MI_CHUNK; ++j)
            if (t0 + j < ntrip) {
                A = ((A + b[2 * j]) + 4.0 * b[2 * j + 1]) + b[2 * j + 2];
                Ps[(size_t)(t0 + j + 1) * nser] = A;
            }
    }
}

// cum(s, i, site) over the whole image of ntot sites: the n sites from `off` on from P and the one or two triples that hold the limit,
// every other site zero.  Grid: x over the nen nser pairs of a site in workgroups of MI_WIDTH, y = site of the image.
__global__ __launch_bounds__(MI_WIDTH) void k_moment_cum(int nser, int ld, int nen, int nv1, int off, int n, const double* __restrict__ ene,
                                                         const double* __restrict__ y, const double* __restrict__ P, double* __restrict__ cum) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * MI_WIDTH + threadIdx.x;
    if (e >= nen * nser) return;
    const int s = e % nser, i = e / nser;
    const int sl = (int)blockIdx.y - off;
    double* out = cum + ((size_t)blockIdx.y * nen + i) * nser + s;
    if (sl < 0 || sl >= n) { *out = 0.0; return; }
    const int itop = nv1 + 9, ntrip = itop / 2;                      // last I (1-based) of the rule's loop; its triples
    const int nfull = min(max((i - 1) / 2, 0), ntrip);               // triples wholly below the limit: 2t + 2 < i
    const double* ys = y + (size_t)sl * nen * ld + s;
    double A = P[((size_t)sl * (ntrip + 1) + nfull) * nser + s];
    A = simpson_fermi_terms(A, 2 * nfull + 2, min(2 * nfull + 4, itop), nen,
                            [&](int k) -> double { return k < i ? 1.0 : (k == i ? 0.5 : 0.0); },
                            [&](int k) -> double { return k < nen ? ys[(size_t)k * ld] : 0.0; });
    const double H = ene[1] - ene[0];
    *out = H * A / 3.0;
}

// mom(p, s, site) over the whole image of ntot sites, one thread per entry (p fastest), serial over the mesh:
//   AINT = ((AINT + Y(I-1) E(I-1)^p) + 4 Y(I) E(I)^p) + Y(I+1) E(I+1)^p,  I = 2, 4, .. <= npts - 1;   AINT = H AINT / 3;
//   if (ea /= ef) AINT = AINT + (ef - ea) ((Y(n) E(n)^p + 4 Y(n+1) E(n+1)^p) + Y(n+2) E(n+2)^p) / 6,  n = npts
// E^0 = 1, E^1 = E, E^2 = E E (what the compiler makes of an integer power).  npts + 2 <= nen: every element read exists.
__global__ __launch_bounds__(MI_WIDTH) void k_moment_fermi(int nser, int ld, int nen, int npts, double H, double ea, double ef, int off, int n, int ntot,
                                                           const double* __restrict__ ene, const double* __restrict__ y, double* __restrict__ mom) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * MI_WIDTH + threadIdx.x;
    if (e >= 3 * nser * ntot) return;
    const int p = e % 3, s = (e / 3) % nser, sl = e / (3 * nser) - off;
    if (sl < 0 || sl >= n) { mom[e] = 0.0; return; }
    const double* ys = y + (size_t)sl * nen * ld + s;
    auto term = [&](int k) -> double {                                 // Y E^p at 0-based k
#pragma clang fp contract(off)
        const double x = ene[k], yk = ys[(size_t)k * ld];
        return yk * (p == 0 ? 1.0 : (p == 1 ? x : x * x));
    };
    auto term4 = [&](int k) -> double {                                // 4 Y E^p: (4 Y) E^p as the reference's expression associates
#pragma clang fp contract(off)
        const double x = ene[k], yk = ys[(size_t)k * ld];
        return 4.0 * yk * (p == 0 ? 1.0 : (p == 1 ? x : x * x));
    };
    const int ntrip = (npts - 1) / 2;
    double A = 0.0;
    for (int t0 = 0; t0 < ntrip; t0 += MI_CHUNK) {
        double b[2 * MI_CHUNK + 1];
#pragma unroll
        for (int j = 0; j <= 2 * MI_CHUNK; ++j) {
            const int k = 2 * t0 + j;
            b[j] = k <= 2 * ntrip ? ((j & 1) ? term4(k) : term(k)) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < MI_CHUNK; ++j)
            if (t0 + j < ntrip) A = ((A + b[2 * j]) + b[2 * j + 1]) + b[2 * j + 2];
    }
    A = H * A / 3.0;
    if (ea != ef) {
        const double S = (term(npts - 1) + term4(npts)) + term(npts + 1);
        A = A + (ef - ea) * S / 6.0;
    }
    mom[e] = A;
}

}  // namespace rsrec
