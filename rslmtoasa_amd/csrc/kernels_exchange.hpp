// Exchange couplings from the intersite Green functions: green%calculate_intersite_gf / _twoindex (green.f90:386-469) and the integrands
// and Fermi-weighted Simpson integrals of exchange%calculate_exchange / _twoindex (exchange.f90:1032-1615).
//
// d_matrix (symbolic_atom.f90:241-265) is diagonal, so every quantity is Im or Re of a trace
//     T(A, B) = Tr(D_i A D_j B) = sum_ab d_i(a) A_ab d_j(b) B_ba            (81 complex MACs instead of three 9x9 matmuls)
// over the 8 Pauli parts (Ginmag, Gix..Giz, Gjnmag, Gjx..Gjz) and the 16 two-index parts (G00ij .. Gz0ji).  42 distinct traces give the
// 41 real integrands of one (pair, energy); g0 of the pair's chains never leaves LDS.
//
// Integrand rows (per pair and energy), the reference's names:
//   0 jtot   1..3 jjtot(k)   4..12 itot(k,l) (k fastest)                      <- calculate_exchange
//   13 jcd  14 jsd  15 jcc  16 jsc  17..19 dcc(k)  20..22 dsc(k)  23..31 isd(k,l)  32..40 isc(k,l)   <- _twoindex (= T_comm_xcparts' order)
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_green.hpp"
#include "kernels_simpson.hpp"

namespace rsrec {

constexpr int XC_NINT = 41;     // integrand rows per (pair, energy)
constexpr int XC_NTR = 42;      // distinct traces per (pair, energy)
constexpr int XC_NOUT = 67;     // integrated numbers per pair: xc (13), so (13), fo (13), parts (28)

struct XcShared {
    double2 rows[XC_NTR * 9];   // row sums of the traces, [trace][a]
    double2 tr[XC_NTR];
    double d[2][9];             // diagonals of D_i, D_j
};

// trace t -> (A, B) of T(A, B); matrices 0..7 the Pauli parts (0 Ginmag, 1+k Gik, 4 Gjnmag, 5+k Gjk), 8..23 the two-index parts
// (8 G00ij, 9 G01ij, 10 G00ji, 11 G01ji, 12+k Gk1ij, 15+k Gk0ij, 18+k Gk1ji, 21+k Gk0ji)
__device__ __forceinline__ void xc_trace_pair(int t, int& ma, int& mb) {
    if (t == 0) { ma = 0; mb = 4; }                                          // dGdG_Jnc
    else if (t < 10) { const int k = (t - 1) % 3, l = (t - 1) / 3; ma = 1 + k; mb = 5 + l; }   // T(Gik, Gjl)
    else if (t < 13) { ma = 0; mb = 5 + (t - 10); }                          // dGdG_Dnc, first product
    else if (t < 16) { ma = 1 + (t - 13); mb = 4; }                          // dGdG_Dnc, second product
    else if (t == 16) { ma = 8; mb = 10; }                                   // jcd
    else if (t == 17) { ma = 9; mb = 11; }                                   // jcc
    else if (t < 21) { ma = 8; mb = 18 + (t - 18); }                         // dsc
    else if (t < 24) { ma = 9; mb = 21 + (t - 21); }                         // dcc
    else if (t < 33) { const int k = (t - 24) % 3, l = (t - 24) / 3; ma = 15 + k; mb = 21 + l; }   // isd
    else { const int k = (t - 33) % 3, l = (t - 33) / 3; ma = 12 + k; mb = 18 + l; }              // isc
}

// the reflection 2*j0 - j of calculate_intersite_gf_twoindex (0-based): l = 0 (s), 1 (p: 1..3), 2 (d: 4..8); m -> -m within the shell
__device__ __forceinline__ int xc_refl(int j) { const int j0 = j == 0 ? 0 : (j < 4 ? 2 : 6); return 2 * j0 - j; }

// Element idx of gij (side 0) or gji (side 1) from g0 of the pair's chains, M(w) = Mb + w * stride (green.f90:446-453); an i == j pair
// reads chain 1 alone.  Shared by the exchange and the damping epilogue.
__device__ __forceinline__ double2 xc_gpair(const double2* Mb, int stride, bool same, int side, int idx) {
#pragma clang fp contract(off)
    const double2 g1 = Mb[idx];
    if (same) return g1;
    const double2 g2 = Mb[stride + idx], g3 = Mb[2 * stride + idx], g4 = Mb[3 * stride + idx];
    const double2 dd = make_double2(g1.x - g2.x, g1.y - g2.y);
    const double2 s = make_double2(g3.y - g4.y, (-g3.x) - (-g4.x));          // 1/i g3 - 1/i g4
    return side == 0 ? make_double2((dd.x + s.x) * 0.5, (dd.y + s.y) * 0.5) : make_double2((dd.x - s.x) * 0.5, (dd.y - s.y) * 0.5);
}

// Workgroup epilogue (256 threads); no FMA contraction, so the elementwise arithmetic is the reference's operation by operation (the
// traces sum in their own fixed order).  M(w) = Mb + w * stride holds g0 of chain w (column-major 18 x 18); S(w) = Sb + w * stride is free
// scratch of 324 complex.  Both are overwritten.  dpar: (4, 3, 2) of the pair; out: the 41 integrand rows of this (pair, energy).
__device__ __forceinline__ void xc_epilogue(double2* Mb, double2* Sb, int stride, XcShared& xs, bool same, double e, const double* __restrict__ dpar,
                                            double* __restrict__ out) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    // d_matrix (symbolic_atom.f90:247-262) in its order: de = (cd wu^2 - cu wd^2 + (wd^2 - wu^2) e) / (wu wd).  Its cu, cd, wu, wd come from
    // cmplx(x, 0.0d0) without a KIND: default (single-precision) complex, so c + vmad and dele pass through float before the double arithmetic
    if (t < 18) {
        const int side = t / 9, a = t % 9, l = a == 0 ? 0 : (a < 4 ? 1 : 2);
        const double* q = dpar + 4 * (l + 3 * side);
        const double cu = (double)(float)q[0], cd = (double)(float)q[1], wu0 = (double)(float)q[2], wd0 = (double)(float)q[3];
        const double wuwd = wu0 * wd0, wu = wu0 * wu0, wd = wd0 * wd0;
        xs.d[side][a] = (cd * wu - cu * wd + (wd - wu) * e) / wuwd;
    }
    // gij / gji (green.f90:446-453) and the 8 Pauli parts (:455-467): part k at S(k / 4) + 81 (k % 4), element (j, i) at j + 9 i
#pragma unroll 1
    for (int it = t; it < 8 * 81; it += 256) {
        const int k = it / 81, el = it % 81, j = el % 9, i = el / 9, side = k >> 2, comp = k & 3;
        double2 v[4];                                  // gij or gji at (j,i), (j+9,i+9), (j,i+9), (j+9,i)
        const int idx[4] = {j + NB * i, (j + 9) + NB * (i + 9), j + NB * (i + 9), (j + 9) + NB * i};
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = xc_gpair(Mb, stride, same, side, idx[r]);
        double2 p;
        if (comp == 0) p = make_double2((v[0].x + v[1].x) * 0.5, (v[0].y + v[1].y) * 0.5);
        else if (comp == 3) p = make_double2(0.5 * (v[0].x - v[1].x), 0.5 * (v[0].y - v[1].y));
        else if (comp == 2) p = make_double2(0.5 * ((-v[2].y) - (-v[3].y)), 0.5 * (v[2].x - v[3].x));   // i gij(j,i+9) - i gij(j+9,i)
        else p = make_double2(0.5 * (v[2].x + v[3].x), 0.5 * (v[2].y + v[3].y));
        Sb[(k >> 2) * stride + 81 * (k & 3) + el] = p;
    }
    __syncthreads();
    // the 16 two-index parts (green.f90:393-421) over the g0 staging: part q at M(q / 4) + 81 (q % 4)
#pragma unroll 1
    for (int it = t; it < 16 * 81; it += 256) {
        const int q = it / 81, el = it % 81, r = el % 9, c = el / 9;
        int pa, pb; bool plus;
        if (q < 4) { pa = q < 2 ? 0 : 4; pb = q < 2 ? 4 : 0; plus = (q & 1) == 0; }
        else { const int g = (q - 4) / 3, k = (q - 4) % 3; pa = (g < 2 ? 1 : 5) + k; pb = (g < 2 ? 5 : 1) + k; plus = (g & 1) == 1; }
        const double2 A = Sb[(pa >> 2) * stride + 81 * (pa & 3) + el];
        double2 B = Sb[(pb >> 2) * stride + 81 * (pb & 3) + xc_refl(c) + 9 * xc_refl(r)];
        if ((r + c) & 1) B = make_double2(-B.x, -B.y);                      // (-1)**(k+j)
        Mb[(q >> 2) * stride + 81 * (q & 3) + el] = plus ? make_double2(0.5 * (A.x + B.x), 0.5 * (A.y + B.y)) : make_double2(0.5 * (A.x - B.x), 0.5 * (A.y - B.y));
    }
    __syncthreads();
    // traces: row a of trace tr = sum_b (d_i(a) A_ab) (d_j(b) B_ba), b in order
#pragma unroll 1
    for (int it = t; it < XC_NTR * 9; it += 256) {
        const int tr = it / 9, a = it % 9;
        int ma, mb;
        xc_trace_pair(tr, ma, mb);
        const double2* A = ma < 8 ? Sb + (ma >> 2) * stride + 81 * (ma & 3) : Mb + ((ma - 8) >> 2) * stride + 81 * ((ma - 8) & 3);
        const double2* B = mb < 8 ? Sb + (mb >> 2) * stride + 81 * (mb & 3) : Mb + ((mb - 8) >> 2) * stride + 81 * ((mb - 8) & 3);
        const double di = xs.d[0][a];
        double sr = 0.0, si = 0.0;
        for (int b = 0; b < 9; ++b) {
            const double2 x = A[a + 9 * b], y = B[b + 9 * a];
            const double dj = xs.d[1][b];
            const double xr = di * x.x, xi = di * x.y, yr = dj * y.x, yi = dj * y.y;
            sr += xr * yr - xi * yi;
            si += xr * yi + xi * yr;
        }
        xs.rows[it] = make_double2(sr, si);
    }
    __syncthreads();
    if (t < XC_NTR) {
        double sr = 0.0, si = 0.0;
        for (int a = 0; a < 9; ++a) { sr += xs.rows[t * 9 + a].x; si += xs.rows[t * 9 + a].y; }
        xs.tr[t] = make_double2(sr, si);
    }
    __syncthreads();
    if (t < XC_NINT) {
        const double2* T = xs.tr;
        double v;
        if (t == 0) v = ((T[0].y - T[1].y) - T[5].y) - T[9].y;                             // Im Tr dGdG_Jnc
        else if (t < 4) v = T[10 + t - 1].x - T[13 + t - 1].x;                            // Re Tr dGdG_Dnc(k)
        else if (t < 13) { const int k = (t - 4) % 3, l = (t - 4) / 3; v = 0.5 * (T[1 + k + 3 * l].y + T[1 + l + 3 * k].y); }   // Im Tr dGdG_Anc(k,l)
        else if (t == 13) v = T[16].y;                                                      // jcd
        else if (t == 14) v = (T[24].y + T[28].y) + T[32].y;                               // jsd
        else if (t == 15) v = T[17].y;                                                      // jcc
        else if (t == 16) v = (T[33].y + T[37].y) + T[41].y;                               // jsc
        else if (t < 20) v = T[21 + t - 17].x;                                              // dcc(k)
        else if (t < 23) v = T[18 + t - 20].x;                                              // dsc(k)
        else if (t < 32) v = T[24 + t - 23].y;                                              // isd(k,l)
        else v = T[33 + t - 32].y;                                                          // isc(k,l)
        out[t] = v;
    }
}

// Green stage of kind 0 for one (pair, energy): wave w of the 256 threads runs chain chain0 + w through block_green_wave with eta = 0 and
// leaves g0 in lds[w].M; an i == j pair runs wave 0 only.  Ends with a workgroup barrier.
constexpr int PAIR_BLOCK_STRIDE = (int)(sizeof(GreenLds) / sizeof(double2));
static_assert(sizeof(GreenLds) % sizeof(double2) == 0, "GreenLds stride");
__device__ __forceinline__ void pair_green_block(GreenLds* lds, bool same, double e, int chain0, int lld, int sym_term, const double* __restrict__ a_inf,
                                                 const double* __restrict__ b_inf, const double2* __restrict__ a_b, const double2* __restrict__ b_sqrt) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave == 0 || !same) {
        const bool act = lane < 54;
        const int ig = act ? lane / 6 : 8, jg = act ? lane % 6 : 5;
        block_green_wave(lds[wave], lane, ig, jg, act, e, chain0 + wave, lld, 0.0, 0.0, sym_term, a_inf, b_inf, a_b, b_sqrt);
    }
    __syncthreads();
}

// kind 0.  grid = (nen, npairs), 256 threads: wave w runs chain w of the pair through green%bgreen (eta = 0: block_green_ij, green.f90:354-384)
// on k_block_green's path; an i == j pair runs chain 1 only (calculate_intersite_gf reads g0(:,:,:,1) alone, and recur_b_ij leaves slots
// 2..4 zero).  a_b, b_sqrt, a_inf, b_inf: the chains of the launch; the pair's first chain is cbase[pair] - cb0 (4 per pair, or 1 for
// an i == j pair when a seeded recursion skipped its repeats).  integ: [pair][nen][41].
__global__ __launch_bounds__(256, GREEN_WAVES_PER_SIMD) void k_exchange_block(int lld, int nen, const double* __restrict__ ene, int sym_term,
                                                                           const double* __restrict__ a_inf, const double* __restrict__ b_inf,
                                                                           const double2* __restrict__ a_b, const double2* __restrict__ b_sqrt,
                                                                           const int* __restrict__ same, const int* __restrict__ cbase, int cb0,
                                                                           const double* __restrict__ dpar, double* __restrict__ integ) {
    __shared__ GreenLds lds[4];
    __shared__ XcShared xs;
    const int ie = blockIdx.x, pair = blockIdx.y;
    pair_green_block(lds, same[pair] != 0, ene[ie], cbase[pair] - cb0, lld, sym_term, a_inf, b_inf, a_b, b_sqrt);
    constexpr int stride = PAIR_BLOCK_STRIDE;
    // (same and e are read again here rather than held across the continued fraction: the kernel then stays within k_block_green's registers)
    xc_epilogue(lds[0].M, lds[0].B, stride, xs, same[pair] != 0, ene[ie], dpar + (size_t)24 * pair, integ + ((size_t)pair * nen + ie) * XC_NINT);
}

// kind 1.  grid = (nen, npairs), 256 threads: g0 of the pair's chains as k_chebyshev_green forms it (chebyshev_green_ij, green.f90:933-992:
// chebyshev_green per chain), into LDS, then the same epilogue.  mu: [chain][nm][324]; dynamic LDS: nm phase factors.
struct XcChebLds {
    double2 g[4][BLK];
    double2 s[4][BLK];
};
// Green stage of kind 1 for one (pair, energy): the phase table into ef (nm entries), then g0 of the pair's chains (1 for an i == j pair)
// into cl.g.  mu: the pair's first chain.  Ends with a workgroup barrier.
__device__ __forceinline__ void pair_green_cheb(XcChebLds& cl, double2* ef, int nm, double e, double a, double b, const double* __restrict__ kern,
                                                const double2* __restrict__ mu, bool same) {
    const double th = acos((e - b) / a);
    for (int i = threadIdx.x; i < nm; i += blockDim.x) ef[i] = chebyshev_phase(i, th, kern[i]);
    __syncthreads();
    const double den = sqrt(a * a - (e - b) * (e - b));
    const int nch = same ? 1 : 4;
    for (int it = threadIdx.x; it < nch * BLK; it += blockDim.x) {
        const int c = it / BLK, el = it % BLK;
        cl.g[c][el] = chebyshev_green_elem(mu + (size_t)c * nm * BLK, ef, nm, el, den);
    }
    __syncthreads();
}
__global__ __launch_bounds__(256) void k_exchange_cheb(int nm, int nen, const double* __restrict__ ene, double a, double b, const double* __restrict__ kern,
                                                      const double2* __restrict__ mu, const int* __restrict__ same, const int* __restrict__ cbase, int cb0,
                                                      const double* __restrict__ dpar, double* __restrict__ integ) {
    extern __shared__ double2 ef[];
    __shared__ XcChebLds cl;
    __shared__ XcShared xs;
    const int ie = blockIdx.x, pair = blockIdx.y;
    const bool sm = same[pair] != 0;
    const double e = ene[ie];
    pair_green_cheb(cl, ef, nm, e, a, b, kern, mu + (size_t)(cbase[pair] - cb0) * nm * BLK, sm);
    xc_epilogue(&cl.g[0][0], &cl.s[0][0], BLK, xs, sm, e, dpar + (size_t)24 * pair, integ + ((size_t)pair * nen + ie) * XC_NINT);
}

// fermifun (math.f90:994-1000) at T = 0 as simpson_f calls it: kBT = kB * 0 + 1e-15
__global__ void k_exchange_fermi(int nen, const double* __restrict__ ene, double ef, double* __restrict__ fw) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nen) return;
    fw[k] = fermifun(ene[k], ef, simpson_kbt(0.0));
}

// integrand y(k) of output q (0..66: xc, so, fo, parts) from the 41 rows at energy k, in the reference's expression order
__device__ __forceinline__ double xc_quantity(const double* __restrict__ r, int q) {
#pragma clang fp contract(off)
    if (q < 13) return r[q];
    if (q < 26) {                                                   // second order (exchange.f90:1148-1270)
        const int o = q - 13;
        if (o == 0) return ((r[13] - r[14]) + r[15]) - r[16];
        if (o < 4) return 2.0 * (r[20 + o - 1] + r[17 + o - 1]);
        return r[23 + o - 4] + r[32 + o - 4];
    }
    if (q < 39) {                                                   // first order
        const int o = q - 26;
        if (o == 0) return ((r[13] + r[14]) - r[15]) - r[16];
        if (o < 4) return 2.0 * (r[20 + o - 1] - r[17 + o - 1]);
        return (-r[23 + o - 4]) + r[32 + o - 4];
    }
    return r[13 + q - 39];
}

// simpson_f(fermi = .true., T = 0) (math.f90:1600-1632) of one integrand y(k) (0-based k; zero from nen on) with the Fermi weights fw:
// the library's one Simpson rule (kernels_simpson.hpp: the reference's summation order, the term it reads past its arrays taken as zero)
// on a weight array.  The rule of the exchange module's integrals (k_exchange_integrate, k_rows_integrate).
template <class Y>
__device__ __forceinline__ double xc_simpson_fermi(int nen, int nv1, double H, const double* __restrict__ fw, Y y) {
    return simpson_fermi(nen, nv1, H, [&](int k) -> double { return fw[k]; }, y);
}

// xc_simpson_fermi of every output of every pair, and the cumulative second-order J of fort.150.
// grid = npairs, 128 threads: thread q < 67 integrates output q in the reference's summation order; thread 67 writes jcum.
__global__ __launch_bounds__(128) void k_exchange_integrate(int nen, int nv1, const double* __restrict__ ene, const double* __restrict__ fw,
                                                            const double* __restrict__ integ, int col0, double* __restrict__ xc, double* __restrict__ so,
                                                            double* __restrict__ fo, double* __restrict__ parts, double* __restrict__ jcum, int jcol0) {
#pragma clang fp contract(off)
    const int q = threadIdx.x, pair = blockIdx.x;
    const double* R = integ + (size_t)pair * nen * XC_NINT;
    const double H = ene[1] - ene[0];
    const double pi = 3.14159265358979323846;
    const int itop = nv1 + 9;                                       // last I (1-based) of the loop
    auto y = [&](int k) -> double { return k < nen ? xc_quantity(R + (size_t)k * XC_NINT, q < XC_NOUT ? q : 13) : 0.0; };
    if (q < XC_NOUT) {
        const double A = xc_simpson_fermi(nen, nv1, H, fw, y);
        const int col = col0 + pair;
        if (q < 13) xc[13 * col + q] = A * 1.0e3 / 4.0 / pi;
        else if (q < 26) so[13 * col + q - 13] = A * 1.0e3 / 4.0 / pi;
        else if (q < 39) fo[13 * col + q - 26] = A * 1.0e3 / 4.0 / pi;
        else {
            const int r = q - 39;
            parts[28 * col + r] = (r >= 4 && r < 10) ? A * 2.0e3 / 4.0 / pi : A * 1.0e3 / 4.0 / pi;
        }
    } else if (q == XC_NOUT && jcum) {
        // Ef = ene(nv): the weights are 1 below nv, 0.5 at nv, 0 above (ene is strictly increasing on a grid far coarser than kBT).
        // The triples entirely below nv are summed once, in order; the (at most two) triples that touch nv are added per point.
        const int ntrip = itop / 2;
        double Afull = 0.0;
        int tfull = 0;                                              // triples summed into Afull (triple t covers 0-based 2t-2 .. 2t)
        for (int n = 0; n < nen; ++n) {
            while (tfull < ntrip && 2 * (tfull + 1) < n) {
                const int k = 2 * (tfull + 1) - 1;
                Afull = ((Afull + y(k - 1)) + 4.0 * y(k)) + y(k + 1);
                ++tfull;
            }
            double A = Afull;
            for (int tt = tfull + 1; tt <= ntrip && 2 * tt - 2 <= n; ++tt) {
                const int k = 2 * tt - 1;
                auto w = [&](int i) { return i < n ? 1.0 : (i == n ? 0.5 : 0.0); };
                A = ((A + y(k - 1) * w(k - 1)) + 4.0 * y(k) * w(k)) + y(k + 1) * w(k + 1);
            }
            A = H * A / 3.0;
            jcum[(size_t)(jcol0 + pair) * nen + n] = A * 1.0e3 / 4.0 / pi;
        }
    }
}

// ---- Gilbert damping (torque correlation): exchange%calculate_gilbert_damping (exchange.f90:674-694) on the same g0 ----
//   Aij = gij - gji^H,  Aji = gji - gij^H,  X_k = T_i^k Aij,  Y_l = (T_j^l)^H Aji,  row m = 3 k + l:  Tr(X_k Y_l) = sum_ab X_k(a,b) Y_l(b,a)
// with the dense 18 x 18 torque matrices of the two atoms' types.  The product X_k Y_l (the reference's temp3) is never formed.
// Rows per (pair, energy): 0..8 the real parts (dtott, l fastest), 9..17 the imaginary parts (dtottim).
constexpr int DP_NROW = 18;
constexpr int DP_TMAT = 6 * BLK;      // complex elements of tmat per pair: (18, 18, 3, side)

struct DampShared {
    double2 rows[9 * NB];             // row sums of the nine traces, [m][a]
};

// Workgroup epilogue (256 threads), every sum in a fixed order; no FMA contraction.  M(w), S(w) as in xc_epilogue: both are overwritten
// (gij, gji -> S(0), S(1);  Aij, Aji -> M(0), M(1);  X_1..3 -> S(0..2);  Y_1..3 -> S(3), M(2), M(3)).  tm: (18, 18, 3, 2) of the pair.
__device__ __forceinline__ void damping_epilogue(double2* Mb, double2* Sb, int stride, DampShared& ds, bool same, const double2* __restrict__ tm,
                                                 double* __restrict__ out) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
#pragma unroll 1
    for (int it = t; it < 2 * BLK; it += 256) {
        const int side = it / BLK, el = it % BLK;
        Sb[side * stride + el] = xc_gpair(Mb, stride, same, side, el);
    }
    __syncthreads();
#pragma unroll 1
    for (int it = t; it < 2 * BLK; it += 256) {                        // A(r,c) = G(r,c) - conjg(G'(c,r))
        const int side = it / BLK, el = it % BLK, r = el % NB, c = el / NB;
        const double2 g = Sb[side * stride + el], o = Sb[(1 - side) * stride + c + NB * r];
        Mb[side * stride + el] = make_double2(g.x - o.x, g.y - (-o.y));
    }
    __syncthreads();
#pragma unroll 1
    for (int it = t; it < 6 * BLK; it += 256) {
        const int q = it / BLK, el = it % BLK, r = el % NB, c = el / NB, side = q / 3;
        const double2* T = tm + (size_t)q * BLK;
        const double2* A = Mb + side * stride + NB * c;
        double sr = 0.0, si = 0.0;
        for (int b = 0; b < NB; ++b) {
            double2 x = side == 0 ? T[r + NB * b] : T[b + NB * r];
            if (side) x.y = -x.y;                                      // transpose(conjg(tmatj))
            const double2 y = A[b];
            sr += x.x * y.x - x.y * y.y;
            si += x.x * y.y + x.y * y.x;
        }
        (q < 4 ? Sb + q * stride : Mb + (q - 2) * stride)[el] = make_double2(sr, si);
    }
    __syncthreads();
#pragma unroll 1
    for (int it = t; it < 9 * NB; it += 256) {
        const int m = it / NB, a = it % NB, k = m / 3, l = m % 3;
        const double2* X = Sb + k * stride;
        const double2* Y = (l == 0 ? Sb + 3 * stride : Mb + (l + 1) * stride) + NB * a;
        double sr = 0.0, si = 0.0;
        for (int b = 0; b < NB; ++b) {
            const double2 x = X[a + NB * b], y = Y[b];
            sr += x.x * y.x - x.y * y.y;
            si += x.x * y.y + x.y * y.x;
        }
        ds.rows[it] = make_double2(sr, si);
    }
    __syncthreads();
    if (t < 9) {
        double sr = 0.0, si = 0.0;
        for (int a = 0; a < NB; ++a) { sr += ds.rows[t * NB + a].x; si += ds.rows[t * NB + a].y; }
        out[t] = sr;
        out[9 + t] = si;
    }
}

// The exchange kernels' grid and Green stage, the damping epilogue.  tmat: [pair][side][k][18 x 18]; rows: [pair][nen][18].
__global__ __launch_bounds__(256, GREEN_WAVES_PER_SIMD) void k_damping_block(int lld, int nen, const double* __restrict__ ene, int sym_term,
                                                                          const double* __restrict__ a_inf, const double* __restrict__ b_inf,
                                                                          const double2* __restrict__ a_b, const double2* __restrict__ b_sqrt,
                                                                          const int* __restrict__ same, const int* __restrict__ cbase, int cb0,
                                                                          const double2* __restrict__ tmat, double* __restrict__ rows) {
    __shared__ GreenLds lds[4];
    __shared__ DampShared ds;
    const int ie = blockIdx.x, pair = blockIdx.y;
    pair_green_block(lds, same[pair] != 0, ene[ie], cbase[pair] - cb0, lld, sym_term, a_inf, b_inf, a_b, b_sqrt);
    damping_epilogue(lds[0].M, lds[0].B, PAIR_BLOCK_STRIDE, ds, same[pair] != 0, tmat + (size_t)DP_TMAT * pair, rows + ((size_t)pair * nen + ie) * DP_NROW);
}

__global__ __launch_bounds__(256) void k_damping_cheb(int nm, int nen, const double* __restrict__ ene, double a, double b, const double* __restrict__ kern,
                                                     const double2* __restrict__ mu, const int* __restrict__ same, const int* __restrict__ cbase, int cb0,
                                                     const double2* __restrict__ tmat, double* __restrict__ rows) {
    extern __shared__ double2 ef[];
    __shared__ XcChebLds cl;
    __shared__ DampShared ds;
    const int ie = blockIdx.x, pair = blockIdx.y;
    const bool sm = same[pair] != 0;
    pair_green_cheb(cl, ef, nm, ene[ie], a, b, kern, mu + (size_t)(cbase[pair] - cb0) * nm * BLK, sm);
    damping_epilogue(&cl.g[0][0], &cl.s[0][0], BLK, ds, sm, tmat + (size_t)DP_TMAT * pair, rows + ((size_t)pair * nen + ie) * DP_NROW);
}

// The two reductions the reference prints, for the np pairs of a chunk: total(m, ie) += dtott(m, ie) of the pairs in ascending order
// (exchange.f90:690-694; the running value carries over from the chunk before, so the sum does not depend on the chunking), and the 18
// rows of every pair at energy index ief0 (0-based) into column col0 + pair of the image.  One thread per output, no atomics.
__global__ __launch_bounds__(256) void k_damping_reduce(int nen, int np, int ief0, const double* __restrict__ rows, int col0, double* __restrict__ at_ef,
                                                        double* __restrict__ total) {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n1 = (size_t)9 * nen, n2 = (size_t)DP_NROW * np;
    if (i < n1) {
        const int m = (int)(i % 9);
        const size_t ie = i / 9;
        double s = total[i];
        for (int p = 0; p < np; ++p) s += rows[((size_t)p * nen + ie) * DP_NROW + m];
        total[i] = s;
    } else if (i < n1 + n2) {
        const size_t j = i - n1, p = j / DP_NROW, m = j % DP_NROW;
        at_ef[(size_t)(col0 + p) * DP_NROW + m] = rows[(p * nen + ief0) * DP_NROW + m];
    }
}
}  // namespace rsrec
