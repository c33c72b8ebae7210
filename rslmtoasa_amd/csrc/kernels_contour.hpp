// The Gauss-Legendre contour stages at the Fermi level: green%calculate_intersite_gf_eta (green.f90:471-536) with
// exchange%calculate_exchange_gauss_legendre (exchange.f90:1804-1865), and the occupations of bands%calculate_moments_gauss_legendre /
// calculate_occupation_gauss_legendre (bands.f90:559-586, :631-650).
//
// Point k of the contour is the complex energy z_k = e0 + i eta_k, eta_k = (1 - x_k) / x_k (rounded to single precision on the host, as the
// reference's cmplx() without a KIND rounds it), and carries the factor w_k / (x_k x_k), applied
// as the reference applies it: (value * w) / (x * x).  The grid runs over (point, pair) or (point, site); g of a pair's chains stays in LDS
// (the Green stages are those of kernels_exchange.hpp / kernels_green.hpp with eta from a per-point table).
//
// Exchange: dmat = real(ee(1:9,1:9) - ee(10:18,10:18)) of the two atoms is a DENSE 9 x 9 matrix, so the T(A, B) shortcut of xc_epilogue does
// not apply.  With P_m = D_i G_im and Q_m = D_j G_jm (m = 0 nmag, 1 x, 2 y, 3 z: eight 9 x 9 x 9 products) and the 16 traces
//     T(a, b) = Tr(P_a Q_b)
// the 13 values of a (pair, point) are, by the cyclic property of the trace,
//     row 0       Re (T(0,0) - T(1,1) - T(2,2) - T(3,3))              rtrace9  of dGdG_Jnc          (exchange.f90:933-959)
//     row k       Im (T(0,k) - T(k,0)),  k = 1..3                     imtrace9 of dGdG_Dnc(:,:,k)   (:961-990)
//     row 4+k+3l  Re (T(1+k,1+l) + T(1+l,1+k)) / 2,  k, l = 0..2      rtrace9  of dGdG_Anc(:,:,k,l) (:992-1026)
// each times the point's factor.  Then per pair the points are summed in ascending order: jij = -sum, dmi = +sum, aij = -sum, each
// * 1.0d3 / 4 / pi (= T_comm_xc).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_exchange.hpp"

namespace rsrec {

constexpr int CT_NROW = 13;     // values per (pair, point), T_comm_xc's order
constexpr int CT_NTR = 16;      // traces per (pair, point)
constexpr int CT_DMAT = 162;    // doubles of dmat per pair: (9, 9, side)

struct ContourShared {
    double2 rows[CT_NTR * 9];   // row sums of the traces, [trace][r]
    double2 tr[CT_NTR];
    double d[2][81];            // D_i, D_j, column-major
};

// principal square root of a complex number
__device__ __forceinline__ double2 csqrt_d(double2 z) {
    const double m = hypot(z.x, z.y);
    if (m == 0.0) return make_double2(0.0, 0.0);
    const double t = sqrt(0.5 * (m + fabs(z.x))), o = 0.5 * z.y / t;
    return z.x >= 0.0 ? make_double2(t, o) : make_double2(fabs(o), copysign(t, z.y));
}
__device__ __forceinline__ double2 cdiv_d(double2 a, double2 b) {
    const double den = b.x * b.x + b.y * b.y;
    return make_double2((a.x * b.x + a.y * b.y) / den, (a.y * b.x - a.x * b.y) / den);
}

// theta = acos(z) for complex z and the denominator sqrt(a^2 - (e0 + i eta - b)^2) of chebyshev_green_eta / _ij_eta (green.f90:1006-1015,
// :1169-1178).  exp(-i theta) = z - i sqrt(1 - z^2) cancels where |z| is large (eta reaches thousands at the first nodes), so it is formed as
// the reciprocal of z + i sqrt(1 - z^2) whenever that one is the larger of the two (their product is 1); theta = i log(exp(-i theta)).
__device__ __forceinline__ void contour_cheb_point(double e0, double eta, double a, double b, double2& theta, double2& den) {
    const double2 wv = make_double2(e0 - b, eta), z = make_double2(wv.x / a, wv.y / a);
    const double2 s = csqrt_d(make_double2(1.0 - (z.x * z.x - z.y * z.y), -2.0 * z.x * z.y));
    const double2 up = make_double2(z.x - s.y, z.y + s.x), um = make_double2(z.x + s.y, z.y - s.x);     // z + i s,  z - i s
    double2 u = um;
    if (up.x * up.x + up.y * up.y > um.x * um.x + um.y * um.y) u = cdiv_d(make_double2(1.0, 0.0), up);
    theta = make_double2(-atan2(u.y, u.x), log(hypot(u.x, u.y)));
    den = csqrt_d(make_double2(a * a - (wv.x * wv.x - wv.y * wv.y), -2.0 * wv.x * wv.y));
}
// -i exp(-i i theta) k for moment i (0-based), theta complex: k exp(i Im theta) (-sin(i Re theta), -cos(i Re theta))
__device__ __forceinline__ double2 contour_cheb_phase(int i, double2 theta, double k) {
    const double xr = (double)i * theta.x, m = exp((double)i * theta.y) * k;
    return make_double2(-sin(xr) * m, -cos(xr) * m);
}
// one element of g at the point: sum_i mu(el, i) ef(i), i ascending, / den
__device__ __forceinline__ double2 contour_cheb_elem(const double2* __restrict__ m, size_t mstride, const double2* ef, int nm, double2 den) {
    double sr = 0.0, si = 0.0;
    for (int i = 0; i < nm; ++i) {
        const double2 v = m[(size_t)i * mstride], f = ef[i];
        sr += v.x * f.x - v.y * f.y;
        si += v.x * f.y + v.y * f.x;
    }
    return cdiv_d(make_double2(sr, si), den);
}

// Workgroup epilogue (256 threads) on g of the pair's chains, M(w) = Mb + w * stride (column-major 18 x 18), S(w) = Sb + w * stride free
// scratch; both are overwritten.  No FMA contraction in the elementwise arithmetic; every sum in a fixed order.  dm: (9, 9, 2) of the pair.
__device__ __forceinline__ void contour_epilogue(double2* Mb, double2* Sb, int stride, ContourShared& cs, bool same, double x, double w,
                                                 const double* __restrict__ dm, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    if (t < CT_DMAT) cs.d[t / 81][t % 81] = dm[t];
    // gij / gji (green.f90:517-521) and the 8 Pauli parts (:524-532): part k at S(k / 4) + 81 (k % 4), element (j, i) at j + 9 i
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
        else if (comp == 2) p = make_double2(0.5 * ((-v[2].y) - (-v[3].y)), 0.5 * (v[2].x - v[3].x));   // i g(j,i+9) - i g(j+9,i)
        else p = make_double2(0.5 * (v[2].x + v[3].x), 0.5 * (v[2].y + v[3].y));
        Sb[(k >> 2) * stride + 81 * (k & 3) + el] = p;
    }
    __syncthreads();
    // P_m = D_i G_im (k = m), Q_m = D_j G_jm (k = 4 + m): product k at M(k / 4) + 81 (k % 4); the sum over the inner index in order
#pragma unroll 1
    for (int it = t; it < 8 * 81; it += 256) {
        const int k = it / 81, el = it % 81, r = el % 9, c = el / 9;
        const double* D = cs.d[k >> 2];
        const double2* G = Sb + (k >> 2) * stride + 81 * (k & 3) + 9 * c;
        double sr = 0.0, si = 0.0;
        for (int b = 0; b < 9; ++b) {
            const double d = D[r + 9 * b];
            const double2 g = G[b];
            sr += d * g.x;
            si += d * g.y;
        }
        Mb[(k >> 2) * stride + 81 * (k & 3) + el] = make_double2(sr, si);
    }
    __syncthreads();
    // row r of trace (a, b): sum_c P_a(r, c) Q_b(c, r), c in order
    if (t < CT_NTR * 9) {
        const int tr = t / 9, r = t % 9, a = tr >> 2, b = tr & 3;
        const double2* P = Mb + 81 * a;
        const double2* Q = Mb + stride + 81 * b;
        double sr = 0.0, si = 0.0;
        for (int c = 0; c < 9; ++c) {
            const double2 p = P[r + 9 * c], q = Q[c + 9 * r];
            sr += p.x * q.x - p.y * q.y;
            si += p.x * q.y + p.y * q.x;
        }
        cs.rows[t] = make_double2(sr, si);
    }
    __syncthreads();
    if (t < CT_NTR) {
        double sr = 0.0, si = 0.0;
        for (int r = 0; r < 9; ++r) { sr += cs.rows[t * 9 + r].x; si += cs.rows[t * 9 + r].y; }
        cs.tr[t] = make_double2(sr, si);
    }
    __syncthreads();
    if (t < CT_NROW) {
        const double2* T = cs.tr;
        double v;
        if (t == 0) v = ((T[0].x - T[5].x) - T[10].x) - T[15].x;
        else if (t < 4) v = T[t].y - T[4 * t].y;
        else { const int k = 1 + (t - 4) % 3, l = 1 + (t - 4) / 3; v = 0.5 * (T[4 * k + l].x + T[4 * l + k].x); }
        out[t] = (v * w) / (x * x);
    }
}

// kind 0.  grid = (npts, npairs), 256 threads: wave c runs chain c of the pair through green%bgreen at ene(fermi_point) with the point's eta
// (block_green_ij_eta; the terminators are those of the chains, computed once per chain); an i == j pair runs chain 1 only.
// eta, x, w: [npts]; dmat: [pair][162]; rows: [pair][npts][13].  The chain addressing is k_exchange_block's.
__global__ __launch_bounds__(256, GREEN_WAVES_PER_SIMD) void k_contour_xc_block(int lld, int npts, double e0, const double* __restrict__ eta,
                                                                             const double* __restrict__ x, const double* __restrict__ w, int sym_term,
                                                                             const double* __restrict__ a_inf, const double* __restrict__ b_inf,
                                                                             const double2* __restrict__ a_b, const double2* __restrict__ b_sqrt,
                                                                             const int* __restrict__ same, const int* __restrict__ cbase, int cb0,
                                                                             const double* __restrict__ dmat, double* __restrict__ rows) {
    __shared__ GreenLds lds[4];
    __shared__ ContourShared cs;
    const int ip = blockIdx.x, pair = blockIdx.y;
    {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if (wave == 0 || same[pair] == 0) {
            const bool act = lane < 54;
            const int ig = act ? lane / 6 : 8, jg = act ? lane % 6 : 5;
            block_green_wave(lds[wave], lane, ig, jg, act, e0, cbase[pair] - cb0 + wave, lld, 0.0, eta[ip], sym_term, a_inf, b_inf, a_b, b_sqrt);
        }
        __syncthreads();
    }
    contour_epilogue(lds[0].M, lds[0].B, PAIR_BLOCK_STRIDE, cs, same[pair] != 0, x[ip], w[ip], dmat + (size_t)CT_DMAT * pair,
                     rows + ((size_t)pair * npts + ip) * CT_NROW);
}

// kind 1.  grid = (npts, npairs), 256 threads: all 324 elements of g of the pair's chains by chebyshev_green_ij_eta (green.f90:960-1023),
// into LDS, then the same epilogue.  mu: [chain][nm][324]; dynamic LDS: nm phase factors.
__global__ __launch_bounds__(256) void k_contour_xc_cheb(int nm, int npts, double e0, const double* __restrict__ eta, const double* __restrict__ x,
                                                        const double* __restrict__ w, double a, double b, const double* __restrict__ kern,
                                                        const double2* __restrict__ mu, const int* __restrict__ same, const int* __restrict__ cbase, int cb0,
                                                        const double* __restrict__ dmat, double* __restrict__ rows) {
    extern __shared__ double2 ef[];
    __shared__ XcChebLds cl;
    __shared__ ContourShared cs;
    const int ip = blockIdx.x, pair = blockIdx.y;
    const bool sm = same[pair] != 0;
    double2 theta, den;
    contour_cheb_point(e0, eta[ip], a, b, theta, den);
    for (int i = threadIdx.x; i < nm; i += blockDim.x) ef[i] = contour_cheb_phase(i, theta, kern[i]);
    __syncthreads();
    const double2* m = mu + (size_t)(cbase[pair] - cb0) * nm * BLK;
    const int nch = sm ? 1 : 4;
    for (int it = threadIdx.x; it < nch * BLK; it += blockDim.x) {
        const int c = it / BLK, el = it % BLK;
        cl.g[c][el] = contour_cheb_elem(m + (size_t)c * nm * BLK + el, BLK, ef, nm, den);
    }
    __syncthreads();
    contour_epilogue(&cl.g[0][0], &cl.s[0][0], BLK, cs, sm, x[ip], w[ip], dmat + (size_t)CT_DMAT * pair, rows + ((size_t)pair * npts + ip) * CT_NROW);
}

// The sum over the points, ascending, of every value of the np pairs of a chunk, with T_comm_xc's signs and scaling (exchange.f90:1848-1865).
// One thread per output, no atomics.
__global__ __launch_bounds__(256) void k_contour_xc_sum(int npts, int np, const double* __restrict__ rows, int col0, double* __restrict__ xc) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np * CT_NROW) return;
    const int p = i / CT_NROW, q = i % CT_NROW;
    const double pi = 3.14159265358979323846;
    double s = 0.0;
    for (int k = 0; k < npts; ++k) s += rows[((size_t)p * npts + k) * CT_NROW + q];
    if (q == 0 || q >= 4) s = -s;
    xc[(size_t)CT_NROW * (col0 + p) + q] = s * 1.0e3 / 4.0 / pi;
}

// ---- occupations: the diagonal of g of every on-site chain at every point, gd: [site][npts][18] ----

// kind 0 (block_green_eta, green.f90:544-581).  grid = (ceil(npts / GREEN_WAVES), nsites): one wave per (site, point), k_block_green's shape.
__global__ __launch_bounds__(GREEN_WAVES * 64, GREEN_WAVES_PER_SIMD) void k_contour_occ_block(int lld, int npts, double e0, const double* __restrict__ eta, int sym_term,
                                                                                           const double* __restrict__ a_inf, const double* __restrict__ b_inf,
                                                                                           const double2* __restrict__ a_b, const double2* __restrict__ b_sqrt,
                                                                                           double2* __restrict__ gd) {
    __shared__ GreenLds lds[GREEN_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ip = blockIdx.x * GREEN_WAVES + wave, site = blockIdx.y;
    if (ip >= npts) return;                                      // wave-uniform; no workgroup barriers below
    GreenLds& L = lds[wave];
    const bool act = lane < 54;
    const int ig = act ? lane / 6 : 8, jg = act ? lane % 6 : 5;
    block_green_wave(L, lane, ig, jg, act, e0, site, lld, 0.0, eta[ip], sym_term, a_inf, b_inf, a_b, b_sqrt);
    if (lane < NB) gd[((size_t)site * npts + ip) * NB + lane] = L.M[lane * (NB + 1)];
}

// kind 1 (chebyshev_green_eta, green.f90:1116-1184): the diagonal only -- the reference refreshes only mu_ng(i,i,..) there.
// grid = (npts, nsites), 64 threads; dynamic LDS: nm phase factors.
__global__ __launch_bounds__(64) void k_contour_occ_cheb(int nm, int npts, double e0, const double* __restrict__ eta, double a, double b,
                                                        const double* __restrict__ kern, const double2* __restrict__ mu, double2* __restrict__ gd) {
    extern __shared__ double2 ef[];
    const int ip = blockIdx.x, site = blockIdx.y;
    double2 theta, den;
    contour_cheb_point(e0, eta[ip], a, b, theta, den);
    for (int i = threadIdx.x; i < nm; i += blockDim.x) ef[i] = contour_cheb_phase(i, theta, kern[i]);
    __syncthreads();
    const int j = threadIdx.x;
    if (j < NB) gd[((size_t)site * npts + ip) * NB + j] = contour_cheb_elem(mu + (size_t)site * nm * BLK + j * (NB + 1), BLK, ef, nm, den);
}

// occ(i, site) = sum_k ((Re g_ii(z_k) w_k) / (x_k x_k)) / pi + 0.5, k ascending (bands.f90:572-585).  One thread per output.
__global__ __launch_bounds__(256) void k_contour_occ_sum(int npts, int ns, const double* __restrict__ x, const double* __restrict__ w,
                                                        const double2* __restrict__ gd, int col0, double* __restrict__ occ) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns * NB) return;
    const int s = i / NB, j = i % NB;
    const double pi = 3.14159265358979323846;
    double o = 0.0;
    for (int k = 0; k < npts; ++k) {
        const double y = (gd[((size_t)s * npts + k) * NB + j].x * w[k]) / (x[k] * x[k]);
        o = o + y / pi;
    }
    occ[(size_t)NB * (col0 + s) + j] = o + 0.5;
}
}  // namespace rsrec
