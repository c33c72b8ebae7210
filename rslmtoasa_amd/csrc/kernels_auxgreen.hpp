// Exchange tensors in the auxiliary Green-function formalism and the spin-lattice coupling of atom trios:
// exchange%calculate_jij_auxgreen (exchange.f90:171-335) and exchange%calculate_jijk (exchange.f90:338-601), as two more epilogues on g0 of
// a pair's chains in LDS (kernels_exchange.hpp: pair_green_block / pair_green_cheb, xc_gpair).
//
// Everything that dresses gij / gji is diagonal, so it is a row and column scaling done while the 9 x 9 up-up and down-down blocks leave
// g0 (the only two spin blocks either routine reads):
//     aux  = diag(dele_i) g diag(dele_j)                                            (green%auxiliary_gij, green.f90:758-808)
//     aux0 = diag(P_i / P0_i) aux diag(P_j / P0_j)  [+ diag((0 - qpar) P / P0) when the two atoms are the same atom]
//                                                                                   (green%transform_auxiliary_gij, green.f90:821-885)
//     P(l, s, e) = (e - (c + vmad)) / dele^2                                        (p_matrix, symbolic_atom.f90:401-430)
//     P0 = P / (1 + (qpar - 0) P)                                                   (transform_pmatrix, symbolic_atom.f90:442-472)
// The reference forms c + vmad, dele, qpar and THE ENERGY with cmplx(x, 0.0_rp) without a KIND: default (single-precision) complex, so
// all four pass through float before the double arithmetic, as c + vmad and dele do in xc_epilogue's d_matrix.  (The compiled reference
// rounds all four: tests/golden/aux_jijk_block.npz is met to 9e-15 with the roundings and missed by 3e-9 or more without the energy's.)  The
// Green function itself is taken at the unrounded energy.  All diagonals are real; the angle weights of exchange.f90:187-234 keep
// cos(pi / 2) = 6.1e-17 as the reference's table has it.
//
// Rows per (pair, energy) of Jij_aux: the 9 tensor components xx, xy, .. zz (imtrace * 0.5), or J00 in row 0 and zeros for an i == j pair
// (imtrace * (-1)).  Rows per (trio, energy) of Jijk: the 9 components (imtrace * 0.5).  The traces are taken before the angle weights
// (the reference weights the matrices, then takes the trace): the same terms in the same order, summed over the orbitals first.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_exchange.hpp"

namespace rsrec {

constexpr int AX_NROW = 9;        // rows per (pair, energy) and per (trio, energy)
constexpr int AX_APAR = 12;       // aux: (c + vmad, dele) x l x spin per side
constexpr int JK_APAR = 18;       // Jijk: (c + vmad, dele, qpar) x l x spin per atom
constexpr int JK_KEEP = 6;        // dressed blocks of a trio that outlive their pair's g0: gki (2), gjk (2), gkj (2)

// the diagonals of one atom, per spin and l
struct AuxDiag {
    double dele[2][3], p[2][3];   // sqrt(Delta) and P, orthogonal representation
    double r[2][3], p0[2][3], add[2][3];   // P / P0, P0 and (0 - qpar) P / P0, canonical representation (Jijk only)
};

__device__ __forceinline__ int ax_l(int a) { return a == 0 ? 0 : (a < 4 ? 1 : 2); }

// q: (c + vmad, dele[, qpar]) of one (l, spin); nq = 2 or 3
__device__ __forceinline__ void ax_diag(AuxDiag& d, int s, int l, const double* __restrict__ q, int nq, double e) {
#pragma clang fp contract(off)
    const double cv = (double)(float)q[0], w = (double)(float)q[1], ef = (double)(float)e;
    const double p = (ef - cv) / (w * w);
    d.dele[s][l] = w;
    d.p[s][l] = p;
    if (nq == 3) {
        const double g = (double)(float)q[2];
        const double p0 = p / (1.0 + (g - 0.0) * p);
        const double r = p / p0;
        d.p0[s][l] = p0;
        d.r[s][l] = r;
        d.add[s][l] = (0.0 - g) * r;
    }
}

// angle weights of component m = 0..8 (xx, xy, xz, yx, .. zz): cc = cos t cos t', w2 = sin t sin t' exp(i (phi' - phi)), w3 = its
// counterpart with exp(i (phi - phi')); t = pi/2 for x and y, 0 for z; phi = pi/2 for y, 0 otherwise
__device__ __forceinline__ void ax_weights(int m, double& cc, double2& w2, double2& w3) {
#pragma clang fp contract(off)
    const double ch = 6.123233995736766e-17;                     // cos(0.5 pi) in double
    const int a = m / 3, b = m % 3;
    const double ct = a == 2 ? 1.0 : ch, st = a == 2 ? 0.0 : 1.0, ctp = b == 2 ? 1.0 : ch, stp = b == 2 ? 0.0 : 1.0;
    const int dphi = (b == 1) - (a == 1);                        // (phi' - phi) / (pi / 2)
    cc = ct * ctp;
    const double ss = st * stp;
    const double er = dphi == 0 ? 1.0 : ch, ei = (double)dphi;    // exp(i (phi' - phi))
    w2 = make_double2(ss * er, ss * ei);
    w3 = make_double2(ss * er, ss * (-ei));
}

__device__ __forceinline__ double2 ax_cmul(double2 x, double2 y) {
#pragma clang fp contract(off)
    return make_double2(x.x * y.x - x.y * y.y, x.x * y.y + x.y * y.x);
}

// row a of Tr(A B) for 9 x 9 column-major A, B: sum_b A(a,b) B(b,a), b in order
__device__ __forceinline__ double2 ax_trace_row(const double2* A, const double2* B, int a) {
#pragma clang fp contract(off)
    double sr = 0.0, si = 0.0;
    for (int b = 0; b < 9; ++b) {
        const double2 x = A[a + 9 * b], y = B[b + 9 * a];
        sr += x.x * y.x - x.y * y.y;
        si += x.x * y.y + x.y * y.x;
    }
    return make_double2(sr, si);
}

// element (a, b) of the 9 x 9 product A B, the inner index in order
__device__ __forceinline__ double2 ax_matmul_el(const double2* A, const double2* B, int a, int b) {
#pragma clang fp contract(off)
    double sr = 0.0, si = 0.0;
    for (int c = 0; c < 9; ++c) {
        const double2 x = A[a + 9 * c], y = B[c + 9 * b];
        sr += x.x * y.x - x.y * y.y;
        si += x.x * y.y + x.y * y.x;
    }
    return make_double2(sr, si);
}

// ---- Jij_aux ----
struct AuxShared {
    AuxDiag d[2];                 // side i, side j
    double2 rows[4 * 9];
    double2 tr[4];
};

// Workgroup epilogue (256 threads), no FMA contraction.  M(w) = Mb + w * stride holds g0 of chain w; Sb is free scratch of 324 complex.
// apar: (2, 3, 2, 2) of the pair; out: the 9 rows of this (pair, energy).
__device__ __forceinline__ void aux_epilogue(const double2* Mb, double2* Sb, int stride, AuxShared& as, bool same, double e, const double* __restrict__ apar,
                                             double* __restrict__ out) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    if (t < 12) {
        const int side = t / 6, s = (t / 3) % 2, l = t % 3;
        ax_diag(as.d[side], s, l, apar + 2 * (l + 3 * (s + 2 * side)), 2, e);
    }
    __syncthreads();
    // temp1 = dP_i aux_gij_uu, temp3 = dP_i aux_gij_dd, temp4 = dP_j aux_gji_uu, temp2 = dP_j aux_gji_dd at Sb + 81 {0, 1, 2, 3};
    // an i == j pair: temp1, -, -, temp2, and temp3 = dP_i (aux_gij_uu - aux_gji_dd) at slot 1
    for (int it = t; it < 4 * 81; it += 256) {
        const int k = it / 81, el = it % 81, a = el % 9, b = el / 9, side = k >> 1, s = k & 1;
        const int la = ax_l(a), lb = ax_l(b);
        const AuxDiag &dr = as.d[side], &dc = as.d[1 - side];
        const double2 g = xc_gpair(Mb, stride, same, side, (a + 9 * s) + NB * (b + 9 * s));
        const double wc = dc.dele[s][lb], wr = dr.dele[s][la];
        const double2 x = make_double2(wr * (g.x * wc), wr * (g.y * wc));           // matmul(cdelta_i, matmul(g, cdelta_j))
        const double dp = dr.p[0][la] - dr.p[1][la];
        if (!same) Sb[it] = make_double2(dp * x.x, dp * x.y);
        else Sb[it] = x;                                                            // (dressed, not yet multiplied by dP)
    }
    __syncthreads();
    if (same) {
        // temp1 -> slot 0, temp2 -> slot 3, temp3 -> slot 1 (slot 2 is not read)
        double2 v0 = make_double2(0.0, 0.0), v3 = v0, v1 = v0;
        const int a = t % 9;
        const AuxDiag &di = as.d[0], &dj = as.d[1];
        const double dpi = di.p[0][ax_l(a)] - di.p[1][ax_l(a)], dpj = dj.p[0][ax_l(a)] - dj.p[1][ax_l(a)];
        if (t < 81) {
            const double2 uu = Sb[t], dd = Sb[3 * 81 + t];
            v0 = make_double2(dpi * uu.x, dpi * uu.y);
            v3 = make_double2(dpj * dd.x, dpj * dd.y);
            v1 = make_double2(dpi * (uu.x - dd.x), dpi * (uu.y - dd.y));
        }
        __syncthreads();
        if (t < 81) { Sb[t] = v0; Sb[3 * 81 + t] = v3; Sb[81 + t] = v1; }
        __syncthreads();
        if (t < 9) as.rows[t] = ax_trace_row(Sb, Sb + 3 * 81, t);                   // Tr(temp1 temp2)
        __syncthreads();
        if (t == 0) {
            double si = 0.0;
            // imtrace(matmul(temp1, temp2) + temp3), diagonal element by diagonal element
            for (int a2 = 0; a2 < 9; ++a2) si += as.rows[a2].y + Sb[81 + a2 + 9 * a2].y;
            out[0] = si * (-1.0);
        } else if (t < AX_NROW) out[t] = 0.0;
        return;
    }
    // traces 0: temp1 temp4, 1: temp3 temp4, 2: temp1 temp2, 3: temp3 temp2
    if (t < 36) {
        const int q = t / 9, a = t % 9;
        as.rows[t] = ax_trace_row(Sb + 81 * (q & 1), Sb + 81 * (q < 2 ? 2 : 3), a);
    }
    __syncthreads();
    if (t < 4) {
        double sr = 0.0, si = 0.0;
        for (int a = 0; a < 9; ++a) { sr += as.rows[t * 9 + a].x; si += as.rows[t * 9 + a].y; }
        as.tr[t] = make_double2(sr, si);
    }
    __syncthreads();
    if (t < AX_NROW) {
        double cc;
        double2 w2, w3;
        ax_weights(t, cc, w2, w3);
        const double2* T = as.tr;
        const double v = ((T[0].y * cc + ax_cmul(T[1], w2).y) + ax_cmul(T[2], w3).y) + T[3].y * cc;
        out[t] = v * 0.5;
    }
}

// The exchange kernels' grid and Green stage, the Jij_aux epilogue.  apar: [pair][24]; rows: [pair][nen][9].
__global__ __launch_bounds__(256, GREEN_WAVES_PER_SIMD) void k_aux_block(int lld, int nen, const double* __restrict__ ene, int sym_term,
                                                                      const double* __restrict__ a_inf, const double* __restrict__ b_inf,
                                                                      const double2* __restrict__ a_b, const double2* __restrict__ b_sqrt,
                                                                      const int* __restrict__ same, const int* __restrict__ cbase, int cb0,
                                                                      const double* __restrict__ apar, double* __restrict__ rows) {
    __shared__ GreenLds lds[4];
    __shared__ AuxShared as;
    const int ie = blockIdx.x, pair = blockIdx.y;
    pair_green_block(lds, same[pair] != 0, ene[ie], cbase[pair] - cb0, lld, sym_term, a_inf, b_inf, a_b, b_sqrt);
    aux_epilogue(lds[0].M, lds[0].B, PAIR_BLOCK_STRIDE, as, same[pair] != 0, ene[ie], apar + (size_t)2 * AX_APAR * pair,
                 rows + ((size_t)pair * nen + ie) * AX_NROW);
}

__global__ __launch_bounds__(256) void k_aux_cheb(int nm, int nen, const double* __restrict__ ene, double a, double b, const double* __restrict__ kern,
                                                 const double2* __restrict__ mu, const int* __restrict__ same, const int* __restrict__ cbase, int cb0,
                                                 const double* __restrict__ apar, double* __restrict__ rows) {
    extern __shared__ double2 ef[];
    __shared__ XcChebLds cl;
    __shared__ AuxShared as;
    const int ie = blockIdx.x, pair = blockIdx.y;
    const bool sm = same[pair] != 0;
    const double e = ene[ie];
    pair_green_cheb(cl, ef, nm, e, a, b, kern, mu + (size_t)(cbase[pair] - cb0) * nm * BLK, sm);
    aux_epilogue(&cl.g[0][0], &cl.s[0][0], BLK, as, sm, e, apar + (size_t)2 * AX_APAR * pair, rows + ((size_t)pair * nen + ie) * AX_NROW);
}

// ---- Jijk ----
// One workgroup per (trio, energy) runs the Green stage of the trio's three pairs one after another, in the order (i,k), (j,k), (i,j):
// of the 10 dressed blocks, the 6 of the first two pairs are kept in LDS (JK_KEEP x 81 complex), and the 4 of (i,j) go to the Green
// stage's own scratch once no pair is left to run.  gik is never formed.
struct JkShared {
    AuxDiag d[3];                 // atoms i, j, k
    double2 keep[JK_KEEP * 81];   // aux0 gki_uu, gki_dd;  dP_j aux0 gjk_uu (temp4), dP_j aux0 gjk_dd (temp9);  aux0 gkj_uu, gkj_dd
};

__device__ __forceinline__ void jk_diag(JkShared& js, double e, const double* __restrict__ apar) {
    const int t = threadIdx.x;
    if (t < 18) {
        const int atom = t / 6, s = (t / 3) % 2, l = t % 3;
        ax_diag(js.d[atom], s, l, apar + 3 * (l + 3 * (s + 2 * atom)), 3, e);
    }
    __syncthreads();
}

// Dressed block (side, spin s) of the pair whose g0 is in M: aux0 of g(ra, ca), multiplied from the left by dP0 of atom ra when `delta`.
__device__ __forceinline__ double2 jk_block_el(const double2* Mb, int stride, bool same, int side, int s, const AuxDiag& dr, const AuxDiag& dc, bool delta,
                                               int el) {
#pragma clang fp contract(off)
    const int a = el % 9, b = el / 9, la = ax_l(a), lb = ax_l(b);
    const double2 g = xc_gpair(Mb, stride, same, side, (a + 9 * s) + NB * (b + 9 * s));
    const double wc = dc.dele[s][lb], wr = dr.dele[s][la], rc = dc.r[s][lb], rr = dr.r[s][la];
    double2 x = make_double2(wr * (g.x * wc), wr * (g.y * wc));                    // auxiliary_gij
    x = make_double2(rr * (x.x * rc), rr * (x.y * rc));                             // transform_auxiliary_gij
    if (same && a == b) x.x = x.x + dr.add[s][la];
    if (delta) {
        const double dp = dr.p0[0][la] - dr.p0[1][la];
        x = make_double2(dp * x.x, dp * x.y);
    }
    return x;
}

// after the Green stage of pair q (0: (i,j), 1: (i,k), 2: (j,k)): what has to outlive g0 (q = 1, 2)
__device__ __forceinline__ void jk_keep(const double2* Mb, int stride, JkShared& js, bool same, int q) {
    const int t = threadIdx.x;
    if (q == 1) {
        for (int it = t; it < 2 * 81; it += 256) js.keep[it] = jk_block_el(Mb, stride, same, 1, it / 81, js.d[2], js.d[0], false, it % 81);          // gki
    } else {
        for (int it = t; it < 4 * 81; it += 256) {
            const int k = it / 81, side = k >> 1;
            js.keep[2 * 81 + it] = jk_block_el(Mb, stride, same, side, k & 1, js.d[side ? 2 : 1], js.d[side ? 1 : 2], side == 0, it % 81);           // gjk, gkj
        }
    }
    __syncthreads();
}

// With g0 of pair (i,j) in M: the rest of exchange.f90:530-550.  Sb(w) = Sb + w * stride: free scratch of 324 complex each; M is
// overwritten.  dmat: the 9 x 9 displacement matrix of the trio (one spin block of disp_matrix).
__device__ __forceinline__ void jk_finish(double2* Mb, double2* Sb, int stride, JkShared& js, bool same, const double2* __restrict__ dmat,
                                          double* __restrict__ out) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    double2* const T0 = Sb;                  // temp3, temp8 (dP_i gij_uu, _dd), temp7, temp10 (dP_j gji_uu, _dd)
    double2* const T1 = Sb + stride;         // temp2, temp1 (U_uu gki_uu, U_dd gki_dd), temp5, temp6 (U_uu gkj_uu, U_dd gkj_dd)
    double2* const T2 = Sb + 2 * stride;     // temp4 temp2, temp9 temp1, temp5 temp10, temp6 temp10
    double2* const T3 = Sb + 3 * stride;     // temp5 temp7, temp6 temp7
    for (int it = t; it < 4 * 81; it += 256) {
        const int k = it / 81, side = k >> 1;
        T0[it] = jk_block_el(Mb, stride, same, side, k & 1, js.d[side], js.d[1 - side], true, it % 81);
    }
    // U_k(a,c) = D(a,c) P0_k(c) + P0_k(a) D(c,a) per spin (udisp_matrix: matmul(dmat, pmat) + matmul(pmat, transpose(dmat)))
    for (int it = t; it < 4 * 81; it += 256) {
        const int k = it / 81, el = it % 81, a = el % 9, b = el / 9, s = k & 1;
        const double2* G = js.keep + (k < 2 ? 0 : 4 * 81) + 81 * s;
        const double pa = js.d[2].p0[s][ax_l(a)];
        double sr = 0.0, si = 0.0;
        for (int c = 0; c < 9; ++c) {
            const double2 d1 = dmat[a + 9 * c], d2 = dmat[c + 9 * a], y = G[c + 9 * b];
            const double pc = js.d[2].p0[s][ax_l(c)];
            const double2 u = make_double2(d1.x * pc + pa * d2.x, d1.y * pc + pa * d2.y);
            sr += u.x * y.x - u.y * y.y;
            si += u.x * y.y + u.y * y.x;
        }
        T1[it] = make_double2(sr, si);
    }
    __syncthreads();
    for (int it = t; it < 6 * 81; it += 256) {
        const int k = it / 81, el = it % 81, a = el % 9, b = el / 9;
        const double2 *A, *B;
        if (k == 0) { A = js.keep + 2 * 81; B = T1; }                   // temp4 temp2
        else if (k == 1) { A = js.keep + 3 * 81; B = T1 + 81; }         // temp9 temp1
        else if (k == 2) { A = T1 + 2 * 81; B = T0 + 3 * 81; }          // temp5 temp10
        else if (k == 3) { A = T1 + 3 * 81; B = T0 + 3 * 81; }          // temp6 temp10
        else if (k == 4) { A = T1 + 2 * 81; B = T0 + 2 * 81; }          // temp5 temp7
        else { A = T1 + 3 * 81; B = T0 + 2 * 81; }                      // temp6 temp7
        (k < 4 ? T2 + 81 * k : T3 + 81 * (k - 4))[el] = ax_matmul_el(A, B, a, b);
    }
    __syncthreads();
    // the 8 terms of :542-549 in their order: (left factor, inner product) = (3, 42) (8, 42) (3, 91) (8, 91) (3, 5.10) (8, 6.10) (3, 57) (8, 67)
    double2* const rows = Mb;                // (g0 of (i,j) has been read)
    if (t < 72) {
        const int q = t / 9, a = t % 9;
        const int inner = q < 2 ? 0 : (q < 4 ? 1 : (q == 4 ? 2 : (q == 5 ? 3 : (q == 6 ? 4 : 5))));
        rows[t] = ax_trace_row(T0 + 81 * (q & 1), inner < 4 ? T2 + 81 * inner : T3 + 81 * (inner - 4), a);
    }
    __syncthreads();
    if (t < 8) {
        double sr = 0.0, si = 0.0;
        for (int a = 0; a < 9; ++a) { sr += rows[t * 9 + a].x; si += rows[t * 9 + a].y; }
        rows[72 + t] = make_double2(sr, si);
    }
    __syncthreads();
    if (t < AX_NROW) {
        double cc;
        double2 w2, w3;
        ax_weights(t, cc, w2, w3);
        const double2* T = rows + 72;
        const double v = ((((((T[0].y * cc + ax_cmul(T[1], w2).y) + ax_cmul(T[2], w3).y) + T[3].y * cc) + ax_cmul(T[4], w3).y) + T[5].y * cc) + T[6].y * cc) +
                         ax_cmul(T[7], w2).y;
        out[t] = v * 0.5;
    }
}

// the order the pairs of a trio are run in: (i,k), (j,k), then (i,j), whose g0 jk_finish reads in place
__device__ __forceinline__ int jk_order(int step) { return step == 2 ? 0 : step + 1; }

// grid = (nen, ntrios), 256 threads.  same, cbase: of the pairs (3 per trio); apar: [trio][54]; dmat: [trio][81]; rows: [trio][nen][9].
__global__ __launch_bounds__(256, GREEN_WAVES_PER_SIMD) void k_jijk_block(int lld, int nen, const double* __restrict__ ene, int sym_term,
                                                                       const double* __restrict__ a_inf, const double* __restrict__ b_inf,
                                                                       const double2* __restrict__ a_b, const double2* __restrict__ b_sqrt,
                                                                       const int* __restrict__ same, const int* __restrict__ cbase, int cb0,
                                                                       const double* __restrict__ apar, const double2* __restrict__ dmat,
                                                                       double* __restrict__ rows) {
    __shared__ GreenLds lds[4];
    __shared__ JkShared js;
    const int ie = blockIdx.x, trio = blockIdx.y;
    jk_diag(js, ene[ie], apar + (size_t)3 * JK_APAR * trio);
#pragma unroll 1
    for (int step = 0; step < 3; ++step) {
        const int q = jk_order(step), pair = 3 * trio + q;
        pair_green_block(lds, same[pair] != 0, ene[ie], cbase[pair] - cb0, lld, sym_term, a_inf, b_inf, a_b, b_sqrt);
        if (q) jk_keep(lds[0].M, PAIR_BLOCK_STRIDE, js, same[pair] != 0, q);
    }
    jk_finish(lds[0].M, lds[0].B, PAIR_BLOCK_STRIDE, js, same[3 * trio] != 0, dmat + (size_t)81 * trio, rows + ((size_t)trio * nen + ie) * AX_NROW);
}

__global__ __launch_bounds__(256) void k_jijk_cheb(int nm, int nen, const double* __restrict__ ene, double a, double b, const double* __restrict__ kern,
                                                  const double2* __restrict__ mu, const int* __restrict__ same, const int* __restrict__ cbase, int cb0,
                                                  const double* __restrict__ apar, const double2* __restrict__ dmat, double* __restrict__ rows) {
    extern __shared__ double2 ef[];
    __shared__ XcChebLds cl;
    __shared__ JkShared js;
    const int ie = blockIdx.x, trio = blockIdx.y;
    const double e = ene[ie];
    jk_diag(js, e, apar + (size_t)3 * JK_APAR * trio);
#pragma unroll 1
    for (int step = 0; step < 3; ++step) {
        const int q = jk_order(step), pair = 3 * trio + q;
        const bool sm = same[pair] != 0;
        pair_green_cheb(cl, ef, nm, e, a, b, kern, mu + (size_t)(cbase[pair] - cb0) * nm * BLK, sm);
        if (q) jk_keep(&cl.g[0][0], BLK, js, sm, q);
    }
    jk_finish(&cl.g[0][0], &cl.s[0][0], BLK, js, same[3 * trio] != 0, dmat + (size_t)81 * trio, rows + ((size_t)trio * nen + ie) * AX_NROW);
}

// simpson_f(fermi = .true., T = 0) of the nrow rows of every unit (pair or trio) of a chunk, unscaled: k_exchange_integrate's rule
// (xc_simpson_fermi) on rows [unit][nen][nrow].  grid = units, 64 threads; out: column col0 + unit of the (nrow, total) image.
__global__ __launch_bounds__(64) void k_rows_integrate(int nen, int nv1, int nrow, const double* __restrict__ ene, const double* __restrict__ fw,
                                                       const double* __restrict__ rows, int col0, double* __restrict__ out) {
    const int q = threadIdx.x, unit = blockIdx.x;
    if (q >= nrow) return;
    const double* R = rows + (size_t)unit * nen * nrow + q;
    out[(size_t)nrow * (col0 + unit) + q] = xc_simpson_fermi(nen, nv1, ene[1] - ene[0], fw, [&](int k) -> double { return k < nen ? R[(size_t)k * nrow] : 0.0; });
}
}  // namespace rsrec
