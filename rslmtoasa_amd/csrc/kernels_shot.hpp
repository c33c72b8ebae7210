// Single-shot Kubo sums (rsrec_kubo_single_shot): the double sum over the moments taken before the moments are formed.
//   L_e = sum_m conj(wl(m, e)) T_{m-1}(H~) r,   R_e = sum_n wr(n, e) T_{n-1}(H~) v_b r,
//   s(:, :, e, v, j) = sum_k [L_e]_k^H [v_out_j R_e]_k = sum_{n,m} wl(m, e) wr(n, e) mu_j(:, :, n, m, v)
// The two recurrences of a vector advance as chains of the same launches; their orders are written by the SpMM's Chebyshev epilogue into a
// ring of P + 2 slots per chain, and after every P orders one pass adds them into the ne accumulators of every chain (k_shot_accum, the
// per-order hot path beside the SpMM).  Behind the last order every output operator is applied to the ne right accumulators and one small
// Gram per (e, j) is formed (k_shot_gram, k_shot_gram_reduce).  No left matrix, no M x M contraction, no moment array.
//
// Accumulation.  Whole-lattice vectors in CI layout: a flat stream of 16-byte complex elements, no join table.  A thread loads its
// element of the pass's orders once and then, column by column, reads y, adds w(p, e) psi_p in ascending order p with the four FMAs of
// map_axpy (kernels_blochmap.hpp: the one written form of y += w x) and stores y: (P + 2 ne) / P block streams per order and chain.
// The FMA sequence of an (element, e) is the same for every P and every ne -- a pass border only stores y and loads it again -- so a
// column's bits depend neither on shot_orders nor on the other columns.  VALU FMAs on purpose: an MFMA K-reduction over the orders
// of a pass would tie the bits to P.  The weights of a pass are uniform over the workgroup: their address depends on blockIdx and loop
// counters alone, and the compiler reads them with scalar loads into SGPRs.
//
// Gram.  For one vector and one output operator, G(e) = L_e^H W_e (W_e = v_out_j R_e), 18 x 18 complex over the 18 kk rows of the CI
// vectors read in place, all ne columns in one launch: grid (slices, ne), one wave per task on v_mfma_f64_16x16x4 (2 x 2 tiles, the
// padding rows and columns repeat column 17 and are never stored).  The slice partition is a function of kk alone (shot_ksplit), the
// partials are summed in ascending slice order by k_shot_gram_reduce, which writes s_full and takes s_diag from the same sums: no
// atomics, and a column's bits do not depend on ne.  Block kk of every vector is the zero block, so the last k-step may end inside it.
// k_shot_gram_valu is the same contraction with the same partition on plain FMAs (kernel set 1).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_mfma.hpp"
#include "kernels_blochmap.hpp"

namespace rsrec {

constexpr int SHOT_THREADS = 256;
constexpr int SHOT_ORDERS_MAX = 16;           // orders a pass adds at most (option shot_orders)
constexpr int SHOT_KSPLIT_MAX = 256;
constexpr int SHOT_GRAM_VALU_THREADS = 384;   // 324 elements of a block, the rest idle

// slices of the Gram's row index: at least 64 k-steps of 4 rows each, a function of the lattice size alone
__host__ __device__ inline int shot_ksplit(int ksteps_total) {
    const int s = ksteps_total / 64;
    return s < 1 ? 1 : (s > SHOT_KSPLIT_MAX ? SHOT_KSPLIT_MAX : s);
}

// Y[chain][e][:] += sum_{p < cnt} w(n0 + p, e) psi_{n0 + p}[chain][:].  grid (workgroups over `total` = kk * 324 elements, chains).
// ring: order n of chain c lies in slot n % nring at ring + slot * slot_stride + c * vstride (complex elements); slot0 = n0 % nring.
// w: complex [2][ne][ll], side 0 = conj(wl) for the left chains (chain < nleft), side 1 = wr for the right chains.
// PT >= cnt orders are held in registers for U elements per thread (PT * U = 16 loads in flight but for PT <= 2).
template <int PT, int U>
__global__ __launch_bounds__(SHOT_THREADS) void k_shot_accum(const double2* __restrict__ ring, size_t slot_stride, int nring, int slot0, int cnt, size_t vstride,
                                                             size_t total, const double2* __restrict__ w, int nleft, int n0, int ll, int ne,
                                                             double2* __restrict__ Y) {
    const int chain = blockIdx.y;
    const size_t base = (size_t)blockIdx.x * (SHOT_THREADS * U) + threadIdx.x;
    const double2* wside = w + ((size_t)(chain < nleft ? 0 : 1) * ne) * ll + n0;
    double2* y = Y + (size_t)chain * ne * vstride;
    bool in[U];
    double2 x[PT][U];
#pragma unroll
    for (int u = 0; u < U; ++u) in[u] = base + (size_t)u * SHOT_THREADS < total;
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        const bool live = p < cnt;                             // (uniform; no early exit: x stays in registers)
        const double2* xs = ring + (size_t)((slot0 + (live ? p : 0)) % nring) * slot_stride + (size_t)chain * vstride;
#pragma unroll
        for (int u = 0; u < U; ++u) x[p][u] = live && in[u] ? xs[base + (size_t)u * SHOT_THREADS] : make_double2(0.0, 0.0);
    }
    for (int e = 0; e < ne; ++e) {
        const double2* we = wside + (size_t)e * ll;
        double2* ye = y + (size_t)e * vstride;
        double2 acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = in[u] ? ye[base + (size_t)u * SHOT_THREADS] : make_double2(0.0, 0.0);
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            if (p < cnt) {
                const double2 wp = we[p];
#pragma unroll
                for (int u = 0; u < U; ++u) map_axpy(acc[u], wp, x[p][u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (in[u]) ye[base + (size_t)u * SHOT_THREADS] = acc[u];
    }
}

// part[e][slice][c + 18 c'] = sum over the slice's rows rho of conj(L_e[rho][c]) W_e[rho][c'].  grid (ksplit, ne), one wave.
// L, W: the first of ne CI vectors, `ls` / `ws` doubles apart.
__global__ __launch_bounds__(64) void k_shot_gram(const double* __restrict__ L, size_t ls, const double* __restrict__ W, size_t ws, int ksteps_total, int ksplit,
                                                  double2* __restrict__ part) {
    const int lane = threadIdx.x, l15 = lane & 15, l4 = lane >> 4;
    const int ks = blockIdx.x, e = blockIdx.y;
    const int per = (ksteps_total + ksplit - 1) / ksplit;
    const int s0 = ks * per, s1 = min(ksteps_total, s0 + per);
    typedef double sg_d2 __attribute__((ext_vector_type(2)));
    const double* pa[2];
    const double* pb[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int i = min(16 * q + l15, NB - 1);
        pa[q] = L + (size_t)e * ls + 2 * i + (size_t)36 * (4 * (size_t)s0 + l4);
        pb[q] = W + (size_t)e * ws + 2 * i + (size_t)36 * (4 * (size_t)s0 + l4);
    }
    double4_t cre[2][2], cim[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int u = 0; u < 2; ++u) { cre[q][u] = (double4_t){0, 0, 0, 0}; cim[q][u] = (double4_t){0, 0, 0, 0}; }
    sg_d2 a0[2], b0[2], a1[2], b1[2];
    auto fetch = [&](sg_d2 (&a)[2], sg_d2 (&b)[2]) {
#pragma unroll
        for (int q = 0; q < 2; ++q) { a[q] = *reinterpret_cast<const sg_d2*>(pa[q]); b[q] = *reinterpret_cast<const sg_d2*>(pb[q]); pa[q] += 144; pb[q] += 144; }
    };
    auto mac = [&](const sg_d2 (&a)[2], const sg_d2 (&b)[2]) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const double ar = a[q][0], ai = a[q][1], nai = -ai;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                cre[q][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, b[u][0], cre[q][u], 0, 0, 0);
                cim[q][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, b[u][1], cim[q][u], 0, 0, 0);
                cre[q][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, b[u][1], cre[q][u], 0, 0, 0);
                cim[q][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(nai, b[u][0], cim[q][u], 0, 0, 0);
            }
        }
    };
    int s = s0;
    if (s < s1) fetch(a0, b0);
#pragma unroll 1
    for (; s + 2 <= s1; s += 2) {
        fetch(a1, b1);
        mac(a0, b0);
        if (s + 2 < s1) fetch(a0, b0);
        mac(a1, b1);
    }
    if (s < s1) mac(a0, b0);
    // D register rr of lane (l15, l4): row l4 + 4 rr, column l15 of the tile
    double2* P = part + ((size_t)e * ksplit + ks) * BLK;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = 16 * q + l4 + 4 * rr, j = 16 * u + l15;
                if (i < NB && j < NB) P[i + NB * j] = make_double2(cre[q][u][rr], cim[q][u][rr]);
            }
}

// the same partials on plain FMAs: thread (c, c') walks the slice's rows in order
__global__ __launch_bounds__(SHOT_GRAM_VALU_THREADS) void k_shot_gram_valu(const double* __restrict__ L, size_t ls, const double* __restrict__ W, size_t ws,
                                                                          int ksteps_total, int ksplit, double2* __restrict__ part) {
    const int t = threadIdx.x, ks = blockIdx.x, e = blockIdx.y;
    if (t >= BLK) return;
    const int c = t % NB, cp = t / NB;
    const int per = (ksteps_total + ksplit - 1) / ksplit;
    const int s0 = ks * per, s1 = min(ksteps_total, s0 + per);
    const double2* a = reinterpret_cast<const double2*>(L + (size_t)e * ls) + c;
    const double2* b = reinterpret_cast<const double2*>(W + (size_t)e * ws) + cp;
    double sr = 0.0, si = 0.0;
    for (size_t rho = 4 * (size_t)s0; rho < 4 * (size_t)s1; ++rho) {
        const double2 av = a[rho * NB], bv = b[rho * NB];
        sr = fma(av.x, bv.x, sr); sr = fma(av.y, bv.y, sr);
        si = fma(av.x, bv.y, si); si = fma(-av.y, bv.x, si);
    }
    part[((size_t)e * ksplit + ks) * BLK + t] = make_double2(sr, si);
}

// s(:, :, e, iv, j) = the slices' partials added in ascending order; the diagonal goes to s_diag from the same sum.  grid (ne).
// full: complex (18,18,ne,nvec,nout), diag: complex (18,ne,nvec,nout), either may be null.
__global__ __launch_bounds__(SHOT_GRAM_VALU_THREADS) void k_shot_gram_reduce(const double2* __restrict__ part, int ksplit, int ne, int iv, int nvec, int j,
                                                                            double2* __restrict__ full, double2* __restrict__ diag) {
    const int t = threadIdx.x, e = blockIdx.x;
    if (t >= BLK) return;
    const double2* p = part + (size_t)e * ksplit * BLK + t;
    double sr = 0.0, si = 0.0;
    for (int ks = 0; ks < ksplit; ++ks) { const double2 v = p[(size_t)ks * BLK]; sr += v.x; si += v.y; }
    const size_t img = (size_t)e + (size_t)ne * ((size_t)iv + (size_t)nvec * j);
    const int c = t % NB, cp = t / NB;
    if (full) full[img * BLK + t] = make_double2(sr, si);
    if (diag && c == cp) diag[img * NB + c] = make_double2(sr, si);
}

}  // namespace rsrec
