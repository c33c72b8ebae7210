// k-resolved Chebyshev moments from one chain per atom (rsrec_chebyshev_bloch).
//
// The Chebyshev vector psi_n started from the identity at atom i holds <j| T_n(H~) |i> at every atom j of its region; its lattice Fourier sum
//   S_i(k, n) = sum_j exp(-i k.(r_j - r_i)) <j| T_n(H~) |i>
// is the k-resolved moment (T_n(H~(k)) itself on a periodic one-atom cell).  Per order and source this is a real GEMM P = W V:
//   W : the phases as rows, two per k-point (row 2 q = Re w_q = cos k_q.d, row 2 q + 1 = Im w_q = -sin k_q.d), one column per atom of the list
//   V : the blocks of the list's atoms as rows of 648 reals
// and out_re(e) = P[2q][re e] - P[2q+1][im e], out_im(e) = P[2q][im e] + P[2q+1][re e].
//
// Lists.  An atom contributes from the order at which it joins the chain's region.  The host sorts the atoms of every (chain, group) by
// (joining level, atom), so the atoms of a group at a level are a prefix of the group's segment; nothing outside that prefix is ever read,
// neither from the phase table nor from the work vector (which holds stale data outside the region).
//
// Phases.  Tabulated once per (chain, list position, k-point) with FP64 sincos (k_bloch_phase) in LIST order, so an A fragment of the GEMM
// is four contiguous 128-byte rows: 2 lld + 2 passes read what one sincos per entry wrote, and the table's bits do not depend on the pass
// that reads it.  Forming them in the pass would cost one sincos (some 10^2 VALU flop) per 2 x 648 matrix flop of every order.
//
// Sums.  K (the atoms) is split over workgroups by bloch_splits(), a function of the list's own length; every split writes its partial,
// k_bloch_reduce adds the partials in ascending order.  No atomics.  The rows of W are independent in the matrix product, and every
// (chain, group) has its own list: an image's bits depend on its own k-point, group atoms and source alone.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_valu.hpp"
#include "kernels_mfma.hpp"

namespace rsrec {

constexpr int BLOCH_MT = 4;                    // M tiles (16 rows of W) a wave keeps per loaded B fragment: 4 MT = 16 flop per byte of the vector
constexpr int BLOCH_NT = 2;                    // N tiles (16 reals of a block) per loaded A fragment
constexpr int BLOCH_MROWS = 16 * BLOCH_MT;     // rows of W per wave; the table's row count is padded to a multiple of it (zero rows)
constexpr int BLOCH_NPAIRS = (BLD + 16 * BLOCH_NT - 1) / (16 * BLOCH_NT);   // 21: 648 = 20 * 32 + 8, the last pair is three quarters padding
constexpr int BLOCH_WAVES = 4;                 // waves per workgroup: four N pairs on the same rows of W and the same atoms
constexpr int BLOCH_NPB = (BLOCH_NPAIRS + BLOCH_WAVES - 1) / BLOCH_WAVES;   // workgroups over N
constexpr int BLOCH_MAXSPLIT = 32;
constexpr int BLOCH_MCHUNK = 512;              // rows of W per launch (256 k-points): bounds the partials, 32 x 512 x 648 doubles per chain
constexpr int BLOCH_THREADS = 384;             // k_bloch_reduce, k_bloch_valu, k_bloch_diverge: 324 elements of a block, the rest idle

// workgroups over K of a list of n atoms: at least 16 k-steps of four atoms each, a function of n alone
__host__ __device__ inline int bloch_splits(int n) {
    const int s = ((n + 3) / 4) / 16;
    return s < 1 ? 1 : (s > BLOCH_MAXSPLIT ? BLOCH_MAXSPLIT : s);
}

// The lists of a batch of chains.  list[chain][kk]: the chain's atoms, one segment per group (seg_off[chain][group]), each sorted by
// (joining level, atom); count[chain][group][nlev]: atoms of the segment inside the region at a level.
struct BlochLists {
    const int* list; const int* seg_off; const int* count;
    int kk, ngroup, nlev;
    __device__ __forceinline__ const int* seg(int chain, int g) const { return list + (size_t)chain * kk + seg_off[chain * ngroup + g]; }
    __device__ __forceinline__ int off(int chain, int g) const { return seg_off[chain * ngroup + g]; }
    __device__ __forceinline__ int cnt(int chain, int g, int level) const { return count[((size_t)chain * ngroup + g) * nlev + level]; }
};

struct BlochGeom { double cell[9], inv[9]; int wrap; };     // column-major 3x3: cell(:,c) = cell[3 c ..]; inv = cell^-1

// table[chain][pos][2 q], [2 q + 1] = cos(k_q.d), -sin(k_q.d), d = cr(:,atom) - cr(:,source) reduced to its minimum image when asked;
// rows 2 nk .. mpad - 1 are zero.  pos runs over the chain's whole list (tot[chain] entries).
__global__ __launch_bounds__(256) void k_bloch_phase(BlochLists BL, const int* __restrict__ tot, const int* __restrict__ src_atom, const double* __restrict__ cr,
                                                     const double* __restrict__ kpt, int nk, int mpad, BlochGeom G, double* __restrict__ table) {
    const int chain = blockIdx.y, half = mpad / 2;
    const size_t n = (size_t)tot[chain] * half;
    const int* list = BL.list + (size_t)chain * BL.kk;
    const int s = src_atom[chain];
    double2* tab = reinterpret_cast<double2*>(table + (size_t)chain * BL.kk * mpad);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const int pos = (int)(idx / half), q = (int)(idx - (size_t)pos * half);
        double2 w = make_double2(0.0, 0.0);
        if (q < nk) {
            const int j = list[pos];
            double d[3] = {cr[3 * j] - cr[3 * s], cr[3 * j + 1] - cr[3 * s + 1], cr[3 * j + 2] - cr[3 * s + 2]};
            if (G.wrap) {
                double f[3];
                for (int i = 0; i < 3; ++i) f[i] = rint(G.inv[i] * d[0] + G.inv[3 + i] * d[1] + G.inv[6 + i] * d[2]);
                for (int i = 0; i < 3; ++i) d[i] -= G.cell[i] * f[0] + G.cell[3 + i] * f[1] + G.cell[6 + i] * f[2];
            }
            const double arg = kpt[3 * q] * d[0] + kpt[3 * q + 1] * d[1] + kpt[3 * q + 2] * d[2];
            double sn, cs;
            sincos(arg, &sn, &cs);
            w = make_double2(cs, -sn);
        }
        tab[(size_t)pos * half + q] = w;
    }
}

// Matrix-core pass on CI vectors.  Workgroup (x = N quarter + BLOCH_NPB * M group, y = K split, z = chain); wave w of it owns the N pair
// BLOCH_WAVES * quarter + w: BLOCH_MT x BLOCH_NT accumulator tiles over the split's k-steps of four atoms.  B fragment: lane (k = l4,
// n = l15) reads real 16 nt + l15 of atom k of the step; A fragment: lane (m = l15, k = l4) reads row m of the table at that atom's
// position.  A step past the list's end contributes exact zeros (neither the table nor the vector is read there).
// partial[chain][split][row of the chunk][648].
__global__ __launch_bounds__(BLOCH_WAVES * 64) void k_bloch_mfma(BlochLists BL, int g, int level, const double* __restrict__ vec, size_t vstride,
                                                                  const double* __restrict__ table, int mpad, int m0, int mrows,
                                                                  double* __restrict__ partial) {
    const int chain = blockIdx.z, split = blockIdx.y;
    const int n = BL.cnt(chain, g, level), nsplit = bloch_splits(n);
    if (split >= nsplit) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int npair = ((int)blockIdx.x % BLOCH_NPB) * BLOCH_WAVES + wave, mg = (int)blockIdx.x / BLOCH_NPB;
    if (npair >= BLOCH_NPAIRS) return;
    const int ksteps = (n + 3) / 4;
    const int ks0 = (int)((long)split * ksteps / nsplit), ks1 = (int)((long)(split + 1) * ksteps / nsplit);
    const int* seg = BL.seg(chain, g);
    const double* v = vec + (size_t)chain * vstride;
    const double* tab = table + ((size_t)chain * BL.kk + BL.off(chain, g)) * mpad + m0 + mg * BLOCH_MROWS + l15;
    // A column past the block (the padding of the last N pair) reads the block's last real instead: a column of D depends on its own
    // column of B alone, and the padded columns are never stored.
    int col[BLOCH_NT], rd[BLOCH_NT];
#pragma unroll
    for (int nt = 0; nt < BLOCH_NT; ++nt) { col[nt] = 16 * (BLOCH_NT * npair + nt) + l15; rd[nt] = min(col[nt], BLD - 1); }
    double4_t acc[BLOCH_MT][BLOCH_NT];
#pragma unroll
    for (int mt = 0; mt < BLOCH_MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < BLOCH_NT; ++nt) acc[mt][nt] = (double4_t){0, 0, 0, 0};
    auto mfma_step = [&](const double (&a)[BLOCH_MT], const double (&b)[BLOCH_NT]) {
#pragma unroll
        for (int mt = 0; mt < BLOCH_MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < BLOCH_NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    };
    // whole k-steps: four atoms of the list, nothing to guard; unrolled so that the loads of several steps are in flight
    const int ksw = min(ks1, n / 4);
    int ks = ks0;
#pragma unroll 8
    for (; ks < ksw; ++ks) {
        const int pos = 4 * ks + l4;
        double a[BLOCH_MT], b[BLOCH_NT];
        const double* trow = tab + (size_t)pos * mpad;
#pragma unroll
        for (int mt = 0; mt < BLOCH_MT; ++mt) a[mt] = trow[16 * mt];
        const double* blk = v + (size_t)BLD * seg[pos];
#pragma unroll
        for (int nt = 0; nt < BLOCH_NT; ++nt) b[nt] = blk[rd[nt]];
        mfma_step(a, b);
    }
    // the list's last step, when its length is no multiple of four: the missing atoms enter as exact zeros on both sides
    for (; ks < ks1; ++ks) {
        const int pos = 4 * ks + l4;
        const bool in = pos < n;
        double a[BLOCH_MT], b[BLOCH_NT];
        const double* trow = tab + (size_t)(in ? pos : 0) * mpad;
#pragma unroll
        for (int mt = 0; mt < BLOCH_MT; ++mt) a[mt] = in ? trow[16 * mt] : 0.0;
        const double* blk = v + (size_t)BLD * (in ? seg[pos] : 0);
#pragma unroll
        for (int nt = 0; nt < BLOCH_NT; ++nt) b[nt] = in ? blk[rd[nt]] : 0.0;
        mfma_step(a, b);
    }
    // D register j of a tile: row 4 j + l4, column l15 (kernels_mfma.hpp)
    double* out = partial + (((size_t)chain * BLOCH_MAXSPLIT + split) * mrows + mg * BLOCH_MROWS) * BLD;
#pragma unroll
    for (int mt = 0; mt < BLOCH_MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < BLOCH_NT; ++nt)
            if (col[nt] < BLD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) out[(size_t)(16 * mt + 4 * j + l4) * BLD + col[nt]] = acc[mt][nt][j];
            }
}

// Second stage: image (k-point q0 + blockIdx.x, group g, chain c0 + blockIdx.y) at moment n = the partials of the list's splits added in
// ascending order, combined into complex numbers and stored as the reference's column-major block.  Thread t is CI element (r, c) = (t / 18, t % 18).
__global__ __launch_bounds__(BLOCH_THREADS) void k_bloch_reduce(BlochLists BL, int g, int level, const double* __restrict__ partial, int mrows, int q0, int nk,
                                                                int c0, int n, int nmom, double2* __restrict__ mu) {
    const int chain = blockIdx.y, ql = blockIdx.x, t = threadIdx.x;
    if (t >= BLK) return;
    const int nsplit = bloch_splits(BL.cnt(chain, g, level));
    double2 pre = make_double2(0.0, 0.0), pim = make_double2(0.0, 0.0);
    for (int s = 0; s < nsplit; ++s) {
        const double2* row = reinterpret_cast<const double2*>(partial + (((size_t)chain * BLOCH_MAXSPLIT + s) * mrows + 2 * ql) * BLD);
        const double2 x = row[t], y = row[BLK + t];
        pre.x += x.x; pre.y += x.y; pim.x += y.x; pim.y += y.y;
    }
    const size_t img = (size_t)(q0 + ql) + (size_t)nk * (g + (size_t)BL.ngroup * (c0 + chain));
    mu[(img * nmom + n) * BLK + (t / NB) + NB * (t % NB)] = make_double2(pre.x - pim.y, pre.y + pim.x);
}

// VALU set: one workgroup per (k-point, chain), one thread per element, the list's atoms in order.  Same table, any layout.
template <class L>
__global__ __launch_bounds__(BLOCH_THREADS) void k_bloch_valu(BlochLists BL, int g, int level, const double* __restrict__ vec, size_t vstride,
                                                              const double* __restrict__ table, int mpad, int nk, int c0, int n, int nmom,
                                                              double2* __restrict__ mu) {
    const int chain = blockIdx.y, q = blockIdx.x, t = threadIdx.x;
    if (t >= BLK) return;
    const int cnt = BL.cnt(chain, g, level);
    const int* seg = BL.seg(chain, g);
    const double* v = vec + (size_t)chain * vstride;
    const double2* tab = reinterpret_cast<const double2*>(table + ((size_t)chain * BL.kk + BL.off(chain, g)) * mpad) + q;
    double2 acc = make_double2(0.0, 0.0);
    for (int pos = 0; pos < cnt; ++pos) {
        const double2 w = tab[(size_t)pos * (mpad / 2)], x = L::ld(v + (size_t)BLD * seg[pos], t % NB, t / NB);
        acc.x = fma(w.x, x.x, acc.x); acc.x = fma(-w.y, x.y, acc.x);
        acc.y = fma(w.x, x.y, acc.y); acc.y = fma(w.y, x.x, acc.y);
    }
    const size_t img = (size_t)q + (size_t)nk * (g + (size_t)BL.ngroup * (c0 + chain));
    mu[(img * nmom + n) * BLK + t] = acc;
}

// the reference's divergence test (recursion.f90:2479) on the source's own block, as k_fan_gather applies it
template <class L>
__global__ __launch_bounds__(BLOCH_THREADS) void k_bloch_diverge(const double* __restrict__ vec, size_t vstride, const int* __restrict__ src_atom, int* status) {
    __shared__ double tr[BLK];
    const int t = threadIdx.x;
    if (t < BLK) tr[t] = L::ld(vec + (size_t)blockIdx.x * vstride + (size_t)BLD * src_atom[blockIdx.x], t % NB, t / NB).x;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int q = 0; q < BLK; ++q) s += tr[q];
        if (s > 1000.0) atomicOr(status, 2);
    }
}

}  // namespace rsrec
