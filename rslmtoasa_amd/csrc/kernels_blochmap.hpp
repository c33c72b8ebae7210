// Functions of H at many k-points from one chain per atom (rsrec_chebyshev_bloch_map): the sums of rsrec_chebyshev_bloch taken in the other order.
//   G_i(k, e) = sum_n w(n, e) S_i(k, n) = sum_j exp(-i k.d(j, i)) Y_e[j],    Y_e = sum_n w(n, e) psi_{n-1}
// The chain accumulates the ne vectors Y_e order by order (k_map_accum, the per-order hot path); one Bloch sum per energy follows the last
// order, with the phase, GEMM and reduce kernels of kernels_bloch.hpp on Y_e in the vector's place (n := e, nmom := ne).  The cost no
// longer grows as orders x k-points, and nothing of the size orders x k-points is ever stored.
//
// Accumulation.  CI and CM blocks are both 324 interleaved complex numbers, and Y_e has the layout of psi: the pass is a flat stream of
// 16-byte elements over the atoms in ATOM order -- consecutive workgroups stream consecutive atoms --, and an atom takes part once its
// joining level (join[chain][atom], INT_MAX for an atom of no group or outside the final region) is reached.  Nothing outside the region
// of the level is read or written.  One read of psi serves all ne energies: 1 + 2 ne block streams per atom.
// Two orders per pass (TWO): psi_{n-1} is still alive when psi_n has been formed, so the pass of every second order adds both and Y_e
// is read and written half as often.  The four fmas of order n-1 come before those of order n, exactly those of two one-order passes: the
// two forms give the same bits.  Per (atom, element, e) the arithmetic does not depend on ne, so an energy's bits do not depend on the
// other columns of w.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include "kernels_bloch.hpp"

namespace rsrec {

constexpr int MAP_THREADS = 256;
constexpr int MAP_UNROLL = 4;                  // 16-byte elements per thread: loads of psi and of Y_e in flight together
constexpr int MAP_WG_ELEMS = MAP_THREADS * MAP_UNROLL;
constexpr int MAP_DIAG_THREADS = 320;          // k_map_diag: 18 orbitals x up to 16 energies

// y += w x, complex: the one place the accumulation's arithmetic is written
__device__ __forceinline__ void map_axpy(double2& y, const double2 w, const double2 x) {
    y.x = fma(w.x, x.x, y.x); y.x = fma(-w.y, x.y, y.x);
    y.y = fma(w.x, x.y, y.y); y.y = fma(w.y, x.x, y.y);
}

// Y_e[j] += w(n, e) cur[j]  (TWO: w(n-1, e) old[j] first, for the atoms already inside at `level_old`) for the atoms with join <= level.
// grid (workgroups over kk * 324 elements, chains).  w: complex (nmom, ne) column-major, row n = the weights of `cur`.
// cur, old: [chain][vstride] complex; Y: [chain][e][vstride].
template <bool TWO>
__global__ __launch_bounds__(MAP_THREADS) void k_map_accum(const int* __restrict__ join, int kk, int level, int level_old, const double2* __restrict__ cur,
                                                           const double2* __restrict__ old, size_t vstride, const double2* __restrict__ w, int n, int nmom,
                                                           int ne, double2* __restrict__ Y) {
    const int chain = blockIdx.y;
    const size_t total = (size_t)kk * BLK, base = (size_t)blockIdx.x * MAP_WG_ELEMS + threadIdx.x;
    const int* jn = join + (size_t)chain * kk;
    const double2* x = cur + (size_t)chain * vstride;
    const double2* xo = old + (size_t)chain * vstride;
    double2* y = Y + (size_t)chain * ne * vstride;
    bool in[MAP_UNROLL], in_old[MAP_UNROLL];
    double2 xc[MAP_UNROLL], xp[MAP_UNROLL];
#pragma unroll
    for (int u = 0; u < MAP_UNROLL; ++u) {
        const size_t idx = base + (size_t)u * MAP_THREADS;
        const int lv = idx < total ? jn[idx / BLK] : INT_MAX;
        in[u] = lv <= level; in_old[u] = TWO && lv <= level_old;
        xc[u] = in[u] ? x[idx] : make_double2(0.0, 0.0);
        xp[u] = in_old[u] ? xo[idx] : make_double2(0.0, 0.0);
    }
    for (int e = 0; e < ne; ++e) {
        const double2 wn = w[(size_t)e * nmom + n], wo = TWO ? w[(size_t)e * nmom + n - 1] : make_double2(0.0, 0.0);
        double2* ye = y + (size_t)e * vstride;
        double2 acc[MAP_UNROLL];
#pragma unroll
        for (int u = 0; u < MAP_UNROLL; ++u)
            if (in[u]) acc[u] = ye[base + (size_t)u * MAP_THREADS];
#pragma unroll
        for (int u = 0; u < MAP_UNROLL; ++u) {
            if (!in[u]) continue;
            if (in_old[u]) map_axpy(acc[u], wo, xp[u]);
            map_axpy(acc[u], wn, xc[u]);
            ye[base + (size_t)u * MAP_THREADS] = acc[u];
        }
    }
}

// Where the images of a k-chunk lie: image (q, g, chain) of the chunk is number (q0 + q) + nk ((g) + ngroup (c0 + chain)) of `p` -- the
// caller's device array itself (q0 = the chunk's first point, nk and c0 the call's), or a staging buffer of the chunk (q0 = c0 = 0, nk =
// the chunk's length).  k_bloch_reduce and k_bloch_valu take the three numbers as they are.
struct MapSlot { int q0, nk, c0; };

// a_k(l, e, image) = -Im g_k(l, l, e, image) / pi from the blocks the final sums left.  grid (k-points of the chunk, groups, chains).
__global__ __launch_bounds__(MAP_DIAG_THREADS) void k_map_diag(const double2* __restrict__ g, MapSlot gs, double* __restrict__ a, MapSlot as, int ngroup, int ne) {
    const int t = threadIdx.x;
    if (t >= NB * ne) return;
    const int e = t / NB, l = t % NB;
    const size_t ig = (size_t)(gs.q0 + blockIdx.x) + (size_t)gs.nk * (blockIdx.y + (size_t)ngroup * (gs.c0 + blockIdx.z));
    const size_t ia = (size_t)(as.q0 + blockIdx.x) + (size_t)as.nk * (blockIdx.y + (size_t)ngroup * (as.c0 + blockIdx.z));
    a[(ia * ne + e) * NB + l] = -g[(ig * ne + e) * BLK + (NB + 1) * l].y / 3.14159265358979323846;
}

}  // namespace rsrec
