// Per-atom blocks of functions of H for a whole cell (rsrec_chebyshev_site_map).
//   z_n[j]     = sum_v conj(c^v_j) [T_{n-1}(H~) x^v]_j          x^v = sum_j c^v_j |j> (x) 1_18, the whole-lattice seeds of the call
//   D(:,:,e,j) = sum_n w(n, e) z_n[j]                            = |c_j|^2 f_e(H~)_jj + sum_{k != j} conj(c_j) c_k f_e(H~)_jk summed over v
// Project first, weight second: the chains of a launch are folded into ONE vector z per order before the ne weight columns see it, so an
// element costs VT + ne complex FMAs per order, not VT ne, and the call keeps ne accumulators for ALL its vectors -- nothing grows as
// atoms x orders or as vectors x ne.  The orders are written by the SpMM's Chebyshev epilogue into a ring of PT + 2 slots per vector; after
// every PT orders one pass per tile of VT vectors adds them into the accumulators (k_site_accum, the per-order hot path beside the SpMM).
// Behind the last batch k_site_out writes the blocks in the reference's column-major order.
//
// Accumulation.  Whole-lattice vectors in CI (or CM) layout and the accumulators alike are flat streams of 16-byte complex elements, 324
// per atom.  A thread owns one element: it loads that element of PT orders of VT vectors (VT PT <= 16 loads in flight) and the VT
// conjugated coefficients of its atom (a dense (kk) table per vector, zero where the vector has no coefficient), forms the PT values z in
// registers -- v ascending, the four FMAs of map_axpy each --, tests them against the call's divergence bound, and then, column by column,
// reads D_e, adds w(p, e) z_p in ascending p with map_axpy and stores D_e: (VT PT + 2 ne) 16 B per element and tile-pass.  The weights
// of a pass are uniform over the workgroup (their address depends on loop counters alone: scalar loads).  A short tile (fewer vectors
// than VT) and a short last pass (fewer orders than PT) are predicated, never left early: everything stays in registers, no scratch.
//
// Reproducibility.  Fixed order, no float atomics (the divergence flag is an integer OR).  The same inputs and the same options give the
// same bits, whatever earlier calls left in the buffers.  The bits of column e depend on neither ne nor the other columns; the bits of an
// atom's block do not depend on which outputs are asked for, nor on host or device destination, and d_diag is bit for bit the diagonal of
// d_full (k_site_out stores both from the same value).  The bits DO depend on the order of the vectors, on sitemap_vtile and on the vector
// batch (kubo_vbatch, or what fits): the accumulator is shared by all vectors, so the sequence of adds into it is (batch, pass, tile,
// order), and sitemap_orders decides where the passes end.  Nothing more is promised.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_blochmap.hpp"
#include "kernels_lattice.hpp"

namespace rsrec {

constexpr int SITE_THREADS = 256;
constexpr int SITE_ORDERS_MAX = 16;           // orders a pass adds at most (option sitemap_orders)
constexpr int SITE_VTILE_MAX = 8;             // vectors a pass folds at most (option sitemap_vtile)
constexpr int SITE_LOADS_MAX = 16;            // VT PT: vector loads a thread has in flight
constexpr int SITE_OUT_THREADS = 384;         // 324 elements of a block, the rest idle

// What a pass reads besides the ring: where it is in the call.
//   ring: order n of vector c of the batch lies at ring + (n % nring) slot_stride + c vstride (complex elements); slot0 = n0 % nring
//   coef: [vector of the batch][kk] conj(c); w: complex [ne][nmom], row n0 + p weights order p of the pass
struct SitePass {
    size_t slot_stride, vstride, total, dstride;   // total = kk 324 elements; dstride: complex elements between two accumulators
    int nring, slot0, cnt, v0, nv, kk, n0, nmom, ne;   // cnt <= PT live orders; vectors v0 .. v0 + nv - 1 of the batch, nv <= VT
    double bound;                                  // 1000 max(1, sum_v sum_j |c^v_j|^2)
};

// D[e][:] += sum_{p < cnt} w(n0 + p, e) z_p[:],  z_p = sum_{v < nv} coef[v0 + v][atom] psi_{n0 + p}[v0 + v][:].  grid: workgroups over `total`.
template <int VT, int PT>
__global__ __launch_bounds__(SITE_THREADS) void k_site_accum(const double2* __restrict__ ring, const double2* __restrict__ coef,
                                                             const double2* __restrict__ w, SitePass S, double2* __restrict__ D, int* status) {
    static_assert(VT * PT <= SITE_LOADS_MAX, "at most 16 loads in flight");
    const size_t idx = (size_t)blockIdx.x * SITE_THREADS + threadIdx.x;
    const bool in = idx < S.total;
    const size_t at = in ? idx : 0;                                // (a thread past the end reads element 0 and stores nothing)
    const int atom = (int)(at / BLK);
    double2 x[VT][PT], cc[VT];
#pragma unroll
    for (int v = 0; v < VT; ++v) {
        const int vv = S.v0 + (v < S.nv ? v : 0);                  // (uniform; a dead vector of a short tile re-reads a live one and is not added)
        cc[v] = coef[(size_t)vv * S.kk + atom];
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            const int slot = (S.slot0 + (p < S.cnt ? p : 0)) % S.nring;
            x[v][p] = ring[(size_t)slot * S.slot_stride + (size_t)vv * S.vstride + at];
        }
    }
    double2 z[PT];
    bool bad = false;
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        z[p] = make_double2(0.0, 0.0);
#pragma unroll
        for (int v = 0; v < VT; ++v)
            if (v < S.nv) map_axpy(z[p], cc[v], x[v][p]);
        if (p < S.cnt) bad = bad || !(fabs(z[p].x) <= S.bound && fabs(z[p].y) <= S.bound);   // (a NaN has diverged too)
    }
    if (bad && in) atomicOr(status, 2);
    const double2* wn = w + S.n0;
    for (int e = 0; e < S.ne; ++e) {
        const double2* we = wn + (size_t)e * S.nmom;
        double2* de = D + (size_t)e * S.dstride + at;
        double2 acc = *de;
#pragma unroll
        for (int p = 0; p < PT; ++p)
            if (p < S.cnt) map_axpy(acc, we[p], z[p]);
        if (in) *de = acc;
    }
}

// The accumulators of atoms j0 .. j0 + nj - 1 as the reference's column-major blocks: full (18,18,ne,nj) and / or diag (18,ne,nj), either
// may be null; both from the same loaded value.  L: the layout of the vectors, and so of an accumulator's block.  grid (ne, atoms).
template <class L>
__global__ __launch_bounds__(SITE_OUT_THREADS) void k_site_out(const double2* __restrict__ D, size_t dstride, int j0, int nj, int ne,
                                                              double2* __restrict__ full, double2* __restrict__ diag) {
    const int t = threadIdx.x, e = blockIdx.x;
    if (t >= BLK) return;
    const int o = lattice_out_index<L>(t), row = o % NB, col = o / NB;
    for (int j = blockIdx.y; j < nj; j += gridDim.y) {
        const double2 v = D[(size_t)e * dstride + (size_t)(j0 + j) * BLK + t];
        const size_t img = (size_t)e + (size_t)ne * j;
        if (full) full[img * BLK + o] = v;
        if (diag && row == col) diag[img * NB + row] = v;
    }
}

}  // namespace rsrec
