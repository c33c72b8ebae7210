// Chebyshev moments from whole-lattice seeds (rsrec_chebyshev_lattice).
//
// The chain starts from |x> = sum_j c_j |j> (x) 1_18 and runs over the whole lattice from order 0; its moment at order n is the seed-weighted
// sum of the vector's own blocks, group by group:
//   M_g(n) = sum_{j in group g} conj(c_j) [T_n(H~) x]_j = <x| P_g T_n(H~) |x>.
// Per order and chain this is a stream: every block of a grouped, seeded atom is read once (5 184 B) and scaled-and-added once, one complex
// FMA per 16 bytes -- 0.5 flop per byte, two orders of magnitude below what the FP64 vector units need to keep up with the HBM.  So the pass
// is plain FMA with 16-byte loads; the matrix cores would add nothing but the 2 ngroup x 16 padding of their M side.  Measured (DESIGN
// section 5): 4.8-5.4 TB/s from 8 chains on and 3.5-4.1 TB/s with one chain on 97 336 atoms, 0.10-0.28 of the call's H|psi> time.
//
// Lists.  The host sorts each chain's seeded atoms by (group, atom) and uploads the list and the conjugated weights in list order; atoms
// without a seed or in group 0 are not in it.  seg_off[chain][g .. g + 1] bounds group g's segment: nothing outside it is read.
//
// Sums.  A segment of n atoms is split over lattice_splits(n) workgroups, a function of n alone; split s takes the positions
// [s n / splits, (s + 1) n / splits).  A thread owns one complex element of the block and adds the split's atoms in list order into four
// accumulators (position % 4 inside the split), combined as (a0 + a1) + (a2 + a3): four independent 16-byte loads in flight per thread.
// Every split writes a 648-real partial; k_lattice_reduce adds the partials in ascending order and stores the reference's column-major block;
// k_lattice_diverge reads the stored blocks for the call's divergence test.
// No atomics in any sum: an image's bits depend on its own chain's vector and on the atom set of its own group alone.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_valu.hpp"
#include "kernels_mfma.hpp"

namespace rsrec {

constexpr int LATTICE_THREADS = 384;          // 324 complex elements of a block, the rest idle
constexpr int LATTICE_MAXSPLIT = 512;
constexpr int LATTICE_SPLIT_ATOMS = 16;       // atoms a split has at least (but for a shorter segment)
constexpr int LATTICE_RWG = 6;                // workgroups of k_lattice_reduce per image ...
constexpr int LATTICE_RELEMS = BLK / LATTICE_RWG;   // ... with 54 complex elements each

// workgroups over a segment of n atoms: a function of n alone (0 for an empty segment)
__host__ __device__ inline int lattice_splits(int n) {
    if (n <= 0) return 0;
    const int s = n / LATTICE_SPLIT_ATOMS;
    return s < 1 ? 1 : (s > LATTICE_MAXSPLIT ? LATTICE_MAXSPLIT : s);
}

// The lists of a batch of chains.  list[chain][kk], weight[chain][kk]: the chain's grouped seeded atoms sorted by (group, atom) and
// conj(c) of each; seg_off[chain][ngroup + 1]: the groups' segments; split_off[chain][ngroup + 1]: where a group's partials begin
// among the chain's `pstride` partial slots (prefix sums of lattice_splits).
struct LatticeLists {
    const int* list; const double2* weight; const int* seg_off; const int* split_off;
    int kk, ngroup, pstride;
};

// where thread t's element (the t-th complex number of a block in memory) lies in the reference's column-major block
template <class L> __device__ __forceinline__ int lattice_out_index(int t);
template <> __device__ __forceinline__ int lattice_out_index<LayoutCM>(int t) { return t; }
template <> __device__ __forceinline__ int lattice_out_index<LayoutCI>(int t) { return t / NB + NB * (t % NB); }

// acc += w x
__device__ __forceinline__ void lattice_cfma(double2& acc, const double2 w, const double2 x) {
    acc.x = fma(w.x, x.x, acc.x); acc.x = fma(-w.y, x.y, acc.x);
    acc.y = fma(w.x, x.y, acc.y); acc.y = fma(w.y, x.x, acc.y);
}

// First stage.  Workgroup (x = partial slot of the chain, y = chain): slot x belongs to the group g with split_off[g] <= x < split_off[g + 1].
// Either layout keeps a block as 324 consecutive complex numbers, so the pass itself is layout-blind.
__global__ __launch_bounds__(LATTICE_THREADS) void k_lattice_project(LatticeLists LL, const double* __restrict__ vec, size_t vstride,
                                                                     double2* __restrict__ partial) {
    const int chain = blockIdx.y, slot = blockIdx.x, t = threadIdx.x;
    const int* soff = LL.split_off + (size_t)chain * (LL.ngroup + 1);
    if (slot >= soff[LL.ngroup] || t >= BLK) return;
    int g = 0;
    while (soff[g + 1] <= slot) ++g;                             // (uniform over the workgroup; empty groups have no slots)
    const int* goff = LL.seg_off + (size_t)chain * (LL.ngroup + 1);
    const int n = goff[g + 1] - goff[g], nsplit = soff[g + 1] - soff[g], s = slot - soff[g];
    const int p0 = (int)((long)s * n / nsplit), p1 = (int)((long)(s + 1) * n / nsplit);
    const int* seg = LL.list + (size_t)chain * LL.kk + goff[g];
    const double2* w = LL.weight + (size_t)chain * LL.kk + goff[g];
    const double2* v = reinterpret_cast<const double2*>(vec + (size_t)chain * vstride) + t;
    double2 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = make_double2(0.0, 0.0);
    int p = p0;
    for (; p + 4 <= p1; p += 4) {
        double2 x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = v[(size_t)BLK * seg[p + q]];
#pragma unroll
        for (int q = 0; q < 4; ++q) lattice_cfma(acc[q], w[p + q], x[q]);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)                                  // the split's last atoms, fewer than four
        if (p + q < p1) lattice_cfma(acc[q], w[p + q], v[(size_t)BLK * seg[p + q]]);
    const double2 lo = make_double2(acc[0].x + acc[1].x, acc[0].y + acc[1].y), hi = make_double2(acc[2].x + acc[3].x, acc[2].y + acc[3].y);
    partial[((size_t)chain * LL.pstride + slot) * BLK + t] = make_double2(lo.x + hi.x, lo.y + hi.y);
}

// Second stage: image (group blockIdx.x, chain c0 + blockIdx.y) at moment n = the partials of the group's splits added in ascending order,
// stored as the reference's column-major block (an empty group: zeros).  The 324 elements are dealt over LATTICE_RWG workgroups of one
// wave (blockIdx.z), so that the serial walk over up to 512 partials runs on several CUs; eight loads in flight, the adds in order.
template <class L>
__global__ __launch_bounds__(64) void k_lattice_reduce(LatticeLists LL, const double2* __restrict__ partial, int c0, int n, int nmom,
                                                       double2* __restrict__ mu) {
    const int chain = blockIdx.y, g = blockIdx.x, t = blockIdx.z * LATTICE_RELEMS + threadIdx.x;
    if (threadIdx.x >= LATTICE_RELEMS) return;
    const int* soff = LL.split_off + (size_t)chain * (LL.ngroup + 1);
    double2 acc = make_double2(0.0, 0.0);
    const double2* p = partial + ((size_t)chain * LL.pstride + soff[g]) * BLK + t;
    const int nsplit = soff[g + 1] - soff[g];
    int s = 0;
    for (; s + 8 <= nsplit; s += 8) {
        double2 x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = p[(size_t)(s + q) * BLK];
#pragma unroll
        for (int q = 0; q < 8; ++q) { acc.x += x[q].x; acc.y += x[q].y; }
    }
    for (; s < nsplit; ++s) { const double2 x = p[(size_t)s * BLK]; acc.x += x.x; acc.y += x.y; }
    const size_t img = (size_t)g + (size_t)LL.ngroup * (c0 + chain);
    mu[(img * nmom + n) * BLK + lattice_out_index<L>(t)] = acc;
}

// The call's divergence test on the sums it forms anyway: sum_g sum(real(M_g(n))) > bound[chain] = 1000 max(1, sum |c|^2).  A recurrence
// that diverges grows wherever the vector is non-zero.  One workgroup per chain of the batch: a thread adds its element's real part over
// the groups in order, thread 0 the elements in order.
__global__ __launch_bounds__(LATTICE_THREADS) void k_lattice_diverge(const double2* __restrict__ mu, int c0, int n, int nmom, int ngroup,
                                                                     const double* __restrict__ bound, int* status) {
    __shared__ double re[BLK];
    const int chain = blockIdx.x, t = threadIdx.x;
    if (t < BLK) {
        double s = 0.0;
        for (int g = 0; g < ngroup; ++g) s += mu[(((size_t)g + (size_t)ngroup * (c0 + chain)) * nmom + n) * BLK + t].x;
        re[t] = s;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int e = 0; e < BLK; ++e) s += re[e];
        if (!(s <= bound[chain])) atomicOr(status, 2);           // (a NaN has diverged too)
    }
}

}  // namespace rsrec
