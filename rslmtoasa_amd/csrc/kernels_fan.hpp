// Pair moments from one Chebyshev chain per atom (rsrec_chebyshev_pairs_direct).
//
// The four chains chebyshev_recur_ij runs per pair (recursion.f90:2376-2487) are only ever recombined (green.f90:446-453) into
//   M_ij(n) = <i| T_n(H~) |j>,   M_ji(n) = <j| T_n(H~) |i>,
// and M_ji(n) is the 18x18 block at atom j of the Chebyshev vector psi_n started from the identity at atom i.  One chain per SOURCE atom
// therefore serves every pair that atom belongs to: after each order k_fan_gather copies the blocks of the chain's TARGET atoms out of the
// vector just written, and at the end k_fan_pack builds the four-slot image the pair stages read.  No Gram pass, no reduction: the only
// sum is the divergence test on the source's own block, which runs in a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_valu.hpp"

namespace rsrec {

constexpr int FAN_THREADS = 384;     // six waves: 324 elements of a block, the rest idle

// One gathered block: target atom `atom` of the chain of source `chain` (index among the call's sources).  `first` is the level of the
// chain's growing region at which the atom joins it (-1: never); `own`: the atom is the source itself.
struct FanEntry { int chain, atom, first, own; };

// One pair: the entries its blocks come from.  mode 0: i == j (ii alone is read); 1: i != j, M_ij := M_ji^H (ji alone is read);
// 2: i != j, all four blocks from their own sources.
struct FanPair { int ji, ij, ii, jj, mode; };

// img[entry][n] = block `atom` of `vec` (the Chebyshev vector of order n, region level `level`) for the entries e0 .. e0 + gridDim.x - 1,
// whose chains are c0 .. of the batch `vec` holds.  A target outside the region at this level is written as exact zeros -- decided from
// `first`, never from what the work vector holds there.  The source's own block also gets the reference's divergence test (:2479).
template <class L>
__global__ __launch_bounds__(FAN_THREADS) void k_fan_gather(const double* __restrict__ vec, size_t vstride, const FanEntry* __restrict__ ent, int e0, int c0,
                                                            int level, int n, int nmom, double2* __restrict__ img, int* status) {
    __shared__ double tr[BLK];
    const int e = e0 + blockIdx.x, tid = threadIdx.x;
    const FanEntry E = ent[e];
    const bool reached = E.first >= 0 && E.first <= level;
    double2 v = make_double2(0.0, 0.0);
    if (tid < BLK) {
        if (reached) v = L::ld(vec + (size_t)(E.chain - c0) * vstride + (size_t)BLD * E.atom, tid % NB, tid / NB);
        img[((size_t)e * nmom + n) * BLK + tid] = v;
    }
    if (!E.own) return;                                      // (uniform over the workgroup)
    if (tid < BLK) tr[tid] = v.x;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int q = 0; q < BLK; ++q) s += tr[q];
        if (s > 1000.0) atomicOr(status, 2);
    }
}

// The four slots of pair blockIdx.y at moment blockIdx.x, and (m_pair != nullptr) M_ij and M_ji themselves.
//   mode 0: h = M_ii / 2 in all four slots (the reference's second seed coefficient overwrites the first)
//   mode 1: s1 = (M_ij + M_ji)/2, s2 = -s1, s3 = i (M_ij - M_ji)/2, s4 = -s3            (the slots without (M_ii + M_jj)/2)
//   mode 2: d = (M_ii + M_jj)/2: s1 = d + o, s2 = d - o, s3 = d + q, s4 = d - q with o, q the values of mode 1
__global__ __launch_bounds__(FAN_THREADS) void k_fan_pack(const double2* __restrict__ img, const FanPair* __restrict__ pairs, int nmom, double2* __restrict__ mu,
                                                          double2* __restrict__ m_pair) {
    const int n = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    if (tid >= BLK) return;
    const FanPair P = pairs[p];
    auto blk = [&](int e) { return img + ((size_t)e * nmom + n) * BLK; };
    double2 mij, mji, s1, s2, s3, s4;
    if (P.mode == 0) {
        mij = mji = blk(P.ii)[tid];
        s1 = s2 = s3 = s4 = make_double2(0.5 * mij.x, 0.5 * mij.y);
    } else {
        mji = blk(P.ji)[tid];
        if (P.mode == 1) {
            const double2 t = blk(P.ji)[tid / NB + NB * (tid % NB)];     // M_ij = M_ji^H
            mij = make_double2(t.x, -t.y);
        } else mij = blk(P.ij)[tid];
        const double2 o = make_double2(0.5 * (mij.x + mji.x), 0.5 * (mij.y + mji.y));
        const double2 q = make_double2(-0.5 * (mij.y - mji.y), 0.5 * (mij.x - mji.x));
        if (P.mode == 1) {
            s1 = o; s2 = make_double2(-o.x, -o.y); s3 = q; s4 = make_double2(-q.x, -q.y);
        } else {
            const double2 a = blk(P.ii)[tid], b = blk(P.jj)[tid];
            const double2 d = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y + b.y));
            s1 = make_double2(d.x + o.x, d.y + o.y); s2 = make_double2(d.x - o.x, d.y - o.y);
            s3 = make_double2(d.x + q.x, d.y + q.y); s4 = make_double2(d.x - q.x, d.y - q.y);
        }
    }
    double2* m = mu + ((size_t)4 * p * nmom + n) * BLK + tid;
    const size_t slot = (size_t)nmom * BLK;
    m[0] = s1; m[slot] = s2; m[2 * slot] = s3; m[3 * slot] = s4;
    if (m_pair) {
        double2* mp = m_pair + ((size_t)2 * p * nmom + n) * BLK + tid;
        mp[0] = mij; mp[slot] = mji;
    }
}

}  // namespace rsrec
