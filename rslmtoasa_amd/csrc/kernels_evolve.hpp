// Wave-packet propagation (rsrec_chebyshev_evolve): one time step is a Chebyshev sum over the orders of a table w the caller computed,
//   psi' = sum_n w_n p_n,   p_n = T_n(H~) psi,
//   chi' = sum_n w_n g_n,   g_0 = chi,  g_1 = H~ g_0 + (1/a) D p_0,  g_{n+1} = 2 H~ g_n - g_{n-1} + (2/a) D p_n,
// so that with D = [X, H] and w the coefficients of exp(-i H tau):  psi' = U psi,  chi' = [X, U] psi + U chi.
// The p chain and the g chain of a vector advance as two chains of the same k_spmm5 launches, whose Chebyshev epilogue writes the
// homogeneous part 2 H~ g_n - g_{n-1}; one more launch per order forms D p_n, and the pass of this header -- the per-order hot path beside
// the SpMM -- adds the source term and the order's share of both sums.
//
// Layout.  Whole-lattice vectors in CI layout as a flat stream of 16-byte complex elements, `total` = kk * 324 of them per chain (block kk,
// the zero block, is never touched).  A slot holds the 2 nb chains of a batch side by side: chains 0 .. nb - 1 are the p chains, chains
// nb .. 2 nb - 1 the g chains of the same vectors.
//
// Source add.  g(n + 1) += f (D p_n), f real (1/a behind order 0, 2/a behind the others): two FMAs per element, stored back because the
// next product reads it.  It runs behind every order.
//
// Accumulation.  y += w_n x in ascending n with the four FMAs of map_axpy (kernels_blochmap.hpp).  Two forms of the same FMA sequence:
//   fused    k_evo_source<true> adds order n + 1 of both chains in the pass that adds the source: y is read and written once per order;
//   batched  k_evo_source<false> adds the source alone (g chains only) and k_evo_accum adds PT orders of a ring per pass, as k_shot_accum
//            does: y is read and written once per PT orders, the orders are read a second time.
// Either way an element sees  y = 0; y += w_0 x_0; y += w_1 x_1; ...  with x_n of the g chain taken after its source add -- a pass border
// only stores y and loads it again -- so the bits depend on neither the form nor the ring's depth.  VALU FMAs on purpose, as in
// kernels_shot.hpp.  The weights are uniform over a workgroup: their address depends on kernel arguments and loop counters alone.
//
// Moments.  m_n = chi^H T_{n-1}(H~) chi is L^H W over the whole lattice with L = chi fixed and W = an order of the moment chain's ring:
// exactly k_shot_gram / k_shot_gram_valu / k_shot_gram_reduce (kernels_shot.hpp) with a left stride of 0 and the ring's slot stride on
// the right, column e of a launch = the e-th order it covers.  Every column is a task of its own with the slice partition of shot_ksplit
// and the fixed-order reduce, so a moment's bits do not depend on how many orders a launch covers.  No kernel of its own is needed.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_blochmap.hpp"
#include "kernels_shot.hpp"

namespace rsrec {

constexpr int EVO_THREADS = 256;
constexpr int EVO_ORDERS_MAX = 16;            // orders a batched pass adds at most (option evolve_orders)
constexpr int EVO_SOURCE_U = 4;               // elements per thread of the per-order pass

// chain 0 of the slots that hold the orders of a batched pass (entries from `cnt` on repeat entry 0 and are never read)
struct EvoOrders { const double2* x[EVO_ORDERS_MAX]; };

// The per-order pass.  grid (workgroups over `total`, chains): chain = chain0 + blockIdx.y of slot X (order n + 1).
//   g chains (chain >= nb):  x += f dp[chain - nb], stored;      every chain, if ACC:  y += w x.
// Fused form: chain0 = 0 over 2 nb chains with ACC; batched form: chain0 = nb over the nb g chains without.
template <bool ACC>
__global__ __launch_bounds__(EVO_THREADS) void k_evo_source(double2* __restrict__ X, const double2* __restrict__ DP, double f, size_t vstride, size_t total, int nb,
                                                            int chain0, const double2* __restrict__ w, double2* __restrict__ Y) {
    const int chain = chain0 + blockIdx.y;
    const bool g = chain >= nb;                                    // (uniform over the workgroup)
    const size_t base = (size_t)blockIdx.x * (EVO_THREADS * EVO_SOURCE_U) + threadIdx.x;
    double2* x = X + (size_t)chain * vstride;
    const double2* dp = DP + (size_t)(g ? chain - nb : 0) * vstride;
    double2* y = Y + (size_t)chain * vstride;
    bool in[EVO_SOURCE_U];
    double2 xv[EVO_SOURCE_U], dv[EVO_SOURCE_U], yv[EVO_SOURCE_U];
#pragma unroll
    for (int u = 0; u < EVO_SOURCE_U; ++u) in[u] = base + (size_t)u * EVO_THREADS < total;
#pragma unroll
    for (int u = 0; u < EVO_SOURCE_U; ++u) {
        const size_t q = base + (size_t)u * EVO_THREADS;
        xv[u] = in[u] ? x[q] : make_double2(0.0, 0.0);
        dv[u] = in[u] && g ? dp[q] : make_double2(0.0, 0.0);
        if (ACC) yv[u] = in[u] ? y[q] : make_double2(0.0, 0.0);
    }
    if (g) {
#pragma unroll
        for (int u = 0; u < EVO_SOURCE_U; ++u) {
            xv[u].x = fma(f, dv[u].x, xv[u].x); xv[u].y = fma(f, dv[u].y, xv[u].y);
            if (in[u]) x[base + (size_t)u * EVO_THREADS] = xv[u];
        }
    }
    if (ACC) {
        const double2 wn = w[0];
#pragma unroll
        for (int u = 0; u < EVO_SOURCE_U; ++u) {
            map_axpy(yv[u], wn, xv[u]);
            if (in[u]) y[base + (size_t)u * EVO_THREADS] = yv[u];
        }
    }
}

// Y[chain][:] += sum_{p < cnt} w[p] X.x[p][chain][:].  grid (workgroups over `total`, chains).  PT >= cnt orders are held in registers
// for U elements per thread (PT * U = 16 loads in flight but for PT <= 2), as in k_shot_accum.
template <int PT, int U>
__global__ __launch_bounds__(EVO_THREADS) void k_evo_accum(EvoOrders X, int cnt, size_t vstride, size_t total, const double2* __restrict__ w, double2* __restrict__ Y) {
    const int chain = blockIdx.y;
    const size_t base = (size_t)blockIdx.x * (EVO_THREADS * U) + threadIdx.x;
    double2* y = Y + (size_t)chain * vstride;
    bool in[U];
    double2 x[PT][U], acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) in[u] = base + (size_t)u * EVO_THREADS < total;
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        const bool live = p < cnt;                             // (uniform; no early exit: x stays in registers)
        const double2* xs = X.x[p] + (size_t)chain * vstride;
#pragma unroll
        for (int u = 0; u < U; ++u) x[p][u] = live && in[u] ? xs[base + (size_t)u * EVO_THREADS] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = in[u] ? y[base + (size_t)u * EVO_THREADS] : make_double2(0.0, 0.0);
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        if (p < cnt) {
            const double2 wp = w[p];
#pragma unroll
            for (int u = 0; u < U; ++u) map_axpy(acc[u], wp, x[p][u]);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (in[u]) y[base + (size_t)u * EVO_THREADS] = acc[u];
}

}  // namespace rsrec
