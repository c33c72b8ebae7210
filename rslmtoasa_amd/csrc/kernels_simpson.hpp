// The one Simpson rule of the library: simpson_f(fermi = .true.) of math_mod (math.f90:1600-1632) with fermifun (:994-1000), in the
// reference's summation order and without FMA contraction.  Used by the exchange module's integrals (kernels_exchange.hpp,
// kernels_auxgreen.hpp) and by the conductivity tensor (kernels_cond.hpp).
//
// The reference's loop runs I = 2, nv1 + 9, 2 and adds Y(I - 1) f(I - 1) + 4 Y(I) f(I) + Y(I + 1) f(I + 1); on the meshes energy%e_mesh
// makes (nen = nv1 + 9) the last I reads Y(nv1 + 10) and Ene(nv1 + 10), one element past both arrays.  Here every term whose index lies
// above nen is ZERO: the value the reference gives whenever the stray element happens to be zero.
#pragma once
#include <hip/hip_runtime.h>

namespace rsrec {

// kBT of simpson_f for its argument T (:1611-1616); T = 0 leaves 1e-15, far below every mesh step: the weights are then 1, 0.5, 0 exactly
__device__ __forceinline__ double simpson_kbt(double T) {
#pragma clang fp contract(off)
    return 0.633362019e-5 * T + 1.0e-15;
}

// fermifun (math.f90:994-1000); exp overflows to inf far above ef by design: 1 / (inf + 1) = 0
__device__ __forceinline__ double fermifun(double e, double ef, double kbt) {
#pragma clang fp contract(off)
    return 1.0 / (exp((e - ef) / kbt) + 1.0);
}

// The terms I = ibeg, ibeg + 2, ... <= iend (1-based, ibeg even) of the rule, added onto A in the reference's order.  w(k), y(k): Fermi weight
// and integrand at 0-based k; y answers zero from nen on.  Precondition: iend <= nen (the callers refuse nen < nv1 + 9), so w(k - 1), which
// is read unguarded, has k - 1 <= nen - 2; w(k) and w(k + 1) are asked for below nen only.  A caller may walk the loop in pieces (weights
// staged tile by tile) and gets the bits of one pass.
template <class W, class Y>
__device__ __forceinline__ double simpson_fermi_terms(double A, int ibeg, int iend, int nen, W w, Y y) {
#pragma clang fp contract(off)
    for (int I = ibeg; I <= iend; I += 2) {
        const int k = I - 1;                                        // 0-based index of Y(I)
        const double f0 = w(k - 1), f1 = k < nen ? w(k) : 0.0, f2 = k + 1 < nen ? w(k + 1) : 0.0;
        A = ((A + y(k - 1) * f0) + 4.0 * y(k) * f1) + y(k + 1) * f2;
    }
    return A;
}

// simpson_f(fermi = .true.) of one integrand: H A / 3 over I = 2 .. nv1 + 9 (nen >= nv1 + 9)
template <class W, class Y>
__device__ __forceinline__ double simpson_fermi(int nen, int nv1, double H, W w, Y y) {
#pragma clang fp contract(off)
    return H * simpson_fermi_terms(0.0, 2, nv1 + 9, nen, w, y) / 3.0;
}

}  // namespace rsrec
