// shamir_arith.hpp -- the arithmetic of ONE output of the small-weight Shamir encode (kernels_shamir.hpp), free of HIP: the kernel
// and a CPU program (tests/cpp/shamir_dump.cpp) run exactly this code.
//
//   y = sum_{k <= d} c_k w_k  mod p,      c_k canonical field elements (c_k < p), w_k plain integers below 2^64
//
// Elements are NL 32-bit limbs (8 over bls12-381 Fr, 2 over Goldilocks), little-endian, canonical in and canonical out: no
// Montgomery form anywhere.  The d + 1 products are summed in an accumulator of NL + 3 limbs and reduced ONCE:
//
//   the bound      (d + 1) (2^64 - 1) (p - 1) < 2^(32 (NL + 3)).  Since p < 2^(32 NL) it holds whenever d + 1 <= 2^32; the route
//                  planner (shamir_route.hpp: SHAMIR_MAX_TERMS) admits far fewer terms than that.
//   the reduction  Barrett on the top four limbs: with a = 32 (NL - 1), A_hi = floor(A / 2^a) < 2^128 and
//                  mu = floor(2^(a + 128) / p) (four limbs), q' = floor(A_hi mu / 2^128) satisfies q - 2 <= q' <= q for
//                  q = floor(A / p): A_hi 2^a / p is within 2^a / p < 2^-30 of A / p, and replacing 2^(a+128) / p by mu loses less
//                  than A_hi / 2^128 < 1.  So r = A - q' p lies in [0, 3 p), is computed modulo 2^(32 (NL + 1)) > 3 p, and at most two
//                  subtractions of p make it canonical.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SHAMIR_HD __host__ __device__ __forceinline__
#define SHAMIR_UNROLL _Pragma("unroll")
#else
#define SHAMIR_HD inline
#define SHAMIR_UNROLL
#endif

namespace hbmpc {
namespace shamir {

// the field of an element width: modulus and Barrett constant as 32-bit limbs
template <int NL>
struct Mod;
template <>
struct Mod<8> {  // bls12-381 Fr
    static SHAMIR_HD uint32_t p(int i) {
        constexpr uint32_t P[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
        return P[i];
    }
    static SHAMIR_HD uint32_t mu(int i) {  // floor(2^352 / p)
        constexpr uint32_t MU[4] = {0x38b5dcb7u, 0xfede377cu, 0x355094edu, 0x00000002u};
        return MU[i];
    }
};
template <>
struct Mod<2> {  // Goldilocks, p = 2^64 - 2^32 + 1
    static SHAMIR_HD uint32_t p(int i) {
        constexpr uint32_t P[2] = {0x00000001u, 0xffffffffu};
        return P[i];
    }
    static SHAMIR_HD uint32_t mu(int i) {  // floor(2^160 / p)
        constexpr uint32_t MU[4] = {0xfffffffeu, 0xffffffffu, 0x00000000u, 0x00000001u};
        return MU[i];
    }
};

template <int NL>
struct Acc {
    uint32_t a[NL + 3];
};

template <int NL>
SHAMIR_HD void acc_zero(Acc<NL>& A) {
SHAMIR_UNROLL
    for (int i = 0; i < NL + 3; ++i) A.a[i] = 0;
}

// A += c * w32 * 2^(32 off), off = 0 or 1 (one multiply-add chain of NL steps, then the carry into the top limbs)
template <int NL>
SHAMIR_HD void acc_mac32(Acc<NL>& A, const uint32_t* c, uint32_t w32, int off) {
    uint64_t carry = 0;
SHAMIR_UNROLL
    for (int j = 0; j < NL; ++j) {
        const uint64_t t = (uint64_t)c[j] * w32 + A.a[j + off] + carry;  // <= (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
        A.a[j + off] = (uint32_t)t;
        carry = t >> 32;
    }
SHAMIR_UNROLL
    for (int j = NL + off; j < NL + 3; ++j) {
        const uint64_t t = (uint64_t)A.a[j] + carry;
        A.a[j] = (uint32_t)t;
        carry = t >> 32;
    }
}

// A += c * w, w < 2^64.  W32: the caller knows w < 2^32 (every weight of the call is: one chain instead of two)
template <int NL, bool W32>
SHAMIR_HD void acc_mac(Acc<NL>& A, const uint32_t* c, uint64_t w) {
    acc_mac32<NL>(A, c, (uint32_t)w, 0);
    if (!W32) acc_mac32<NL>(A, c, (uint32_t)(w >> 32), 1);
}

// out = A mod p, canonical (A < 2^(32 (NL + 3)): the bound above)
template <int NL>
SHAMIR_HD void acc_reduce(const Acc<NL>& A, uint32_t* out) {
    typedef Mod<NL> M;
    // prod = A_hi * mu, eight limbs; q' = its top four
    uint32_t prod[8];
SHAMIR_UNROLL
    for (int i = 0; i < 8; ++i) prod[i] = 0;
SHAMIR_UNROLL
    for (int i = 0; i < 4; ++i) {
        uint64_t carry = 0;
SHAMIR_UNROLL
        for (int j = 0; j < 4; ++j) {
            const uint64_t t = (uint64_t)A.a[NL - 1 + i] * M::mu(j) + prod[i + j] + carry;
            prod[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
        prod[i + 4] = (uint32_t)carry;
    }
    // qp = q' p modulo 2^(32 (NL + 1))
    uint32_t qp[NL + 1];
SHAMIR_UNROLL
    for (int i = 0; i < NL + 1; ++i) qp[i] = 0;
SHAMIR_UNROLL
    for (int i = 0; i < 4; ++i) {
        uint64_t carry = 0;
SHAMIR_UNROLL
        for (int j = 0; j < NL; ++j) {
            if (i + j < NL + 1) {
                const uint64_t t = (uint64_t)prod[4 + i] * M::p(j) + qp[i + j] + carry;
                qp[i + j] = (uint32_t)t;
                carry = t >> 32;
            }
        }
        if (i + NL < NL + 1) qp[i + NL] += (uint32_t)carry;  // i = 0 only: the limb was still zero
    }
    // r = A - qp modulo 2^(32 (NL + 1)), in [0, 3 p)
    uint32_t r[NL + 1];
    uint32_t borrow = 0;
SHAMIR_UNROLL
    for (int i = 0; i < NL + 1; ++i) {
        const uint64_t t = (uint64_t)A.a[i] - qp[i] - borrow;
        r[i] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
    }
    // at most two subtractions of p
SHAMIR_UNROLL
    for (int pass = 0; pass < 2; ++pass) {
        uint32_t s[NL + 1];
        borrow = 0;
SHAMIR_UNROLL
        for (int i = 0; i < NL + 1; ++i) {
            const uint64_t t = (uint64_t)r[i] - (i < NL ? M::p(i) : 0u) - borrow;
            s[i] = (uint32_t)t;
            borrow = (uint32_t)(t >> 63);
        }
        if (!borrow) {  // r >= p
SHAMIR_UNROLL
            for (int i = 0; i < NL + 1; ++i) r[i] = s[i];
        }
    }
SHAMIR_UNROLL
    for (int i = 0; i < NL; ++i) out[i] = r[i];
}

// one output, start to end: what the CPU program checks against big-integer arithmetic
template <int NL, bool W32>
SHAMIR_HD void dot_mod(const uint32_t* coeffs, const uint64_t* w, int terms, uint32_t* out) {
    Acc<NL> A;
    acc_zero<NL>(A);
    for (int k = 0; k < terms; ++k) acc_mac<NL, W32>(A, coeffs + (long)k * NL, w[k]);
    acc_reduce<NL>(A, out);
}

}  // namespace shamir
}  // namespace hbmpc
