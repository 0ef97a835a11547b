// kernels_sqrt.hpp -- square roots, inverses and RandBit's last step on the device (fpmul/rand_bit.rs:197-220).
//
// Both fields have p - 1 = 2^32 T with T odd, and ark-ff 0.5 takes square roots by Tonelli-Shanks with z = omega = 7^T
// (TWO_ADIC_ROOT_OF_UNITY), w = A^((T-1)/2), x = A w, b = x w, then the loop "find the order 2^k of b, w = z^(2^(v-k-1)),
// z = w^2, b *= z, x *= w, v = k".  That loop branches on the data; its result has a closed form (tests/randbit_ref.py checks it
// against a line-by-line restatement of the loop):
//   u = A^((T-1)/2), g = u^2 A = A^T = omega^L with L in [0, 2^32)
//   A is a square iff L is even; then ark returns x = A u omega^E with E = (-L/2) mod 2^31
// (each iteration multiplies x by omega^(2^(31-k_i)) for strictly decreasing k_i in [1, 31], so E < 2^31, and x^2 = A forces
// 2E = -L mod 2^32).  L is a discrete log in the 2^32-element subgroup: four 8-bit Pohlig-Hellman windows, each a reverse look-up in
// the 256-element subgroup keyed by a bit slice of a hash of the value's two low limbs (the host proves the slice collision-free,
// tables_sqrt.hpp).
// RandBit needs only x^-1 2^-1, and x^-1 = u omega^(-(L + E)): since u^2 A = omega^L, x u omega^(-L-E) = A u^2 omega^-L = 1 -- so the
// finalize runs no inversion at all.  Every product is in Montgomery form (device-constant form: mont(a, b) = a b / R); the
// table entries are stored in that form, so the look-up keys are slices of Montgomery-form values.
#pragma once
#include "fr_gold.hpp"
#include "fr_sat.hpp"
#include "fr_u29.hpp"
#include "sqrt_args.hpp"

namespace hbmpc {

enum { RB_OK = 0, RB_ZERO = 1, RB_NO_ROOT = 2 };

template <class F>
HB_DEV typename F::E sq_mul(const typename F::E& a, const typename F::E& b) {
    return F::cond_sub_r(F::mont(a, b));
}
template <class F>
HB_DEV typename F::E sq_mulc(const typename F::E& a, const uint32_t* __restrict__ c) {
    return F::cond_sub_r(F::mont(a, c));
}
// x^e for a fixed, wave-uniform exponent whose top bit is bit nbits - 1 (the branch is uniform: no divergence)
template <class F>
HB_DEV typename F::E pow_fixed(const typename F::E& x, const uint32_t* __restrict__ e, int nbits) {
    typename F::E acc = x;
    for (int i = nbits - 2; i >= 0; --i) {
        acc = sq_mul<F>(acc, acc);
        if ((e[i >> 5] >> (i & 31)) & 1u) acc = sq_mul<F>(acc, x);
    }
    return acc;
}
// the look-up key: a multiplicative hash (SQRT_KEY_MUL, sqrt_args.hpp) of the two low limbs (Goldilocks' subgroup elements repeat in either 32-bit half)
template <class F>
HB_DEV uint32_t sqrt_key(const SqrtTab& t, const typename F::E& x) {
    const uint64_t w = ((uint64_t)x.l[1] << 32) | x.l[0];
    return t.keyt[(uint32_t)((w * SQRT_KEY_MUL) >> t.kshift) & t.kmask];
}
// omega^v for any v < 2^32 (three products of table entries)
template <class F>
HB_DEV typename F::E omega_pow(const SqrtTab& t, uint32_t v) {
    constexpr int NL = F::NL;
    typename F::E w = F::load_const(t.posw + (size_t)(v & 255u) * NL);
    w = sq_mulc<F>(w, t.posw + (size_t)(256 + ((v >> 8) & 255u)) * NL);
    w = sq_mulc<F>(w, t.posw + (size_t)(512 + ((v >> 16) & 255u)) * NL);
    return sq_mulc<F>(w, t.posw + (size_t)(768 + (v >> 24)) * NL);
}
// am: A in Montgomery form, canonical.  Returns u = A^((T-1)/2) (Montgomery form) and L with A^T = omega^L.
template <class F>
HB_DEV typename F::E sqrt_core(const SqrtTab& t, const typename F::E& am, uint32_t& L) {
    using E = typename F::E;
    constexpr int NL = F::NL;
    const E u = pow_fixed<F>(am, t.e_sqrt, t.bits_sqrt);
    const E g = sq_mul<F>(sq_mul<F>(u, u), am);
    E g8 = g;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) g8 = sq_mul<F>(g8, g8);
    E g16 = g8;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) g16 = sq_mul<F>(g16, g16);
    E h = g16;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) h = sq_mul<F>(h, h);
    const uint32_t l0 = sqrt_key<F>(t, h);  // g^(2^24) = omega^(l0 2^24)
    h = sq_mulc<F>(g16, t.negw + (size_t)(512 + l0) * NL);
    const uint32_t l1 = sqrt_key<F>(t, h);
    h = sq_mulc<F>(sq_mulc<F>(g8, t.negw + (size_t)(256 + l0) * NL), t.negw + (size_t)(512 + l1) * NL);
    const uint32_t l2 = sqrt_key<F>(t, h);
    h = sq_mulc<F>(sq_mulc<F>(sq_mulc<F>(g, t.negw + (size_t)l0 * NL), t.negw + (size_t)(256 + l1) * NL), t.negw + (size_t)(512 + l2) * NL);
    const uint32_t l3 = sqrt_key<F>(t, h);
    L = l0 | (l1 << 8) | (l2 << 16) | (l3 << 24);
    return u;
}
template <class F>
HB_DEV typename F::E to_mont(const SqrtTab& t, const typename F::E& a) {
    return F::cond_sub_r(F::mulc(a, t.r2));
}

// Field::sqrt of every element: root_out = ark's root (0 where there is none), has_root_out = 1 / 0 (sqrt(0) = 0 has a root)
template <class F>
__global__ __launch_bounds__(256) void k_sqrt(const uint32_t* __restrict__ a, size_t N, SqrtTab t, uint32_t* __restrict__ root_out,
                                              uint8_t* __restrict__ has_root_out) {
    using E = typename F::E;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const E A = F::load(a + i * F::EW);
    const bool zero = F::is_zero_canon(A);
    const E am = to_mont<F>(t, A);
    uint32_t L;
    const E u = sqrt_core<F>(t, am, L);
    const bool ok = zero || (L & 1u) == 0;
    E x = F::zero();
    if (!zero && ok) {
        const uint32_t Ee = (0u - (L >> 1)) & 0x7fffffffu;
        x = sq_mul<F>(sq_mul<F>(am, u), omega_pow<F>(t, Ee));
        x = sq_mulc<F>(x, t.one_p);  // leave Montgomery form
    }
    F::store_lt2r(root_out + i * F::EW, x);
    has_root_out[i] = ok ? 1 : 0;
}

// Field::inverse of every element (Fermat), B per lane by Montgomery's trick: one inversion and 3 (B - 1) products for B elements;
// zero enters the product as 1 and gets ok = 0 and a zero output
template <class F, int B>
__global__ __launch_bounds__(256) void k_inverse(const uint32_t* __restrict__ a, size_t N, SqrtTab t, uint32_t* __restrict__ inv_out,
                                                 uint8_t* __restrict__ ok_out) {
    using E = typename F::E;
    const size_t base = (size_t)blockIdx.x * blockDim.x * B + threadIdx.x;
    if (base >= N) return;
    const E one = to_mont<F>(t, F::load_const(t.one_p));
    E x[B], pre[B];
    bool live[B];
    E run = one;
#pragma unroll
    for (int k = 0; k < B; ++k) {
        const size_t i = base + (size_t)k * blockDim.x;
        live[k] = false;
        x[k] = one;
        if (i < N) {
            const E v = F::load(a + i * F::EW);
            live[k] = !F::is_zero_canon(v);
            if (live[k]) x[k] = to_mont<F>(t, v);
        }
        pre[k] = run;  // product of the entries before k
        run = sq_mul<F>(run, x[k]);
    }
    E inv = pow_fixed<F>(run, t.e_inv, t.bits_inv);  // (prod x)^-1
#pragma unroll
    for (int k = B - 1; k >= 0; --k) {
        const E inv_k = sq_mul<F>(inv, pre[k]);
        inv = sq_mul<F>(inv, x[k]);
        const size_t i = base + (size_t)k * blockDim.x;
        if (i >= N) continue;
        F::store_lt2r(inv_out + i * F::EW, live[k] ? sq_mulc<F>(inv_k, t.one_p) : F::zero());
        ok_out[i] = live[k] ? 1 : 0;
    }
}

// RandBit phase 2 (rand_bit.rs:197-220) for `parties` parties: a [parties][N] the shares of a, sq [N] the opened squares A = a^2.
//   out[p][i] = ([a]_p b^-1 + 1) 2^-1 = [a]_p s + 2^-1 with s = b^-1 2^-1, b = A.sqrt()
// status[i] = 0 ok, 1 A = 0 (ZeroSquare), 2 no root (SquareRoot); a failed element's shares are zero for every party.
template <class F>
__global__ __launch_bounds__(256) void k_randbit_finalize(const uint32_t* __restrict__ a, const uint32_t* __restrict__ sq, size_t N,
                                                          unsigned parties, SqrtTab t, uint32_t* __restrict__ out,
                                                          uint8_t* __restrict__ status, RandBitSummaryDev* __restrict__ summary) {
    using E = typename F::E;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const E A = F::load(sq + i * F::EW);
    const bool zero = F::is_zero_canon(A);
    const E am = to_mont<F>(t, A);
    uint32_t L;
    const E u = sqrt_core<F>(t, am, L);
    const uint32_t st = zero ? RB_ZERO : (L & 1u) ? RB_NO_ROOT : RB_OK;
    status[i] = (uint8_t)st;
    if (st != RB_OK) {
        atomicMin(&summary->first, ((unsigned long long)st << 32) | (unsigned long long)i);
        atomicAdd(&summary->n_failed, 1u);
        for (unsigned p = 0; p < parties; ++p) F::store_lt2r(out + ((size_t)p * N + i) * F::EW, F::zero());
        return;
    }
    const uint32_t Ee = (0u - (L >> 1)) & 0x7fffffffu;
    // s = x^-1 2^-1 = u omega^(-(L + E)) 2^-1, Montgomery form
    const E s = sq_mulc<F>(sq_mul<F>(u, omega_pow<F>(t, 0u - (L + Ee))), t.half);
    const E hp = F::load_const(t.half_p);
    for (unsigned p = 0; p < parties; ++p) {
        const size_t ip = (size_t)p * N + i;
        const E v = sq_mul<F>(F::load(a + ip * F::EW), s);  // a_p s, canonical data
        F::store_loose(out + ip * F::EW, F::add(v, hp));
    }
}
}  // namespace hbmpc
