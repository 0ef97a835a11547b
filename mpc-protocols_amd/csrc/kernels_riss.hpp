// kernels_riss.hpp -- PRandBit / PRandInt on the device (fpmul/prandbitd.rs): the fold of the senders' replicated shares
// (:638-647, :667-684), the RISS-to-Shamir conversion (try_advance_from_riss, :311-356) and the last step of PRandBit
// (try_finalize_bit, :189-211).
//
// The conversion is a constant-matrix map.  For the maximal unqualified sets T (combinations(0..n, t)) and a party j,
//   share_F[j][i]  = sum_T r_T[i] f_T(alpha_j)             in the context's prime field
//   share_2[j][i]  = xor_T (r_T[i] & 1) f2_T(3^j)          in GF(2^8) (AES polynomial 0x11B)
// with f_T(x) = prod_{m in T} (1 - x / alpha_m); f_T(alpha_j) = 0 exactly when j is in T.  A folded r_T is below 2^62 (the
// reference's capacity check k + l + 2 + ceil(log2 n) < 64), so it is a plain integer of two 32-bit words and F::from never
// reduces it: a term is a 64-bit x 256-bit (Goldilocks: 64 x 64) INTEGER product, and the sum over T is reduced once.
//
// Form of the products: vector multiply-adds into lazy columns, not matrix cores.  With r = r1 2^32 + r0 and the coefficient in
// 32-bit words c_0 .. c_7, the product r_a c_b goes to column a + b: a 64-bit sum with a 32-bit carry count (one v_mad_u64_u32
// with carry out + one v_addc per product, the form of Gold::Acc in fr_gold.hpp), 32 instructions per Fr term, 8 per Goldilocks
// term.  Accumulator bound proven for the supported shapes: a column receives at most 2 products < 2^64 per term and there are at
// most RISS_MAX_TSETS = 8192 terms, so a column sum is < 2^78 and is held exactly in its 64 + 32 bits (headroom: 2^31 terms).  The
// whole sum is < 2^13 2^62 2^255 = 2^330: eleven 32-bit words after the carries are resolved, reduced as
// lo + 2^224 hi with lo < 2^224, hi < 2^106 -- two Montgomery products by constants in the context's own representation.
// A lane is an element and a wave is a set of parties, so the coefficients are wave-uniform and come through the scalar cache.
#pragma once
#include "fr_gold.hpp"
#include "fr_sat.hpp"
#include "fr_u29.hpp"
#include "riss_args.hpp"

namespace hbmpc {

template <class F>
HB_DEV typename F::E riss_from_words(const uint32_t w[8]) {
    typename F::E r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = w[i];
    return r;
}
template <>
HB_DEV U29::E riss_from_words<U29>(const uint32_t w[8]) {
    return U29::from_words(w);
}

// the lazy sum of one output element: Fr (both implementations share it: the terms are plain integers)
template <class F>
struct RissAcc {
    static constexpr int NC = 8;       // coefficient words
    static constexpr int WORDS = 27;   // 32-bit words of the state (the in-block merge moves them through LDS)
    uint64_t c[9];
    uint32_t h[9];
    HB_DEV void zero() {
#pragma unroll
        for (int i = 0; i < 9; ++i) c[i] = 0, h[i] = 0;
    }
    // one term, ONE asm statement (separate statements that touch vcc get hazard nops between them): the product r_a k_b goes to
    // column a + b.  Operands: %0-%8 columns, %9-%17 carry counts, %18 %19 r0 r1, %20-%27 the coefficient (SGPRs)
#define HB_RISS_P(COL, CNT, A, K) "v_mad_u64_u32 %" #COL ", vcc, %" #A ", %" #K ", %" #COL "\n\tv_addc_co_u32_e32 %" #CNT ", vcc, 0, %" #CNT ", vcc\n\t"
    HB_DEV void mac(uint32_t r0, uint32_t r1, const uint32_t (&k)[8]) {
        asm(HB_RISS_P(0, 9, 18, 20) HB_RISS_P(1, 10, 18, 21) HB_RISS_P(2, 11, 18, 22) HB_RISS_P(3, 12, 18, 23)
            HB_RISS_P(4, 13, 18, 24) HB_RISS_P(5, 14, 18, 25) HB_RISS_P(6, 15, 18, 26) HB_RISS_P(7, 16, 18, 27)
            HB_RISS_P(1, 10, 19, 20) HB_RISS_P(2, 11, 19, 21) HB_RISS_P(3, 12, 19, 22) HB_RISS_P(4, 13, 19, 23)
            HB_RISS_P(5, 14, 19, 24) HB_RISS_P(6, 15, 19, 25) HB_RISS_P(7, 16, 19, 26) HB_RISS_P(8, 17, 19, 27)
            : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]), "+v"(c[8]),
              "+v"(h[0]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3]), "+v"(h[4]), "+v"(h[5]), "+v"(h[6]), "+v"(h[7]), "+v"(h[8])
            : "v"(r0), "v"(r1), "s"(k[0]), "s"(k[1]), "s"(k[2]), "s"(k[3]), "s"(k[4]), "s"(k[5]), "s"(k[6]), "s"(k[7])
            : "vcc");
    }
#undef HB_RISS_P
    HB_DEV uint32_t word(int i) const { return i < 18 ? ((i & 1) ? (uint32_t)(c[i >> 1] >> 32) : (uint32_t)c[i >> 1]) : h[i - 18]; }
    // += another partial sum given by its words
    template <class Get>
    HB_DEV void merge(Get get) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const uint64_t o = ((uint64_t)get(2 * i + 1) << 32) | get(2 * i), s = c[i] + o;
            h[i] += get(18 + i) + (s < o);
            c[i] = s;
        }
    }
    // the carries resolved: the sum as eleven 32-bit words (it is < 2^330)
    HB_DEV void resolve(uint32_t (&w)[11]) const {
        uint64_t carry = 0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {  // word k: low half of column k, high half of column k - 1, the count of column k - 2
            uint64_t s = carry;
            if (k < 9) s += (uint32_t)c[k];
            if (k >= 1 && k <= 9) s += c[k - 1] >> 32;
            if (k >= 2) s += h[k - 2];
            w[k] = (uint32_t)s;
            carry = s >> 32;
        }
    }
    // w mod r as store_loose takes it: lo + 2^224 hi
    static HB_DEV typename F::E reduce_words(const uint32_t (&w)[11], const uint32_t* __restrict__ red) {
        const uint32_t lo[8] = {w[0], w[1], w[2], w[3], w[4], w[5], w[6], 0};
        const uint32_t hi[8] = {w[7], w[8], w[9], w[10], 0, 0, 0, 0};
        const typename F::E a = F::cond_sub_r(F::mont(riss_from_words<F>(lo), red));
        const typename F::E b = F::cond_sub_r(F::mont(riss_from_words<F>(hi), red + F::NL));
        return F::add(a, b);
    }
    HB_DEV typename F::E reduce(const uint32_t* __restrict__ red) const {
        uint32_t w[11];
        resolve(w);
        return reduce_words(w, red);
    }
};
// Goldilocks: Gold's own lazy dot product (three columns)
template <>
struct RissAcc<Gold> {
    static constexpr int NC = 2;
    static constexpr int WORDS = 9;
    Gold::Acc A;
    HB_DEV void zero() { Gold::acc_zero(A); }
    HB_DEV void mac(uint32_t r0, uint32_t r1, const uint32_t (&k)[2]) {
        const Gold::E a = {{r0, r1}};
        Gold::acc_mac_pinned(A, a, k);
    }
    HB_DEV uint32_t word(int i) const {
        const uint64_t c[3] = {A.c0, A.c1, A.c2};
        const uint32_t h[3] = {A.h0, A.h1, A.h2};
        return i < 6 ? ((i & 1) ? (uint32_t)(c[i >> 1] >> 32) : (uint32_t)c[i >> 1]) : h[i - 6];
    }
    template <class Get>
    HB_DEV void merge(Get get) {
        uint64_t* c[3] = {&A.c0, &A.c1, &A.c2};
        uint32_t* h[3] = {&A.h0, &A.h1, &A.h2};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint64_t o = ((uint64_t)get(2 * i + 1) << 32) | get(2 * i), s = *c[i] + o;
            *h[i] += get(6 + i) + (s < o);
            *c[i] = s;
        }
    }
    HB_DEV Gold::E reduce(const uint32_t* __restrict__) {
        return Gold::acc_reduce(A);
    }
};

// ---- fold (prandbitd.rs:667-684, bound test :638-647) ----------------------------------------------------------------------
// contrib [n][Tn][B] -> sums [Tn][B] (all n contributions, wrapping at 2^64 only where a verdict is set) and bad [n][Tn] bytes
// (zeroed by the caller): 1 where any value of (sender, set) exceeds bound = 2^lk.  A lane that sees an offending value stores the
// byte itself: every such store writes the same 1.
template <int U>  // senders whose loads are in flight together
__global__ __launch_bounds__(256) void k_riss_fold(const uint64_t* __restrict__ contrib, unsigned n, size_t Tn, size_t B, uint64_t bound,
                                                   uint64_t* __restrict__ sums, uint8_t* __restrict__ bad) {
    const size_t nb = (B + 255) / 256;
    const size_t T = blockIdx.x / nb, i = (blockIdx.x % nb) * 256 + threadIdx.x;
    if (i >= B) return;
    const uint64_t* p = contrib + T * B + i;
    const size_t stride = Tn * B;
    uint64_t sum = 0;
#pragma unroll U
    for (unsigned s = 0; s < n; ++s) {
        const uint64_t v = __builtin_nontemporal_load(p + (size_t)s * stride);
        sum += v;
        if (v > bound) bad[(size_t)s * Tn + T] = 1;
    }
    sums[T * B + i] = sum;
}

// ---- convert (prandbitd.rs:311-356) -------------------------------------------------------------------------------------------
// r [Tn][B]; a lane is one element, a workgroup 64 elements.  Its four waves are PG = 4 / KS party groups times KS slices of the
// sets; a wave sums PPW parties: party index (blockIdx.y PG + g) PPW + q, column cols[party] (cols NULL: the party index itself).
// KS > 1: the slices' partial sums meet in LDS and the wave of slice 0 reduces and stores.  Which form runs is the caller's choice
// (capi_riss.inc; the sliced one measured faster wherever there are sets to slice).
// out [parties][B] field elements, out2 [parties][B] bytes (GF2 only).
template <class F, int PPW, int KS, bool GF2>
__global__ __launch_bounds__(256) void k_riss_convert(const uint64_t* __restrict__ r, size_t B, unsigned Tn, RissTab tab,
                                                      const uint32_t* __restrict__ cols, unsigned parties, uint32_t* __restrict__ out,
                                                      uint8_t* __restrict__ out2) {
    static_assert(KS == 1 || PPW == 1, "the in-block merge is sized for one party per wave");
    using Acc = RissAcc<F>;
    constexpr int NC = Acc::NC, PG = 4 / KS, LW = Acc::WORDS + 1;
    // several Fr parties per wave: the resolved sums wait in LDS (a lane reads back only what it wrote) and ONE copy of the two
    // Montgomery products reduces them party by party -- unrolled per party, the accumulators no longer stay in registers
    constexpr bool STAGED = PPW > 1 && Acc::NC == 8;
    __shared__ uint32_t lds[KS > 1 ? (KS - 1) * LW * 64 : STAGED ? 4 * PPW * 11 * 64 : 1];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned g = w % PG, ks = w / PG;
    const size_t i = (size_t)blockIdx.x * 64 + lane;
    const size_t il = i < B ? i : B - 1;  // lanes past the end read the last element and store nothing
    unsigned col[PPW];
    bool live[PPW];
#pragma unroll
    for (int q = 0; q < PPW; ++q) {
        const unsigned p = (blockIdx.y * PG + g) * PPW + q;
        live[q] = p < parties;
        col[q] = live[q] ? (cols ? cols[p] : p) : 0;
    }
    Acc acc[PPW];
    uint32_t a2[PPW];
#pragma unroll
    for (int q = 0; q < PPW; ++q) acc[q].zero(), a2[q] = 0;
    const unsigned T0 = (unsigned)((uint64_t)Tn * ks / KS), T1 = (unsigned)((uint64_t)Tn * (ks + 1) / KS);
    const uint64_t* rp = r + il;
    const unsigned Tlast = T1 - 1;  // loads past the slice re-read its last set (and are not used): every load is unconditional,
                                    // so the next step's loads stay in flight behind this step's products
    constexpr int U = 4;            // sets per step
    constexpr int GU = 1;           // several parties per wave: a set's coefficients are fetched when its turn comes
    if (T0 >= T1) goto merge;
    if constexpr (PPW > 1) {
        uint64_t cur[U], nxt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = rp[(size_t)(T0 + u < Tlast ? T0 + u : Tlast) * B];
        for (unsigned T = T0; T < T1; T += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = rp[(size_t)(T + U + u < Tlast ? T + U + u : Tlast) * B];
#pragma unroll
            for (int u0 = 0; u0 < U; u0 += GU) {
                uint32_t k[GU][PPW][NC], k2[GU][PPW];
#pragma unroll
                for (int gu = 0; gu < GU; ++gu)
#pragma unroll
                    for (int q = 0; q < PPW; ++q) {
                        const unsigned Tu = T + u0 + gu < Tlast ? T + u0 + gu : Tlast;
                        const size_t e = (size_t)Tu * tab.ncols + col[q];
#pragma unroll
                        for (int x = 0; x < NC; ++x) k[gu][q][x] = tab.coef[e * NC + x];
                        k2[gu][q] = GF2 ? tab.coef2[e] : 0;
                    }
#pragma unroll
                for (int gu = 0; gu < GU; ++gu) {
                    const int u = u0 + gu;
                    if (T + u >= T1) break;
                    const uint32_t r0 = (uint32_t)cur[u], r1 = (uint32_t)(cur[u] >> 32);
#pragma unroll
                    for (int q = 0; q < PPW; ++q) {
                        uint32_t any = 0;  // f_T(alpha_j) = 0 exactly when j is in T: nothing to add (n - t of n parties have a term)
#pragma unroll
                        for (int x = 0; x < NC; ++x) any |= k[gu][q][x];
                        if (!live[q] || any == 0) continue;
                        acc[q].mac(r0, r1, k[gu][q]);
                        if (GF2) a2[q] ^= (0u - (r0 & 1u)) & k2[gu][q];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    } else {
        // one party per wave: the coefficients of the NEXT step are fetched (scalar loads) before this step's products, carried
        // across the loop -- fetched where they are used, every term would wait out a scalar-load latency
        uint64_t cur[U], nxt[U];
        uint32_t kc[U][NC], kc2[U], kn[U][NC], kn2[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned Tu = T0 + u < Tlast ? T0 + u : Tlast;
            cur[u] = rp[(size_t)Tu * B];
            const size_t e = (size_t)Tu * tab.ncols + col[0];
#pragma unroll
            for (int x = 0; x < NC; ++x) kc[u][x] = tab.coef[e * NC + x];
            kc2[u] = GF2 ? tab.coef2[e] : 0;
        }
        for (unsigned T = T0; T < T1; T += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned Tu = T + U + u < Tlast ? T + U + u : Tlast;
                nxt[u] = rp[(size_t)Tu * B];
                const size_t e = (size_t)Tu * tab.ncols + col[0];
#pragma unroll
                for (int x = 0; x < NC; ++x) kn[u][x] = tab.coef[e * NC + x];
                kn2[u] = GF2 ? tab.coef2[e] : 0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (T + u >= T1) break;
                uint32_t any = 0;  // f_T(alpha_j) = 0 exactly when j is in T: nothing to add
#pragma unroll
                for (int x = 0; x < NC; ++x) any |= kc[u][x];
                if (!live[0] || any == 0) continue;
                acc[0].mac((uint32_t)cur[u], (uint32_t)(cur[u] >> 32), kc[u]);
                if (GF2) a2[0] ^= (0u - ((uint32_t)cur[u] & 1u)) & kc2[u];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cur[u] = nxt[u], kc2[u] = kn2[u];
#pragma unroll
                for (int x = 0; x < NC; ++x) kc[u][x] = kn[u][x];
            }
        }
    }
merge:
    if (KS > 1) {
        if (ks > 0) {
            uint32_t* dst = lds + (size_t)(ks - 1) * LW * 64 + lane;
#pragma unroll
            for (int x = 0; x < Acc::WORDS; ++x) dst[x * 64] = acc[0].word(x);
            dst[Acc::WORDS * 64] = a2[0];
        }
        __syncthreads();
        if (ks > 0) return;
#pragma unroll
        for (int o = 0; o < KS - 1; ++o) {
            const uint32_t* src = lds + (size_t)o * LW * 64 + lane;
            acc[0].merge([&](int x) { return src[x * 64]; });
            a2[0] ^= src[Acc::WORDS * 64];
        }
    }
    const unsigned p0 = (blockIdx.y * PG + g) * PPW;
    if constexpr (STAGED) {
        if constexpr (Acc::NC == 8) {
            uint32_t* mine = lds + (size_t)w * PPW * 11 * 64 + lane;
#pragma unroll
            for (int q = 0; q < PPW; ++q) {
                uint32_t ws[11];
                acc[q].resolve(ws);
#pragma unroll
                for (int x = 0; x < 11; ++x) mine[(q * 11 + x) * 64] = ws[x];
                if (GF2 && live[q] && i < B) out2[(size_t)(p0 + q) * B + i] = (uint8_t)a2[q];
            }
            if (i >= B) return;
#pragma unroll 1
            for (unsigned q = 0; q < PPW && p0 + q < parties; ++q) {
                uint32_t ws[11];
#pragma unroll
                for (int x = 0; x < 11; ++x) ws[x] = mine[(q * 11 + x) * 64];
                F::store_loose(out + ((size_t)(p0 + q) * B + i) * F::EW, Acc::reduce_words(ws, tab.red));
            }
        }
    } else {
        if (i >= B) return;
#pragma unroll
        for (int q = 0; q < PPW; ++q) {
            if (!live[q]) continue;
            const size_t o = (size_t)(p0 + q) * B + i;
            F::store_loose(out + o * F::EW, acc[q].reduce(tab.red));
            if (GF2) out2[o] = (uint8_t)a2[q];
        }
    }
}

// ---- finalize (try_finalize_bit, prandbitd.rs:189-211) ------------------------------------------------------------------------
// v [N] the opened r + b (canonical Goldilocks values), r_p [parties][N] Fr, r_2 [parties][N] bytes:
//   bp[p][i] = G(v[i]) - r_p[p][i],  b2[p][i] = r_2[p][i] ^ lsb(v[i]);  blockIdx.y = party
template <class F>
__global__ __launch_bounds__(256) void k_prandbit_finalize(const uint64_t* __restrict__ v, const uint32_t* __restrict__ r_p,
                                                           const uint8_t* __restrict__ r_2, size_t N, uint32_t* __restrict__ bp,
                                                           uint8_t* __restrict__ b2) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint64_t x = v[i];
    const uint32_t w[8] = {(uint32_t)x, (uint32_t)(x >> 32), 0, 0, 0, 0, 0, 0};
    const size_t o = (size_t)blockIdx.y * N + i;
    F::store_loose(bp + o * F::EW, F::template sub<2>(riss_from_words<F>(w), F::load(r_p + o * F::EW)));
    b2[o] = r_2[o] ^ (uint8_t)(x & 1u);
}
}  // namespace hbmpc
