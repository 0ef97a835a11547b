// PRandBit / PRandInt for all parties of a SMALL batch in one launch: a workgroup per chunk of t + 1 elements
// (fpmul/prandbitd.rs: the fold :638-647, :667-684, the RISS-to-Shamir conversion :311-356, r + b, BatchRecon of degree t :437-446,
// try_finalize_bit :189-211; driven by honeybadger/mod.rs:1951-2150).
//
// The separate steps are eight launches over two contexts -- fold, the conversion over Fr (with GF(2^8)) and over Goldilocks, the add,
// the encode / the recipients' P(0) decodes / the coefficient decode of r + b, the finalize -- and the reference runs them at
// (n, t) = (4,1) .. (10,3): 4 to 120 sets, a few thousand multiply-adds.  A chunk of t + 1 elements depends on nothing outside it from
// the senders' values to the bit shares, so one workgroup of 256 lanes takes it all the way: a lane per (set, element) for the fold, a
// lane per (slice of the sets, party, element) for the conversion (RissAcc's lazy integer sums, merged through LDS, ONE reduction per
// output), a lane per (party, recipient) for the encode, a lane per table row for the decodes, a lane per (party, element) for the
// finalize.  The open decodes from senders 0 .. 2t exactly (no OEC round: a failed chunk is final), as k_randbit_wg's does.
// The coefficient tables of both fields stay in LDS (PRandBitWgLds, prandbit_route.hpp): that bounds the shapes it covers.
//
// Every buffer a caller can see gets the bytes of the separate launches (tests/test_gpu_prandbit_parties.py).
#pragma once
#include "wave_core.hpp"
#include "kernels_riss.hpp"
#include "prandbit_route.hpp"

namespace hbmpc {

struct PRandBitWgArgs {
    const uint64_t* contrib;  // [n][Tn][B] the senders' values
    const uint64_t* b_q;      // [n][B] Goldilocks shares of the bits
    const uint32_t *coefF, *coef2, *red;  // the Fr context's table (tables_riss.hpp): [Tn][n][8], [Tn][n], [2][NL]
    const uint32_t* coefG;                // the Goldilocks context's: [Tn][n][2]
    const uint32_t *vmat, *tab;           // Goldilocks: [n][t + 1] constants alpha_j^k; the decodes' table (ids 0 .. 2t, d = t)
    uint64_t* sums;           // [Tn][B]
    uint8_t* bad;             // [n][Tn], zeroed by the caller
    uint32_t* r_p;            // [n][B] Fr
    uint8_t* r_2;             // [n][B]
    uint64_t *r_q, *rb, *opened;  // [n][B], [n][B], [B]
    uint32_t* b_p;            // [n][B] Fr
    uint8_t *b_2, *rstatus;   // [n][B]; [n G] as the two decodes leave it
    uint32_t *sm_first, *sm;
    uint32_t* counters;       // the stream's decode counters (the Goldilocks context's): ([24], [25]) the recipients' decodes, ([0], [1]) the revealed values'
    size_t B;                 // gridDim.x = ceil(B / (t + 1)) chunks
    uint64_t bound;           // 2^lk
    int n, t, Tn;
};

// RissAcc<F>::mac with the coefficient in VGPRs: here a lane is a (party, element), so the coefficients differ from lane to lane
template <class F>
HB_DEV void riss_mac_lane(RissAcc<F>& A, uint32_t r0, uint32_t r1, const uint32_t (&k)[8]) {
#define HB_RISS_P(COL, CNT, A_, K) "v_mad_u64_u32 %" #COL ", vcc, %" #A_ ", %" #K ", %" #COL "\n\tv_addc_co_u32_e32 %" #CNT ", vcc, 0, %" #CNT ", vcc\n\t"
    asm(HB_RISS_P(0, 9, 18, 20) HB_RISS_P(1, 10, 18, 21) HB_RISS_P(2, 11, 18, 22) HB_RISS_P(3, 12, 18, 23)
        HB_RISS_P(4, 13, 18, 24) HB_RISS_P(5, 14, 18, 25) HB_RISS_P(6, 15, 18, 26) HB_RISS_P(7, 16, 18, 27)
        HB_RISS_P(1, 10, 19, 20) HB_RISS_P(2, 11, 19, 21) HB_RISS_P(3, 12, 19, 22) HB_RISS_P(4, 13, 19, 23)
        HB_RISS_P(5, 14, 19, 24) HB_RISS_P(6, 15, 19, 25) HB_RISS_P(7, 16, 19, 26) HB_RISS_P(8, 17, 19, 27)
        : "+v"(A.c[0]), "+v"(A.c[1]), "+v"(A.c[2]), "+v"(A.c[3]), "+v"(A.c[4]), "+v"(A.c[5]), "+v"(A.c[6]), "+v"(A.c[7]), "+v"(A.c[8]),
          "+v"(A.h[0]), "+v"(A.h[1]), "+v"(A.h[2]), "+v"(A.h[3]), "+v"(A.h[4]), "+v"(A.h[5]), "+v"(A.h[6]), "+v"(A.h[7]), "+v"(A.h[8])
        : "v"(r0), "v"(r1), "v"(k[0]), "v"(k[1]), "v"(k[2]), "v"(k[3]), "v"(k[4]), "v"(k[5]), "v"(k[6]), "v"(k[7])
        : "vcc");
#undef HB_RISS_P
}

// BIT: PRandBit; otherwise PRandInt (the fold and the Fr conversion only; the last workgroup may hold fewer than t + 1 elements)
template <class F, bool BIT>
__global__ __launch_bounds__(256) void k_prandbit_wg(PRandBitWgArgs a) {
    using E = typename F::E;
    using GE = Gold::E;
    constexpr int LW = PRANDBIT_WG_MERGE_WORDS;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x, n = a.n, t = a.t, M = t + 1, nv = t, Tn = a.Tn;
    const size_t c = blockIdx.x, G = gridDim.x, e0 = c * (size_t)M;
    const int Mc = a.B - e0 < (size_t)M ? (int)(a.B - e0) : M;  // elements of this workgroup
    const PRandBitWgLds L(n, t, Tn);
    uint32_t *cF = lds + L.cF, *cG = lds + L.cG, *c2 = lds + L.c2, *vmat = lds + L.vmat, *tab = lds + L.tab, *Sl = lds + L.S, *X = lds + L.X;
    uint32_t *Yl = lds + L.Y, *Zl = lds + L.Z, *Ol = lds + L.O, *flags = lds + L.flags, *mg = lds + L.merge;

    // ---- the constants, by everyone ----------------------------------------------------------------------------------------------------
    for (int w = tid; w < Tn * n * 8; w += 256) cF[w] = a.coefF[w];
    if constexpr (BIT) {
        for (int w = tid; w < Tn * n * 2; w += 256) cG[w] = a.coefG[w];
        for (int w = tid; w < Tn * n; w += 256) c2[w] = a.coef2[w];
        for (int w = tid; w < n * M * 2; w += 256) vmat[w] = a.vmat[w];
        for (int w = tid; w < (nv + M) * M * 2; w += 256) tab[w] = a.tab[w];
        if (tid < n + 1) flags[tid] = 0;
    }

    // ---- the fold (prandbitd.rs:667-684, bound test :638-647), a lane per (set, element): as k_riss_fold -----------------------------------
    {
        const size_t stride = (size_t)Tn * a.B;
        for (int it = tid; it < Tn * M; it += 256) {
            const int T = it / M, k = it - T * M;
            if (k >= Mc) continue;
            const size_t o = (size_t)T * a.B + e0 + k;
            uint64_t sum = 0;
            for (int s = 0; s < n; ++s) {
                const uint64_t v = a.contrib[(size_t)s * stride + o];
                sum += v;
                if (v > a.bound) a.bad[(size_t)s * Tn + T] = 1;
            }
            a.sums[o] = sum;
            Sl[2 * it] = (uint32_t)sum, Sl[2 * it + 1] = (uint32_t)(sum >> 32);
        }
    }
    __syncthreads();

    // ---- the conversion (prandbitd.rs:311-356): lane = (slice sl of the sets, party p, element k); slice 0 reduces and stores ----------------
    const int outs = n * M, KS = L.ks;
    const int sl = tid / outs, po = tid - sl * outs, p = po / M, k = po - p * M;
    const bool conv = sl < KS && k < Mc;
    const size_t oi = (size_t)p * a.B + e0 + k;  // this lane's (party, element) in a [n][B] buffer
    RissAcc<F> accF;
    RissAcc<Gold> accG;
    uint32_t a2 = 0;
    accF.zero(), accG.zero();
    if (conv) {
        const int T0 = (int)((long)Tn * sl / KS), T1 = (int)((long)Tn * (sl + 1) / KS);
        for (int T = T0; T < T1; ++T) {
            const uint32_t* kp = cF + ((size_t)T * n + p) * 8;
            uint32_t kw[8], any = 0;
#pragma unroll
            for (int x = 0; x < 8; ++x) kw[x] = kp[x], any |= kw[x];
            if (any == 0) continue;  // f_T(alpha_p) = 0 exactly when p is in T: nothing to add, in either field
            const uint32_t r0 = Sl[2 * (T * M + k)], r1 = Sl[2 * (T * M + k) + 1];
            riss_mac_lane<F>(accF, r0, r1, kw);
            if constexpr (BIT) {
                const GE rv = {{r0, r1}};
                Gold::acc_mac(accG.A, rv, cG + ((size_t)T * n + p) * 2);
                a2 ^= (0u - (r0 & 1u)) & c2[(size_t)T * n + p];
            }
        }
        if (sl > 0) {
            uint32_t* dst = mg + ((size_t)(sl - 1) * outs + po) * LW;
#pragma unroll
            for (int x = 0; x < 27; ++x) dst[x] = accF.word(x);
            if constexpr (BIT) {
#pragma unroll
                for (int x = 0; x < 9; ++x) dst[27 + x] = accG.word(x);
                dst[36] = a2;
            }
        }
    }
    __syncthreads();
    E rp = F::zero();  // the canonical r_p of this lane's (party, element): the finalize subtracts it
    if (conv && sl == 0) {
        for (int s = 1; s < KS; ++s) {
            const uint32_t* src = mg + ((size_t)(s - 1) * outs + po) * LW;
            accF.merge([&](int x) { return src[x]; });
            if constexpr (BIT) {
                accG.merge([&](int x) { return src[27 + x]; });
                a2 ^= src[36];
            }
        }
        rp = F::canon_loose(accF.reduce(a.red));
        put_words<F>(a.r_p + oi * 8, rp);
        if constexpr (BIT) {
            a.r_2[oi] = (uint8_t)a2;
            const GE rq = accG.reduce(nullptr);
            const GE v = Gold::add(rq, Gold::e(a.b_q[oi]));  // r + b, as the element-wise add computes it
            a.r_q[oi] = Gold::u(rq);
            a.rb[oi] = Gold::u(v);
            put_limbs<Gold>(X + (p * M + k) * 2, v);
        }
    }
    if constexpr (!BIT) return;
    __syncthreads();

    auto gdot = [&](auto&& value_of, const uint32_t* row) -> GE { return dot_rows<Gold>(value_of, row, M, 0, 0); };  // a lane per row

    // ---- BatchRecon (degree t) of r + b over Goldilocks, as k_randbit_wg's open runs it (batch_recon.rs:157-165, :384-391, :457-467) -------
    // the encode: a lane per (party q, recipient j): y = sum_k alpha_j^k x_q[k]
    for (int it = tid; it < n * n; it += 256) {
        const int q = it / n, j = it - q * n;
        put_limbs<Gold>(Yl + it * 2, gdot([&](int i) { return Gold::load_const(X + (q * M + i) * 2); }, vmat + (size_t)j * M * 2));
    }
    __syncthreads();
    // the EvalBatch arm: recipient j opens its value from senders 0 .. 2t: t verify rows and the P(0) row
    {
        const int j = tid / (nv + 1), r = tid - j * (nv + 1);
        const bool mine = tid < n * (nv + 1);
        GE kept = Gold::zero();
        if (mine) {
            kept = gdot([&](int i) { return Gold::load_const(Yl + (i * n + j) * 2); }, tab + (size_t)(r < nv ? r : nv) * M * 2);
            if (r < nv && !Gold::eq_canon(kept, Gold::load_const(Yl + ((M + r) * n + j) * 2))) flags[j] = 1;
        }
        __syncthreads();
        if (mine && r == nv) {
            const bool ok = flags[j] == 0;
            put_limbs<Gold>(Zl + j * 2, ok ? kept : Gold::zero());
            const size_t g = (size_t)j * G + c;
            if (j > 0) a.rstatus[g] = ok ? 0 : (uint8_t)DecodingError;  // recipient 0's is rewritten by the second decode
            if (!ok) {
                atomicAdd(a.counters + 24, 1u);
                atomicMax(a.counters + 25, 0xffffffffu - (uint32_t)g);
            }
        }
    }
    __syncthreads();
    // the RevealBatch arm: everyone interpolates the t + 1 opened values from the broadcast z_0 .. z_2t: t verify rows, t + 1 coefficient rows
    {
        const int r = tid;
        const bool mine = tid < nv + M;
        GE kept = Gold::zero();
        if (mine) {
            kept = gdot([&](int i) { return Gold::load_const(Zl + i * 2); }, tab + (size_t)r * M * 2);
            if (r < nv && !Gold::eq_canon(kept, Gold::load_const(Zl + (M + r) * 2))) flags[n] = 1;
        }
        __syncthreads();
        if (mine) {
            const bool ok = flags[n] == 0;
            if (r >= nv) {
                const GE o = ok ? kept : Gold::zero();
                put_limbs<Gold>(Ol + (r - nv) * 2, o);
                a.opened[c * M + (r - nv)] = Gold::u(o);
            }
            if (r == nv) {
                a.rstatus[c] = ok ? 0 : (uint8_t)DecodingError;
                if (!ok) {
                    atomicAdd(a.counters + 0, 1u);
                    atomicMax(a.counters + 1, 0xffffffffu - (uint32_t)c);
                }
            }
        }
    }
    __syncthreads();

    // ---- try_finalize_bit (prandbitd.rs:189-211), a lane per (party, element): b_p = G(v) - r_p, b_2 = r_2 ^ lsb(v), as k_prandbit_finalize ----
    if (conv && sl == 0) {
        const uint32_t w[8] = {Ol[k * 2], Ol[k * 2 + 1], 0, 0, 0, 0, 0, 0};
        F::store_loose(a.b_p + oi * 8, F::template sub<2>(riss_from_words<F>(w), rp));
        a.b_2[oi] = (uint8_t)a2 ^ (uint8_t)(w[0] & 1u);
    }

    // ---- the summaries: the last workgroup turns the counters into them and leaves the counters at zero ------------------------------------
    finish_direct(a.counters, {{a.sm_first, 24}, {a.sm, 0}});
}

}  // namespace hbmpc
