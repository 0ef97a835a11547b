// RandBit for all parties of a SMALL batch in one launch: a workgroup per chunk of t + 1 elements
// (fpmul/rand_bit.rs:242-293, 197-220; mul/multiplication.rs:417-426, 57-100; BatchRecon's two arms, batch_recon.rs:157-165, :384-391,
// :457-467).
//
// The separate steps are nine launches -- the shares Multiply opens, the encode / the recipients' P(0) decodes / the coefficient decode
// of d and e, finalize_mul, the same three of a^2, phase 2 -- and the protocol runs them over a few hundred to a few thousand elements
// (one refill of the PRandBit pool, honeybadger/mod.rs:1951-2086).  With all parties on one device a chunk of t + 1 elements depends on
// nothing outside it from the input shares to the bit shares (the independence k_triplegen_wg uses), so one workgroup of 256 lanes
// takes it all the way: a lane per (party, element) for the element-wise steps, a lane per (party, recipient) for the encodes, lane
// pairs or quads per table row for the decodes over U29 (dot_shared; over Goldilocks a lane per row), a lane per element for the
// square root.  Both opens decode from senders 0 .. 2t exactly (no OEC round: a failed chunk is final), whatever n is: covers
// 2t + 1 <= n <= 16, t >= 1.  The encoded messages and the revealed values stay in LDS.
//
// Every buffer a caller can see gets the bytes of the nine launches (tests/test_gpu_randbit_parties.py).
#pragma once
#include "wave_core.hpp"
#include "kernels_sqrt.hpp"

namespace hbmpc {

struct RandBitWgArgs {
    const uint32_t *a, *ta, *tb, *tc;  // [party][N]
    const uint32_t* vmat;              // [n][t + 1] constants alpha_j^k
    const uint32_t* tab;               // the decodes' table (ids 0 .. 2t, d = t): [t verify rows | t + 1 coefficient rows][t + 1]
    uint32_t *desh, *deop, *sq, *sqop, *out;  // desh[party][2][N], deop[2 N] (d, then e), sq[party][N], sqop[N], out[party][N]
    uint8_t *status, *rst_de, *rst_sq;        // status[N]: phase 2's; rst_*[n G] as the two decodes of an open leave it
    uint32_t *sm_de_first, *sm_de, *sm_sq_first, *sm_sq;
    RandBitSummaryDev* rb;             // initialised by the caller (first = all ones, n_failed = 0)
    uint32_t* counters;                // the stream's decode counters: ([24], [25]) and ([0], [1]) the first open's two decodes,
                                       // ([26], [27]) and ([28], [29]) the second's
    SqrtTab st;
    size_t N;                          // gridDim.x = N / (t + 1) chunks
    int n, t;
    uint32_t r2[9];                    // R^2: canonical -> Montgomery
};

// LDS words: X[2][n][M] | Y[2][n][n] | Z[2][n] | O[2][M] | S[M] (elements in limb form, `ls` words apart) | bad flags [2][n + 1],
// phase 2's status [M] | vmat | tab   (nl words per constant: 9 and ls = 12 for U29, 2 and 2 for Goldilocks)
struct RandBitWgLds {
    int X, Y, Z, O, S, flags, pst, vmat, tab, total;
    __host__ __device__ RandBitWgLds(int n, int t, int ls, int nl) {
        const int M = t + 1;
        X = 0, Y = X + 2 * n * M * ls, Z = Y + 2 * n * n * ls, O = Z + 2 * n * ls, S = O + 2 * M * ls, flags = S + M * ls;
        pst = flags + 2 * (n + 1);
        vmat = (pst + M + 3) & ~3;
        tab = vmat + n * M * nl;
        total = tab + (t + M) * M * nl;
    }
};

template <class F>
__global__ __launch_bounds__(256) void k_randbit_wg(RandBitWgArgs a) {
    using E = typename F::E;
    constexpr bool SHARE = F::NL == 9;  // U29: a row's products shared by adjacent lanes (dot_shared); Goldilocks' are cheap
    constexpr int NL = F::NL, EW = F::EW, LS = SHARE ? 12 : F::NL;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x, n = a.n, t = a.t, M = t + 1, nv = t;
    const size_t c = blockIdx.x, Gsq = gridDim.x, Gde = 2 * Gsq;
    const RandBitWgLds L(n, t, LS, NL);
    uint32_t *X = lds + L.X, *Yl = lds + L.Y, *Zl = lds + L.Z, *Ol = lds + L.O, *Sl = lds + L.S, *flags = lds + L.flags, *pst = lds + L.pst;
    uint32_t *vmat = lds + L.vmat, *tab = lds + L.tab;
    // lanes that share a row's products: as many as leave every row of a step inside the workgroup's one pass
    auto share_log = [&](int rows) {
        int lk = 0;
        if constexpr (SHARE)
            while (lk < 2 && (rows << (lk + 1)) <= 256 && (2 << lk) <= M) ++lk;
        return lk;
    };

    // BatchRecon (degree t) of W chunks of this workgroup, X[w][party][M] -> Ol[w][M] and `opened`; chunk w is chunk w * Gsq + c of
    // the open's G.  cf, cs: the counters of the recipients' decodes and of the revealed values' decode.  Starts and ends at a barrier.
    auto open = [&](int W, size_t G, uint32_t* opened, uint8_t* rst, int cf, int cs) {
        if (tid < 2 * (n + 1)) flags[tid] = 0;
        // the encode (batch_recon.rs:157-165): a lane per (chunk, party p, recipient j): y = sum_k alpha_j^k x_p[k]
        for (int it = tid; it < W * n * n; it += 256) {
            const int wp = it / n, j = it - wp * n;  // wp = w n + p
            const E y = F::canon_loose(dot_rows<F>([&](int k) { return F::load_const(X + (wp * M + k) * LS); }, vmat + (size_t)j * M * NL, M, 0, 0));
            put_limbs<F>(Yl + (wp * n + j) * LS, y);
        }
        __syncthreads();
        // the EvalBatch arm (:384-391): recipient j opens its value from senders 0 .. 2t: t verify rows and the P(0) row
        {
            const int lk = share_log(W * n * (nv + 1));
            const int q = tid >> lk, sidx = tid & ((1 << lk) - 1), wj = q / (nv + 1), r = q - wj * (nv + 1);  // wj = w n + j
            const int w = wj / n, j = wj - w * n;
            const bool mine = q < W * n * (nv + 1);
            E kept = F::zero();
            if (mine) {
                kept = dot_rows<F>([&](int i) { return F::load_const(Yl + ((w * n + i) * n + j) * LS); }, tab + (size_t)(r < nv ? r : nv) * M * NL, M, lk, sidx);
                if (r < nv && sidx == 0 && !F::eq_canon(F::canon_loose(kept), F::load_const(Yl + ((w * n + M + r) * n + j) * LS)))
                    flags[w * (n + 1) + j] = 1;
            }
            __syncthreads();
            if (mine && r == nv && sidx == 0) {
                const bool ok = flags[w * (n + 1) + j] == 0;
                put_limbs<F>(Zl + wj * LS, ok ? F::canon_loose(kept) : F::zero());
                const size_t g = (size_t)j * G + (size_t)w * Gsq + c;
                if (j > 0) rst[g] = ok ? 0 : (uint8_t)DecodingError;  // recipient 0's is rewritten by the second decode
                if (!ok) {
                    atomicAdd(a.counters + cf, 1u);
                    atomicMax(a.counters + cf + 1, 0xffffffffu - (uint32_t)g);
                }
            }
        }
        __syncthreads();
        // the RevealBatch arm (:457-467): everyone interpolates the t + 1 opened values from the broadcast z_0 .. z_2t: t verify rows and
        // t + 1 coefficient rows
        {
            const int lk = share_log(W * (nv + M));
            const int q = tid >> lk, sidx = tid & ((1 << lk) - 1), w = q / (nv + M), r = q - w * (nv + M);
            const bool mine = q < W * (nv + M);
            E kept = F::zero();
            if (mine) {
                kept = dot_rows<F>([&](int i) { return F::load_const(Zl + (w * n + i) * LS); }, tab + (size_t)r * M * NL, M, lk, sidx);
                if (r < nv && sidx == 0 && !F::eq_canon(F::canon_loose(kept), F::load_const(Zl + (w * n + M + r) * LS))) flags[w * (n + 1) + n] = 1;
            }
            __syncthreads();
            if (mine && sidx == 0) {
                const bool ok = flags[w * (n + 1) + n] == 0;
                const size_t g = (size_t)w * Gsq + c;
                if (r >= nv) {
                    const E o = ok ? F::canon_loose(kept) : F::zero();
                    put_limbs<F>(Ol + (w * M + (r - nv)) * LS, o);
                    put_words<F>(opened + (g * M + (r - nv)) * EW, o);
                }
                if (r == nv) {
                    rst[g] = ok ? 0 : (uint8_t)DecodingError;
                    if (!ok) {
                        atomicAdd(a.counters + cs, 1u);
                        atomicMax(a.counters + cs + 1, 0xffffffffu - (uint32_t)g);
                    }
                }
            }
        }
        __syncthreads();
    };

    // ---- loads: a lane per (party, element of the chunk); the tables by everyone ------------------------------------------------------
    const int pk_p = tid / M, pk_k = tid - pk_p * M;
    const bool pk = tid < n * M;
    const size_t e = pk ? (size_t)pk_p * a.N + c * M + pk_k : 0;
    E va = F::zero(), vtc = F::zero();
    for (int w = tid; w < n * M * NL; w += 256) vmat[w] = a.vmat[w];
    for (int w = tid; w < (nv + M) * M * NL; w += 256) tab[w] = a.tab[w];
    // Multiply::init(a, a, triple): d = ta - a, e = tb - a (multiplication.rs:417-426), canonical as k_beaver_open_pair stores them
    if (pk) {
        va = F::load(a.a + e * EW), vtc = F::load(a.tc + e * EW);
        const E d_sh = F::canon_loose(F::template sub<2>(F::load(a.ta + e * EW), va));
        const E e_sh = F::canon_loose(F::template sub<2>(F::load(a.tb + e * EW), va));
        put_limbs<F>(X + (pk_p * M + pk_k) * LS, d_sh);
        put_limbs<F>(X + ((n + pk_p) * M + pk_k) * LS, e_sh);
        const size_t o = (size_t)pk_p * 2 * a.N + c * M + pk_k;
        put_words<F>(a.desh + o * EW, d_sh);
        put_words<F>(a.desh + (o + a.N) * EW, e_sh);
    }
    __syncthreads();

    // ---- the first open: the d-chunk (chunk c of Gde) and the e-chunk (chunk Gsq + c) -------------------------------------------------
    open(2, Gde, a.deop, a.rst_de, 24, 0);

    // ---- finalize_mul (multiplication.rs:57-100): [a^2] = tc - d (e + [a]) - e [a], as k_beaver_finalize computes it ----------------------
    if (pk) {
        const E ev = F::load_const(Ol + (M + pk_k) * LS);
        const E dm = F::mulc(F::load_const(Ol + pk_k * LS), a.r2), em = F::mulc(ev, a.r2);  // Montgomery forms, normalised, < 2r
        const E dey = F::mont(F::add(ev, va), dm);
        const E ex = F::mont(va, em);
        const E s = F::canon_loose(F::template sub<4>(F::template sub<4>(vtc, dey), ex));
        put_limbs<F>(X + (pk_p * M + pk_k) * LS, s);
        put_words<F>(a.sq + e * EW, s);
    }
    __syncthreads();

    // ---- the second open (rand_bit.rs:281-290) ------------------------------------------------------------------------------------------
    open(1, Gsq, a.sqop, a.rst_sq, 26, 28);

    // ---- phase 2 (rand_bit.rs:197-220), a lane per element: s = b^-1 2^-1 = u omega^(-(L + E)) 2^-1 as in k_randbit_finalize ---------------
    if (tid < M) {
        const size_t i = c * M + tid;
        const E A = F::load_const(Ol + tid * LS);
        const bool zero = F::is_zero_canon(A);
        const E am = to_mont<F>(a.st, A);
        uint32_t Lg;
        const E u = sqrt_core<F>(a.st, am, Lg);
        const uint32_t st = zero ? RB_ZERO : (Lg & 1u) ? RB_NO_ROOT : RB_OK;
        a.status[i] = (uint8_t)st;
        pst[tid] = st;
        if (st != RB_OK) {
            atomicMin(&a.rb->first, ((unsigned long long)st << 32) | (unsigned long long)i);
            atomicAdd(&a.rb->n_failed, 1u);
        } else {
            const uint32_t Ee = (0u - (Lg >> 1)) & 0x7fffffffu;
            put_limbs<F>(Sl + tid * LS, sq_mulc<F>(sq_mul<F>(u, omega_pow<F>(a.st, 0u - (Lg + Ee))), a.st.half));
        }
    }
    __syncthreads();
    // out_p = [a]_p s + 2^-1; a failed element's shares are zero for every party
    if (pk) {
        if (pst[pk_k] != RB_OK) {
            F::store_lt2r(a.out + e * EW, F::zero());
        } else {
            const E v = sq_mul<F>(va, F::load_const(Sl + pk_k * LS));
            F::store_loose(a.out + e * EW, F::add(v, F::load_const(a.st.half_p)));
        }
    }

    // ---- the summaries: the last workgroup turns the counters into them and leaves the counters at zero.  finish_direct
    // (kernels_recover.hpp) written out: with it this kernel, 85 KB of text, measured 1.5 % slower at 1024 chunks over Fr and no slower
    // at 1 or 4096 -- where the code lands, not what it does -- and with its own tail it is the earlier kernel instruction for
    // instruction (profiles/wave_core.txt, section 4) -----------------------------------------------------------------------------------
    __syncthreads();
    if (tid != 0) return;
    __threadfence();
    const unsigned nblocks = gridDim.x, sub = blockIdx.x % DIRECT_FAN, quota = nblocks / DIRECT_FAN + (sub < nblocks % DIRECT_FAN ? 1u : 0u);
    if (atomicAdd(a.counters + 8 + sub, 1u) != quota - 1) return;
    const unsigned groups = nblocks < DIRECT_FAN ? nblocks : DIRECT_FAN;
    if (atomicAdd(a.counters + 3, 1u) != groups - 1) return;
    __threadfence();
#pragma unroll
    for (unsigned k = 0; k < DIRECT_FAN; ++k) store_handoff(a.counters + 8 + k, 0u);
    auto summarise = [&](uint32_t* summary, int slot) {
        const uint32_t f = load_handoff(a.counters + slot), l = load_handoff(a.counters + slot + 1);
        summary[0] = f, summary[1] = f;
        summary[2] = f ? 0xffffffffu - l : 0xffffffffu;
        summary[3] = f ? (uint32_t)DecodingError : 0u;
        store_handoff(a.counters + slot, 0u);
        store_handoff(a.counters + slot + 1, 0u);
    };
    summarise(a.sm_de_first, 24);
    summarise(a.sm_de, 0);
    summarise(a.sm_sq_first, 26);
    summarise(a.sm_sq, 28);
    store_handoff(a.counters + 2, 0u);
    store_handoff(a.counters + 3, 0u);
}

}  // namespace hbmpc
