// RanSha and DouSha + RanDouSha for all parties of a SMALL batch in one launch each: a workgroup per batch element (column k)
// (share_gen/share_gen.rs:232-289, 401-454, 516-530, 199-203; double_share/double_share_generation.rs:151-215,
// ran_dou_sha/mod.rs:371-449, 569-602, 314-331).
//
// The separate steps are a deal, a mixing call, a reset of the verdict and one to three verifier launches per sharing, 7 - 14 us each
// at protocol sizes.  With all parties on one device a column depends on nothing outside it: n dealers' polynomials (or their dealt
// shares) in, every party's output shares, what the parties send the verifiers and the verifiers' verdicts out.  One workgroup of
// 256 lanes takes it all the way:
//   loads    a lane per (dealer, coefficient) or per (dealer, recipient); the n x n Vandermonde table (its first columns are the
//            deal's matrix) and the verifiers' tables by everyone
//   deal     a lane per (recipient j, dealer p): dealt[p][j] = sum_c alpha_j^c coeffs[p][c]          (only from coefficients)
//   mix      a lane per (row i, party j):        y[i][j] = sum_p alpha_i^p dealt[p][j]; output rows to the parties' lists, the
//            verifiers' rows party-major to yv and kept in LDS
//   verify   a lane group per (verifier, table row): the rows of the decode the separate launches run (rec_table: the verify rows,
//            then the coefficient rows) --
//              RanSha              senders 0 .. t interpolate, senders t + 1 .. 2t must agree, coefficient t must not be zero
//              RanDouSha, Fr       per sharing of degree d: the first d + 1 points interpolate, the other n - d - 1 must agree, only
//                                  coefficients 0 and d are computed; then the two constant terms are compared
//              RanDouSha, Gold.    per sharing the full interpolation through all n points (there is no selective decode over
//                                  Goldilocks, and a product is a few instructions): the degree and the constant term
//   verdict  one lane per workgroup counts its failing verifiers and its column in the stream's decode counters (vector atomics); the
//            last workgroup to finish turns the counters into bad[2] (and RanSha's decode summary) and leaves them at zero -- bad is
//            WRITTEN, so no launch resets it first.
// Every buffer a caller can read gets the bytes of the separate launches (tests/test_gpu_producers_parties.py); the separate launches'
// workspace is not touched.
//
// LDS (ProducersWgLds; elements in limb form `ls` words apart, constants `nl` words: 12 and 9 over U29, 2 and 2 over Goldilocks), per
// sharing: dealt [n][n] | mixed [n][n] (the coefficients are staged where the mixed block goes) | the verifiers' table; once: the
// Vandermonde table [n][n], the kept coefficients [2][nver][2], flags.  At (16, 5) over Fr RanDouSha takes 24.0 KB for both dealt
// blocks, 24.0 KB for both mixed blocks, 9.0 KB for the Vandermonde table, 9.6 KB for the two check tables (16 x 6 and 16 x 11
// constants) and 2.1 KB for the kept coefficients and flags: 68.7 KB, two workgroups per CU of 160 KB (71.7 KB at most, n = 16, t = 7);
// RanSha at (16, 5) takes 37.5 KB.  Over Goldilocks RanDouSha at (16, 5) takes 14.6 KB, RanSha 7.1 KB.
//
// Banks (on paper, not measured): elements 12 words apart keep adjacent lanes of the deal and the mix at most 3 to a bank.  In the verify
// stage the verifiers' rows of the mixed block are n LS words apart -- 192 at n = 16 over U29, 0 modulo the 64 banks -- so the 3 to 5
// verifiers a wave spans conflict on every value load; beside 81 multiply-adds per term that was left (4 words of row padding remove it).
//
// Measured on an MI355X (profiles/fused_producers_sweep.txt; ms per eager call at (16, 5) from the dealers' polynomials, one launch /
// separate launches / the handle's run()): RanSha over Fr 0.016 / 0.029 / 0.026 at 1 column, 0.023 / 0.055 / 0.061 at 256,
// 0.113 / 0.060 / 0.059 at the node's 2 048; RanDouSha over Fr 0.029 / 0.053 / 0.049, 0.039 / 0.110 / 0.121, 0.144 / 0.117 / 0.115 at
// the node's 1 536.  A workgroup per column is ahead while the columns fit the chip at once and behind after: the defaults of
// hbmpc_set_fused_producers are 256 columns over both fields.
#pragma once
#include "wave_core.hpp"

namespace hbmpc {

struct ProducersWgSharing {
    const uint32_t* coeffs;  // [dealer][K][deg + 1], column 0 the secret; null: `dealt` is the input
    uint32_t* dealt;         // [dealer][recipient][K]
    uint32_t* out;           // [party][K][rows]: the parties' lists
    uint32_t* yv;            // [party][verifier][K]: what the parties send the verifiers
    const uint32_t* tab;     // the verifiers' table: [nv verify rows | M coefficient rows][M]
    uint32_t* sel;           // RanDouSha over Fr: (constant term, coefficient deg) [verifier K + k][2]; over Goldilocks: the constant term
                             // [verifier K + k]; RanSha: unused
    void* st;                // status bytes [verifier K + k] (RanSha: may be null); RanDouSha over Goldilocks: the degrees, uint32
    int deg;                 // of the dealers' polynomials
    int M, nv;               // the verifiers' decode: M points interpolate, nv verify
};
struct ProducersWgArgs {
    ProducersWgSharing sh[2];  // RanSha: sh[0] alone
    const uint32_t* vmat;      // alpha_j^k, [n][n] constants
    uint32_t* summary;         // RanSha: the decode's summary
    uint32_t* bad;             // [2]: failing (verifier, column) pairs, the lowest failing column
    uint32_t* counters;        // the stream's decode counters ([0], [1]: RanSha's decode; [24], [25]: the verdict)
    size_t K;
    int n, t;
    int row0, rows;            // mixed rows [row0, row0 + rows) are the parties' lists
    int nver, ver0;            // verifiers ver0 .. ver0 + nver - 1 (= the other mixed rows, in this order)
};

struct ProducersWgLds {
    int D[2], Y[2], tab[2], tab_words[2], vmat, vmat_words, kept, flags, total;
    __host__ __device__ static int up4(int w) { return (w + 3) & ~3; }
    // tab0_consts, tab1_consts: the constants of the two sharings' tables, (nv + M) M each
    __host__ __device__ ProducersWgLds(int n, int ns, int nver, int tab0_consts, int tab1_consts, int ls, int nl) {
        int at = 0;
        for (int s = 0; s < 2; ++s) {
            D[s] = at, at = up4(at + (s < ns ? n * n * ls : 0));
            Y[s] = at, at = up4(at + (s < ns ? n * n * ls : 0));
        }
        vmat_words = n * n * nl, vmat = at, at = up4(at + vmat_words);
        tab_words[0] = tab0_consts * nl, tab_words[1] = ns > 1 ? tab1_consts * nl : 0;
        tab[0] = at, at = up4(at + tab_words[0]);
        tab[1] = at, at = up4(at + tab_words[1]);
        kept = at, at = up4(at + 2 * nver * 2 * ls);
        flags = at, at = up4(at + 64);  // [0, 32): a verifier's decode failed, per sharing; [32, 64): its degree (Goldilocks RanDouSha)
        total = at;
    }
};

// the tail of finish_direct (kernels_recover.hpp) with the verdict pair (24, 25) written as bad[2] and the decode pair (0, 1) as the summary
HB_DEV void finish_producers(uint32_t* counters, uint32_t* summary, uint32_t* bad) {
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned nblocks = gridDim.x, b = blockIdx.x;
    const unsigned sub = b % DIRECT_FAN, quota = nblocks / DIRECT_FAN + (sub < nblocks % DIRECT_FAN ? 1u : 0u);
    __threadfence();  // release: this workgroup's counts before its ticket
    if (atomicAdd(counters + 8 + sub, 1u) != quota - 1) return;
    const unsigned groups = nblocks < DIRECT_FAN ? nblocks : DIRECT_FAN;
    if (atomicAdd(counters + 3, 1u) != groups - 1) return;
    __threadfence();  // acquire: every other workgroup's counts before they are read
#pragma unroll
    for (unsigned k = 0; k < DIRECT_FAN; ++k) store_handoff(counters + 8 + k, 0u);
    const uint32_t failed = load_handoff(counters), low = load_handoff(counters + 1);
    const uint32_t wrong = load_handoff(counters + 24), wlow = load_handoff(counters + 25);
    if (summary) {
        summary[0] = failed, summary[1] = failed;
        summary[2] = failed ? 0xffffffffu - low : 0xffffffffu;
        summary[3] = failed ? (uint32_t)DecodingError : 0u;
    }
    bad[0] = wrong, bad[1] = wrong ? 0xffffffffu - wlow : 0xffffffffu;
#pragma unroll
    for (int k = 0; k < 4; ++k) store_handoff(counters + k, 0u);
    store_handoff(counters + 24, 0u), store_handoff(counters + 25, 0u);
}

// DOUBLE: RanDouSha (two sharings, the verdict on both), else RanSha
template <class F, bool DOUBLE>
HB_DEV void producers_wg(const ProducersWgArgs& a) {
    using E = typename F::E;
    constexpr bool SHARE = F::NL == 9;        // U29: a row's products shared by adjacent lanes (dot_shared); Goldilocks' are cheap
    constexpr bool FULL = DOUBLE && !SHARE;   // Goldilocks RanDouSha: the full interpolation
    constexpr int NL = F::NL, EW = F::EW, LS = SHARE ? 12 : F::NL, NS = DOUBLE ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x, n = a.n, nver = a.nver;
    const size_t k = blockIdx.x, K = a.K;
    const ProducersWgLds L(n, NS, nver, (a.sh[0].nv + a.sh[0].M) * a.sh[0].M, (a.sh[1].nv + a.sh[1].M) * a.sh[1].M, LS, NL);
    uint32_t *vmat = lds + L.vmat, *kept = lds + L.kept, *flags = lds + L.flags;

    // ---- loads: every global load is issued before the first LDS write ----------------------------------------------------------------
    const bool from_coeffs = a.sh[0].coeffs != nullptr;
    E in[NS];
    bool have[NS];
    int at[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const ProducersWgSharing& sh = a.sh[s];
        in[s] = F::zero(), have[s] = false, at[s] = 0;
        if (from_coeffs) {  // a lane per (dealer p, coefficient c), staged [c][p] where the mixed block goes
            const int m = sh.deg + 1, p = tid / m, c = tid - p * m;
            if (tid < n * m) have[s] = true, at[s] = L.Y[s] + (c * n + p) * LS, in[s] = F::load(sh.coeffs + (((size_t)p * K + k) * m + c) * EW);
        } else if (tid < n * n) {  // a lane per (dealer p, recipient j)
            have[s] = true, at[s] = L.D[s] + tid * LS, in[s] = F::load(sh.dealt + ((size_t)tid * K + k) * EW);
        }
    }
    TableStage sv, st[NS];
    sv.load(a.vmat, L.vmat_words);
#pragma unroll
    for (int s = 0; s < NS; ++s) st[s].load(a.sh[s].tab, L.tab_words[s]);
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if (have[s]) put_limbs<F>(lds + at[s], in[s]);
    sv.store(vmat, a.vmat, L.vmat_words);
#pragma unroll
    for (int s = 0; s < NS; ++s) st[s].store(lds + L.tab[s], a.sh[s].tab, L.tab_words[s]);
    if (tid < 64) flags[tid] = 0;
    __syncthreads();

    // ---- deal (compute_shares of every dealer's polynomial): a lane per (recipient j, dealer p) ---------------------------------------
    if (from_coeffs) {
        const int j = tid / n, p = tid - j * n;
        if (tid < n * n) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const ProducersWgSharing& sh = a.sh[s];
                const uint32_t* C = lds + L.Y[s];
                const E v = F::canon_loose(dot_rows<F>([&](int c) { return F::load_const(C + (c * n + p) * LS); }, vmat + (size_t)j * n * NL, sh.deg + 1, 0, 0));
                put_limbs<F>(lds + L.D[s] + (p * n + j) * LS, v);
                put_words<F>(sh.dealt + (((size_t)p * n + j) * K + k) * EW, v);
            }
        }
        __syncthreads();
    }

    // ---- mix (make_vandermonde(n, n - 1) over the dealers): a lane per (row i, party j) --------------------------------------------------
    {
        const int i = tid / n, j = tid - i * n;
        if (tid < n * n) {
            const bool list = i >= a.row0 && i < a.row0 + a.rows;
            const int other = i < a.row0 ? i : i - a.rows;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const ProducersWgSharing& sh = a.sh[s];
                const uint32_t* D = lds + L.D[s];
                const E y = F::canon_loose(dot_rows<F>([&](int p) { return F::load_const(D + (p * n + j) * LS); }, vmat + (size_t)i * n * NL, n, 0, 0));
                put_limbs<F>(lds + L.Y[s] + (i * n + j) * LS, y);
                uint32_t* dst = list ? sh.out + (((size_t)j * K + k) * a.rows + (i - a.row0)) * EW : sh.yv + (((size_t)j * nver + other) * K + k) * EW;
                put_words<F>(dst, y);
            }
        }
    }
    __syncthreads();

    // ---- verify: a lane group per (verifier q, table row r); verifier q reads the senders' y[ver0 + q][sender] ----------------------------
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const ProducersWgSharing& sh = a.sh[s];
        const int M = sh.M, nv = sh.nv;
        const int R = FULL ? M : nv + (DOUBLE ? 2 : 1), groups = nver * R;
        int lk = 0;
        if constexpr (SHARE)
            while (lk < 2 && (groups << (lk + 1)) <= 256 && (2 << lk) <= M) ++lk;
        const int gq = tid >> lk, sidx = tid & ((1 << lk) - 1), q = gq / R, r = gq - q * R;
        if (gq < groups) {  // whole groups: the lanes that share a row are all in or all out
            // the coefficient rows kept: RanSha coefficient t; RanDouSha over Fr 0 and deg; the full interpolation every one
            const int row = FULL || r < nv ? r : DOUBLE ? (r == nv ? nv : nv + sh.deg) : nv + a.t;
            const uint32_t* Yq = lds + L.Y[s] + (a.ver0 + q) * n * LS;
            const E c = F::canon_loose(dot_rows<F>([&](int i) { return F::load_const(Yq + i * LS); }, lds + L.tab[s] + (size_t)row * M * NL, M, lk, sidx));
            if (sidx == 0) {
                if constexpr (FULL) {
                    if (r > 0 && !F::is_zero_canon(c)) atomicMax(reinterpret_cast<int*>(flags) + 32 + s * 16 + q, r);
                    if (r == 0) put_limbs<F>(kept + ((s * nver + q) * 2) * LS, c);
                } else if (r < nv) {
                    if (!F::eq_canon(c, F::load_const(Yq + (M + r) * LS))) flags[s * 16 + q] = 1;
                } else {
                    put_limbs<F>(kept + ((s * nver + q) * 2 + (r - nv)) * LS, c);
                }
            }
        }
    }
    __syncthreads();

    // ---- the verifiers' results and the verdict: lane q of the first wave is verifier q ---------------------------------------------------
    if (tid < 64) {
        bool wrong = false;
        if (tid < nver) {
            const int q = tid;
            const size_t g = (size_t)q * K + k;
            if constexpr (!DOUBLE) {
                const bool ok = flags[q] == 0;
                uint8_t* status = reinterpret_cast<uint8_t*>(a.sh[0].st);
                if (status) status[g] = ok ? 0 : (uint8_t)DecodingError;
                if (!ok) {
                    atomicAdd(a.counters, 1u);
                    atomicMax(a.counters + 1, 0xffffffffu - (uint32_t)g);
                }
                wrong = !ok || (a.t > 0 && F::is_zero_canon(F::load_const(kept + q * 2 * LS)));
            } else if constexpr (FULL) {
                const int deg_t = (int)flags[32 + q], deg_2t = (int)flags[48 + q];
                const E c_t = F::load_const(kept + (q * 2) * LS), c_2t = F::load_const(kept + ((nver + q) * 2) * LS);
                put_words<F>(a.sh[0].sel + g * EW, c_t);
                put_words<F>(a.sh[1].sel + g * EW, c_2t);
                reinterpret_cast<uint32_t*>(a.sh[0].st)[g] = (uint32_t)deg_t;
                reinterpret_cast<uint32_t*>(a.sh[1].st)[g] = (uint32_t)deg_2t;
                wrong = deg_t != a.t || deg_2t != 2 * a.t || !F::eq_canon(c_t, c_2t);
            } else {
                E c0[2];
                bool topz[2], ok[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    ok[s] = flags[s * 16 + q] == 0;
                    const uint32_t* kq = kept + ((s * nver + q) * 2) * LS;
                    c0[s] = ok[s] ? F::load_const(kq) : F::zero();
                    const E top = ok[s] ? F::load_const(kq + LS) : F::zero();
                    topz[s] = F::is_zero_canon(top);
                    put_words<F>(a.sh[s].sel + (g * 2) * EW, c0[s]);
                    put_words<F>(a.sh[s].sel + (g * 2 + 1) * EW, top);
                    reinterpret_cast<uint8_t*>(a.sh[s].st)[g] = ok[s] ? 0 : (uint8_t)DecodingError;
                }
                wrong = !ok[0] || !ok[1] || (a.t > 0 && (topz[0] || topz[1])) || !F::eq_canon(c0[0], c0[1]);
            }
        }
        const unsigned long long mask = __ballot(wrong);
        if (tid == 0 && mask != 0) {
            atomicAdd(a.counters + 24, (uint32_t)__popcll(mask));
            atomicMax(a.counters + 25, 0xffffffffu - (uint32_t)k);
        }
    }

    // ---- the last workgroup turns the counters into the summary and bad[2] and leaves the counters at zero -----------------------------------
    finish_producers(a.counters, a.summary, a.bad);
}

template <class F>
__global__ __launch_bounds__(256) void k_ransha_wg(ProducersWgArgs a) {
    producers_wg<F, false>(a);
}
template <class F>
__global__ __launch_bounds__(256) void k_randousha_wg(ProducersWgArgs a) {
    producers_wg<F, true>(a);
}

}  // namespace hbmpc
