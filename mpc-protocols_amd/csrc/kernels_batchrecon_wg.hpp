// BatchReconNode for all parties of a SMALL batch in one launch: a workgroup per chunk of d + 1 shared values
// (honeybadger/batch_recon/batch_recon.rs: init_batch_reconstruct_many :144-185, the EvalBatch arm :371-391, the RevealBatch arm
// :451-467).
//
// The separate steps are three launches -- every party's encode, the recipients' P(0) decodes, the coefficient decode of the revealed
// values -- of 7 - 14 us each at protocol sizes (kernels_triplegen_wg.hpp).  With all parties on one device a chunk depends on nothing
// outside it, so one workgroup of 256 lanes takes it from the shares to the opened values: a lane per (party, element) for the loads,
// a lane per (party, recipient) for the encode, a lane group per (recipient, table row) and per table row for the two decodes
// (dot_shared over U29; over Goldilocks a lane per row).  This is k_triplegen_wg without the local products, for any degree d and any
// two sender sets of exactly d + t + 1 parties (no OEC round: a failed chunk is final), n <= 16.
//
// Every buffer a caller can see gets the bytes of the three launches (tests/test_gpu_batchrecon.py).
#pragma once
#include "wave_core.hpp"

namespace hbmpc {

struct BatchReconWgArgs {
    const uint32_t* x;              // [party][N]
    const uint32_t* vmat;           // [n][d + 1] constants alpha_j^k
    const uint32_t *tab1, *tab2;    // the decodes' tables of the two sender sets: [t verify rows | d + 1 coefficient rows][d + 1]
    uint32_t *Y, *Z, *opened;       // Y[party][recipient][G], Z[recipient][G], opened[G][d + 1]
    uint8_t *rstatus, *status;      // [n G] (byte j G + g: recipient j's decode of chunk g), [G]; either may be null
    uint32_t *summary_first, *summary;
    uint32_t* counters;             // the stream's decode counters ([24], [25]: the recipients' decodes)
    size_t G, N;
    int n, t, d;
    int lk1;                        // the EvalBatch arm: log2 of the lanes that share a (recipient, row)'s products (plan_batchrecon)
    int same;                       // tab2 == tab1: one copy in LDS
    uint8_t ids1[16], ids2[16];     // the d + t + 1 sender ids of each arm, ascending (the order of the tables' rows)
};

// LDS words: X[n][M] | Y[n][n] | Z[n] (elements in limb form, `ls` words apart) | bad flags [n + 1] | vmat | tab1 | tab2
// (nl words per constant: 9 and ls = 12 for U29, 2 and 2 for Goldilocks).  tab1 holds the t verify rows and the P(0) row, tab2 all
// t + M rows; when the sets are equal tab1 is tab2.  Every offset is a multiple of 4 words.
struct BatchReconWgLds {
    int X, Y, Z, flags, vmat, tab1, tab2, total;
    int vmat_words, tab1_words, tab2_words;
    __host__ __device__ static int up4(int w) { return (w + 3) & ~3; }
    __host__ __device__ BatchReconWgLds(int n, int t, int d, int ls, int nl, bool same) {
        const int M = d + 1;
        vmat_words = n * M * nl, tab2_words = (t + M) * M * nl, tab1_words = same ? tab2_words : (t + 1) * M * nl;
        X = 0, Y = up4(X + n * M * ls), Z = up4(Y + n * n * ls), flags = up4(Z + n * ls);
        vmat = up4(flags + n + 1);
        tab1 = up4(vmat + vmat_words);
        tab2 = same ? tab1 : up4(tab1 + tab1_words);
        total = up4(tab2 + tab2_words);
    }
};

template <class F>
__global__ __launch_bounds__(256) void k_batchrecon_wg(BatchReconWgArgs a) {
    using E = typename F::E;
    constexpr bool SHARE = F::NL == 9;  // U29: a row's products shared by adjacent lanes (dot_shared); Goldilocks' are cheap
    constexpr int NL = F::NL, EW = F::EW, LS = SHARE ? 12 : F::NL;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x, n = a.n, t = a.t, M = a.d + 1, nv = t;
    const size_t g = blockIdx.x;
    const BatchReconWgLds L(n, t, a.d, LS, NL, a.same != 0);
    uint32_t *X = lds + L.X, *Yl = lds + L.Y, *Zl = lds + L.Z, *flags = lds + L.flags, *vmat = lds + L.vmat, *tab1 = lds + L.tab1, *tab2 = lds + L.tab2;
    // ids[i], i < 16, from the scalar side (row_of_lane, kernels_recover.hpp, says why)
    auto id_of = [](const uint8_t (&ids)[16], int i) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (i == k) v = ids[k];
        return v;
    };

    // ---- loads: a lane per (party, element of the chunk); the tables by everyone ------------------------------------------------------
    const int pk_p = tid / M, pk_k = tid - pk_p * M;
    const bool pk = tid < n * M;
    E vx = F::zero();
    if (pk) vx = F::load(a.x + ((size_t)pk_p * a.N + g * M + pk_k) * EW);
    TableStage sv, s1, s2;
    sv.load(a.vmat, L.vmat_words);
    s1.load(a.tab1, L.tab1_words);
    if (!a.same) s2.load(a.tab2, L.tab2_words);
    if (pk) put_limbs<F>(X + (pk_p * M + pk_k) * LS, vx);
    sv.store(vmat, a.vmat, L.vmat_words);
    s1.store(tab1, a.tab1, L.tab1_words);
    if (!a.same) s2.store(tab2, a.tab2, L.tab2_words);
    if (tid <= n) flags[tid] = 0;
    __syncthreads();

    // ---- encode (batch_recon.rs:157-165): a lane per (party p, recipient j): y = sum_k alpha_j^k x_p[k] --------------------------------
    {
        const int p = tid / n, j = tid - p * n;
        if (tid < n * n) {
            const E y = F::canon_loose(dot_rows<F>([&](int k) { return F::load_const(X + (p * M + k) * LS); }, vmat + (size_t)j * M * NL, M, 0, 0));
            put_limbs<F>(Yl + (p * n + j) * LS, y);
            put_words<F>(a.Y + (((size_t)p * n + j) * a.G + g) * EW, y);
        }
    }
    __syncthreads();

    // ---- the EvalBatch arm (:384-391): recipient j opens its value from the eval senders' y_p[j], sender i of the sorted set at LDS
    // row ids1[i]: t verify rows and the P(0) row, a lane group per (recipient, row) -----------------------------------------------------
    {
        const int lk = SHARE ? a.lk1 : 0;
        const int q = tid >> lk, sidx = tid & ((1 << lk) - 1), j = q / (nv + 1), r = q - j * (nv + 1);
        const bool mine = q < n * (nv + 1);  // whole groups: the lanes that share a row are all in or all out
        E kept = F::zero();
        if (mine) {
            kept = dot_rows<F>([&](int i) { return F::load_const(Yl + (id_of(a.ids1, i) * n + j) * LS); }, tab1 + (size_t)r * M * NL, M, lk, sidx);
            if (r < nv && sidx == 0 && !F::eq_canon(F::canon_loose(kept), F::load_const(Yl + (id_of(a.ids1, M + r) * n + j) * LS))) flags[j] = 1;
        }
        __syncthreads();
        if (mine && r == nv && sidx == 0) {
            const bool ok = flags[j] == 0;
            const E z = ok ? F::canon_loose(kept) : F::zero();
            put_limbs<F>(Zl + j * LS, z);
            put_words<F>(a.Z + ((size_t)j * a.G + g) * EW, z);
            if (a.rstatus) a.rstatus[(size_t)j * a.G + g] = ok ? 0 : (uint8_t)DecodingError;
            if (!ok) {
                atomicAdd(a.counters + 24, 1u);
                atomicMax(a.counters + 25, 0xffffffffu - (uint32_t)((size_t)j * a.G + g));
            }
        }
    }
    __syncthreads();

    // ---- the RevealBatch arm (:457-467): everyone interpolates the d + 1 opened values from the reveal senders' z_j: t verify rows and
    // d + 1 coefficient rows, a lane group per row -------------------------------------------------------------------------------------
    {
        int lk = 0;
        if constexpr (SHARE)
            while (lk < 2 && (2 << lk) <= M) ++lk;  // (nv + M) << 2 <= 64 lanes: d + t + 1 <= n <= 16
        const int r = tid >> lk, sidx = tid & ((1 << lk) - 1);
        E kept = F::zero();
        if (r < nv + M) {
            kept = dot_rows<F>([&](int i) { return F::load_const(Zl + id_of(a.ids2, i) * LS); }, tab2 + (size_t)r * M * NL, M, lk, sidx);
            if (r < nv && sidx == 0 && !F::eq_canon(F::canon_loose(kept), F::load_const(Zl + id_of(a.ids2, M + r) * LS))) flags[n] = 1;
        }
        __syncthreads();
        const bool ok = flags[n] == 0;
        if (r >= nv && r < nv + M && sidx == 0) put_words<F>(a.opened + (g * M + (r - nv)) * EW, ok ? F::canon_loose(kept) : F::zero());
        if (tid == 0) {
            if (a.status) a.status[g] = ok ? 0 : (uint8_t)DecodingError;
            if (!ok) {
                atomicAdd(a.counters, 1u);
                atomicMax(a.counters + 1, 0xffffffffu - (uint32_t)g);
            }
        }
    }

    // ---- the summaries: the last workgroup turns the counters into them and leaves the counters at zero ------------------------------
    finish_direct(a.counters, {{a.summary_first, 24}, {a.summary, 0}});
}

}  // namespace hbmpc
