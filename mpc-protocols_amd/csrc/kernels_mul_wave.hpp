// Multiply (Beaver, mul/multiplication.rs:417-426,102-139,57-100) for all parties of a SMALL batch in one launch: a wave per
// batch element.
//
// This is the first half of k_fpmul_wave (kernels_fpmul_wave.hpp) on its own, up to and including z: the shares Multiply opens,
// their decode and finalize_mul.  The separate steps are three launches of 4 - 13 us each whatever the batch
// (profiles/r04_small_batch_fpmul.txt); here an element is one round trip of loads, the open with a lane per table row (a - x
// in lanes 0 .. 31, b - y in lanes 32 .. 63; the t verify rows, the P(0) row and the P(0) R row; the products of a row shared
// by a DPP quad where the rows fit, dot_shared), and finalize_mul with a lane per (party, product).
//
// The bytes of every buffer a caller can see are those of the three launches (tests/test_gpu_mul.py): each value is stored
// canonical, and a chunk that fails its verification opens to zero and is counted, exactly as there.
#pragma once
#include "wave_core.hpp"

namespace hbmpc {

struct MulWaveArgs {
    const uint32_t *ta, *tb, *tc, *x, *y;  // [party][N]: the triple's shares, the factors' shares
    const uint32_t* tab;                   // [t verify rows | P(0) row | P(0) * R row][t + 1] constants (hbmpc_capi.hip, fpmul_wave_table)
    uint32_t* de_out;                      // [2 N]: the opened a - x, then the opened b - y
    uint32_t* z;                           // [party][N]
    uint8_t* status;                       // [2 N] as the decode of the 2 N values leaves it, or null
    uint32_t* summary;                     // the open's summary
    uint32_t* counters;                    // the stream's decode counters, zero at the start and at the end
    size_t N;
    int parties, needed, M;                // needed = 2 t + 1 senders, M = t + 1
    int lk;                                // log2 of the lanes that share a table row's products (0 .. 2)
    RowsArg rows;                          // rows[i] = party id of the i-th lowest sender
};

// LDS words of one workgroup (4 elements): per wave the senders' two values, the parties' operands, the two products and the
// broadcast values; then the table.  Limbs sit at the 12-word stride of wave_core.hpp; every offset is a multiple of 4 words.
struct MulWaveLds {
    size_t per_wave, ysd, yse, ops, res, bc, tab, total;
    __host__ __device__ MulWaveLds(int needed, int parties, int tab_words) {
        ysd = 0, yse = ysd + (size_t)needed * 12;  // limbs
        ops = yse + (size_t)needed * 12;           // [3][party] canonical words: y, x, c
        res = ops + (size_t)3 * parties * 8;       // [2][party] limbs
        bc = res + (size_t)2 * parties * 12;       // d, e (8 words each) | d R, e R (12 each)
        per_wave = bc + 16 + 24;
        tab = 4 * per_wave;
        total = tab + (((size_t)tab_words + 3) & ~(size_t)3);
    }
};

template <class F>
__global__ __launch_bounds__(256) void k_mul_wave(MulWaveArgs a) {
    using E = typename F::E;
    static_assert(F::EW == 8 && F::NL == 9, "U29 only");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t g_raw = (size_t)blockIdx.x * 4 + wave;
    const bool live = g_raw < a.N;  // the last workgroup's idle waves redo element N - 1 and store nothing
    const size_t g = live ? g_raw : a.N - 1;
    const int M = a.M, nv = a.needed - M, P = a.parties;
    const int tab_words = (nv + 2) * M * 9;
    const MulWaveLds L(a.needed, P, tab_words);
    uint32_t* W = lds + (size_t)wave * L.per_wave;
    uint32_t *ysd = W + L.ysd, *yse = W + L.yse, *ops = W + L.ops, *res = W + L.res, *bc = W + L.bc;
    uint32_t* tab = lds + L.tab;

    // ---- every global load of the element, then the LDS writes (wave_core.hpp) ---------------------------------------------------
    // operand item q of party p: 0 y, 1 x, 2 c
    const int nops = 3 * P;
    auto op_src = [&](int it) -> const uint32_t* {
        const int q = it / P, p = it - q * P;
        const uint32_t* base = q == 0 ? a.y : q == 1 ? a.x : a.tc;
        return base + ((size_t)p * a.N + g) * 8;
    };
    TableStage tabs;
    PairStage<F> pair;
    OperandStage opers;
    tabs.load(a.tab, tab_words);
    pair.load(a.ta, a.x, a.tb, a.y, a.rows, a.needed, a.N, g);
    opers.load(op_src, nops);
    tabs.store(tab, a.tab, tab_words);
    pair.store(ysd, yse, a.needed);
    opers.store(ops, op_src, nops);
    __syncthreads();

    // ---- the open (multiplication.rs:102-139): chunk g is the a - x of the element, chunk N + g its b - y ------------------------
    open_pair<F>(ysd, yse, tab, bc, a.lk, nv, M, live, g, a.N, a.counters, a.de_out, a.status, a.status ? a.status + a.N : nullptr);
    __syncthreads();

    // ---- finalize_mul (multiplication.rs:57-100): a product per lane -----------------------------------------------------------
    //   q = 0: (e + y_p) d R    1: x_p e R
    for (int task = lane; task < 2 * P; task += 64) {
        const int q = task / P, p = task - q * P;
        lane_product<F>(res + (q * P + p) * 12, ops + (q * P + p) * 8, 0, bc + 16 + q * 12, 1,
                        [&](const E& v) { return q == 0 ? F::normalize(F::add(v, F::load(bc + 8))) : v; });
    }
    __syncthreads();
    for (int p = lane; p < P; p += 64) {  // z_p = c_p - both
        E acc = F::template sub<4>(F::load(ops + (2 * P + p) * 8), F::load_const(res + p * 12));
        acc = F::template sub<4>(acc, F::load_const(res + (P + p) * 12));
        if (live) put_words<F>(a.z + ((size_t)p * a.N + g) * 8, F::canon_loose(acc));
    }

    // ---- the summary: the last workgroup turns the counters into it and leaves the counters at zero ----------------------------
    finish_direct(a.counters, a.summary);
}

}  // namespace hbmpc
