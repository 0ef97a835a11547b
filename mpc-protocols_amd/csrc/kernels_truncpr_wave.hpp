// TruncPrNode (fpmul/truncpr.rs:185-318) and FPDivConstNode (fpdiv/fpdiv_const.rs:61-99: a local product with a public
// reciprocal, then the same TruncPr) for all parties of a SMALL batch in one launch: a wave per batch element.
//
// This is the second half of k_fpmul_wave (kernels_fpmul_wave.hpp) on its own: the value that is truncated comes from the caller
// (a, or a * w with the public multiplier w of the element) instead of from a Beaver multiplication.  The separate steps -- the
// product + r' + the share TruncPr opens, its decode, the last step -- are three launches of 4 - 13 us each whatever the batch
// (profiles/r04_small_batch_fpmul.txt); here an element is one round trip of loads, the parties' products spread over the lanes
// (a lane per (party, product): every product is "sum of a_k * c_k, then one REDC", so the lanes stay converged), the decode
// with a lane per table row (the t verify rows and the P(0) row; the products of a row shared by a DPP quad where the rows
// fit, dot_shared), and the last step with a lane per party.
//
// The bytes of every buffer a caller can see are those of the three launches (tests/test_gpu_truncpr.py): each value is stored
// canonical, and a chunk that fails its verification opens to zero and is counted, exactly as there.
#pragma once
#include "wave_core.hpp"

namespace hbmpc {

struct TruncprWaveArgs {
    const uint32_t *a, *r_bits, *r_int;    // [party][N], [party][m][N], [party][N]
    const uint32_t* w;                     // [N] public canonical multipliers (HAS_W instances)
    const uint32_t* pow2;                  // [m] constants 2^j
    const uint32_t* tab;                   // [t verify rows | P(0) row][t + 1] constants (the head of fpmul_wave_table)
    uint32_t *c, *r_dash, *open_sh, *out;  // [party][N]; c = a * w (HAS_W instances)
    uint32_t* c_open;                      // [N]
    uint8_t* status;                       // [N] as the decode leaves it, or null
    uint32_t* summary;                     // the open's summary
    uint32_t* counters;                    // the stream's decode counters, zero at the start and at the end
    size_t N;
    int parties, m, needed, M;             // needed = 2 t + 1 senders, M = t + 1
    int mask_bits;                         // TruncPr's modulus 2^m as a bit count (min(m, 256))
    int lk;                                // log2 of the lanes that share a table row's products (0 .. 2)
    RowsArg rows;                          // rows[i] = party id of the i-th lowest sender
    uint32_t c0[9], c1[9], cinv[9], r2[9]; // 2^m (constant form), 2^(k-1) (plain limbs), 2^-m (constant form), R^2
};

// LDS words of one workgroup (4 elements): per wave the parties' operands (and the multiplier), the products, the open shares
// and the broadcast values; then pow2 | c0 | the table.  Limbs sit at the 12-word stride of wave_core.hpp.
struct TruncprWaveLds {
    size_t per_wave, ops, res, val, bc, consts, tab, total;
    __host__ __device__ TruncprWaveLds(int parties, int m, int tab_words) {
        ops = 0;                                          // [2 + m][party] canonical words: a, r_int, bits; then w
        res = ops + ((size_t)(2 + m) * parties + 1) * 8;  // [3][party] limbs: a * w, 2^m r_int, r'
        val = res + (size_t)3 * parties * 12;             // [party] limbs: the shares TruncPr opens
        bc = val + (size_t)parties * 12;                  // the opened value (8 words) | w R (12)
        per_wave = bc + 8 + 12;
        consts = 4 * per_wave;                            // [m + 1][12]: pow2 then c0
        tab = consts + (size_t)(m + 1) * 12;
        total = tab + (((size_t)tab_words + 3) & ~(size_t)3);
    }
};

template <class F, bool HAS_W>
__global__ __launch_bounds__(256) void k_truncpr_wave(TruncprWaveArgs a) {
    using E = typename F::E;
    static_assert(F::EW == 8 && F::NL == 9, "U29 only");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t g_raw = (size_t)blockIdx.x * 4 + wave;
    const bool live = g_raw < a.N;  // the last workgroup's idle waves redo element N - 1 and store nothing
    const size_t g = live ? g_raw : a.N - 1;
    const int M = a.M, nv = a.needed - M, P = a.parties;
    const int tab_words = (nv + 1) * M * 9;
    const TruncprWaveLds L(P, a.m, tab_words);
    uint32_t* W = lds + (size_t)wave * L.per_wave;
    uint32_t *ops = W + L.ops, *res = W + L.res, *val = W + L.val, *bc = W + L.bc;
    uint32_t *cst = lds + L.consts, *tab = lds + L.tab;

    // ---- every global load of the element, then the LDS writes (wave_core.hpp) ---------------------------------------------------
    // operand item q of party p: 0 a, 1 r_int, 2 + j bit j; the item after the last is the element's multiplier
    const int nparty = (2 + a.m) * P, nops = nparty + (HAS_W ? 1 : 0);
    auto op_src = [&](int it) -> const uint32_t* {
        if (HAS_W && it == nparty) return a.w + g * 8;
        const int q = it / P, p = it - q * P;
        return q < 2 ? (q == 0 ? a.a : a.r_int) + ((size_t)p * a.N + g) * 8 : a.r_bits + (((size_t)p * a.m + (q - 2)) * a.N + g) * 8;
    };
    TableStage tabs;
    Pow2Stage pows;
    OperandStage opers;
    tabs.load(a.tab, tab_words);
    pows.load(a.pow2, a.c0, a.m);
    opers.load(op_src, nops);
    tabs.store(tab, a.tab, tab_words);
    pows.store(cst, a.pow2, a.c0, a.m);
    opers.store(ops, op_src, nops);
    __syncthreads();

    // ---- the public multiplier in Montgomery form, once per element (every lane forms it: the wave is idle anyway) -----------
    if constexpr (HAS_W) {
        const E wm = F::mulc(F::load(ops + nparty * 8), a.r2);
        if (lane == 0) put_limbs<F>(bc + 8, wm);
        __syncthreads();
    }

    // ---- a * w (fpdiv_const.rs:79), 2^m r_int, r' (truncpr.rs:277-283): a product per lane -------------------------------------
    //   q = 0: a_p (w R)    1: r_int_p 2^m    2: sum_j bit_pj 2^j
    constexpr int Q0 = HAS_W ? 0 : 1;
    for (int task = lane; task < (3 - Q0) * P; task += 64) {
        const int q = Q0 + task / P, p = task % P;
        const uint32_t* cs = q == 0 ? bc + 8 : q == 1 ? cst + a.m * 12 : cst;
        lane_product<F>(res + (q * P + p) * 12, ops + (q * P + p) * 8, P * 8, cs, q == 2 ? a.m : 1, [](const E& v) { return v; });
    }
    __syncthreads();
    E vc = F::zero(), rd = F::zero();  // party `lane`'s truncated value and r', kept for the last step
    if (lane < P) {
        const int p = lane;
        vc = HAS_W ? F::canon_loose(F::load_const(res + p * 12)) : F::load(ops + p * 8);
        rd = F::canon_loose(F::load_const(res + (2 * P + p) * 12));
        E o = F::add(vc, F::load_const(a.c1));
        o = F::add(o, F::load_const(res + (P + p) * 12));
        o = F::canon_loose(F::add(o, rd));
        put_limbs<F>(val + p * 12, o);
        if (live) {
            const size_t ip = (size_t)p * a.N + g;
            if constexpr (HAS_W) put_words<F>(a.c + ip * 8, vc);
            put_words<F>(a.r_dash + ip * 8, rd);
            put_words<F>(a.open_sh + ip * 8, o);
        }
    }
    __syncthreads();

    // ---- the open (truncpr.rs:215) -------------------------------------------------------------------------------------------
    open_single<F>(val, tab, bc, a.lk, nv, M, a.rows, live, g, a.counters, a.c_open, a.status);
    __syncthreads();

    // ---- TruncPr's last step ---------------------------------------------------------------------------------------------------
    if (lane < P) {
        const E o = truncpr_last<F>(bc, a.mask_bits, rd, vc, a.cinv);
        if (live) F::store_lt2r(a.out + ((size_t)lane * a.N + g) * 8, o);
    }

    // ---- the summary: the last workgroup turns the counters into it and leaves the counters at zero ----------------------------
    finish_direct(a.counters, a.summary);
}

}  // namespace hbmpc
