// FPMulNode for all parties of a SMALL batch in one launch: a wave per batch element (fpmul/fpmul.rs:61-110).
//
// At the batch sizes the protocols run a fixed-point multiplication at (a few hundred to a few thousand elements) the five
// launches of the separate steps -- the shares Multiply opens, their decode, finalize_mul + r' + the share TruncPr opens, its
// decode, TruncPr's last step -- cost 4 - 13 us each whatever the batch (profiles/r04_small_batch_fpmul.txt): a lone wave
// per SIMD walks a chain of v_mad_u64_u32 at ~10 cycles each (profiles/r01_isa_rates.txt) behind a memory round trip, five times over.  With all parties on one
// device every step of an element depends on that element alone, so one wave can take it from the triple to the output
// shares: one round trip of loads, and the multiplications of a step spread over the lanes the step would leave idle
// (a lane per table row in the decodes; a lane per (party, product) between them -- every product of a step is the same
// instruction stream, "sum of a_k * c_k, then one REDC", so the lanes stay converged).
//
// The bytes of every buffer a caller can see are those of the separate launches (tests/test_gpu_pipelines.py): each value is
// stored canonical, and a chunk that fails its verification opens to zero and is counted, exactly as there.
//
// The two opens and TruncPr's last step are wave_core.hpp's, as in k_mul_wave and k_truncpr_wave (the two halves of this kernel).
// The staging, the products and the summary tail keep their own text here, word for word what wave_core.hpp's staging structs,
// lane_product and finish_direct hold: composed of those, this kernel replayed as a graph measured 0.8 us slower at 64 elements
// (0.0218 against 0.0211 ms; 0.3 us at 256), the compiler scheduling the longer body differently, and with these three written
// out it is the earlier kernel's time again (profiles/wave_core.txt, section 4).  A change to one of them belongs in both places.
#pragma once
#include "wave_core.hpp"

namespace hbmpc {

struct FpmulWaveArgs {
    const uint32_t *ta, *tb, *tc, *x, *y;  // [party][N]: the triple's shares, the factors' shares
    const uint32_t *r_bits, *r_int;        // [party][m][N], [party][N]
    const uint32_t* pow2;                  // [m] constants 2^j
    const uint32_t* tab;                   // [t verify rows | P(0) row | P(0) * R row][t + 1] constants (hbmpc_capi.hip, fpmul_wave_table)
    uint32_t *de_out;                      // [2 N]: the opened a - x, then the opened b - y
    uint32_t *z, *r_dash, *open_sh, *out;  // [party][N]
    uint32_t* c_open;                      // [N]
    uint8_t* status;                       // [2 N] as the two decodes leave it: [0, N) the second open's, [N, 2 N) the b - y half of the first
    uint32_t *summary_first, *summary;     // the two opens' summaries
    uint32_t* counters;                    // the stream's decode counters, zero at the start and at the end ([24], [25]: the first open)
    size_t N;
    int parties, m, needed, M;             // needed = 2 t + 1 senders, M = t + 1
    int mask_bits;                         // TruncPr's modulus 2^m as a bit count (min(m, 256))
    int lk1, lk3;                          // log2 of the lanes that share a table row's products in the first / second open (0 .. 2)
    RowsArg rows;                          // rows[i] = party id of the i-th lowest sender
    uint32_t c0[9], c1[9], cinv[9];        // 2^m (constant form), 2^(k-1) (plain limbs), 2^-m (constant form)
};

// LDS words of one workgroup (4 elements): per wave the senders' two values, the parties' operands, the products, the open
// shares and the broadcast values; then pow2 | c0 | the table.  Limbs sit at the 12-word stride of wave_core.hpp.
struct FpmulWaveLds {
    size_t per_wave, ysd, yse, ops, res, val, bc, consts, tab, total;
    __host__ __device__ FpmulWaveLds(int needed, int parties, int m, int tab_words) {
        ysd = 0, yse = ysd + (size_t)needed * 12;     // limbs
        ops = yse + (size_t)needed * 12;              // [4 + m][party] canonical words: y, x, c, r_int, bits
        res = ops + (size_t)(4 + m) * parties * 8;    // [4][party] limbs
        val = res + (size_t)4 * parties * 12;         // [party] limbs
        bc = val + (size_t)parties * 12;              // d, e (8 words each) | d R, e R (12 each) | the second open (8)
        per_wave = bc + 16 + 24 + 8;
        consts = 4 * per_wave;                        // [m + 1][12]: pow2 then c0
        tab = consts + (size_t)(m + 1) * 12;
        total = tab + (((size_t)tab_words + 3) & ~(size_t)3);
    }
};

template <class F>
__global__ __launch_bounds__(256) void k_fpmul_wave(FpmulWaveArgs a) {
    using E = typename F::E;
    static_assert(F::EW == 8 && F::NL == 9, "U29 only");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t g_raw = (size_t)blockIdx.x * 4 + wave;
    const bool live = g_raw < a.N;
    const size_t g = live ? g_raw : a.N - 1;
    const int M = a.M, nv = a.needed - M, P = a.parties;
    const int tab_words = (nv + 2) * M * 9;
    const FpmulWaveLds L(a.needed, P, a.m, tab_words);
    uint32_t* W = lds + (size_t)wave * L.per_wave;
    uint32_t *ysd = W + L.ysd, *yse = W + L.yse, *ops = W + L.ops, *res = W + L.res, *val = W + L.val, *bc = W + L.bc;
    uint32_t *cst = lds + L.consts, *tab = lds + L.tab;

    // ---- every global load of the element, then the LDS writes -------------------------------------------------------------
    const int tq = tab_words >> 2;
    uint4 t0 = make_uint4(0, 0, 0, 0), t1 = t0;
    if ((int)threadIdx.x < tq) t0 = reinterpret_cast<const uint4*>(a.tab)[threadIdx.x];
    if ((int)threadIdx.x + 256 < tq) t1 = reinterpret_cast<const uint4*>(a.tab)[threadIdx.x + 256];
    uint32_t cw = 0;  // pow2 [m][9] and c0 at a 12-word stride
    const int ncw = (a.m + 1) * 9;
    if ((int)threadIdx.x < ncw) cw = (int)threadIdx.x < a.m * 9 ? a.pow2[threadIdx.x] : a.c0[threadIdx.x - a.m * 9];
    E sa = F::zero(), sx = F::zero(), sb = F::zero(), sy = F::zero();
    if (lane < a.needed) {
        const size_t ip = (size_t)row_of_lane(a.rows, lane) * a.N + g;
        sa = F::load(a.ta + ip * 8), sx = F::load(a.x + ip * 8), sb = F::load(a.tb + ip * 8), sy = F::load(a.y + ip * 8);
    }
    // operand item q of party p: 0 y, 1 x, 2 c, 3 r_int, 4 + j bit j
    const int nops = (4 + a.m) * P;
    auto op_src = [&](int it) -> const uint32_t* {
        const int q = it / P, p = it - q * P;
        const uint32_t* base = q == 0 ? a.y : q == 1 ? a.x : q == 2 ? a.tc : a.r_int;
        return q < 4 ? base + ((size_t)p * a.N + g) * 8 : a.r_bits + (((size_t)p * a.m + (q - 4)) * a.N + g) * 8;
    };
    uint4 o0[2] = {t0, t0}, o1[2] = {t0, t0};
    if (lane < nops) {
        const uint32_t* s = op_src(lane);
        o0[0] = *reinterpret_cast<const uint4*>(s), o0[1] = *reinterpret_cast<const uint4*>(s + 4);
    }
    if (lane + 64 < nops) {
        const uint32_t* s = op_src(lane + 64);
        o1[0] = *reinterpret_cast<const uint4*>(s), o1[1] = *reinterpret_cast<const uint4*>(s + 4);
    }
    if ((int)threadIdx.x < tq) reinterpret_cast<uint4*>(tab)[threadIdx.x] = t0;
    if ((int)threadIdx.x + 256 < tq) reinterpret_cast<uint4*>(tab)[threadIdx.x + 256] = t1;
    for (int q = threadIdx.x + 512; q < tq; q += 256) reinterpret_cast<uint4*>(tab)[q] = reinterpret_cast<const uint4*>(a.tab)[q];
    for (int w = (tq << 2) + threadIdx.x; w < tab_words; w += 256) tab[w] = a.tab[w];
    if ((int)threadIdx.x < ncw) cst[(threadIdx.x / 9) * 12 + threadIdx.x % 9] = cw;
    for (int w = threadIdx.x + 256; w < ncw; w += 256) cst[(w / 9) * 12 + w % 9] = w < a.m * 9 ? a.pow2[w] : a.c0[w - a.m * 9];
    if (lane < a.needed) {  // the shares Multiply opens (mul/multiplication.rs:417-426), canonical as k_beaver_open_pair stores them
        put_limbs<F>(ysd + lane * 12, F::canon_loose(F::template sub<2>(sa, sx)));
        put_limbs<F>(yse + lane * 12, F::canon_loose(F::template sub<2>(sb, sy)));
    }
    if (lane < nops) {
        *reinterpret_cast<uint4*>(ops + lane * 8) = o0[0];
        *reinterpret_cast<uint4*>(ops + lane * 8 + 4) = o0[1];
    }
    if (lane + 64 < nops) {
        *reinterpret_cast<uint4*>(ops + (lane + 64) * 8) = o1[0];
        *reinterpret_cast<uint4*>(ops + (lane + 64) * 8 + 4) = o1[1];
    }
    for (int it = lane + 128; it < nops; it += 64) {
        const uint32_t* s = op_src(it);
        *reinterpret_cast<uint4*>(ops + it * 8) = *reinterpret_cast<const uint4*>(s);
        *reinterpret_cast<uint4*>(ops + it * 8 + 4) = *reinterpret_cast<const uint4*>(s + 4);
    }
    __syncthreads();

    // ---- the first open (multiplication.rs:102-139): chunk g is the a - x of the element, chunk N + g its b - y; the a - x half's
    // status byte is the second open's to write ----------------------------------------------------------------------------------
    open_pair<F>(ysd, yse, tab, bc, a.lk1, nv, M, live, g, a.N, a.counters + 24, a.de_out, nullptr, a.status ? a.status + a.N : nullptr);
    __syncthreads();

    // ---- finalize_mul (multiplication.rs:57-100), r' (truncpr.rs:277-283), 2^m r_int: a product per lane ---------------------
    //   q = 0: (e + y_p) d R    1: x_p e R    2: r_int_p 2^m    3: sum_j bit_pj 2^j
    for (int task = lane; task < 4 * P; task += 64) {
        const int q = task / P, p = task - q * P;
        const int terms = q == 3 ? a.m : 1;
        const uint32_t* cs = q == 0 ? bc + 16 : q == 1 ? bc + 28 : q == 2 ? cst + a.m * 12 : cst;
        typename F::Acc acc;
        F::acc_zero(acc);
        int pending = 0;
        for (int k = 0; k < terms; ++k) {
            if (pending == F::MAX_DOT_TERMS) {
                F::acc_fold(acc);
                pending = 1;
            }
            E v = F::load(ops + ((q == 0 ? 0 : q == 1 ? 1 : q == 2 ? 3 : 4 + k) * P + p) * 8);
            if (q == 0) v = F::normalize(F::add(v, F::load(bc + 8)));
            F::acc_mac(acc, v, cs + k * 12);
            ++pending;
        }
        F::acc_fold(acc);
        put_limbs<F>(res + (q * P + p) * 12, F::acc_reduce(acc));
    }
    __syncthreads();
    E zc = F::zero(), rd = F::zero();  // party `lane`'s z and r', kept for TruncPr's last step
    for (int p = lane; p < P; p += 64) {
        E acc = F::template sub<4>(F::load(ops + (2 * P + p) * 8), F::load_const(res + p * 12));
        acc = F::template sub<4>(acc, F::load_const(res + (P + p) * 12));
        zc = F::canon_loose(acc);
        rd = F::canon_loose(F::load_const(res + (3 * P + p) * 12));
        E o = F::add(zc, F::load_const(a.c1));
        o = F::add(o, F::load_const(res + (2 * P + p) * 12));
        o = F::canon_loose(F::add(o, rd));
        put_limbs<F>(val + p * 12, o);
        if (live) {
            const size_t ip = (size_t)p * a.N + g;
            put_words<F>(a.z + ip * 8, zc);
            put_words<F>(a.r_dash + ip * 8, rd);
            put_words<F>(a.open_sh + ip * 8, o);
        }
    }
    __syncthreads();

    // ---- the second open (truncpr.rs:215) ---------------------------------------------------------------------------------
    open_single<F>(val, tab, bc + 40, a.lk3, nv, M, a.rows, live, g, a.counters, a.c_open, a.status);
    __syncthreads();

    // ---- TruncPr's last step ---------------------------------------------------------------------------------------------------
    if (P <= 64) {
        if (lane < P) {
            const E o = truncpr_last<F>(bc + 40, a.mask_bits, rd, zc, a.cinv);
            if (live) F::store_lt2r(a.out + ((size_t)lane * a.N + g) * 8, o);
        }
    }

    // ---- the summaries: the last workgroup turns the counters into them and leaves the counters at zero ------------------------
    __syncthreads();
    if (threadIdx.x != 0) return;
    __threadfence();
    const unsigned nblocks = gridDim.x, sub = blockIdx.x % DIRECT_FAN, quota = nblocks / DIRECT_FAN + (sub < nblocks % DIRECT_FAN ? 1u : 0u);
    if (atomicAdd(a.counters + 8 + sub, 1u) != quota - 1) return;
    const unsigned groups = nblocks < DIRECT_FAN ? nblocks : DIRECT_FAN;
    if (atomicAdd(a.counters + 3, 1u) != groups - 1) return;
    __threadfence();
#pragma unroll
    for (unsigned k = 0; k < DIRECT_FAN; ++k) store_handoff(a.counters + 8 + k, 0u);
    const uint32_t f1 = load_handoff(a.counters + 24), l1 = load_handoff(a.counters + 25);
    const uint32_t f2 = load_handoff(a.counters), l2 = load_handoff(a.counters + 1);
    if (a.summary_first) {
        a.summary_first[0] = f1, a.summary_first[1] = f1;
        a.summary_first[2] = f1 ? 0xffffffffu - l1 : 0xffffffffu;
        a.summary_first[3] = f1 ? (uint32_t)DecodingError : 0u;
    }
    if (a.summary) {
        a.summary[0] = f2, a.summary[1] = f2;
        a.summary[2] = f2 ? 0xffffffffu - l2 : 0xffffffffu;
        a.summary[3] = f2 ? (uint32_t)DecodingError : 0u;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) store_handoff(a.counters + k, 0u);
    store_handoff(a.counters + 24, 0u);
    store_handoff(a.counters + 25, 0u);
}

}  // namespace hbmpc
