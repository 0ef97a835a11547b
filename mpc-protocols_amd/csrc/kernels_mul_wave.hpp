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
#include "kernels_recover.hpp"

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
// broadcast values; then the table.  Limbs sit at a 12-word stride: 16-byte aligned, and with one row per lane the 32 lanes of a
// bank group start 12 banks apart -- at most 3 lanes to a bank (gcd(12, 32) = 4), against 8 at a 32-word stride and an
// unaligned row at 9.  Every offset is a multiple of 4 words, so the uint4 stores of the operands and of d, e are aligned.
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

    auto put_limbs = [&](uint32_t* dst, const E& v) {
#pragma unroll
        for (int i = 0; i < 9; ++i) dst[i] = v.l[i];
    };
    auto put_words = [&](uint32_t* dst, const E& canon) {
        uint32_t w[8];
        F::to_words(canon, w);
        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<uint4*>(dst + 4) = make_uint4(w[4], w[5], w[6], w[7]);
    };

    // ---- every global load of the element, then the LDS writes -------------------------------------------------------------
    const int tq = tab_words >> 2;
    uint4 t0 = make_uint4(0, 0, 0, 0), t1 = t0;
    if ((int)threadIdx.x < tq) t0 = reinterpret_cast<const uint4*>(a.tab)[threadIdx.x];
    if ((int)threadIdx.x + 256 < tq) t1 = reinterpret_cast<const uint4*>(a.tab)[threadIdx.x + 256];
    E sa = F::zero(), sx = F::zero(), sb = F::zero(), sy = F::zero();
    if (lane < a.needed) {
        const size_t ip = (size_t)row_of_lane(a.rows, lane) * a.N + g;
        sa = F::load(a.ta + ip * 8), sx = F::load(a.x + ip * 8), sb = F::load(a.tb + ip * 8), sy = F::load(a.y + ip * 8);
    }
    // operand item q of party p: 0 y, 1 x, 2 c
    const int nops = 3 * P;
    auto op_src = [&](int it) -> const uint32_t* {
        const int q = it / P, p = it - q * P;
        const uint32_t* base = q == 0 ? a.y : q == 1 ? a.x : a.tc;
        return base + ((size_t)p * a.N + g) * 8;
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
    if (lane < a.needed) {  // the shares Multiply opens (mul/multiplication.rs:417-426), canonical as k_beaver_open_pair stores them
        put_limbs(ysd + lane * 12, F::canon_loose(F::template sub<2>(sa, sx)));
        put_limbs(yse + lane * 12, F::canon_loose(F::template sub<2>(sb, sy)));
    }
    if (lane < nops) {
        *reinterpret_cast<uint4*>(ops + lane * 8) = o0[0];
        *reinterpret_cast<uint4*>(ops + lane * 8 + 4) = o0[1];
    }
    if (lane + 64 < nops) {
        *reinterpret_cast<uint4*>(ops + (lane + 64) * 8) = o1[0];
        *reinterpret_cast<uint4*>(ops + (lane + 64) * 8 + 4) = o1[1];
    }
    for (int it = lane + 128; it < nops; it += 64) {  // live from P = 43 on
        const uint32_t* s = op_src(it);
        *reinterpret_cast<uint4*>(ops + it * 8) = *reinterpret_cast<const uint4*>(s);
        *reinterpret_cast<uint4*>(ops + it * 8 + 4) = *reinterpret_cast<const uint4*>(s + 4);
    }
    __syncthreads();

    // ---- the open (multiplication.rs:102-139): a - x in lanes 0 .. 31, b - y in lanes 32 .. 63; row r of the table per lane ---
    // (r < nv verify rows; nv: P(0); nv + 1: P(0) R, what finalize_mul multiplies by)
    {
        const int h = lane >> 5, r = (lane & 31) >> a.lk, sidx = lane & ((1 << a.lk) - 1);
        const uint32_t* ys = h ? yse : ysd;
        bool bad = false;
        E kept = F::zero();
        if (r < nv + 2) {  // whole quads: the lanes that share a row are all in or all out
            kept = dot_shared<F>([&](int i) { return F::load_const(ys + i * 12); }, tab + (size_t)r * M * 9, M, a.lk, sidx);
            if (r < nv) bad = !F::eq_canon(F::canon_loose(kept), F::load_const(ys + (M + r) * 12));
        }
        const unsigned long long vote = __ballot(bad);
        const bool ok_d = (uint32_t)vote == 0, ok_e = (uint32_t)(vote >> 32) == 0, ok = h ? ok_e : ok_d;
        if (r == nv && sidx == 0) {
            const E v = ok ? F::canon_loose(kept) : F::zero();
            put_words(bc + h * 8, v);
            if (live) {
                put_words(a.de_out + ((size_t)h * a.N + g) * 8, v);
                if (a.status) a.status[(size_t)h * a.N + g] = ok ? 0 : (uint8_t)DecodingError;
            }
        }
        if (r == nv + 1 && sidx == 0) put_limbs(bc + 16 + h * 12, ok ? kept : F::zero());
        if (live && lane == 0 && !(ok_d && ok_e)) {  // chunk g is the a - x of the element, chunk N + g its b - y
            atomicAdd(a.counters, (ok_d ? 0u : 1u) + (ok_e ? 0u : 1u));
            atomicMax(a.counters + 1, 0xffffffffu - (uint32_t)(ok_d ? a.N + g : g));
        }
    }
    __syncthreads();

    // ---- finalize_mul (multiplication.rs:57-100): a product per lane -----------------------------------------------------------
    //   q = 0: (e + y_p) d R    1: x_p e R
    for (int task = lane; task < 2 * P; task += 64) {
        const int q = task / P, p = task - q * P;
        typename F::Acc acc;
        F::acc_zero(acc);
        E v = F::load(ops + (q * P + p) * 8);
        if (q == 0) v = F::normalize(F::add(v, F::load(bc + 8)));
        F::acc_mac(acc, v, bc + 16 + q * 12);
        F::acc_fold(acc);
        put_limbs(res + (q * P + p) * 12, F::acc_reduce(acc));
    }
    __syncthreads();
    for (int p = lane; p < P; p += 64) {  // z_p = c_p - both
        E acc = F::template sub<4>(F::load(ops + (2 * P + p) * 8), F::load_const(res + p * 12));
        acc = F::template sub<4>(acc, F::load_const(res + (P + p) * 12));
        if (live) put_words(a.z + ((size_t)p * a.N + g) * 8, F::canon_loose(acc));
    }

    // ---- the summary: the last workgroup turns the counters into it and leaves the counters at zero ----------------------------
    finish_direct(a.counters, a.summary);
}

}  // namespace hbmpc
