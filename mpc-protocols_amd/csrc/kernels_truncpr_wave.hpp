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
#include "kernels_recover.hpp"

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
// and the broadcast values; then pow2 | c0 | the table.  Limbs sit at a 12-word stride: 16-byte aligned, and with one row per
// lane the 32 lanes of a bank group start 12 banks apart -- at most 3 lanes to a bank (gcd(12, 32) = 4), against 8 at a
// 32-word stride and an unaligned row at 9.
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
    uint32_t cw = 0;  // pow2 [m][9] and c0 at a 12-word stride
    const int ncw = (a.m + 1) * 9;
    if ((int)threadIdx.x < ncw) cw = (int)threadIdx.x < a.m * 9 ? a.pow2[threadIdx.x] : a.c0[threadIdx.x - a.m * 9];
    // operand item q of party p: 0 a, 1 r_int, 2 + j bit j; the item after the last is the element's multiplier
    const int nparty = (2 + a.m) * P, nops = nparty + (HAS_W ? 1 : 0);
    auto op_src = [&](int it) -> const uint32_t* {
        if (HAS_W && it == nparty) return a.w + g * 8;
        const int q = it / P, p = it - q * P;
        return q < 2 ? (q == 0 ? a.a : a.r_int) + ((size_t)p * a.N + g) * 8 : a.r_bits + (((size_t)p * a.m + (q - 2)) * a.N + g) * 8;
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

    // ---- the public multiplier in Montgomery form, once per element (every lane forms it: the wave is idle anyway) -----------
    if constexpr (HAS_W) {
        const E wm = F::mulc(F::load(ops + nparty * 8), a.r2);
        if (lane == 0) put_limbs(bc + 8, wm);
        __syncthreads();
    }

    // ---- a * w (fpdiv_const.rs:79), 2^m r_int, r' (truncpr.rs:277-283): a product per lane -------------------------------------
    //   q = 0: a_p (w R)    1: r_int_p 2^m    2: sum_j bit_pj 2^j
    constexpr int Q0 = HAS_W ? 0 : 1;
    for (int task = lane; task < (3 - Q0) * P; task += 64) {
        const int q = Q0 + task / P, p = task % P;
        const int terms = q == 2 ? a.m : 1;
        const uint32_t* cs = q == 0 ? bc + 8 : q == 1 ? cst + a.m * 12 : cst;
        typename F::Acc acc;
        F::acc_zero(acc);
        int pending = 0;
        for (int k = 0; k < terms; ++k) {
            if (pending == F::MAX_DOT_TERMS) {
                F::acc_fold(acc);
                pending = 1;
            }
            F::acc_mac(acc, F::load(ops + ((q == 2 ? 2 + k : q) * P + p) * 8), cs + k * 12);
            ++pending;
        }
        F::acc_fold(acc);
        put_limbs(res + (q * P + p) * 12, F::acc_reduce(acc));
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
        put_limbs(val + p * 12, o);
        if (live) {
            const size_t ip = (size_t)p * a.N + g;
            if constexpr (HAS_W) put_words(a.c + ip * 8, vc);
            put_words(a.r_dash + ip * 8, rd);
            put_words(a.open_sh + ip * 8, o);
        }
    }
    __syncthreads();

    // ---- the open (truncpr.rs:215): row r of the table per lane, r < nv verify rows, nv the P(0) row ---------------------------
    {
        bool bad = false;
        E kept = F::zero();
        const int r = lane >> a.lk, sidx = lane & ((1 << a.lk) - 1);
        if (r < nv + 1) {  // whole quads: the lanes that share a row are all in or all out
            kept = dot_shared<F>([&](int i) { return F::load_const(val + a.rows[i] * 12); }, tab + (size_t)r * M * 9, M, a.lk, sidx);
            if (r < nv) bad = !F::eq_canon(F::canon_loose(kept), F::load_const(val + row_of_lane(a.rows, M + r) * 12));
        }
        const bool ok = __ballot(bad) == 0;
        if (r == nv && sidx == 0) {
            const E v = ok ? F::canon_loose(kept) : F::zero();
            put_words(bc, v);
            if (live) {
                put_words(a.c_open + g * 8, v);
                if (a.status) a.status[g] = ok ? 0 : (uint8_t)DecodingError;
                if (!ok) {
                    atomicAdd(a.counters, 1u);
                    atomicMax(a.counters + 1, 0xffffffffu - (uint32_t)g);
                }
            }
        }
    }
    __syncthreads();

    // ---- TruncPr's last step (truncpr.rs:216-220, fpmul/mod.rs:381-406): (v - ((c mod 2^m) - r')) 2^-m ------------------------
    if (lane < P) {
        uint32_t w[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int lo_bit = 32 * q;
            const uint32_t mask = a.mask_bits >= lo_bit + 32 ? 0xffffffffu : (a.mask_bits <= lo_bit ? 0u : ((1u << (a.mask_bits - lo_bit)) - 1u));
            w[q] = bc[q] & mask;
        }
        E tt = F::template sub<2>(rd, F::from_words(w));
        tt = F::add(tt, vc);
        const E o = F::mulc(tt, a.cinv);
        if (live) F::store_lt2r(a.out + ((size_t)lane * a.N + g) * 8, o);
    }

    // ---- the summary: the last workgroup turns the counters into it and leaves the counters at zero ----------------------------
    finish_direct(a.counters, a.summary);
}

}  // namespace hbmpc
