// The pieces that the one-launch protocol kernels are composed of: k_mul_wave and k_truncpr_wave (a wave per batch element) use
// all of them, k_input_wave the table stage and the single open, k_fpmul_wave the opens, the last step and the LDS element helpers
// (its staging and products are written out there, kernels_fpmul_wave.hpp says why), k_triplegen_wg, k_randbit_wg and k_prandbit_wg
// (a workgroup per chunk) the LDS element helpers.
// The summary tail is finish_direct (kernels_recover.hpp); k_fpmul_wave and k_randbit_wg keep theirs written out.
//
// LDS layout the wave kernels share: canonical operands are 8 words apart, limb-form values (U29) 12.  12 is 16-byte aligned, and
// with one row per lane the 32 lanes of a bank group start 12 banks apart -- at most 3 lanes to a bank (gcd(12, 32) = 4), against 8
// at a 32-word stride and an unaligned row at 9.  Every offset of the layout structs is a multiple of 4 words, so the uint4 stores
// of the operands and of the opened values are aligned.
#pragma once
#include "kernels_recover.hpp"

namespace hbmpc {

// ---- LDS element helpers ---------------------------------------------------------------------------------------------------------
template <class F>
HB_DEV void put_limbs(uint32_t* dst, const typename F::E& v) {
#pragma unroll
    for (int i = 0; i < F::NL; ++i) dst[i] = v.l[i];
}
// canonical value -> the stored form, in LDS or global memory (U29: dst is 16-byte aligned)
template <class F>
HB_DEV void put_words(uint32_t* dst, const typename F::E& canon) {
    if constexpr (F::NL == 9) {
        uint32_t w[8];
        F::to_words(canon, w);
        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<uint4*>(dst + 4) = make_uint4(w[4], w[5], w[6], w[7]);
    } else {
        F::store_lt2r(dst, canon);
    }
}
// a table row times M values.  U29: the products shared by 2^lk adjacent lanes, which must be active together (dot_shared,
// kernels_recover.hpp); Goldilocks' products are a few instructions: a lane per row, lk and sidx unused
template <class F, class Y>
HB_DEV typename F::E dot_rows(Y&& value_of, const uint32_t* row, int M, int lk, int sidx) {
    if constexpr (F::NL == 9) {
        return dot_shared<F>(value_of, row, M, lk, sidx);
    } else {
        typename F::Acc acc;
        F::acc_zero(acc);
        for (int i = 0; i < M; ++i) F::acc_mac(acc, value_of(i), row + i * F::NL);
        return F::acc_reduce(acc);
    }
}

// ---- staging a wave's element: every global load of the element is issued (load) before the first LDS write (store) ----------------
// The in-flight registers of one kind of input; a kernel calls every load, then every store, then its barrier.

// the workgroup's table of `words` constants: two uint4 per thread in flight, what is left copied at the store
struct TableStage {
    uint4 t0, t1;
    HB_DEV void load(const uint32_t* src, int words) {
        const int tq = words >> 2;
        t0 = make_uint4(0, 0, 0, 0), t1 = t0;
        if ((int)threadIdx.x < tq) t0 = reinterpret_cast<const uint4*>(src)[threadIdx.x];
        if ((int)threadIdx.x + 256 < tq) t1 = reinterpret_cast<const uint4*>(src)[threadIdx.x + 256];
    }
    HB_DEV void store(uint32_t* tab, const uint32_t* src, int words) const {
        const int tq = words >> 2;
        if ((int)threadIdx.x < tq) reinterpret_cast<uint4*>(tab)[threadIdx.x] = t0;
        if ((int)threadIdx.x + 256 < tq) reinterpret_cast<uint4*>(tab)[threadIdx.x + 256] = t1;
        for (int q = threadIdx.x + 512; q < tq; q += 256) reinterpret_cast<uint4*>(tab)[q] = reinterpret_cast<const uint4*>(src)[q];
        for (int w = (tq << 2) + threadIdx.x; w < words; w += 256) tab[w] = src[w];
    }
};
// the workgroup's pow2 [m][9] (global) and c0 [9] (kernel argument), to a 12-word stride
struct Pow2Stage {
    uint32_t cw;
    HB_DEV void load(const uint32_t* pow2, const uint32_t (&c0)[9], int m) {
        cw = 0;
        if ((int)threadIdx.x < (m + 1) * 9) cw = (int)threadIdx.x < m * 9 ? pow2[threadIdx.x] : c0[threadIdx.x - m * 9];
    }
    HB_DEV void store(uint32_t* cst, const uint32_t* pow2, const uint32_t (&c0)[9], int m) const {
        const int ncw = (m + 1) * 9;
        if ((int)threadIdx.x < ncw) cst[(threadIdx.x / 9) * 12 + threadIdx.x % 9] = cw;
        for (int w = threadIdx.x + 256; w < ncw; w += 256) cst[(w / 9) * 12 + w % 9] = w < m * 9 ? pow2[w] : c0[w - m * 9];
    }
};
// the wave's `nops` operand items of 8 canonical words, item `it` read at op_src(it): two per lane in flight, what is left copied
// at the store (live from 129 items on: Multiply's 3 P at P = 43)
struct OperandStage {
    uint4 o0[2], o1[2];
    template <class Src>
    HB_DEV void load(Src&& op_src, int nops) {
        const int lane = threadIdx.x & 63;
        o0[0] = o0[1] = o1[0] = o1[1] = make_uint4(0, 0, 0, 0);
        if (lane < nops) {
            const uint32_t* s = op_src(lane);
            o0[0] = *reinterpret_cast<const uint4*>(s), o0[1] = *reinterpret_cast<const uint4*>(s + 4);
        }
        if (lane + 64 < nops) {
            const uint32_t* s = op_src(lane + 64);
            o1[0] = *reinterpret_cast<const uint4*>(s), o1[1] = *reinterpret_cast<const uint4*>(s + 4);
        }
    }
    template <class Src>
    HB_DEV void store(uint32_t* ops, Src&& op_src, int nops) const {
        const int lane = threadIdx.x & 63;
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
    }
};
// the shares Multiply opens (mul/multiplication.rs:417-426): sender `lane` of the `needed` lowest; a - x and b - y stored as limbs,
// canonical as k_beaver_open_pair stores them
template <class F>
struct PairStage {
    typename F::E sa, sx, sb, sy;
    HB_DEV void load(const uint32_t* ta, const uint32_t* x, const uint32_t* tb, const uint32_t* y, const RowsArg& rows, int needed, size_t N, size_t g) {
        const int lane = threadIdx.x & 63;
        sa = F::zero(), sx = F::zero(), sb = F::zero(), sy = F::zero();
        if (lane < needed) {
            const size_t ip = (size_t)row_of_lane(rows, lane) * N + g;
            sa = F::load(ta + ip * 8), sx = F::load(x + ip * 8), sb = F::load(tb + ip * 8), sy = F::load(y + ip * 8);
        }
    }
    HB_DEV void store(uint32_t* ysd, uint32_t* yse, int needed) const {
        const int lane = threadIdx.x & 63;
        if (lane < needed) {
            put_limbs<F>(ysd + lane * 12, F::canon_loose(F::template sub<2>(sa, sx)));
            put_limbs<F>(yse + lane * 12, F::canon_loose(F::template sub<2>(sb, sy)));
        }
    }
};

// ---- the opens: a lane per table row, rows [nv verify | P(0) | ..] of M constants each in `tab` ------------------------------------
// Both vote with __ballot, so EVERY lane of the wave must call them: they take no lane and test `live` themselves -- call them
// from wave-uniform control flow only, never under a branch on the lane, the party or `live`.  A chunk that fails its
// verification opens to zero and is counted in counters[0] (how many) and counters[1] (the lowest, as 0xffffffff - chunk).

// Multiply's open (multiplication.rs:102-139) of both values at once: a - x (limbs at ysd, sender i at i * 12) in lanes 0 .. 31,
// chunk g; b - y (yse) in lanes 32 .. 63, chunk N + g.  Row nv: P(0); row nv + 1: P(0) R, what finalize_mul multiplies by.
// Leaves d, e as canonical words at bc, bc + 8 and d R, e R as limbs at bc + 16, bc + 28; the opened values go to
// de_out[h N + g] and, where the pointer is not null, the status bytes to status_d[g] / status_e[g].
template <class F>
HB_DEV void open_pair(const uint32_t* ysd, const uint32_t* yse, const uint32_t* tab, uint32_t* bc, int lk, int nv, int M, bool live, size_t g,
                      size_t N, uint32_t* counters, uint32_t* de_out, uint8_t* status_d, uint8_t* status_e) {
    using E = typename F::E;
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5, r = (lane & 31) >> lk, sidx = lane & ((1 << lk) - 1);
    const uint32_t* ys = h ? yse : ysd;
    bool bad = false;
    E kept = F::zero();
    if (r < nv + 2) {  // whole quads: the lanes that share a row are all in or all out
        kept = dot_rows<F>([&](int i) { return F::load_const(ys + i * 12); }, tab + (size_t)r * M * 9, M, lk, sidx);
        if (r < nv) bad = !F::eq_canon(F::canon_loose(kept), F::load_const(ys + (M + r) * 12));
    }
    const unsigned long long vote = __ballot(bad);
    const bool ok_d = (uint32_t)vote == 0, ok_e = (uint32_t)(vote >> 32) == 0, ok = h ? ok_e : ok_d;
    if (r == nv && sidx == 0) {
        const E v = ok ? F::canon_loose(kept) : F::zero();
        put_words<F>(bc + h * 8, v);
        uint8_t* status = h ? status_e : status_d;
        if (live) put_words<F>(de_out + ((size_t)h * N + g) * 8, v);
        if (live && status) status[g] = ok ? 0 : (uint8_t)DecodingError;
    }
    if (r == nv + 1 && sidx == 0) put_limbs<F>(bc + 16 + h * 12, ok ? kept : F::zero());
    if (live && lane == 0 && !(ok_d && ok_e)) {
        atomicAdd(counters, (ok_d ? 0u : 1u) + (ok_e ? 0u : 1u));
        atomicMax(counters + 1, 0xffffffffu - (uint32_t)(ok_d ? N + g : g));
    }
}

// TruncPr's open (truncpr.rs:215) of chunk g: party p's share as limbs at val + p * 12, the senders picked by `rows`.  Row nv:
// P(0).  Leaves the opened value as canonical words at `opened`; it goes to c_open[g], the status byte to status[g] (or null).
// Returns whether the chunk verified, the same in every lane (Input's last step must not run on a zero that stands for a failure).
template <class F>
HB_DEV bool open_single(const uint32_t* val, const uint32_t* tab, uint32_t* opened, int lk, int nv, int M, const RowsArg& rows, bool live,
                        size_t g, uint32_t* counters, uint32_t* c_open, uint8_t* status) {
    using E = typename F::E;
    const int lane = threadIdx.x & 63;
    bool bad = false;
    E kept = F::zero();
    const int r = lane >> lk, sidx = lane & ((1 << lk) - 1);
    if (r < nv + 1) {  // whole quads: the lanes that share a row are all in or all out
        kept = dot_rows<F>([&](int i) { return F::load_const(val + rows[i] * 12); }, tab + (size_t)r * M * 9, M, lk, sidx);
        if (r < nv) bad = !F::eq_canon(F::canon_loose(kept), F::load_const(val + row_of_lane(rows, M + r) * 12));
    }
    const bool ok = __ballot(bad) == 0;
    if (r == nv && sidx == 0) {
        const E v = ok ? F::canon_loose(kept) : F::zero();
        put_words<F>(opened, v);
        if (live) {
            put_words<F>(c_open + g * 8, v);
            if (status) status[g] = ok ? 0 : (uint8_t)DecodingError;
            if (!ok) {
                atomicAdd(counters, 1u);
                atomicMax(counters + 1, 0xffffffffu - (uint32_t)g);
            }
        }
    }
    return ok;
}

// ---- a product per lane: res = sum_k op_k c_k with one reduction ("sum of a_k * c_k, then one REDC": the lanes stay converged) ---
// op_k: canonical words at op + k * op_stride, the first passed through `first`; c_k: constant at cs + k * 12
template <class F, class T>
HB_DEV void lane_product(uint32_t* res, const uint32_t* op, int op_stride, const uint32_t* cs, int terms, T&& first) {
    typename F::Acc acc;
    F::acc_zero(acc);
    int pending = 0;
    for (int k = 0; k < terms; ++k) {
        if (pending == F::MAX_DOT_TERMS) {
            F::acc_fold(acc);
            pending = 1;  // the folded columns count as less than one term
        }
        typename F::E v = F::load(op + k * op_stride);
        if (k == 0) v = first(v);
        F::acc_mac(acc, v, cs + k * 12);
        ++pending;
    }
    F::acc_fold(acc);
    put_limbs<F>(res, F::acc_reduce(acc));
}

// ---- TruncPr's last step (truncpr.rs:216-220, fpmul/mod.rs:381-406): (v - ((c mod 2^mask_bits) - r')) 2^-m, c the opened words ----
template <class F>
HB_DEV typename F::E truncpr_last(const uint32_t* opened, int mask_bits, const typename F::E& rd, const typename F::E& v, const uint32_t (&cinv)[9]) {
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int lo_bit = 32 * q;
        const uint32_t mask = mask_bits >= lo_bit + 32 ? 0xffffffffu : (mask_bits <= lo_bit ? 0u : ((1u << (mask_bits - lo_bit)) - 1u));
        w[q] = opened[q] & mask;
    }
    typename F::E tt = F::template sub<2>(rd, F::from_words(w));
    tt = F::add(tt, v);
    return F::mulc(tt, cinv);
}

}  // namespace hbmpc
