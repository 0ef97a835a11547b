// kernels_mfma_bfly_lab.hpp -- laboratory forms of k_mfma_bfly (csrc/kernels_mfma_bfly.hpp), for the microbenchmarks under tools/ only;
// nothing here is compiled into the library.  k_mfma_bfly_lab<M, WAVES, NP, ABL, TRIPLE, TRIPLE_DEPTH, DEG, LINES> calls the
// production kernel's own pieces where that header has them as functions (the table copy, bfly_pair with its ABL hooks, the output
// offsets, the degree, the dropped stores); the input loads, the store, the tile loop and the TRIPLE walk are written in place in
// k_mfma_bfly -- as functions they change its instructions (profiles/bfly_shared_body.txt) -- and are COPIES of that text here,
// without LISTS and DEG's store_rows, kept equal by hand.  On top of it:
//   ABL    timing-only ablations: 1 = no epilogue arithmetic (the stores stay and depend on every accumulator register),
//          2 = no MFMAs (EVERY dword of every loaded input is folded into the accumulators), 4 = no LDS operand reads either
//          (both in bfly_pair), 8 = (TRIPLE) no field products (the three operands of every element are XOR-ed: every load stays)
//   LINES  (chunk-major inputs) a tile's M KB requested as whole lines -- lane l takes 16-byte piece i * 64 + l -- and turned into
//          the operand layout through a wave-private LDS slot (chunk c at c * (32 M + 16) bytes), instead of M 16-byte gathers per
//          lane at a stride of 32 M bytes; bit-identical, not faster (profiles/r03_mfma_bfly_followup.txt)
// Round 3's ablations folded only one dword of each loaded vector, and hipcc dropped about half of the input loads as dead
// (VERDICT r3 / ADVICE r3).  Check every ablated instance before quoting its time:
//   python3 tools/count_loads.py tools/ubench_mfma_bfly.hip -DBFLY_ABLATE
#pragma once
#include "../mpc-protocols_amd/csrc/kernels_mfma_bfly.hpp"

namespace hbmpc {
namespace mf {

// this half's four words of output k (pe + pt) or of its partner (pe - pt, MINUS) for both laboratory kernels: the sum or
// difference of the un-normalised digit pairs, one carry pass and reduction; ABL & 1: four adds instead.  (The library kernels
// keep these lines in place: as a function they reorder the instructions of every instance.)
template <bool MINUS, int ABL>
HB_DEV void bfly_words_lab(const uint32_t (&pe)[8], const uint32_t (&pt)[8], const Half& H, uint32_t (&Rw)[4]) {
    uint32_t s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = MINUS ? pe[j] - pt[j] : pe[j] + pt[j];
    if constexpr ((ABL & 1) != 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Rw[j] = s[2 * j] + s[2 * j + 1];
    } else {
        uint64_t T[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) T[j] = (uint64_t)s[2 * j + 1] * H.k16 + s[2 * j];
        reduce_words(T, Rw, H);
    }
}

template <int M>
constexpr int bfly_slot_bytes() { return 32 * (M * 32 + 16); }
template <int M, int WAVES, int NP = 0, int ABL = 0, bool TRIPLE = false, int TRIPLE_DEPTH = 1, bool DEG = false, bool LINES = false>
__global__ __launch_bounds__(64 * WAVES) void k_mfma_bfly_lab(MfmaRowsArgs a) {
    static_assert(M >= 2 && M <= 16, "digit sums must stay below 0xff0000 (tables_mfma.hpp: proved per table for M = 16)");
    constexpr int ROWB = M * 1024 + MF_BFLY_BIAS;
    constexpr int NT = 64 * WAVES;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];  // role.nrows * ROWB
    const int blk8 = (int)blockIdx.x >> 3, role_id = a.blk_role[blk8];
    const int wg_in_role = (int)a.blk_idx[blk8] * 8 + ((int)blockIdx.x & 7);
    MfmaRole role = a.role[0];
    int role_wgs = a.role_nwg[0];
#pragma unroll
    for (int k = 1; k < MF_MAX_ROLES; ++k)
        if (k == role_id) role = a.role[k], role_wgs = a.role_nwg[k];
    bfly_table_to_lds<NT>(lds, a.table + (size_t)role.row0 * ROWB, role.nrows * (ROWB / 16));
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const Half H = make_half(h);
    const size_t ntiles = (a.G + 31) / 32;
    const size_t tstep = (size_t)role_wgs * WAVES;
    // NP > 0: nothing inside the tile loop is conditional -- the next tile's loads are issued even past the end (clamped to
    // the last chunk) and stores go through a buffer descriptor that drops what must not be written (dead lanes: an offset
    // beyond the buffer; a partner point that does not exist: a buffer of zero bytes) -- so that hipcc knows how many vector
    // memory operations follow a load and waits for a tile's inputs with vmcnt(stores + later loads) instead of vmcnt(0).
    // vmcnt retires in order: with a conditional load or store in between, the wait for the OLDER input set also drains
    // the set requested a moment ago, i.e. every other tile would pay a full HBM round trip.
    constexpr bool STATIC = NP > 0;
    // inputs: chunk-major x[G][M] (compute_shares, apply_vandermonde) or M rows, row i at in + rows[i] * row_stride * 32 (the
    // producers' mixing step reads the dealt shares where the dealers' encodes left them: S[dealer][..])
    [[maybe_unused]] uint32_t waddr[LINES ? M : 1];  // where this lane's piece i of a tile goes in the slot
    [[maybe_unused]] uint8_t* slot = lds + (size_t)role.nrows * ROWB + (size_t)wave * bfly_slot_bytes<M>();
    if constexpr (LINES) {
#pragma unroll
        for (int i = 0; i < M; ++i) {
            const uint32_t byte = (uint32_t)(i * 64 + lane) * 16u;
            waddr[i] = byte / (M * 32u) * (M * 32u + 16u) + byte % (M * 32u);
        }
    }
    auto load_inputs = [&](size_t t, v4i (&dst)[M]) {
        const size_t gi = t * 32 + c;
        const uint32_t g = (uint32_t)(gi < a.G ? gi : a.G - 1);
        if constexpr (LINES) {
            const size_t total = a.G * (size_t)(M * 32), tb = t * 32 * (size_t)(M * 32);
#pragma unroll
            for (int i = 0; i < M; ++i) {
                const size_t off = tb + (size_t)(i * 64 + lane) * 16;
                dst[i] = *reinterpret_cast<const v4i*>(a.in + (off + 16 <= total ? off : total - 16));  // past the end: any in-bounds piece
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < M; ++i) {
            if (a.in_chunk_major) {
                dst[i] = *reinterpret_cast<const v4i*>(a.in + (size_t)i * 32 + (g * (M * 32u) + 16u * h));
            } else {
                uint32_t ri = (uint32_t)a.rows[i];
                asm volatile("" : "+s"(ri));  // recomputed at every use (scalar registers, as in k_mfma_rows)
                dst[i] = *reinterpret_cast<const v4i*>(a.in + (size_t)ri * a.row_stride * 32 + (g * 32u + 16u * h));
            }
        }
    };
    const uint32_t row_bytes = (uint32_t)([&] {
        const size_t b = a.out_party_major ? a.G * 32 : a.G * a.out_stride * 32;
        return b < 0xffffffe0ull ? b : 0xffffffe0ull;
    }());
    auto store_row = [&](uint8_t* out, uint32_t k, bool exists, bool live, uint32_t qo, const uint32_t (&Rw)[4]) {
        uint8_t* qb = a.out_party_major ? out + (size_t)k * a.out_stride * 32 : out + (size_t)k * 32;  // wave-uniform
        if constexpr (STATIC) {
            v4i val;
            val[0] = (int)Rw[0], val[1] = (int)Rw[1], val[2] = (int)Rw[2], val[3] = (int)Rw[3];
            __builtin_amdgcn_raw_buffer_store_b128(val, rt_rsrc(qb, exists ? row_bytes : 0u), (int)(live ? qo : RT_OOB), 0, 0);
        } else {
            if (exists && live) *reinterpret_cast<uint4*>(qb + qo) = make_uint4(Rw[0], Rw[1], Rw[2], Rw[3]);
        }
    };
    // the pairs of one tile from its B operands (sign-flipped bytes)
    auto pairs_of_tile = [&](size_t t, const v4i (&data)[M], uint8_t* out) {
        const BflyOut o = bfly_out(a, t, c, h);
        [[maybe_unused]] uint32_t degree = 0;
#pragma unroll
        for (int p = 0; p < (STATIC ? NP : role.nrows); ++p) {
            uint32_t pe[8], pt[8];
            bfly_pair<M, ABL>(lds + (size_t)p * ROWB, lane, h, data, pe, pt);
            uint32_t k32 = (uint32_t)(role.row0 + p);
            asm volatile("" : "+s"(k32));  // the output row bases are recomputed, not kept per unrolled pair (scalar registers)
            uint32_t Rw[4];
            bfly_words_lab<false, ABL>(pe, pt, H, Rw);
            store_row(out, k32, true, o.live, o.qo, Rw);
            if constexpr (DEG) bfly_note_degree(degree, k32, true, Rw);
            const bool partner = (int)k32 + a.half < a.nout;
            if (STATIC || partner) {
                bfly_words_lab<true, ABL>(pe, pt, H, Rw);
                store_row(out, k32 + (uint32_t)a.half, partner, o.live, o.qo, Rw);
                if constexpr (DEG) bfly_note_degree(degree, k32 + (uint32_t)a.half, partner, Rw);
            }
        }
        if constexpr (DEG) {  // one more counted store: lanes that do not write get an offset beyond the buffer
            const size_t db = a.G * 4;
            __builtin_amdgcn_raw_buffer_store_b32(degree, rt_rsrc(a.ncoeffs, (uint32_t)(db < 0xffffffe0ull ? db : 0xffffffe0ull)),
                                                  (int)(o.live && h == 0 ? o.g * 4u : RT_OOB), 0, 0);
        }
    };
    auto process_tile = [&](size_t t, v4i (&data)[M]) {
        if constexpr (LINES) {  // pieces -> slot -> operands (the same wave writes and reads: no barrier)
#pragma unroll
            for (int i = 0; i < M; ++i) *reinterpret_cast<v4i*>(slot + waddr[i]) = data[i];
#pragma unroll
            for (int i = 0; i < M; ++i) data[i] = *reinterpret_cast<const v4i*>(slot + c * (M * 32 + 16) + i * 32 + 16 * h);
        }
#pragma unroll
        for (int i = 0; i < M; ++i) data[i] = flip(data[i]);
        pairs_of_tile(t, data, a.out);
    };
    auto dropped_stores = [&] { bfly_dropped_stores<2 * NP + (DEG ? 1 : 0)>(a.out); };
    if constexpr (TRIPLE) {
        using F = U29;
        constexpr int NS = (M + 1) / 2;  // slots: slot j holds coefficient 2 j + h of this lane's chunk
        struct Slot {
            v4i a[2], b[2], r[2];
        };
        // (party, tile) of this wave's current work item, advanced without a division; parties beyond the last are clamped
        // for the loads past the end
        auto load_slot = [&](uint32_t pp, size_t t, int j) {
            const size_t gi = t * 32 + c;
            const size_t g = (size_t)(pp < (uint32_t)a.parties ? pp : (uint32_t)a.parties - 1) * a.G + (gi < a.G ? gi : a.G - 1);
            const int i = 2 * j + h < M ? 2 * j + h : M - 1;  // M odd: the last slot of the upper lanes repeats the last coefficient (unused)
            const size_t off = (g * M + (size_t)i) * 32;
            Slot sl;
            sl.a[0] = *reinterpret_cast<const v4i*>(a.in + off), sl.a[1] = *reinterpret_cast<const v4i*>(a.in + off + 16);
            sl.b[0] = *reinterpret_cast<const v4i*>(a.in_b + off), sl.b[1] = *reinterpret_cast<const v4i*>(a.in_b + off + 16);
            sl.r[0] = *reinterpret_cast<const v4i*>(a.in_r + off), sl.r[1] = *reinterpret_cast<const v4i*>(a.in_r + off + 16);
            return sl;
        };
        auto elem = [](const v4i (&w)[2]) {
            const uint32_t ww[8] = {(uint32_t)w[0][0], (uint32_t)w[0][1], (uint32_t)w[0][2], (uint32_t)w[0][3],
                                    (uint32_t)w[1][0], (uint32_t)w[1][1], (uint32_t)w[1][2], (uint32_t)w[1][3]};
            return F::from_words(ww);
        };
        // x = (a b - r2t) R^-1 (R = 2^261, the Montgomery radix of fr_u29.hpp) as 8 words of a value below 2 r -- any
        // representative below 2^256 serves, the table is linear in the bytes -- from ONE reduction: the 81 limb products of
        // a b and the limbs of 2 r - r2t go into the same 18 columns (U_SUBC2 keeps every limb difference non-negative), then
        // the 72 multiply-adds of the Montgomery reduction.  The factor R^-1 is undone by the TABLE, whose rows are
        // alpha^i R for this kernel (hbmpc_capi.hip: "mfbflyR"), so no operand is ever converted to Montgomery form.
        auto product = [&](const Slot& sl, v4i& lo, v4i& hi) {
            if constexpr ((ABL & 8) != 0) {  // timing only: no field arithmetic, every load stays
#pragma unroll
                for (int k = 0; k < 4; ++k) lo[k] = sl.a[0][k] ^ sl.b[0][k] ^ sl.r[0][k], hi[k] = sl.a[1][k] ^ sl.b[1][k] ^ sl.r[1][k];
                return;
            }
            const F::E ea = elem(sl.a), eb = elem(sl.b), er = elem(sl.r);
            F::Acc A;
            F::acc_zero(A);
#pragma unroll
            for (int i = 0; i < 9; ++i) A.c[i] += (uint64_t)(consts::U_SUBC2[i] - er.l[i]);
            F::acc_mac_pinned(A, ea, eb.l);
            const F::E cc = F::canon_loose(F::acc_reduce(A));
            uint32_t w[8];
            F::to_words(cc, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) lo[k] = (int)w[k], hi[k] = (int)w[4 + k];
        };
        uint32_t pp = 0;
        size_t t = (size_t)wg_in_role * WAVES + wave;
        auto settle = [&](uint32_t& q, size_t& u) {
            while (u >= ntiles && q < (uint32_t)a.parties) u -= ntiles, ++q;
        };
        settle(pp, t);
        // slots are requested SD ahead of their use, across the item boundary: while the last slots of an item are multiplied
        // and while its pairs run, the first SD slots of the wave's next item are on their way
        constexpr int SD = TRIPLE_DEPTH;
        static_assert(SD >= 1 && SD <= NS, "slot prefetch depth");
        Slot ring[SD];
        if (pp < (uint32_t)a.parties) {
#pragma unroll
            for (int j = 0; j < SD; ++j) ring[j] = load_slot(pp, t, j);
            if constexpr (STATIC) dropped_stores();
        }
        v4i data[M];
        while (pp < (uint32_t)a.parties) {
            uint32_t ppn = pp;
            size_t tn = t + tstep;
            settle(ppn, tn);
            const size_t tnc = tn < ntiles ? tn : ntiles - 1;
            // positions 0 .. NSP - 1, NSP = the slot count rounded up to the ring size: a slot always returns to the ring entry
            // it had in the previous item (positions >= NS are empty: nothing is multiplied, nothing requested for them)
            constexpr int NSP = (NS + SD - 1) / SD * SD;
#pragma unroll
            for (int j = 0; j < NSP; ++j) {
                v4i lo, hi;
                if (j < NS) product(ring[j % SD], lo, hi);
                if (j + SD < NS) ring[j % SD] = load_slot(pp, t, j + SD);
                else if (j + SD >= NSP) ring[j % SD] = load_slot(ppn, tnc, j + SD - NSP);
                if (j < NS) {
                    // lower lanes hold coefficient 2 j, upper lanes 2 j + 1: the swap leaves (low half | high half) of 2 j in lo
                    // and of 2 j + 1 in hi, each lane with its own 16 bytes
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const auto sw = __builtin_amdgcn_permlane32_swap((uint32_t)lo[k], (uint32_t)hi[k], false, false);
                        lo[k] = (int)sw[0], hi[k] = (int)sw[1];
                    }
                    data[2 * j] = flip(lo);
                    if (2 * j + 1 < M) data[2 * j + 1] = flip(hi);
                }
            }
            pairs_of_tile(t, data, a.out + (size_t)pp * (size_t)a.nout * a.out_stride * 32);
            pp = ppn, t = tn;
        }
    } else {
        // the tile loop of k_mfma_rows: two input register sets, the loads of a wave's NEXT tile issued before it starts on the
        // current one
        v4i setA[M], setB[M];
        size_t t = (size_t)wg_in_role * WAVES + wave;
        if (t < ntiles) {
            load_inputs(t, setA);
            if constexpr (STATIC) dropped_stores();
        }
        while (t < ntiles) {
            if (STATIC || t + tstep < ntiles) load_inputs(t + tstep, setB);
            process_tile(t, setA);
            t += tstep;
            if (t >= ntiles) break;
            if (STATIC || t + tstep < ntiles) load_inputs(t + tstep, setA);
            process_tile(t, setB);
            t += tstep;
        }
    }
}

}  // namespace mf
}  // namespace hbmpc
