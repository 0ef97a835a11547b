// encode_route.hpp -- which kernel a Vandermonde encode takes: ONE place for the rule (plain C++, no HIP).
//
// plan_encode maps the context's knobs and the call's shape to the ordered candidates the executors in hbmpc_capi.hip try:
// each builds the table its route needs, fills the kernel arguments and launches; a launcher that declines (it does not
// instantiate the shape) or a point-pair table whose digit-sum bound does not hold (tables_mfma.hpp) moves on to the next
// candidate.  The last candidate of every plan cannot decline.  Three kinds of call:
//   chunk-major   x[parties][G][d + 1] -> y[parties][n][G] (compute_shares, vandermonde_apply and its _parties / _strided forms)
//   rows          x as d + 1 rows of G elements, optionally writing the producers' lists (vandermonde_apply_rows[_lists|_split])
//   triple        the local products a b - r2t of triple generation, then the chunk-major encode of parties x G chunks
// The measurements behind every threshold are in the comments at the gates below and in DESIGN.md.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "mfma_plan.hpp"
#include "tables.hpp"
#include "tables_mfma.hpp"
#include "tables_mfma_gl.hpp"

namespace hbmpc {

// the hbmpc_ctx fields the rule reads
struct EncodeKnobs {
    int impl;
    bool force_generic, matrix_cores, mfma_team, mfma_bfly, list_rows_in_kernel;
    size_t wide_max_chunks, mfma_min_encode, mfma_min_gold;
    int mfma_wgs, n_cus;
};
enum class EncodeKind { ChunkMajor, Rows, Triple };
struct EncodeShape {
    EncodeKind kind;
    size_t G, n, d;
    size_t parties = 1;
    size_t ys = 0;              // output row stride (0: G)
    bool lists = false;         // rows: the call writes the producers' lists
    bool workspace = false;     // triple: a workspace for the two-step form was passed
};
enum class EncodeKernel {
    WideDot,       // k_eval_wide_dot: small batches, a wave per chunk, the table product
    Wide,          // k_eval_wide
    MfmaRowsTeam,  // k_mfma_rows_team: a workgroup per tile, one table row per point, a launch per party
    MfmaRows,      // k_mfma_rows: one table row per point, a launch per party
    Bfly,          // k_mfma_bfly: the points in pairs, a launch per party
    BflyParties,   // k_mfma_bfly<.., LISTS>, every row party-major: ONE launch over all parties' chunks
    BflyLists,     // k_mfma_bfly<.., LISTS> with list rows: the producers' mixing step writes its lists itself
    BflyTriple,    // k_mfma_bfly<.., TRIPLE>: the local products inside the encode
    MfmaRowsGl,    // k_mfma_rows_gl (Goldilocks), a launch per party
    Fft1,          // k_eval_fft1: single-pass FFT, domains of up to 16 points (Fr below 16, Fr 16, Goldilocks)
    Fft1Mix,       // k_eval_fft1_mix: the mixing step from rows, lists and party-major rows written by the kernel
    Fft1Triple,    // k_eval_fft1_triple: the local products inside the single-pass FFT (Fr or Goldilocks)
    FftP,          // k_eval_fftP: multi-pass FFT (+ fold), domains of up to 256 points
    Transpose,     // rows: transpose into the workspace, then the chunk-major encode (a plan of its own)
    LocalProduct,  // triple: the local products into the workspace, then the chunk-major encode (a plan of its own)
    Generic,       // k_eval_generic
};
struct EncodeRoute {
    EncodeKernel kernel;
    mf::MfPlan plan;  // the matrix-core routes: the table rows every workgroup keeps (mf_plan_roles / mf_plan_pairs)
};
struct EncodePlan {
    EncodeRoute route[8];
    int count = 0;
    void add(EncodeKernel k, const mf::MfPlan& p = mf::MfPlan{}) { route[count++] = EncodeRoute{k, p}; }
};

// x[P][G][M] -> y[P][n][G] as ONE launch of the point-pair kernel over the P G chunks (k_mfma_bfly<.., LISTS> with every row party-major,
// tu_mfma_bfly.inc: launch_lists): domains of 8 and 16 points, M <= 11, dense output rows, enough tiles over all parties to fill the chip
inline bool encode_parties_one_launch(const EncodeKnobs& k, const EncodeShape& s) {
    const size_t size = domain_size(s.n), dp1 = s.d + 1, nwg = (size_t)(k.mfma_wgs ? k.mfma_wgs : k.n_cus);
    return s.kind == EncodeKind::ChunkMajor && s.parties > 1 && s.ys == 0 && k.impl == IMPL_U29 && k.matrix_cores && k.mfma_bfly &&
           !k.force_generic && size >= 8 && size <= 16 && s.n > size / 2 && dp1 >= 2 && dp1 <= 11 && (s.parties * s.G + 31) / 32 > nwg * 2 &&
           s.parties * s.n * s.G * 32 < ((size_t)1 << 32) && s.parties * s.G * dp1 * 32 < ((size_t)1 << 32);
}

// the matrix-core candidates of a U29 encode, in the order they are tried: the points in pairs (one launch over all parties, then
// a launch per party), then one table row per point (the workgroup-per-tile kernel for batches with up to two tiles per workgroup)
inline void plan_mfma(const EncodeKnobs& k, const EncodeShape& s, EncodePlan* out) {
    const size_t n = s.n, dp1 = s.d + 1, tiles = (s.G + 31) / 32;
    const bool rows = s.kind == EncodeKind::Rows;
    const int nwg = k.mfma_wgs ? k.mfma_wgs : k.n_cus;
    const size_t rowb = mf_row_bytes(dp1);
    const bool parties_one = encode_parties_one_launch(k, s);
    // (measured, 4 096 .. 16 384 chunks: n = 20, d = 6: 6.7 .. 10.0 us against 19 .. 20; n = 31, d = 10 -- three roles --
    // 9.8 and 15.1 us against 17.6 and 18.2 at 4 096 and 8 192 chunks, behind at 16 384)
    bool team = k.mfma_team && !rows && dp1 <= MF_MAX_M && tiles <= (size_t)nwg * 2 && !parties_one;
    mf::MfPlan plain{};
    bool plain_ok = !rows && dp1 <= MF_MAX_M && mf::mf_plan_roles((int)n, 0, (int)((160 * 1024 - (team ? 128 : 0)) / rowb), nwg, &plain);
    if (plain_ok && team && plain.nroles > 1 && tiles > (size_t)nwg) {
        team = false;
        plain_ok = mf::mf_plan_roles((int)n, 0, (int)((160 * 1024) / rowb), nwg, &plain);
    }
    if (!plain_ok) team = false;  // the point pairs below may still fit (half the rows)
    // Large batches take the points in pairs (k, k + size / 2): alpha_{k + size/2} = -alpha_k, so both outputs come from
    // the same M MFMAs (kernels_mfma_bfly.hpp) -- config 2: 0.16 ms against 0.18, config 3's encode 0.32 against 0.50
    // (profiles/r03_mfma_bfly_ubench.txt).  The workgroup-per-tile kernel keeps the plain rows.
    const size_t half = domain_size(n) / 2;
    mf::MfPlan pairs = plain;
    if (!team && k.mfma_bfly && half >= 2 && n > half && mf::mf_plan_pairs((int)half, (int)((160 * 1024) / mf_bfly_row_bytes(dp1)), nwg, &pairs)) {
        // tu_mfma_bfly.inc: launch_lists takes one role of 4 or 8 pairs (list rows: 4 pairs up to M = 8, 8 from M = 5 on)
        const bool one4or8 = pairs.nroles == 1 && (pairs.role[0].nrows == 4 || pairs.role[0].nrows == 8);
        if (s.lists) {
            if (pairs.nroles == 1 && dp1 >= 5 && pairs.role[0].nrows == (dp1 <= 8 ? 4 : 8)) out->add(EncodeKernel::BflyLists, pairs);
            return;
        }
        // the dealers' encodes of the producers: all parties in one launch
        if (parties_one && one4or8) out->add(EncodeKernel::BflyParties, pairs);
        out->add(EncodeKernel::Bfly, pairs);
    }
    if (plain_ok && !s.lists) out->add(team ? EncodeKernel::MfmaRowsTeam : EncodeKernel::MfmaRows, plain);
}

inline EncodePlan plan_chunk_major(const EncodeKnobs& k, const EncodeShape& s) {
    EncodePlan p;
    const size_t n = s.n, G = s.G, size = domain_size(n), dp1 = s.d + 1, P = s.parties;
    const size_t nwg = (size_t)(k.mfma_wgs ? k.mfma_wgs : k.n_cus), tiles = (G + 31) / 32;
    const bool u29 = k.impl == IMPL_U29, gold = k.impl == IMPL_GOLD, fg = k.force_generic;
    if (G * P <= k.wide_max_chunks / 4 && !fg) {  // small batch: wave per chunk
        // as a table product, the lanes sharing a point's terms (k_eval_wide_dot)
        p.add(u29 && n * dp1 * 36 <= 48 * 1024 ? EncodeKernel::WideDot : EncodeKernel::Wide);
        return p;
    }
    // mid-size batches on small domains as well: up to two tiles per workgroup the workgroup-per-tile matrix-core kernel
    // beats the single-pass FFT on latency -- n = 16, d = 5: 5.8 us against 12.3 us at 2 100 .. 4 096 chunks, 8.4 against
    // 13.3 at 16 384 (profiles/r02_team_kernel_encode.txt); at 2^20 the two tie
    const bool team_gate = u29 && size <= 16 && k.matrix_cores && k.mfma_team && !fg && P == 1 && dp1 >= 2 && dp1 <= MF_MAX_M &&
                           G >= k.mfma_min_encode && tiles <= nwg * 2;
    // large batches on small domains: with the points taken in pairs the matrix-core encode is ahead of the single-pass FFT
    const bool bfly_gate = u29 && size <= 16 && size >= 8 && k.matrix_cores && k.mfma_bfly && !fg && P <= 64 && dp1 >= 2 &&
                           dp1 <= MF_BFLY_MAX_M && tiles > nwg * 2 && G * dp1 * 32 < ((size_t)1 << 32);
    // several parties' mid-size batches: one launch over all of them (the dealers' encodes of the producers)
    if (team_gate || bfly_gate || encode_parties_one_launch(k, s)) plan_mfma(k, s, &p);
    if ((u29 || gold) && size <= 16 && !fg) {
        p.add(EncodeKernel::Fft1);  // when its launcher declines: straight to the generic kernel
    } else {
        // domains beyond 16 points: the dense n x (d + 1) map on the matrix cores beats the multi-pass FFT (config 3's
        // encode: 0.45 ms against 0.62 ms); up to 16 points the single-pass FFT stays (config 2: a tie at 0.187 ms)
        if (u29 && k.matrix_cores && !fg && P <= 64 && dp1 >= 2 && dp1 <= (k.mfma_bfly ? MF_BFLY_MAX_M : MF_MAX_M) && G >= k.mfma_min_encode &&
            G * dp1 * 32 < ((size_t)1 << 32) && n <= 255)
            plan_mfma(k, s, &p);
        else if (gold && k.matrix_cores && !fg && P <= 64 && dp1 >= 2 && dp1 <= MFGL_MAX_M && G >= k.mfma_min_gold && n <= 255 &&
                 mfgl_table_bytes(n, dp1) + 2048 <= 160 * 1024)  // all n rows in every workgroup's LDS
            p.add(EncodeKernel::MfmaRowsGl);
        if ((u29 || gold) && size <= 256 && dp1 <= 32 && !fg) p.add(EncodeKernel::FftP);
    }
    p.add(EncodeKernel::Generic);
    return p;
}

// x given as d + 1 rows: the point-pair matrix-core kernel reads them in place; every other shape goes through the workspace
// (transpose, then the chunk-major encode)
inline EncodePlan plan_rows(const EncodeKnobs& k, const EncodeShape& s) {
    EncodePlan p;
    const size_t n = s.n, G = s.G, size = domain_size(n), dp1 = s.d + 1;
    const bool mf_shape = k.impl == IMPL_U29 && k.matrix_cores && k.mfma_bfly && !k.force_generic && dp1 >= 2 && dp1 <= MF_BFLY_MAX_M && size >= 8 &&
                          n <= 255 && (G + 31) / 32 > (size_t)(k.mfma_wgs ? k.mfma_wgs : k.n_cus) * 2 && G * 32 < ((size_t)1 << 32);
    // the list rows straight from the kernel that computes them (k_mfma_bfly<.., LISTS>): one role, G < 2^32 chunks
    if (s.lists && mf_shape && k.list_rows_in_kernel) plan_mfma(k, s, &p);
    // Goldilocks, n inputs as rows, a domain of 4 .. 16 points: the single-pass lane kernel reads the rows in place and writes the lists and the
    // party-major rows itself (k_eval_fft1_mix) -- one launch instead of a transpose either side of the encode
    // (over Fr the same kernel on domains of 4 and 8 points -- 3 .. 8 parties -- where the matrix-core list kernel above did not take the call)
    const bool mix_gl = k.impl == IMPL_GOLD && size <= 16, mix_fr = k.impl == IMPL_U29 && size <= 8;
    if (s.lists && (mix_gl || mix_fr) && k.list_rows_in_kernel && !k.force_generic && dp1 == n && n >= 3) p.add(EncodeKernel::Fft1Mix);
    // all rows to y from the rows in place, the lists copied out afterwards
    if (mf_shape) {
        EncodeShape plain = s;
        plain.lists = false;
        plan_mfma(k, plain, &p);
    }
    p.add(EncodeKernel::Transpose);
    return p;
}

inline EncodePlan plan_triple(const EncodeKnobs& k, const EncodeShape& s) {
    EncodePlan p;
    const size_t n = s.n, G = s.G, size = domain_size(n), dp1 = s.d + 1, P = s.parties;
    // small batches with a workspace: the product kernel + the wave-per-chunk evaluation are two short launches, the fused
    // kernel one long one (a lane walks ~12 k instructions for its chunk): 1100 triples x 16 parties, the whole triple
    // generation 0.043 ms against 0.057 ms
    const bool small_two = s.workspace && G * P <= k.wide_max_chunks / 4;
    // Large batches on 9 .. 32 points: the products are computed inside the matrix-core encode with the points in pairs
    // (k_mfma_bfly<.., TRIPLE>, kernels_mfma_bfly.hpp) -- config 4's 16 parties x 381 300 chunks: 2.22 - 2.28 ms against
    // 2.53 - 2.55 of the fused FFT kernel on the same box (profiles/r03_mfma_bfly_triple.txt).  From 2^14 chunks over all parties: at the
    // reference node's batch of 4 096 chunks x 16 parties the whole TripleGen step takes 0.073 ms against 0.093 with the lane kernel, a tie
    // at 2^14 (profiles/r04_protocol_batch_sizes.txt)
    if (k.impl == IMPL_U29 && k.matrix_cores && k.mfma_bfly && !k.force_generic && dp1 >= 2 && dp1 <= MF_MAX_M && size >= 16 && size <= 32 &&
        n > size / 2 && G * P >= ((size_t)1 << 14) && G * dp1 * 32 < ((size_t)1 << 32) && P <= 65535) {
        const size_t half = size / 2;
        mf::MfPlan pairs{};
        if (half * mf_bfly_row_bytes(dp1) <= 160 * 1024 && mf::mf_plan_pairs((int)half, (int)half, k.mfma_wgs ? k.mfma_wgs : k.n_cus, &pairs))
            p.add(EncodeKernel::BflyTriple, pairs);
    }
    if (!small_two && k.impl == IMPL_U29 && size <= 16 && !k.force_generic) p.add(EncodeKernel::Fft1Triple);
    if (k.impl == IMPL_GOLD && size <= 16 && !k.force_generic) p.add(EncodeKernel::Fft1Triple);
    p.add(EncodeKernel::LocalProduct);
    return p;
}

inline EncodePlan plan_encode(const EncodeKnobs& k, const EncodeShape& s) {
    switch (s.kind) {
    case EncodeKind::Rows: return plan_rows(k, s);
    case EncodeKind::Triple: return plan_triple(k, s);
    default: return plan_chunk_major(k, s);
    }
}

// does the producers' mixing step (d = n - 1, rows with lists) write its lists from the kernel that computes them?
inline bool encode_lists_in_kernel(const EncodeKnobs& k, size_t G, size_t n, size_t d) {
    EncodeShape s{EncodeKind::Rows, G, n, d};
    s.lists = true;
    const EncodeKernel first = plan_rows(k, s).route[0].kernel;
    return first == EncodeKernel::BflyLists || first == EncodeKernel::Fft1Mix;
}

}  // namespace hbmpc
