// recover_route.hpp -- which kernels a batch decode takes: ONE place for the rule (plain C++, no HIP).
//
// batch_recover_dev (capi_recover.inc) asks three things of it, in this order:
//   recover_cover        is the call's form covered: run, HBMPC_NOT_FUSED, or the single-coefficient form's InvalidInput.  The
//                        grouped form is answered before the senders are validated, the others after.
//   plan_recover         the OEC rounds, the ordered candidates of the first kernel and the tail behind it.  The executor builds
//                        the tables the route needs, fills the kernel arguments and launches; the first candidate that runs does
//                        the call.  The last candidate of a general-form plan cannot decline; a plan of the pair or select-two form
//                        that runs out answers HBMPC_NOT_FUSED, with nothing but the counters' clear enqueued.
//   plan_interpolate     batch_interpolate_dev: the inverse DFT on point pairs, or the t = 0 decode.
// Two declines stay with the executor because they depend on the table cache or on a launcher, not on the call's shape:
//   - a matrix-core route while a graph is being captured whose table is not cached (nothing may be built then);
//   - a launcher that does not instantiate m (launch_recover, launch_gold_recover, launch_second_chance_m -- which falls back to
//     the generic second chance -- and the matrix-core launchers, which also decline when the LDS attribute cannot be set).
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
struct RecoverKnobs {
    int impl;
    bool force_generic, matrix_cores, mfma_team, mfma_bfly, direct_fail, second_chance, list_rows_in_kernel;
    int lazy_fallback_tables;
    size_t wide_max_chunks, mfma_min_cached, mfma_min_direct, mfma_min_gold_direct, mfma_min_gold_oec;
    int mfma_wgs, n_cus;
};
// the call: G chunks from S senders, degree d, t faults
struct RecoverShape {
    size_t G, n, d, t, S;
    bool p0 = false;          // one output per chunk: P(0), or coefficient only_coeff
    int only_coeff = 0;       // > 0: the P(0)-shaped call keeps coefficient k instead (RanSha's exact-degree test)
    int second_coeff = -1;    // >= 0: the select-two form, coefficients only_coeff and second_coeff of every chunk
    size_t group = 0;         // > 0: the chunks are groups of `group`, each at its own offset in the sender rows
    bool slots = false;       // the caller's rows live at their senders' slots
    bool pair = false;        // the senders' values are differences formed after loading (hbmpc_dev_fpmul_parties)
    size_t pair_N = 0;
    bool host_call = false;   // a host-pointer entry point (it synchronises anyway)
};
// read by the executor before it plans
struct RecoverFacts {
    bool capturing = false;         // a graph capture is in progress on the calling thread
    bool fallback_cached = false;   // the OEC/Gao (and second-chance) tables of this sender set are cached
};
enum class RecoverCover { Run, NotFused, SingleCoeffInvalid };
enum class RecoverKernel {
    MfmaRowsSub,   // k_mfma_rows<.., SUB>: the pair form's differences formed after loading
    MfmaRowsGl,    // k_mfma_rows_gl (Goldilocks)
    MfmaRowsTeam,  // k_mfma_rows_team: a workgroup per tile
    MfmaRows,      // k_mfma_rows
    Wide,          // k_batch_recover_wide: a wave per chunk
    RecoverM,      // k_batch_recover<U29, m>: register-resident, a lane per chunk
    GoldRecoverM,  // k_batch_recover<Gold, m>
    Generic,       // k_batch_recover_generic
};
enum class SecondKernel { None, M, Generic };  // the tail's second chance: k_second_chance_m<U29, m>, or k_second_chance
struct RecoverRoute {
    RecoverKernel kernel;
    bool one_launch;                // the whole call in this launch: no tail
    bool second_in_kernel = false;  // Wide: a flagged chunk tries the second-chance candidates in the same kernel
    int ow_sel = 0;                 // Wide: 2 in the select-two form (the table holds the two selected rows)
    bool team = false;              // MfmaRowsTeam
    mf::MfPlan plan{};              // the matrix-core routes with roles (MfmaRowsSub, MfmaRowsTeam, MfmaRows)
};
struct RecoverPlan {
    size_t rmax = 0;        // OEC rounds (known sets of d + t + 1 + r senders, r = 1 .. rmax)
    bool second = false;    // the second chance runs (in the first kernel or in the tail)
    bool lazy = false;      // the fallback tables are built after the first kernel, and only when it has flagged a chunk
    RecoverRoute route[4];
    int count = 0;
    // the tail behind a route that is not one launch
    SecondKernel second_kernel = SecondKernel::None;  // unless the route that ran did it in-kernel
    bool gao_inline = false;                          // k_gao un-scales its own results; otherwise k_unscale follows
    void add(const RecoverRoute& r) { route[count++] = r; }
};

inline bool mfma_recover_team(const RecoverKnobs& k, const RecoverShape& s) {
    // up to two tiles per workgroup: the workgroup-per-tile kernel (its LDS also holds 32 flag words).  Measured crossover
    // (tools/time_team.py, profiles/r02_team_kernel.txt): ahead at 8 000 and 16 384 chunks for every shape, behind at 32 768
    const int nwg = k.mfma_wgs ? k.mfma_wgs : k.n_cus;
    return !s.pair && k.mfma_team && (s.G + 31) / 32 <= (size_t)nwg * 2;
}

// Whether the form of the call is covered.  before_validation: the answer given before the senders are validated (the grouped
// form); otherwise the answer after them.
inline RecoverCover recover_cover(const RecoverKnobs& k, const RecoverShape& s, bool before_validation) {
    const size_t m = s.d + 1, needed = s.d + s.t + 1;
    // group > 0: only as ONE launch of the wave-per-chunk kernel without OEC rounds
    if (s.group && (s.G % s.group != 0 || s.S != needed || !k.direct_fail || s.G > k.wide_max_chunks || k.force_generic || s.slots || s.pair))
        return RecoverCover::NotFused;
    if (before_validation) return RecoverCover::Run;
    // second_coeff >= 0 (with p0 = false): the "do these S points lie on a polynomial of degree <= d" form -- t is S - d - 1 whatever n
    // is (no Byzantine bound: every point beyond the first d + 1 is a verify row).  Wave-per-chunk or matrix-core kernels only.
    if (s.second_coeff >= 0 &&
        !(!s.p0 && s.S == needed && s.S > s.d && k.direct_fail && k.impl == IMPL_U29 && !k.force_generic && (size_t)s.second_coeff <= s.d &&
          (size_t)s.only_coeff <= s.d && (s.G <= k.wide_max_chunks || k.matrix_cores)))
        return RecoverCover::NotFused;
    // only_coeff = k > 0: a P(0)-shaped call whose one output per chunk is coefficient k (RanSha's exact-degree test needs the top
    // coefficient alone, share_gen.rs:516-530).  Only for calls without OEC rounds (S == d + t + 1): the fallback kernels know P(0) only.
    if (s.only_coeff > 0 && s.second_coeff < 0 && !(s.p0 && s.S == needed && k.direct_fail && (size_t)s.only_coeff <= s.d))
        return RecoverCover::SingleCoeffInvalid;
    // pair: only a P(0) call without OEC rounds that is ONE launch of the matrix-core kernel can take the form
    if (s.pair && !(s.S == needed && k.direct_fail && k.impl == IMPL_U29 && !k.force_generic && k.matrix_cores && s.p0 && s.pair_N % 32 == 0 &&
                    mfma_sub_covers(m)))
        return RecoverCover::NotFused;
    return RecoverCover::Run;
}

// The matrix-core decode (kernels_mfma.hpp): verify rows and coefficient rows as int8 MFMA tiles.  False when the shape is outside
// what that path covers.
inline bool plan_mfma_recover(const RecoverKnobs& k, const RecoverShape& s, bool direct, RecoverRoute* out) {
    // second_coeff >= 0: TWO outputs per chunk, coefficients only_coeff and second_coeff (chunk-major [G][2]; p0 is false then)
    const size_t m = s.d + 1, needed = s.d + s.t + 1, nv = needed - m, ow = s.second_coeff >= 0 ? 2 : s.p0 ? 1 : m;
    if (k.impl != IMPL_U29 || !k.matrix_cores || k.force_generic) return false;
    if (m < 2 || m > MF_MAX_M) return false;
    const int nwg = k.mfma_wgs ? k.mfma_wgs : k.n_cus;
    const bool team = mfma_recover_team(k, s);
    const int cap = (int)((160 * 1024 - (team ? 128 : 0)) / mf_row_bytes(m));
    // lane offsets inside a row / inside the output are 32-bit
    if (s.G * 32 >= ((size_t)1 << 32) || s.G * ow * 32 >= ((size_t)1 << 32)) return false;
    mf::MfPlan p{};
    if (!mf::mf_plan_roles((int)(nv + ow), (int)nv, cap, nwg, &p)) return false;
    // the whole call in this launch (no OEC round): only when one role serves verify AND output rows -- with two, the
    // role that writes the coefficients does not know the verdict and the call keeps its k_gao launch
    const bool one_launch = direct && p.nroles == 1;
    if (s.pair && !one_launch) return false;
    // the single-launch threshold applies to single-launch calls only (a two-role decode of 2048 .. 4095 chunks
    // used to take this path below its measured crossover)
    const size_t min_cached = one_launch ? std::min(k.mfma_min_cached, k.mfma_min_direct) : k.mfma_min_cached;
    if (s.G < min_cached) return false;
    *out = RecoverRoute{s.pair ? RecoverKernel::MfmaRowsSub : team ? RecoverKernel::MfmaRowsTeam : RecoverKernel::MfmaRows, one_launch};
    out->team = team;
    out->plan = p;
    return true;
}

// The same over Goldilocks (kernels_mfma_gl.hpp): the table is a few KB and costs microseconds to build, every row of a call
// fits one workgroup's LDS, so there is neither a sighting rule nor a role plan.
inline bool plan_mfma_recover_gl(const RecoverKnobs& k, const RecoverShape& s, bool direct) {
    const size_t m = s.d + 1, needed = s.d + s.t + 1, nv = needed - m, ow = s.p0 ? 1 : m;
    if (k.impl != IMPL_GOLD || !k.matrix_cores || k.force_generic || s.only_coeff != 0 || s.group) return false;
    if (m < 2 || m > MFGL_MAX_M || s.G < (direct ? k.mfma_min_gold_direct : k.mfma_min_gold_oec)) return false;
    return mfgl_table_bytes(nv + ow, m) + 2048 <= 160 * 1024;
}

// the plan of a covered call (recover_cover answered Run)
inline RecoverPlan plan_recover(const RecoverKnobs& k, const RecoverShape& s, const RecoverFacts& f) {
    RecoverPlan p;
    const size_t m = s.d + 1, needed = s.d + s.t + 1;
    const bool fg = k.force_generic;
    // oec_decode rounds (robust_interpolate.rs:589-593); the second-chance tables (k_second_chance) only when at least one exists
    p.rmax = s.S > needed ? std::min(s.t, s.S - needed) : 0;
    p.second = p.rmax >= 1 && k.second_chance;
    // A NEW sender set with OEC rounds available: the Gao rounds' and the second-chance tables are host work (0.4 - 1.3 ms
    // for n = 31 .. 64) that only chunks which fail the verification ever read.  They are built when the first kernel of
    // the call has flagged a chunk -- one look at its counter, i.e. one stream synchronisation in a call that would
    // otherwise have spent that time building -- and not at all while the senders are honest.  By default only for the
    // host-pointer entry points (which synchronise anyway): a device-pointer call stays a pure enqueue, and a graph capture
    // finds every table its eager warm-up run left behind (hbmpc_set_lazy_fallback_tables(ctx, 2) extends it to them).
    p.lazy = (k.lazy_fallback_tables == 2 || (k.lazy_fallback_tables == 1 && s.host_call)) && !f.capturing && p.rmax > 0 && !f.fallback_cached;
    // S == d + t + 1 (what BatchRecon passes): no OEC round exists, a chunk that fails the verification fails for good,
    // and the first kernel writes that itself -- ONE launch per decode (kernels_recover.hpp, fail_chunk / finish_direct)
    const bool direct = p.rmax == 0 && !p.second && k.direct_fail;
    // grid-stride over the flagged list
    if (p.second) p.second_kernel = k.impl == IMPL_U29 && !fg ? SecondKernel::M : SecondKernel::Generic;
    // small batch: OEC/Gao un-scales its own results and is the last kernel of the call (no k_unscale launch).  The same
    // when the call has no OEC round at all (S == d + t + 1, what BatchRecon passes: it decodes as soon as that many
    // senders have arrived, batch_recon.rs:371-389): a flagged chunk can only fail, there is nothing to un-scale
    p.gao_inline = (s.G <= k.wide_max_chunks && !fg) || p.rmax == 0;

    RecoverRoute r{};
    if (s.pair) {  // direct by recover_cover: S == needed leaves no OEC round and no second-chance window
        if (plan_mfma_recover(k, s, direct, &r)) p.add(r);
        return p;
    }
    if (plan_mfma_recover_gl(k, s, direct)) p.add(RecoverRoute{RecoverKernel::MfmaRowsGl, direct});
    // The matrix cores overtake the wave-per-chunk kernels at ~4 000 chunks (a call costs ~15 us whatever the batch: the
    // workgroup-per-tile kernel and three launches on empty lists), the lane-per-chunk kernels from the start -- 15 us against
    // 18 us at 4 096 chunks of config 3 (tools/sweep_recover.py).  A call without OEC rounds is one launch there, flat at
    // 7 - 12 us from 512 to 16 384 chunks, while the wave-per-chunk kernel grows with the batch: ahead from ~2 000 chunks
    // (tools/time_team_vs_wide.py).
    const bool consider_mfma = s.G > k.wide_max_chunks || s.G >= k.mfma_min_cached || (direct && s.G >= k.mfma_min_direct);
    // chunks that fail the verification keep whatever the coefficient rows produced until the fallback kernels rewrite them
    // (accepted candidate, decoded polynomial, or zeros)
    if (!s.group && consider_mfma && plan_mfma_recover(k, s, direct, &r)) p.add(r);
    if (s.G <= k.wide_max_chunks && !fg) {
        // small batch: a wave per chunk; a chunk that fails the verification tries the second-chance candidates in the
        // same kernel (one launch less) when the windows fit a wave
        RecoverRoute w{RecoverKernel::Wide, direct};
        w.second_in_kernel = p.second && !p.lazy && needed + p.rmax - m <= 64 && m <= 64;
        w.ow_sel = s.second_coeff >= 0 ? 2 : 0;
        p.add(w);
        return p;
    }
    if (s.second_coeff >= 0) return p;  // no other kernel family writes two selected coefficients
    if (k.impl == IMPL_U29 && m <= 16 && !fg) p.add(RecoverRoute{RecoverKernel::RecoverM, direct});
    if (k.impl == IMPL_GOLD && m <= 16 && !fg) p.add(RecoverRoute{RecoverKernel::GoldRecoverM, direct});
    p.add(RecoverRoute{RecoverKernel::Generic, direct});
    return p;
}

// batch_interpolate_dev: the inverse DFT on point pairs (with the degrees in the kernel where it has an instance for them, n = 8, 16),
// else the t = 0 decode; either is followed by poly_degree / take_c0 unless the kernel wrote what was asked
enum class InterpKernel { IdftDegrees, Idft, Decode };
struct InterpPlan {
    InterpKernel route[3];
    int count = 0;
    bool c0_only = false;  // IdftDegrees: only coefficient 0 is stored (the call wants c0 and the degrees: nothing follows)
    mf::MfPlan pairs{};
};
inline InterpPlan plan_interpolate(const RecoverKnobs& k, size_t G, size_t n, size_t S, size_t row_stride, bool degrees, bool c0) {
    InterpPlan p;
    const int nwg = k.mfma_wgs ? k.mfma_wgs : k.n_cus;
    // All n parties of a full power-of-two domain (the RanDouSha verifier: n = 16 shares of each sharing): the interpolation
    // is the inverse DFT, c_i = (1/n) sum_k y_k omega^(-i k), whose rows i and i + n/2 differ by the sign of the odd columns
    // -- the point-pair matrix-core kernel with the inverse rows as its table (kernels_mfma_bfly.hpp), the shares read from
    // their sender rows in place, the coefficients written chunk-major.  0.16 ms per 699 050 columns against 0.60 of the
    // lane kernel (profiles/r03_producers.txt).
    if (k.impl == IMPL_U29 && k.matrix_cores && k.mfma_bfly && !k.force_generic && S == n && n == domain_size(n) && n >= 8 && n <= MF_BFLY_MAX_M &&
        (G + 31) / 32 > (size_t)nwg * 2 && G * n * 32 < ((size_t)1 << 32) && (row_stride == 0 || row_stride >= G) &&
        mf::mf_plan_pairs((int)(n / 2), (int)((160 * 1024) / mf_bfly_row_bytes(n)), nwg, &p.pairs)) {
        if (degrees) p.route[p.count++] = InterpKernel::IdftDegrees;
        p.c0_only = degrees && c0 && k.list_rows_in_kernel;
        p.route[p.count++] = InterpKernel::Idft;
    }
    // otherwise: interpolation through S points == batch_recover with degree S-1 and no redundancy (t = 0): the
    // verify set is empty and every chunk takes the S x S Lagrange mat-vec
    p.route[p.count++] = InterpKernel::Decode;
    return p;
}

}  // namespace hbmpc
