// protocol_route.hpp -- which form a "whole protocol step for all parties" call takes: ONE place for the rule (plain C++, no HIP).
//
// hbmpc_[gl_]dev_triplegen_parties, hbmpc_dev_fpmul_parties, hbmpc_dev_truncpr_parties, hbmpc_[gl_]dev_mul_parties,
// hbmpc_[gl_]dev_randbit_parties and hbmpc_[gl_]dev_input_parties each ask plan_protocol once; either form writes the same bytes
// to every output buffer.  hbmpc_[gl_]dev_batchrecon_parties asks plan_batchrecon, below, the same way,
// hbmpc_[gl_]dev_ransha_parties and hbmpc_[gl_]dev_randousha_parties plan_producers.
// Two declines stay with the executor because they depend on a launcher or on the decode, not on the call's shape:
//   - the launchers' dry run (launch_*_wave(.., true): the LDS size and the LDS attribute): the call then runs its separate launches;
//   - the HBMPC_NOT_FUSED answer of batch_recover_dev to the pair form: the open then writes the shares and decodes them.
#pragma once
#include <stddef.h>

#include "field_dispatch.hpp"

namespace hbmpc {

// the hbmpc_ctx fields the rule reads
struct ProtocolKnobs {
    int impl;
    bool force_generic, direct_fail;
    size_t fused_triplegen_max, fused_fpmul_max, fused_truncpr_max, fused_mul_max, fused_randbit_max;  // chunks, 3 x elements, chunks
    size_t pair_decode_min;
    size_t fused_input_max = 0;  // elements; last, with a default: callers that list the fields above stay as they are
};
enum class ProtocolCall { TripleGen, FpMul, TruncPr, Mul, RandBit, Input };
// the call: N elements per party, n parties, t faults, S senders (FPMul, TruncPr, Mul, Input), m truncated bits (FPMul)
struct ProtocolShape {
    ProtocolCall call;
    size_t N, n, t, S, m;
};
struct ProtocolPlan {
    bool one_launch;  // a wave per element (FPMul, TruncPr, Mul, Input) or a workgroup per chunk (TripleGen, RandBit) instead of the separate launches
    // the wave kernels: 1 << lk adjacent lanes (a DPP quad at most) share the products of a table row
    int lk_row;       // FPMul's lk1, Mul's lk: while the t + 2 rows fit half a wave
    int lk_wave;      // FPMul's lk3, TruncPr's and Input's lk: while the t + 1 rows fit the wave
    bool pair_first;  // FPMul, Mul: the separate launches offer the open of a - x and b - y to the decode's pair form first
};

inline int lane_share(size_t rows, size_t lanes, size_t t) {
    int lk = 0;
    while (lk < 2 && (rows << (lk + 1)) <= lanes && ((size_t)2 << lk) <= t + 1) ++lk;
    return lk;
}

inline ProtocolPlan plan_protocol(const ProtocolKnobs& k, const ProtocolShape& s) {
    const bool gold = k.impl == IMPL_GOLD, fpmul = s.call == ProtocolCall::FpMul, mul = s.call == ProtocolCall::Mul;
    // one launch has no OEC round and writes a failed chunk itself, as the one-launch decodes do (recover_route.hpp)
    const bool any = !k.force_generic && k.direct_fail;
    // the wave-per-element kernels: Fr in 29-bit limbs, exactly 2t + 1 senders, a decode's rows fit the wave
    const bool wave = any && k.impl == IMPL_U29 && s.S == 2 * s.t + 1 && s.n <= 64 && s.t <= 30;
    bool one = false;
    switch (s.call) {
    case ProtocolCall::TripleGen:
        // a chunk is 2t + 1 triples.  n = 3t + 1 <= 16: every recipient decodes from exactly d + t + 1 senders, and the (party, recipient)
        // pairs fit the workgroup.  Over Goldilocks the four launches are flat at ~28 us and overtake at ~600 chunks: half the threshold
        one = any && k.impl != IMPL_SAT32 && s.N / (2 * s.t + 1) <= k.fused_triplegen_max / (gold ? 2 : 1) && s.n == 3 * s.t + 1 && s.n <= 16;
        break;
    case ProtocolCall::FpMul: one = wave && s.N <= k.fused_fpmul_max && (4 + s.m) * s.n <= 4096; break;  // 4 + m operands per party in LDS
    case ProtocolCall::TruncPr: one = wave && s.N <= k.fused_truncpr_max; break;
    case ProtocolCall::Mul: one = wave && s.N <= k.fused_mul_max; break;
    case ProtocolCall::RandBit:
        // a chunk is t + 1 elements; both opens decode from exactly 2t + 1 senders, and the pairs of one open fit the workgroup
        one = any && k.impl != IMPL_SAT32 && s.N / (s.t + 1) <= k.fused_randbit_max && s.n <= 16 && s.t >= 1;
        break;
    case ProtocolCall::Input: one = wave && s.N <= k.fused_input_max; break;
    }
    // the pair form: ahead from ~8 000 elements (tools/sweep_fused_fpmul.py); Goldilocks has none
    return ProtocolPlan{one, lane_share(s.t + 2, 32, s.t), lane_share(s.t + 1, 64, s.t), (fpmul || mul) && !gold && s.N >= k.pair_decode_min};
}

// ---- hbmpc_[gl_]dev_batchrecon_parties --------------------------------------------------------------------------------------------
// BatchRecon has a degree and two sender sets, which ProtocolShape has no place for, and its threshold is a context's own: a shape, a
// plan and a function of its own, so that ProtocolKnobs, ProtocolCall and every answer of plan_protocol stay as they are.
// the call: N elements per party in chunks of d + 1, n parties, t faults, S1 EvalBatch senders, S2 RevealBatch senders
struct BatchReconShape {
    size_t N, n, t, d, S1, S2;
};
struct BatchReconPlan {
    bool one_launch;  // a workgroup per chunk (kernels_batchrecon_wg.hpp) instead of the three launches
    int lk_eval;      // the EvalBatch arm: 1 << lk_eval adjacent lanes share the products of a (recipient, row)
};
// fused_batchrecon_max: hbmpc_set_fused_batchrecon, in chunks (0: never one launch)
inline BatchReconPlan plan_batchrecon(const ProtocolKnobs& k, size_t fused_batchrecon_max, const BatchReconShape& s) {
    // one launch has no OEC round and writes a failed chunk itself, so both arms decode from exactly d + t + 1 senders (a failed chunk is
    // final: what the separate decodes then do in one launch each); the (party, recipient) pairs fit the workgroup
    const bool one = !k.force_generic && k.direct_fail && (k.impl == IMPL_U29 || k.impl == IMPL_GOLD) && s.n <= 16 && s.S1 == s.d + s.t + 1 &&
                     s.S2 == s.S1 && s.N / (s.d + 1) <= fused_batchrecon_max;
    // lane pairs over U29 while the n (t + 1) rows fit half the workgroup (n = 16, t = 5: 192 lanes); n (t + 1) <= 256 for every covered shape
    return BatchReconPlan{one, k.impl == IMPL_U29 && 2 * s.n * (s.t + 1) <= 256 ? 1 : 0};
}

// ---- hbmpc_[gl_]dev_ransha_parties, hbmpc_[gl_]dev_randousha_parties ---------------------------------------------------------------
// The producers have K columns per dealer instead of N elements, RanSha a verifier sender count, and their threshold is a context's own:
// a shape, a plan and a function of their own, as for BatchRecon.
enum class ProducerCall { RanSha, RanDouSha };
// the call: K columns per dealer, n parties, t faults, S verify senders (RanSha; RanDouSha's verifiers read all n)
struct ProducersShape {
    ProducerCall call;
    size_t K, n, t, S;
};
struct ProducersPlan {
    bool one_launch;  // a workgroup per column (kernels_producers_wg.hpp) instead of the separate launches
};
// the LDS of a workgroup of the one-launch form (ProducersWgLds, kernels_producers_wg.hpp: elements 12 words apart and constants of 9
// over U29, 2 and 2 over Goldilocks): per sharing the dealt and the mixed block and the verifiers' table, the Vandermonde table, the kept
// coefficients and flags
inline size_t producers_lds_bytes(bool gold, const ProducersShape& s) {
    const size_t ls = gold ? 2 : 12, nl = gold ? 2 : 9, n = s.n, t = s.t;
    const bool dou = s.call == ProducerCall::RanDouSha;
    const size_t nver = dou ? n - t - 1 : 2 * t;
    // the tables' constants: RanSha (2t + 1)(t + 1); RanDouSha over Fr n (t + 1) + n (2t + 1), over Goldilocks n n for each sharing
    const size_t tabs = !dou ? (2 * t + 1) * (t + 1) : gold ? 2 * n * n : n * (3 * t + 2);
    const size_t words = (dou ? 4 : 2) * n * n * ls + n * n * nl + tabs * nl + 4 * nver * ls + 64;
    return (words + 16) * 4;  // every block starts on a multiple of 4 words
}
// fused_producers_max: hbmpc_set_fused_producers, in columns (0: never one launch)
inline ProducersPlan plan_producers(const ProtocolKnobs& k, size_t fused_producers_max, const ProducersShape& s) {
    // one launch has no OEC round and writes a failed column itself: RanSha's verifiers decode from exactly 2t + 1 senders, and below
    // n = 3t + 1 recover_secret refuses every column, which the separate launches report.  t = 0 has no verifier's table to speak of (RanSha has
    // no verifier at all) and stays with the separate launches.  The (row, party) pairs fit the workgroup: n <= 16.
    const bool field = k.impl == IMPL_U29 || k.impl == IMPL_GOLD;
    const bool shape = s.n <= 16 && s.t >= 1 && s.n > 2 * s.t && (s.call == ProducerCall::RanDouSha || (s.S == 2 * s.t + 1 && s.n >= 3 * s.t + 1));
    const bool one = !k.force_generic && k.direct_fail && field && shape && producers_lds_bytes(k.impl == IMPL_GOLD, s) <= 160 * 1024 &&
                     s.K <= fused_producers_max;
    return ProducersPlan{one};
}

}  // namespace hbmpc
