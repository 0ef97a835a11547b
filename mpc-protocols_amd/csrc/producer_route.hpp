// producer_route.hpp -- which form the preprocessing producers' device calls take (RanSha, RanDouSha of capi_pipelines.hip): ONE place
// for the rule (plain C++, no HIP, no library types).  The dealers' encodes: how many dealers go into one call.  The verifiers' checks:
// one call per verifier, or all verifiers in one -- with the geometry of those calls and the workspace the form needs, so that what a
// producer sizes and what it enqueues cannot disagree.  Every form writes the same bytes to the producer's outputs and the same verdict.
// Precondition (the producers refuse everything else before they ask): n > 2t, K >= 1.
#pragma once
#include <stddef.h>

namespace hbmpc {

// all verifiers' columns in ONE launch of the wave-per-chunk decode (groups): ahead of the other forms up to this many chunks -- at 6 144 and
// 8 192 (n = 7 at the node's 1 536 / 2 048 columns) the party-major form below takes 0.070 / 0.037 ms against 0.121 / 0.071
// (profiles/r04_protocol_batch_sizes.txt)
constexpr size_t kGroupedMax = 4096;
// above: a launch per dealer.  Measured (tools/time_dealers_together.py, n = 16, degree 5): 0.037 ms against 0.146 at 16 000 polynomials per
// dealer, 0.159 / 0.295 at 65 536, 0.613 / 0.787 at 262 144 -- a launch of one dealer's batch spends a visible part of its time filling and
// draining the chip until the batch has some 10^6 polynomials
constexpr size_t kDealersTogetherMax = ((size_t)1 << 20) - 1;

// compute_shares of every dealer's K polynomials of degree deg: coeffs [dealer][K][deg + 1] -> S [dealer][recipient][K] is the party-batched
// encode's layout (vandermonde_apply_parties).  Returns the dealers per call; 1 = a compute_shares call per dealer.  A launch per dealer is at
// the memory rate only from some 10^6 polynomials; below that as many dealers go into ONE launch over (dealer, polynomial) as its 32-bit
// offsets allow (4 GiB of outputs, of inputs), whatever kernel family the size takes: the wave-per-chunk kernels up to 2 048 chunks, the
// point-pair matrix-core kernel on domains of 8 / 16 points from 16 384, the lane kernels elsewhere.  At the node's batch sizes
// (K ~ 7 000 .. 15 000, n = 16) 16 launches of 10 us each were 45 % of the producers' time (profiles/r04_protocol_batch_sizes.txt); at small
// ones (n = 16, 367 polynomials per dealer) one launch takes 12.6 us against 23.7 for slices that stay within the wave-per-chunk kernels'
// range, at 1 024 polynomials 13.2 against 48.7.
inline size_t plan_deal(size_t eb, size_t n, size_t K, size_t deg) {
    if (K > kDealersTogetherMax) return 1;
    const size_t lim = ((size_t)1 << 32) - 1, outs = lim / (n * K * eb), ins = lim / (K * (deg + 1) * eb);
    const size_t per = n < outs ? (n < ins ? n : ins) : (outs < ins ? outs : ins);
    return per >= 2 ? per : 1;
}

enum class VerifyForm {
    None,         // no verifier (RanSha with t = 0)
    Grouped,      // one call over (verifier, column) chunks; verifier i's sender rows where the mixing call wrote them, y + i n K
    Together,     // one call; the mixing call wrote the verifiers' rows party-major (yv): a sender's shares for all verifiers are one row
    PerVerifier,  // a call per verifier on y + i n K, each reusing one verifier's workspace
};
// RanDouSha: how a verifier answers "both degrees right, same constant term"
enum class VerifyCheck {
    Selected,      // interpolate_degree_check_strided + check_double_share_sel: (constant term, top coefficient) without the full interpolation
    ConstantTerm,  // batch_interpolate_c0 + check_double_share_c0_columns: Goldilocks has no selective decode
};
struct VerifyPlan {
    VerifyForm form;
    VerifyCheck check;
    // the verifier calls, in elements
    bool party_major;                    // the source is yv, not y
    size_t calls;                        // call i reads its source block + src0 + i * call_stride
    size_t src0, call_stride;
    size_t row_stride;                   // between the senders' rows
    size_t columns;                      // the call's G
    size_t groups, group_stride;         // (not read by batch_interpolate_c0: its G covers the verifiers)
    size_t verdict_G, verdict_columns;   // RanDouSha's verdict call; columns = 0: one verifier's
    // the workspace that depends on the form
    size_t yv_el;                        // of each party-major block (0: none)
    size_t poly_el, status_b;            // RanSha: the decode's workspace (elements) and status (bytes)
    size_t vr, vc;                       // RanDouSha: verifiers whose results are kept side by side, and whose full interpolations are
};

// Mid-size batches (the reference's own: some thousands of columns per dealer): one verifier's decode is a launch of ~10 us that
// does not fill the chip, and there are 2t (RanSha) or 2 (n - t - 1) (RanDouSha) of them.  Where the mixing kernel can write the
// verifiers' rows party-major, all verifiers of a kind are ONE decode over (verifier, column) chunks (profiles/r04_protocol_batch_sizes.txt).
// Measured ahead of a call per verifier up to 250 000 columns (n = 16: RanSha 0.742 -> 0.616 ms at 80 000, RanDouSha 4.39 -> 3.92 at 250 000), level
// with it at 699 050 (config 4's producers); from 2^19 columns on -- and where the party-major block would pass 4 GiB -- a call each, without the
// extra rows.  Shapes no list kernel covers (lists_in_kernel = 0: more than 16 parties; 9 .. 16 over Fr at small batches) pay one more pass for
// the party-major rows (k_rows_party_major): from three verifiers on that is still fewer launches.
inline bool verifiers_together(size_t eb, size_t n, size_t K, size_t nver, bool lists_in_kernel) {
    return nver >= 2 && K < ((size_t)1 << 19) && n * nver * K * eb < ((size_t)1 << 32) && (lists_in_kernel || nver >= 3);
}

// the geometry all forms share: verifiers first .. first + nver - 1, verifier i's sender rows at y + i n K, K apart
inline VerifyPlan plan_verifiers(VerifyForm form, size_t n, size_t K, size_t first, size_t nver) {
    VerifyPlan p{};
    p.form = form;
    p.party_major = form == VerifyForm::Together;
    p.calls = form == VerifyForm::PerVerifier ? nver : form == VerifyForm::None ? 0 : 1;
    p.src0 = p.party_major ? 0 : first * n * K;
    p.call_stride = n * K;
    p.row_stride = p.party_major ? nver * K : K;
    p.columns = K;
    p.groups = form == VerifyForm::PerVerifier ? 1 : nver;
    p.group_stride = form == VerifyForm::PerVerifier ? 0 : p.party_major ? K : n * K;
    p.yv_el = p.party_major ? nver * n * K : 0;
    return p;
}

// RanSha: verifiers 0 .. 2t - 1 decode the K columns from the first verify_senders parties' shares and test the degree
// (recover_check_degree_strided).  The party-major form has no OEC round to offer: exactly 2t + 1 senders.
inline VerifyPlan plan_ransha(size_t eb, size_t n, size_t t, size_t K, size_t verify_senders, bool lists_in_kernel) {
    const size_t nver = 2 * t;
    const VerifyForm form = nver == 0                                                                          ? VerifyForm::None
                            : nver * K <= kGroupedMax                                                          ? VerifyForm::Grouped
                            : verify_senders == 2 * t + 1 && verifiers_together(eb, n, K, nver, lists_in_kernel) ? VerifyForm::Together
                                                                                                               : VerifyForm::PerVerifier;
    VerifyPlan p = plan_verifiers(form, n, K, 0, nver);
    const bool all = form != VerifyForm::PerVerifier;  // one call: workspace and status for every verifier's columns
    p.poly_el = K * (all && nver > t + 1 ? nver : t + 1);
    p.status_b = all ? nver * K + 1 : K;
    return p;
}

// RanDouSha: verifiers t + 1 .. n - 1 interpolate both sharings through all n shares.  Grouped over Fr only (the wave-per-chunk selective
// decode); over Goldilocks the together form is ONE full interpolation over all verifiers' columns, G = nver K.
inline VerifyPlan plan_randousha(size_t eb, size_t n, size_t t, size_t K, bool lists_in_kernel) {
    const size_t nver = n - t - 1;
    const bool gl = eb == 8;
    const VerifyForm form = nver * K <= kGroupedMax && !gl                      ? VerifyForm::Grouped
                            : verifiers_together(eb, n, K, nver, lists_in_kernel) ? VerifyForm::Together
                                                                                : VerifyForm::PerVerifier;
    VerifyPlan p = plan_verifiers(form, n, K, t + 1, nver);
    p.check = gl ? VerifyCheck::ConstantTerm : VerifyCheck::Selected;
    p.vr = form == VerifyForm::PerVerifier ? 1 : nver;
    p.vc = form == VerifyForm::Together && gl ? nver : 1;
    if (p.vc > 1) p.columns = nver * K;
    p.verdict_G = p.vr * K;
    p.verdict_columns = form == VerifyForm::PerVerifier ? 0 : K;
    return p;
}

}  // namespace hbmpc
