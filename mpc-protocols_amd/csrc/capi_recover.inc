// capi_recover.inc -- batch_recover_secret / recover_secret / gao_rs_decode entry points
// (included at the end of hbmpc_capi.hip).

namespace {

struct SortedSenders {
    std::vector<size_t> ids;  // ascending
    std::vector<int> rows;    // rows[s] = position of ids[s] in the caller's arrays
};

// validation order of robust_interpolate.rs:290-341
// honest_majority: the caller has checked n >= 2t + 1 itself (RandBit's opens, capi_randbit.inc: exactly 2t + 1 senders, no OEC round)
ShareErrorCode validate_senders(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, size_t G, size_t n, size_t d,
                                size_t t, SortedSenders* out, bool honest_majority = false) {
    if (n < (honest_majority ? 2 : 3) * t + 1) return fail(ctx, InvalidInput, "n must be >= 3t + 1 for Byzantine fault tolerance");
    if (S == 0) return fail(ctx, InvalidInput, "No evaluations provided");
    if (G == 0) return fail(ctx, InvalidInput, "Empty batch");
    std::vector<std::pair<size_t, int>> v(S);
    for (size_t i = 0; i < S; ++i) v[i] = {sender_ids[i], (int)i};
    std::stable_sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (size_t i = 0; i < S; ++i) {
        if (i > 0 && v[i].first == v[i - 1].first) return fail(ctx, InvalidInput, "Duplicate sender id");
        if (v[i].first >= n) return fail(ctx, InvalidInput, "Sender id out of range");
    }
    if (S < d + t + 1) return fail(ctx, InvalidInput, "Not enough evaluations");
    if (domain_size(n) > ((size_t)1 << 32)) return fail(ctx, NoSuitableDomain, "no radix-2 domain of that size");
    out->ids.resize(S);
    out->rows.resize(S);
    for (size_t i = 0; i < S; ++i) {
        out->ids[i] = v[i].first;
        out->rows[i] = v[i].second;
    }
    return ShareSuccess;
}

// pts: the ids are integer evaluation points (the Shamirshare scheme, capi_shamir.inc), not indices into the roots-of-unity domain:
// a different table for the same numbers, so a different key
std::string ids_key(const char* kind, const std::vector<size_t>& ids, size_t count, size_t n, size_t d, size_t t,
                    int impl, bool pts = false) {
    std::string k = pts ? "pt-" : "";
    k += kind;
    k += ":" + std::to_string(n) + ":" + std::to_string(d) + ":" + std::to_string(t) + ":";
    for (size_t i = 0; i < count; ++i) k += std::to_string(ids[i]) + ",";
    return k + "#" + std::to_string(impl);
}

// Tables of the OEC rounds for id-sorted senders (shared by every chunk of a batch).
// Layout of the returned buffer (u32 words):
//   [0 .. 4*n_rounds)            GaoRound records
//   then per round: g0 (required+1 elements), LB (required^2 elements)
//   then alpha_s (S elements), one_plain (NL), r2 (NL), inv_exp (8)
struct GaoLayout {
    int n_rounds = 0;
    size_t alpha_off = 0, one_off = 0, r2_off = 0, exp_off = 0;
};
// the per-n domain data every table of a sender set starts from (tables.hpp: DomainInv), cached in the context
template <class H>
std::shared_ptr<const DomainInv<H>> domain_inv(hbmpc_ctx* ctx, size_t n);
template <>
std::shared_ptr<const DomainInv<HFr>> domain_inv<HFr>(hbmpc_ctx* ctx, size_t n) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto& slot = ctx->dom_fr[n];
    if (!slot) slot = std::make_shared<DomainInv<HFr>>(n);
    return slot;
}
template <>
std::shared_ptr<const DomainInv<HGl>> domain_inv<HGl>(hbmpc_ctx* ctx, size_t n) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto& slot = ctx->dom_gl[n];
    if (!slot) slot = std::make_shared<DomainInv<HGl>>(n);
    return slot;
}

template <class H>
std::vector<uint32_t> build_gao_tables_t(const DomainInv<H>& D, const std::vector<std::vector<size_t>>& known_sets, const std::vector<int>& ks,
                                         const std::vector<size_t>& alpha_ids, int impl, GaoLayout* lay, bool alpha_points = false) {
    const int NL = impl_nl(impl);
    const std::vector<H>& el = D.el;
    H rdev = H::one();
    {
        H two = H::from_u64(2);
        const int bits = impl == IMPL_U29 ? 261 : impl == IMPL_SAT32 ? 256 : 0;  // Goldilocks: no Montgomery form
        for (int i = 0; i < bits; ++i) rdev = rdev * two;
    }
    // one round = g0 (the product of the known points' linear factors: the A of their Lagrange basis) and the basis,
    // required^2 constants.  The rounds are independent and each is O(required^2) products: with several of them they are
    // built on their own host threads (ten rounds for n = 31: 1 ms on one thread).
    auto one_round = [&](size_t r, std::vector<uint32_t>* g0w, std::vector<uint32_t>* lbw) {
        const std::vector<size_t>& ks_ids = known_sets[r];
        const size_t req = ks_ids.size();
        std::vector<H> g0;
        std::vector<std::vector<H>> basis;
        if (req > 0) basis = lagrange_basis_ids<H>(D, ks_ids.data(), req, &g0, nullptr);  // basis[j][k]
        else g0.assign(1, H::one());
        for (const H& c : g0) put_const(*g0w, c, impl);
        for (size_t k = 0; k < req; ++k)
            for (size_t j = 0; j < req; ++j) put_const(*lbw, basis[j][k] * rdev, impl);
    };
    const size_t R = known_sets.size();
    std::vector<std::vector<uint32_t>> g0w(R), lbw(R);
    if (R >= 3 && known_sets.back().size() >= 16) {
        std::vector<std::future<void>> jobs;
        for (size_t r = 1; r < R; ++r) jobs.push_back(std::async(std::launch::async, one_round, r, &g0w[r], &lbw[r]));
        one_round(0, &g0w[0], &lbw[0]);
        for (auto& j : jobs) j.get();
    } else {
        for (size_t r = 0; r < R; ++r) one_round(r, &g0w[r], &lbw[r]);
    }
    std::vector<uint32_t> out(R * 4, 0);
    lay->n_rounds = (int)R;
    for (size_t r = 0; r < R; ++r) {
        const size_t req = known_sets[r].size();
        out[r * 4 + 0] = (uint32_t)req;
        out[r * 4 + 1] = (uint32_t)((req + (size_t)ks[r]) / 2);
        out[r * 4 + 2] = (uint32_t)out.size();
        out.insert(out.end(), g0w[r].begin(), g0w[r].end());
        out[r * 4 + 3] = (uint32_t)out.size();
        out.insert(out.end(), lbw[r].begin(), lbw[r].end());
    }
    lay->alpha_off = out.size();
    for (size_t id : alpha_ids) put_const(out, alpha_points ? H::from_u64(id) : el[id], impl);  // integer points: F::from(id)
    lay->one_off = out.size();
    put_plain(out, H::one(), impl);
    while ((int)(out.size() - lay->one_off) < NL) out.push_back(0);
    lay->r2_off = out.size();
    put_const(out, rdev, impl);
    lay->exp_off = out.size();
    uint64_t e[4];
    H::inv_exponent(e);
    for (int i = 0; i < 4; ++i) {
        out.push_back((uint32_t)e[i]);
        out.push_back((uint32_t)(e[i] >> 32));
    }
    return out;
}

std::vector<uint32_t> build_gao_tables(hbmpc_ctx* ctx, const std::vector<std::vector<size_t>>& known_sets, const std::vector<int>& ks,
                                       const std::vector<size_t>& alpha_ids, size_t n, int impl, GaoLayout* lay) {
    return impl == IMPL_GOLD ? build_gao_tables_t<HGl>(*domain_inv<HGl>(ctx, n), known_sets, ks, alpha_ids, impl, lay)
                             : build_gao_tables_t<HFr>(*domain_inv<HFr>(ctx, n), known_sets, ks, alpha_ids, impl, lay);
}
// the hbmpc_ctx fields of the decode's rule (recover_route.hpp)
RecoverKnobs recover_knobs(const hbmpc_ctx* ctx) {
    return RecoverKnobs{ctx->impl, ctx->force_generic, ctx->matrix_cores, ctx->mfma_team, ctx->mfma_bfly, ctx->direct_fail, ctx->second_chance,
                        ctx->list_rows_in_kernel, ctx->lazy_fallback_tables, ctx->wide_max_chunks, ctx->mfma_min_cached, ctx->mfma_min_direct,
                        ctx->mfma_min_gold_direct, ctx->mfma_min_gold_oec, ctx->mfma_wgs, ctx->n_cus};
}
// ... and of the protocol calls' rule (protocol_route.hpp)
ProtocolKnobs protocol_knobs(const hbmpc_ctx* ctx) {
    return ProtocolKnobs{ctx->impl, ctx->force_generic, ctx->direct_fail, ctx->fused_triplegen_max, ctx->fused_fpmul_max, ctx->fused_truncpr_max,
                         ctx->fused_mul_max, ctx->fused_randbit_max, ctx->pair_decode_min, ctx->fused_input_max};
}

// One batch decode.  Its forms (group, second_coeff, only_coeff, pair) are those of RecoverShape (recover_route.hpp); a form that
// does not cover the call answers HBMPC_NOT_FUSED with nothing enqueued, and the caller runs the separate launches.
struct RecoverCall {
    const size_t* sender_ids = nullptr;
    size_t S = 0;
    const void* evals = nullptr;   // unused by the pair form: its values are the differences of `pair`
    size_t row_stride = 0;         // 0: G
    size_t G = 0, n = 0, d = 0, t = 0;
    void* out = nullptr;
    uint32_t* ncoeffs = nullptr;
    uint8_t* status = nullptr;
    hbmpc_recover_summary* summary = nullptr;
    bool p0 = false;
    void* stream = nullptr;
    const size_t* slots = nullptr;  // the caller's row i lives at evals + slots[i] * row_stride (rows in place at their senders' slots)
    bool host_call = false;
    const PairInput* pair = nullptr;
    int only_coeff = 0, second_coeff = -1;
    size_t group = 0, group_stride = 0;  // group q's values q * group_stride elements further on in every sender row (RecoverArgs::group)
    bool honest_majority = false;        // n >= 2t + 1 is enough (validate_senders)
    // the integer-point scheme (capi_shamir.inc): sender i sits at F::from(points[i]), not at a domain element.  The caller has made the
    // scheme's checks (distinct non-zero field elements); t == 0, S == d + 1 <= 255, n == S, sender_ids unused
    const uint64_t* points = nullptr;
};

// the decode's table of a sender set: the verify rows (vm), then the coefficient rows (bc)
template <class H>
ShareErrorCode rec_table(hbmpc_ctx* ctx, const DomainInv<H>& dom, const std::vector<size_t>& ids, size_t n, size_t d, size_t t, const uint32_t** out,
                         bool pts = false) {
    return get_table(ctx, ids_key("rec", ids, d + t + 1, n, d, t, ctx->impl, pts), [&] {
        if (pts) {  // no verify row: the S x S coefficient rows
            std::vector<uint32_t> bc;
            for (const auto& row : point_coeff_rows<H>(ids))
                for (const H& v : row) put_const(bc, v, ctx->impl);
            return bc;
        }
        const RecoverTables T = build_recover_tables<H>(dom, ids, d, t, ctx->impl);
        std::vector<uint32_t> both = T.vm;
        both.insert(both.end(), T.bc.begin(), T.bc.end());
        return both;
    }, out);
}

// The matrix-core routes of plan_recover (MfmaRowsSub, MfmaRowsTeam, MfmaRows): the sender set's table, the arguments, the launch.
// Returns false when the route does not run and nothing was enqueued (a capture would have to build the table, or the launcher
// declines); true when it ran or *rc_out holds an error.
bool run_mfma_recover(hbmpc_ctx* ctx, const RecoverRoute& r, const SortedSenders& ss, const RecoverArgs& ra, const RecoverCall& c, hipStream_t s,
                      ShareErrorCode* rc_out) {
    const size_t n = c.n, d = c.d, t = c.t, m = d + 1, needed = d + t + 1, nv = needed - m, ow = c.second_coeff >= 0 ? 2 : c.p0 ? 1 : m;
    const size_t rowb = mf_row_bytes(m);
    *rc_out = ShareSuccess;
    // The table of a sender set not seen before: its rows x m coefficients come from the host (tables.hpp: no field
    // inversion, ~0.05 ms for config 3), the 32 shifted digit copies of each -- 239 KB for config 3 -- are expanded on the
    // device (kernels_tables.hpp: two short launches on the context's stream).  Round 2 built all of it on the host
    // (0.4 - 0.6 ms + the upload) and therefore took this path for mid-size batches only when a sender set came back; now
    // every batch from the crossover on takes it.
    // only_coeff = k > 0 (a P(0)-shaped call that keeps coefficient k instead of coefficient 0): its own table, the verify rows
    // followed by coefficient row k
    const bool sel = c.only_coeff > 0 || c.second_coeff >= 0;
    const std::string tkey = ids_key(sel ? ("mfrec_k" + std::to_string(c.only_coeff) + "_" + std::to_string(c.second_coeff)).c_str() : "mfrec", ss.ids,
                                     needed, n, d, t, ctx->impl, c.points != nullptr);
    const auto dom = domain_inv<HFr>(ctx, n);  // before the table calls: their builders run under the context's lock, which this takes too
    auto table_rows = [&] {
        std::vector<std::vector<HFr>> rows_all = c.points ? point_coeff_rows<HFr>(ss.ids) : recover_coeff_rows<HFr>(*dom, ss.ids, d, t);
        if (sel) {
            std::vector<std::vector<HFr>> picked(rows_all.begin(), rows_all.begin() + nv);
            picked.push_back(rows_all[nv + c.only_coeff]);
            if (c.second_coeff >= 0) picked.push_back(rows_all[nv + c.second_coeff]);
            return picked;
        }
        return rows_all;
    };
    if (g_capturing && !table_cached(ctx, tkey)) return false;  // nothing may be built now: the kernels whose tables the eager run built
    const uint32_t* tab;
    if (ctx->device_tables) {
        const size_t rows = sel ? nv + ow : nv + m;  // the P(0)-only call uses the first nv + 1 rows of the same table
        *rc_out = get_table_expanded(ctx, tkey, rows * rowb / 4,
                                     [&] {
                                         std::vector<uint32_t> w = mf_coeff_words(table_rows(), m);
                                         w.resize(2 * w.size());  // second half: the per-(row, input) partial sums of the expansion
                                         return w;
                                     },
                                     [&](uint32_t* dev, uint32_t* seed, hipStream_t bs) {
                                         uint64_t e[4];
                                         mf_bias_e(m, e);
                                         launch_mfma_table((const uint64_t*)seed, (int)m, (int)rows, e, mf_bias_mag(m), (uint8_t*)dev,
                                                           (uint64_t*)seed + rows * m * 4, bs);
                                     }, &tab);
    } else {
        *rc_out = get_table(ctx, tkey, [&] { return build_mfma_table(table_rows(), m); }, &tab);
    }
    if (*rc_out != ShareSuccess) return true;
    mf::MfmaRowsArgs a;
    memset(&a, 0, sizeof a);
    mf::mf_take_plan(r.plan, &a);
    a.in = (const uint8_t*)ra.evals;
    a.G = ra.G;
    a.in_chunk_major = 0;
    a.row_stride = ra.row_stride;
    a.rows = ra.rows;
    a.table = (const uint8_t*)tab;  // rows [0, nv) verify, then the coefficient rows: P(0) only = the first nv + 1 rows
    a.nv = (int)nv;
    a.out = (uint8_t*)ra.out;
    a.out_party_major = 0;
    a.out_stride = ow;
    a.ncoeffs = ra.ncoeffs;
    a.status = ra.status;
    a.flagged = ra.flagged;
    a.counters = ra.counters;
    a.summary = ra.summary;
    a.direct = r.one_launch ? 1 : 0;
    const int mi = (int)m;
    if (c.pair) {
        const PairInput* pair = c.pair;
        a.in = (const uint8_t*)pair->a, a.sub_x = (const uint8_t*)pair->x, a.in2 = (const uint8_t*)pair->b, a.sub_x2 = (const uint8_t*)pair->y;
        a.sub_half = pair->N, a.row_stride = pair->N;
        return launch_mfma_rows_sub(mi, a, ctx->device, s);
    }
    return launch_mfma_rows(mi, a, ctx->device, s, r.team);
}

// the same over Goldilocks (MfmaRowsGl)
bool run_mfma_recover_gl(hbmpc_ctx* ctx, const RecoverRoute& r, const SortedSenders& ss, const RecoverArgs& ra, const RecoverCall& c, hipStream_t s,
                         ShareErrorCode* rc_out) {
    const size_t n = c.n, d = c.d, t = c.t, m = d + 1, needed = d + t + 1, nv = needed - m, ow = c.p0 ? 1 : m;
    const auto domain_inv_gl = domain_inv<HGl>(ctx, n);
    const uint32_t* tab;
    *rc_out = get_table(ctx, ids_key("mfrecgl", ss.ids, needed, n, d, t, ctx->impl, c.points != nullptr), [&] {
        return build_mfma_table_gl(c.points ? point_coeff_rows<HGl>(ss.ids) : recover_coeff_rows<HGl>(*domain_inv_gl, ss.ids, d, t), m);
    }, &tab);
    if (*rc_out != ShareSuccess) return true;
    mf::MfmaGlArgs a;
    memset(&a, 0, sizeof a);
    a.in = (const uint8_t*)ra.evals;
    a.G = ra.G;
    a.in_chunk_major = 0;
    a.row_stride = ra.row_stride;
    a.rows = ra.rows;
    a.table = (const uint8_t*)tab;  // rows [0, nv) verify, then the coefficient rows: P(0) only = the first nv + 1 rows
    a.m = (int)m, a.nrows = (int)(nv + ow), a.nv = (int)nv;
    a.out = (uint8_t*)ra.out;
    a.out_party_major = 0;
    a.out_stride = ow;
    a.ncoeffs = ra.ncoeffs;
    a.status = ra.status;
    a.flagged = ra.flagged;
    a.counters = ra.counters;
    a.summary = ra.summary;
    a.direct = r.one_launch ? 1 : 0;
    const size_t ntiles = (ra.G + 31) / 32;
    const unsigned grid = (unsigned)std::min<size_t>((ntiles + 3) / 4, (size_t)(ctx->mfma_wgs ? ctx->mfma_wgs : ctx->n_cus * 4));
    return launch_mfma_rows_gl(a, grid, ctx->device, s);
}

void launch_gao(int impl, const GaoArgs& ga, size_t n, unsigned grid, hipStream_t s, bool inline_unscale = false) {
    if (impl == IMPL_U29) launch_gao_u29(ga, n, grid, s, inline_unscale);
    else if (impl == IMPL_SAT32) launch_gao_sat(ga, n, grid, s, inline_unscale);
    else launch_gao_gold(ga, n, grid, s, inline_unscale);
}

// Which kernels a decode takes is decided in one place, recover_cover and plan_recover (recover_route.hpp); this validates, builds
// the tables the chosen route needs, fills the kernel arguments and walks the plan.
ShareErrorCode batch_recover_dev(hbmpc_ctx* ctx, RecoverCall c) {
    if (c.row_stride == 0) c.row_stride = c.G;
    const size_t S = c.S, G = c.G, n = c.n, d = c.d, t = c.t;
    if (ctx && c.row_stride < (c.group ? c.group : G)) return fail(ctx, InvalidInput, "row_stride must be >= G");
    if (!ctx) return InvalidInput;
    const bool pts = c.points != nullptr;
    if (S && !c.sender_ids && !pts) return fail(ctx, InvalidInput, "null sender_ids");
    const RecoverKnobs k = recover_knobs(ctx);
    RecoverShape sh{G, n, d, t, S};
    sh.p0 = c.p0, sh.only_coeff = c.only_coeff, sh.second_coeff = c.second_coeff, sh.group = c.group;
    sh.slots = c.slots != nullptr, sh.pair = c.pair != nullptr, sh.pair_N = c.pair ? c.pair->N : 0, sh.host_call = c.host_call;
    if (recover_cover(k, sh, true) != RecoverCover::Run) return HBMPC_NOT_FUSED;
    SortedSenders ss;
    ShareErrorCode rc = ShareSuccess;
    if (pts) {  // the points in the caller's order: row i is point i
        if (G == 0 || t != 0 || S != d + 1 || n != S) return fail(ctx, InvalidInput, "integer points: the plain interpolation only");
        ss.ids.assign(c.points, c.points + S);
        ss.rows.resize(S);
        for (size_t i = 0; i < S; ++i) ss.rows[i] = (int)i;
    } else {
        rc = validate_senders(ctx, c.sender_ids, S, G, n, d, c.second_coeff >= 0 ? 0 : t, &ss, c.honest_majority);
    }
    if (rc != ShareSuccess) return rc;
    if (n > 255) return fail(ctx, InvalidInput, "n > 255 (HoneyBadgerMPCNodeOpts limits n to 255)");
    if (c.slots)
        for (size_t i = 0; i < S; ++i)
            if (c.slots[i] > 255) return fail(ctx, InvalidInput, "row slot out of range (0..255)");
    if ((!c.evals && !c.pair) || !c.out) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, c.stream);
    switch (recover_cover(k, sh, false)) {
    case RecoverCover::NotFused: return HBMPC_NOT_FUSED;
    case RecoverCover::SingleCoeffInvalid: return fail(ctx, InvalidInput, "a single coefficient: P(0)-shaped calls with exactly d + t + 1 senders, k <= d");
    case RecoverCover::Run: break;
    }
    const int impl = ctx->impl;
    const size_t m = d + 1, needed = d + t + 1;

    // --- tables (cached per sender set) ---
    const std::shared_ptr<const DomainInv<HFr>> dom_fr = impl == IMPL_GOLD ? nullptr : domain_inv<HFr>(ctx, n);
    const std::shared_ptr<const DomainInv<HGl>> dom_gl = impl == IMPL_GOLD ? domain_inv<HGl>(ctx, n) : nullptr;
    const uint32_t* vm_bc;
    rc = impl == IMPL_GOLD ? rec_table(ctx, *dom_gl, ss.ids, n, d, t, &vm_bc, pts) : rec_table(ctx, *dom_fr, ss.ids, n, d, t, &vm_bc, pts);
    if (rc != ShareSuccess) return rc;
    const size_t vm_words = (needed - m) * m * impl_nl(impl);
    const uint32_t* sel2 = nullptr;  // second_coeff >= 0: [verify rows | row only_coeff | row second_coeff], contiguous
    if (c.second_coeff >= 0) {
        rc = get_table(ctx, ids_key(("rec_k" + std::to_string(c.only_coeff) + "_" + std::to_string(c.second_coeff)).c_str(), ss.ids, needed, n, d, t, impl), [&] {
            const RecoverTables T2 = build_recover_tables<HFr>(*dom_fr, ss.ids, d, t, impl);
            const size_t rw = m * impl_nl(impl);
            std::vector<uint32_t> w = T2.vm;
            w.insert(w.end(), T2.bc.begin() + c.only_coeff * rw, T2.bc.begin() + (c.only_coeff + 1) * rw);
            w.insert(w.end(), T2.bc.begin() + c.second_coeff * rw, T2.bc.begin() + (c.second_coeff + 1) * rw);
            return w;
        }, &sel2);
        if (rc != ShareSuccess) return rc;
    }
    const std::string gao_key = ids_key("gao", ss.ids, S, n, d, t, impl, pts), sc_key = ids_key("sc", ss.ids, S, n, d, t, impl, pts);
    RecoverFacts facts;
    facts.capturing = g_capturing > 0;
    // (only a call with OEC rounds has fallback tables: the others skip the look-ups)
    facts.fallback_cached = S > needed && table_cached(ctx, gao_key) && (!ctx->second_chance || table_cached(ctx, sc_key));
    const RecoverPlan plan = plan_recover(k, sh, facts);
    GaoLayout lay;
    std::vector<std::vector<size_t>> known_sets;
    std::vector<int> ks;
    for (size_t r = 1; r <= plan.rmax; ++r) {  // oec_decode rounds (:589-593)
        known_sets.emplace_back(ss.ids.begin(), ss.ids.begin() + needed + r);
        ks.push_back((int)m);
    }
    const uint32_t *gao_dev = nullptr, *sc_dev = nullptr;
    SecondTables sct;
    auto fetch_fallback_tables = [&]() -> ShareErrorCode {
        // table and layout are one cache entry, published under one lock (two threads may decode the same new sender
        // set at once: the second finds either nothing or both)
        std::array<size_t, 5> aux = {0, 0, 0, 0, 0};
        ShareErrorCode frc = get_table(ctx, gao_key, [&] {
            GaoLayout built;
            std::vector<uint32_t> host = impl == IMPL_GOLD ? build_gao_tables_t<HGl>(*dom_gl, known_sets, ks, ss.ids, impl, &built, pts)
                                                           : build_gao_tables_t<HFr>(*dom_fr, known_sets, ks, ss.ids, impl, &built, pts);
            aux = {(size_t)built.n_rounds, built.alpha_off, built.one_off, built.r2_off, built.exp_off};
            return host;
        }, &gao_dev, &aux);
        if (frc != ShareSuccess) return frc;
        lay.n_rounds = (int)aux[0];
        lay.alpha_off = aux[1];
        lay.one_off = aux[2];
        lay.r2_off = aux[3];
        lay.exp_off = aux[4];
        if (plan.second) {
            // the layout is a pure function of the shape: recompute it without the values when the table is cached
            frc = get_table(ctx, sc_key, [&] {
                sct = impl == IMPL_GOLD ? build_second_tables<HGl>(*dom_gl, ss.ids, d, needed + plan.rmax, impl)
                                        : build_second_tables<HFr>(*dom_fr, ss.ids, d, needed + plan.rmax, impl);
                return sct.words;
            }, &sc_dev);
            if (frc != ShareSuccess) return frc;
            sct.layout(m, needed + plan.rmax, (size_t)impl_nl(impl));
        }
        return ShareSuccess;
    };
    lay.n_rounds = (int)known_sets.size();
    if (!plan.lazy) {
        rc = fetch_fallback_tables();
        if (rc != ShareSuccess) return rc;
    }

    // --- scratch: [0, 64) counters + local summary | two flagged lists (G u32 each) | scales ---
    const size_t scale_words = (size_t)impl_nl(impl) + 1;  // per flagged chunk: pending flag + l^N
    return with_decode_counters(ctx, s, 2048 + 2 * G * 4 + G * scale_words * 4, [&](uint32_t* counters) -> ShareErrorCode {
        uint32_t* flagged_list = counters + 512;
        uint32_t* flagged_list2 = flagged_list + G;  // what the second-chance kernel leaves for OEC/Gao
        uint32_t* scales = flagged_list2 + G;
        uint32_t* summ = c.summary ? (uint32_t*)c.summary : counters + 4;
        // There is no init launch: the row permutation travels in the ARGUMENTS of every kernel, and the first kernel
        // initialises the summary.
        RowsArg rows_arg;
        memset(&rows_arg, 0, sizeof rows_arg);
        for (size_t i = 0; i < S; ++i) rows_arg.set(i, (unsigned)(c.pair ? ss.ids[i] : c.slots ? c.slots[ss.rows[i]] : ss.rows[i]));
        RecoverArgs ra;
        ra.evals = (const uint32_t*)c.evals;
        ra.G = G;
        ra.row_stride = c.row_stride;
        ra.rows = rows_arg;
        ra.needed = (int)needed;
        ra.m = (int)m;
        ra.vm = vm_bc;
        ra.bc = vm_bc + vm_words + (size_t)c.only_coeff * m * impl_nl(impl);  // the P(0)-only kernels read one coefficient row: row 0, or row k
        if (sel2) ra.vm = sel2, ra.bc = sel2 + vm_words;
        ra.out = (uint32_t*)c.out;
        ra.ncoeffs = c.ncoeffs;
        ra.status = c.status;
        ra.flagged = flagged_list;
        ra.counters = counters;
        ra.summary = summ;
        ra.group = c.group, ra.group_stride = c.group_stride;
        const unsigned grid = (unsigned)((G + 255) / 256);
        SecondArgs sa;
        if (plan.second) {
            sa.evals = (const uint32_t*)c.evals;
            sa.G = G;
            sa.row_stride = c.row_stride;
            sa.rows = rows_arg;
            sa.m = (int)m;
            sa.P = (int)(needed + plan.rmax);
            sa.rmax = (int)plan.rmax;
            sa.out_width = c.p0 ? 1 : (int)m;
            sa.flagged = flagged_list;
            sa.flagged2 = flagged_list2;
            sa.counters = counters;
            sa.out = (uint32_t*)c.out;
            sa.ncoeffs = c.ncoeffs;
            sa.status = c.status;
            sa.summary = summ;
        }
        auto second_tables_into_args = [&] {
            if (!plan.second) return;
            sa.n_windows = sct.n_windows;
            for (int w = 0; w < SECOND_MAX_WINDOWS; ++w) {
                sa.win_start[w] = sct.win_start[w];
                sa.ev[w] = sc_dev + sct.ev_off[w];
                sa.bc[w] = sc_dev + sct.bc_off[w];
            }
        };
        if (!plan.lazy) second_tables_into_args();

        // the first kernel: the candidates of plan_recover in order, the first that runs does the call
        const RecoverRoute* ran = nullptr;
        for (int i = 0; i < plan.count && !ran; ++i) {
            const RecoverRoute& r = plan.route[i];
            ra.direct = r.one_launch ? 1 : 0;
            bool hit = true;
            switch (r.kernel) {
            case RecoverKernel::MfmaRowsSub:
            case RecoverKernel::MfmaRowsTeam:
            case RecoverKernel::MfmaRows: hit = run_mfma_recover(ctx, r, ss, ra, c, s, &rc); break;
            case RecoverKernel::MfmaRowsGl: hit = run_mfma_recover_gl(ctx, r, ss, ra, c, s, &rc); break;
            case RecoverKernel::Wide: launch_recover_wide(impl, c.p0, ra, r.second_in_kernel ? &sa : nullptr, s, r.ow_sel); break;
            case RecoverKernel::RecoverM: hit = launch_recover((int)m, c.p0, ra, grid, s); break;
            case RecoverKernel::GoldRecoverM: hit = launch_gold_recover((int)m, c.p0, ra, grid, s); break;
            case RecoverKernel::Generic: launch_recover_generic(impl, c.p0, ra, grid, s); break;
            }
            if (rc != ShareSuccess) return rc;
            if (hit) ran = &r;
        }
        if (!ran) return HBMPC_NOT_FUSED;  // the pair and select-two forms: nothing was enqueued (the counters' clear is harmless)
        HIP_TRY(ctx, hipGetLastError());
        if (ran->one_launch) return ShareSuccess;  // the kernel's last block left the counters at zero

        // --- the tail ---
        if (plan.lazy) {
            uint32_t n_flagged = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&n_flagged, counters, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            // nothing for the fallback kernels to do: the summary is as the first kernel initialised it (no fallback, no
            // failure) and the counters never left zero -- exactly what their launches on empty lists would leave
            if (n_flagged == 0) return ShareSuccess;
            rc = fetch_fallback_tables();
            if (rc != ShareSuccess) return rc;
            second_tables_into_args();
        }
        if (plan.second && !ran->second_in_kernel) {
            // grid-stride over the flagged list
            if (!(plan.second_kernel == SecondKernel::M && launch_second_chance_m((int)m, sa, std::min(grid, 1024u), s)))
                launch_second_chance(impl, sa, std::min(grid, 1024u), s);
            HIP_TRY(ctx, hipGetLastError());
        }
        GaoArgs ga;
        ga.evals = (const uint32_t*)c.evals;
        ga.G = G;
        ga.row_stride = c.row_stride;
        ga.rows = rows_arg;
        ga.reset = counters;
        ga.alpha_s = gao_dev + lay.alpha_off;
        ga.rounds = (const GaoRound*)gao_dev;
        ga.n_rounds = lay.n_rounds;
        ga.tables = gao_dev;
        ga.k = (int)m;
        ga.accept_min = (int)needed;
        ga.out_width = c.p0 ? 1 : (int)m;
        ga.flagged = plan.second ? flagged_list2 : flagged_list;
        ga.counters = plan.second ? counters + 1 : counters;
        ga.out = (uint32_t*)c.out;
        ga.ncoeffs = c.ncoeffs;
        ga.status = c.status;
        ga.summary = summ;
        ga.one_plain = gao_dev + lay.one_off;
        ga.r2 = gao_dev + lay.r2_off;
        ga.inv_exp = gao_dev + lay.exp_off;
        ga.scales = scales;
        // blocks stride over the flagged list; more blocks than resident slots just exit (3 waves/SIMD of 64..256 lanes)
        const unsigned ggrid = (unsigned)std::min<size_t>(G, 2048);
        launch_gao(impl, ga, n, ggrid, s, plan.gao_inline);
        HIP_TRY(ctx, hipGetLastError());
        return ShareSuccess;  // the whole sequence is on the stream: its last kernel leaves the counters at zero
    });
}

ShareErrorCode batch_recover_host(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const void* evals, size_t G,
                                  size_t n, size_t d, size_t t, void* out, uint32_t* ncoeffs, uint8_t* status,
                                  bool p0) {
    if (!ctx) return InvalidInput;
    SortedSenders ss;
    ShareErrorCode rc = validate_senders(ctx, sender_ids, S, G, n, d, t, &ss);
    if (rc != ShareSuccess) return rc;
    if (!evals || !out) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ow = p0 ? 1 : d + 1, eb = ebytes(ctx);
    Stage stg(ctx, S * G * eb + G * ow * eb + G * 5, 4);
    void *de, *dout, *dn, *dst;
    HIP_TRY(ctx, stg.in(evals, S * G * eb, &de));
    HIP_TRY(ctx, stg.alloc(G * ow * eb, &dout));
    HIP_TRY(ctx, stg.alloc(G * 4, &dn));
    HIP_TRY(ctx, stg.alloc(G, &dst));
    // no device summary on this path: the status bytes come home anyway and say the same (and which failure is
    // reported no longer depends on which failing chunk finished last)
    rc = batch_recover_dev(ctx, {.sender_ids = sender_ids, .S = S, .evals = de, .G = G, .n = n, .d = d, .t = t, .out = dout, .ncoeffs = (uint32_t*)dn,
                                 .status = (uint8_t*)dst, .p0 = p0, .host_call = true});
    if (rc != ShareSuccess) return rc;
    std::vector<uint8_t> st_local;
    if (!status) {
        st_local.resize(G);
        status = st_local.data();
    }
    HIP_TRY(ctx, stg.out(out, dout, G * ow * eb));
    HIP_TRY(ctx, stg.out(ncoeffs, dn, G * 4));
    HIP_TRY(ctx, stg.out(status, dst, G));
    HIP_TRY(ctx, stg.finish());
    for (size_t g = 0; g < G; ++g)
        if (status[g] > HBMPC_CHUNK_FALLBACK) {
            g_err = "chunk " + std::to_string(g) + ": Online Error Correction failed to find a valid polynomial";
            return (ShareErrorCode)status[g];
        }
    return ShareSuccess;
}

// hbmpc_[gl_]dev_recover_check_degree_strided: the decode of `groups` verifiers' G chunks each (group q's values q * group_stride
// elements further on in every sender row) and the exact-degree test of what it decoded
template <class T>
ShareErrorCode recover_check_degree_dev(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const T* evals_dev, size_t row_stride, size_t G, size_t n,
                                        size_t t, size_t groups, size_t group_stride, T* ws_dev, uint8_t* status_out_dev,
                                        hbmpc_recover_summary* summary_dev, uint32_t* bad_dev, void* stream) {
    if (!ctx) return InvalidInput;
    if (!ws_dev || !bad_dev || groups == 0) return fail(ctx, InvalidInput, "null buffer or no group");
    // a verifier that fires at 2t + 1 arrivals has no OEC round: the top coefficient alone decides the exact degree
    const bool top_only = ctx->list_rows_in_kernel && S == 2 * t + 1 && ctx->direct_fail;
    RecoverCall c{.sender_ids = sender_ids, .S = S, .evals = evals_dev, .row_stride = row_stride, .G = G, .n = n, .d = t, .t = t, .out = ws_dev,
                  .status = status_out_dev, .summary = summary_dev, .stream = stream};
    if (top_only) c.p0 = true, c.only_coeff = (int)t;
    if (groups > 1) {  // several verifiers: one launch where the wave-per-chunk decode takes them, else one by one
        if (top_only) {
            RecoverCall all = c;
            all.G = groups * G;
            // groups that follow each other inside the sender rows (group_stride == G) are one plain call of groups * G chunks
            if (group_stride != G) all.group = G, all.group_stride = group_stride;
            const ShareErrorCode rc = batch_recover_dev(ctx, all);
            if (rc == ShareSuccess) return check_top_coeff_any(ctx, ws_dev, status_out_dev, groups * G, t, bad_dev, stream, G);
            if (rc != HBMPC_NOT_FUSED) return rc;
        }
        for (size_t q = 0; q < groups; ++q) {
            const ShareErrorCode rc = recover_check_degree_dev(ctx, sender_ids, S, evals_dev + q * group_stride, row_stride, G, n, t, 1, 0, ws_dev,
                                                               status_out_dev, summary_dev, bad_dev, stream);
            if (rc != ShareSuccess) return rc;
        }
        return ShareSuccess;
    }
    const ShareErrorCode rc = batch_recover_dev(ctx, c);
    if (rc != ShareSuccess) return rc;
    if (top_only) return hbmpc_dev_check_top_coeff(ctx, ws_dev, status_out_dev, G, t, bad_dev, stream);
    return hbmpc_dev_check_degree(ctx, ws_dev, status_out_dev, G, t + 1, t, bad_dev, stream);
}

}  // namespace

#define TYPED_RECOVER(T, REQ, PFX)                                                                                        \
    extern "C" ShareErrorCode PFX##dev_batch_recover(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const T* evals_dev, \
                                                     size_t G, size_t n, size_t d, size_t t, T* coeffs_out_dev,           \
                                                     uint32_t* ncoeffs_out_dev, uint8_t* status_out_dev,                  \
                                                     hbmpc_recover_summary* summary_dev, void* stream) {                  \
        REQ(ctx);                                                                                                         \
        return batch_recover_dev(ctx, {.sender_ids = sender_ids, .S = S, .evals = evals_dev, .G = G, .n = n, .d = d, .t = t,    \
                                       .out = coeffs_out_dev, .ncoeffs = ncoeffs_out_dev, .status = status_out_dev,         \
                                       .summary = summary_dev, .stream = stream});                                          \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##dev_batch_recover_p0(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S,               \
                                                        const T* evals_dev, size_t G, size_t n, size_t d, size_t t,       \
                                                        T* secrets_out_dev, uint8_t* status_out_dev,                      \
                                                        hbmpc_recover_summary* summary_dev, void* stream) {               \
        REQ(ctx);                                                                                                         \
        return batch_recover_dev(ctx, {.sender_ids = sender_ids, .S = S, .evals = evals_dev, .G = G, .n = n, .d = d, .t = t,    \
                                       .out = secrets_out_dev, .status = status_out_dev, .summary = summary_dev, .p0 = true, \
                                       .stream = stream});                                                                  \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##dev_batch_recover_strided(                                                             \
        hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const T* evals_dev, size_t row_stride, size_t G, size_t n,    \
        size_t d, size_t t, int p0_only, T* out_dev, uint32_t* ncoeffs_out_dev, uint8_t* status_out_dev,                  \
        hbmpc_recover_summary* summary_dev, void* stream) {                                                               \
        REQ(ctx);                                                                                                         \
        return batch_recover_dev(ctx, {.sender_ids = sender_ids, .S = S, .evals = evals_dev, .row_stride = row_stride, .G = G, \
                                       .n = n, .d = d, .t = t, .out = out_dev, .ncoeffs = p0_only ? nullptr : ncoeffs_out_dev, \
                                       .status = status_out_dev, .summary = summary_dev, .p0 = p0_only != 0, .stream = stream}); \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##dev_batch_recover_coeff_strided(                                                       \
        hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const T* evals_dev, size_t row_stride, size_t G, size_t n,    \
        size_t d, size_t t, size_t k, T* out_dev, uint8_t* status_out_dev, hbmpc_recover_summary* summary_dev,            \
        void* stream) {                                                                                                   \
        REQ(ctx);                                                                                                         \
        if (ctx && k > d) return fail(ctx, InvalidInput, "k must be <= d");                                               \
        return batch_recover_dev(ctx, {.sender_ids = sender_ids, .S = S, .evals = evals_dev, .row_stride = row_stride, .G = G, \
                                       .n = n, .d = d, .t = t, .out = out_dev, .status = status_out_dev, .summary = summary_dev, \
                                       .p0 = true, .stream = stream, .only_coeff = (int)k});                                \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##dev_recover_check_degree_strided(                                                      \
        hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const T* evals_dev, size_t row_stride, size_t G, size_t n,    \
        size_t t, size_t groups, size_t group_stride, T* ws_dev, uint8_t* status_out_dev,                                 \
        hbmpc_recover_summary* summary_dev, uint32_t* bad_dev, void* stream) {                                            \
        REQ(ctx);                                                                                                         \
        return recover_check_degree_dev(ctx, sender_ids, S, evals_dev, row_stride, G, n, t, groups, group_stride, ws_dev, \
                                        status_out_dev, summary_dev, bad_dev, stream);                                    \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##dev_batch_recover_slots(                                                               \
        hbmpc_ctx* ctx, const size_t* sender_ids, const size_t* row_slots, size_t S, const T* evals_dev, size_t row_stride, \
        size_t G, size_t n, size_t d, size_t t, int p0_only, T* out_dev, uint32_t* ncoeffs_out_dev,                       \
        uint8_t* status_out_dev, hbmpc_recover_summary* summary_dev, void* stream) {                                      \
        REQ(ctx);                                                                                                         \
        if (ctx && S && !row_slots) return fail(ctx, InvalidInput, "null row_slots");                                     \
        return batch_recover_dev(ctx, {.sender_ids = sender_ids, .S = S, .evals = evals_dev, .row_stride = row_stride, .G = G, \
                                       .n = n, .d = d, .t = t, .out = out_dev, .ncoeffs = p0_only ? nullptr : ncoeffs_out_dev, \
                                       .status = status_out_dev, .summary = summary_dev, .p0 = p0_only != 0, .stream = stream, \
                                       .slots = row_slots});                                                                \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##batch_recover(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const T* evals,      \
                                                 size_t G, size_t n, size_t d, size_t t, T* coeffs_out,                   \
                                                 uint32_t* ncoeffs_out, uint8_t* status_out) {                            \
        REQ(ctx);                                                                                                         \
        return batch_recover_host(ctx, sender_ids, S, evals, G, n, d, t, coeffs_out, ncoeffs_out, status_out, false);     \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##batch_recover_p0(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const T* evals,   \
                                                    size_t G, size_t n, size_t d, size_t t, T* secrets_out,               \
                                                    uint8_t* status_out) {                                                \
        REQ(ctx);                                                                                                         \
        return batch_recover_host(ctx, sender_ids, S, evals, G, n, d, t, secrets_out, nullptr, status_out, true);         \
    }
TYPED_RECOVER(U256, REQ_FR, hbmpc_)
TYPED_RECOVER(uint64_t, REQ_GL, hbmpc_gl_)

// ---- batched plain Lagrange interpolation through ALL supplied shares (NonRobustShare::recover_secret,
// common/share/shamir.rs:199-239, as the RanDouSha verifier runs it per column, ran_dou_sha/mod.rs:569-602)
// c0_out_dev != nullptr: the caller wants the constant terms c0[G] and the degrees only (the RanDouSha verifier's tests);
// coeffs_out_dev is then a [G][S] workspace that the fused kernel does not touch
static ShareErrorCode batch_interpolate_dev(hbmpc_ctx* ctx, const size_t* ids, size_t S, const void* evals_dev,
                                            size_t row_stride, size_t G, size_t n, void* coeffs_out_dev,
                                            uint32_t* degree_out_dev, void* stream, void* c0_out_dev = nullptr,
                                            const uint64_t* points = nullptr) {
    // points: the integer-point scheme (capi_shamir.inc, which has checked them): ids unused, n == S, no inverse DFT
    if (!ctx) return InvalidInput;
    if (S == 0 || G == 0) return fail(ctx, InvalidInput, "empty input");            // shamir.rs:204
    if ((!ids && !points) || !evals_dev || !coeffs_out_dev) return fail(ctx, InvalidInput, "null buffer");
    ShareErrorCode rc = ShareSuccess;
    bool done = false, degree_in_kernel = false;
    const InterpPlan plan = plan_interpolate(recover_knobs(ctx), G, n, S, row_stride, degree_out_dev != nullptr, c0_out_dev != nullptr);
    if (!points && plan.route[0] != InterpKernel::Decode) {  // the inverse DFT on point pairs (recover_route.hpp)
        SortedSenders ss;
        rc = validate_senders(ctx, ids, S, G, n, S - 1, 0, &ss);
        if (rc != ShareSuccess) return rc;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick(ctx, stream);
        const size_t half = n / 2;
        const uint32_t* tab;
        std::array<size_t, 5> aux = {0, 0, 0, 0, 0};
        rc = get_table(ctx, key("mfinv", {n}, ctx->impl), [&] {
            const std::vector<HFr> el = domain_elements<HFr>(n, n);  // el[k] = omega^k
            const HFr ninv = HFr::from_u64(n).inv();
            std::vector<std::vector<HFr>> C(n, std::vector<HFr>(n));
            for (size_t i = 0; i < n; ++i)
                for (size_t k = 0; k < n; ++k) C[i][k] = el[(n - (i * k) % n) % n] * ninv;  // omega^(-i k) / n
            std::vector<uint32_t> tbl = build_mfma_bfly_table(C, n, half);
            aux[0] = tbl.size();
            return tbl;
        }, &tab, &aux);
        if (rc != ShareSuccess) return rc;
        if (aux[0] != 0) {
            mf::MfmaRowsArgs a;
            memset(&a, 0, sizeof a);
            mf::mf_take_plan(plan.pairs, &a);
            a.in = (const uint8_t*)evals_dev, a.G = G, a.in_chunk_major = 0, a.row_stride = row_stride ? row_stride : G;
            for (size_t k = 0; k < n; ++k) a.rows.set(k, (unsigned)ss.rows[k]);  // input k = the share of party k
            a.table = (const uint8_t*)tab, a.nv = 0, a.half = (int)half, a.nout = (int)n;
            for (int i = 0; i < plan.count && !done; ++i) {
                a.ncoeffs = nullptr, a.out = (uint8_t*)coeffs_out_dev, a.out_stride = n, a.store_rows = 0;
                if (plan.route[i] == InterpKernel::IdftDegrees) {
                    a.ncoeffs = degree_out_dev;  // the kernel writes the degrees itself where an instance for it exists (n = 8, 16)
                    if (plan.c0_only) a.out = (uint8_t*)c0_out_dev, a.out_stride = 1, a.store_rows = 1;  // only coefficient 0 is stored
                    done = degree_in_kernel = launch_mfma_bfly((int)n, a, ctx->device, s);
                } else if (plan.route[i] == InterpKernel::Idft) {
                    done = launch_mfma_bfly((int)n, a, ctx->device, s);
                }
            }
            if (done) HIP_TRY(ctx, hipGetLastError());
            if (degree_in_kernel && plan.c0_only) return ShareSuccess;  // c0 and the degrees are written
        }
    }
    if (!done)
        rc = batch_recover_dev(ctx, {.sender_ids = ids, .S = S, .evals = evals_dev, .row_stride = row_stride, .G = G, .n = n, .d = S - 1, .t = 0,
                                     .out = coeffs_out_dev, .stream = stream, .points = points});
    if (rc != ShareSuccess) return rc;
    if (degree_out_dev && !degree_in_kernel) {  // one pass for the degree and, where asked for, the constant term
        launch_poly_degree((const uint64_t*)coeffs_out_dev, G, (int)S, (int)(ebytes(ctx) / 8), degree_out_dev, pick(ctx, stream), (uint64_t*)c0_out_dev);
        HIP_TRY(ctx, hipGetLastError());
        return ShareSuccess;
    }
    if (c0_out_dev) {
        launch_take_c0((int)(ebytes(ctx) / 8), (const uint64_t*)coeffs_out_dev, G, (int)S, (uint64_t*)c0_out_dev, pick(ctx, stream));
        HIP_TRY(ctx, hipGetLastError());
    }
    return ShareSuccess;
}
static ShareErrorCode batch_interpolate_host(hbmpc_ctx* ctx, const size_t* ids, size_t S, const void* evals, size_t G,
                                             size_t n, void* coeffs_out, uint32_t* degree_out) {
    if (!ctx) return InvalidInput;
    if (S == 0 || G == 0) return fail(ctx, InvalidInput, "empty input");
    if (!ids || !evals || !coeffs_out) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t eb = ebytes(ctx);
    Stage stg(ctx, 2 * S * G * eb + G * 4, 3);
    void *de, *dc, *dd;
    HIP_TRY(ctx, stg.in(evals, S * G * eb, &de));
    HIP_TRY(ctx, stg.alloc(S * G * eb, &dc));
    HIP_TRY(ctx, stg.alloc(G * 4, &dd));
    ShareErrorCode rc = batch_interpolate_dev(ctx, ids, S, de, G, G, n, dc, (uint32_t*)dd, nullptr);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, stg.out(coeffs_out, dc, S * G * eb));
    HIP_TRY(ctx, stg.out(degree_out, dd, G * 4));
    HIP_TRY(ctx, stg.finish());
    return ShareSuccess;
}

static bool elem_is_zero(const uint8_t* p, size_t eb) {
    for (size_t i = 0; i < eb; ++i)
        if (p[i]) return false;
    return true;
}
// trims trailing zero coefficients (DensePolynomial normal form), copies them out, returns the length
static size_t emit_trimmed(const std::vector<uint8_t>& co, size_t len, size_t eb, void* coeffs_out, void* secret_out) {
    while (len > 0 && elem_is_zero(co.data() + (len - 1) * eb, eb)) --len;
    memcpy(coeffs_out, co.data(), len * eb);
    if (len) memcpy(secret_out, co.data(), eb);
    else memset(secret_out, 0, eb);
    return len;
}

// ---- a6: RobustShare::recover_secret for one polynomial (robust_interpolate.rs:94-157) ---------
static ShareErrorCode recover_secret_any(hbmpc_ctx* ctx, const size_t* ids, const size_t* degrees, const void* vals,
                                         size_t S, size_t n, size_t t, void* coeffs_out, size_t* ncoeffs_out,
                                         void* secret_out) {
    if (!ctx) return InvalidInput;
    if (n < 3 * t + 1) return fail(ctx, InvalidInput, "n must be >= 3t + 1 for Byzantine fault tolerance");  // :100
    if (S == 0) return fail(ctx, InvalidInput, "Share slice is empty");                                      // :108
    if (!ids || !degrees || !vals || !coeffs_out || !ncoeffs_out || !secret_out) return fail(ctx, InvalidInput, "null");
    const size_t d = degrees[0];
    for (size_t i = 0; i < S; ++i)
        if (degrees[i] != d) return fail(ctx, DegreeMismatch, "mismatch degree between shares");  // :114
    {
        std::vector<size_t> srt(ids, ids + S);
        std::sort(srt.begin(), srt.end());
        for (size_t i = 1; i < S; ++i)
            if (srt[i] == srt[i - 1]) return fail(ctx, InvalidInput, "Duplicate share Ids");  // :118
        if (srt.back() >= n) return fail(ctx, InvalidInput, "Share id out of range");        // :125
    }
    if (S < d + t + 1) return fail(ctx, InvalidInput, "Not enough shares provided");  // :135
    // one chunk: evals[S][1] is exactly vals
    const size_t eb = ebytes(ctx);
    std::vector<uint8_t> co((d + 1) * eb);
    uint32_t nco = 0;
    uint8_t st = 0;
    ShareErrorCode rc = batch_recover_host(ctx, ids, S, vals, 1, n, d, t, co.data(), &nco, &st, false);
    if (rc != ShareSuccess) return rc;
    // the un-batched call returns DensePolynomial-normalised coefficients on BOTH paths (:149, :154)
    *ncoeffs_out = emit_trimmed(co, st == HBMPC_CHUNK_OPTIMISTIC ? d + 1 : nco, eb, coeffs_out, secret_out);
    return ShareSuccess;
}

// ---- gao_rs_decode alone (robust_interpolate.rs:456-538) ---------------------------------------
static ShareErrorCode gao_rs_decode_any(hbmpc_ctx* ctx, const void* received, size_t k, size_t n,
                                        const size_t* erasure_positions, size_t n_erasures, void* coeffs_out,
                                        size_t* ncoeffs_out) {
    if (!ctx) return InvalidInput;
    if (k > n) return fail(ctx, InvalidInput, "k must be less than or equal to n");  // :462
    if (n == 0 || n > 255) return fail(ctx, InvalidInput, "n must be in 1..255");
    if (!received || !coeffs_out || !ncoeffs_out) return fail(ctx, InvalidInput, "null buffer");
    if (n_erasures && !erasure_positions) return fail(ctx, InvalidInput, "null erasure positions");
    std::vector<uint8_t> erased(n, 0);
    for (size_t i = 0; i < n_erasures; ++i)
        if (erasure_positions[i] < n) erased[erasure_positions[i]] = 1;
    std::vector<size_t> known;
    for (size_t i = 0; i < n; ++i)
        if (!erased[i]) known.push_back(i);
    if ((known.size() + k) / 2 == 0)
        return fail(ctx, PolynomialOperationError, "degenerate decode (the reference divides by the zero polynomial)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int impl = ctx->impl;
    const size_t eb = ebytes(ctx);
    GaoLayout lay;
    std::vector<uint32_t> host = build_gao_tables(ctx, {known}, {(int)k}, known, n, impl, &lay);
    DevBuf dt, de, dout, dn, dsc;
    HIP_TRY(ctx, dsc.alloc(ctx, 64));
    HIP_TRY(ctx, dt.alloc(ctx, host.size() * 4));
    HIP_TRY(ctx, de.alloc(ctx, n * eb));
    HIP_TRY(ctx, dout.alloc(ctx, (k ? k : 1) * eb));
    HIP_TRY(ctx, dn.alloc(ctx, 8));
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(dt.p, host.data(), host.size() * 4, hipMemcpyHostToDevice, s));
    RowsArg rows_arg;
    memset(&rows_arg, 0, sizeof rows_arg);
    for (size_t i = 0; i < known.size(); ++i) rows_arg.set(i, (unsigned)known[i]);
    HIP_TRY(ctx, hipMemcpyAsync(de.p, received, n * eb, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(dn.p, 0, 8, s));
    GaoArgs ga;
    const uint32_t* gd = (const uint32_t*)dt.p;
    ga.evals = (const uint32_t*)de.p;
    ga.G = 1;
    ga.row_stride = 1;
    ga.rows = rows_arg;
    ga.reset = nullptr;
    ga.alpha_s = gd + lay.alpha_off;
    ga.rounds = (const GaoRound*)gd;
    ga.n_rounds = 1;
    ga.tables = gd;
    ga.k = (int)k;
    ga.accept_min = 0;
    ga.out_width = (int)k;
    ga.flagged = nullptr;
    ga.counters = nullptr;
    ga.out = (uint32_t*)dout.p;
    ga.ncoeffs = (uint32_t*)dn.p;
    ga.status = (uint8_t*)dn.p + 4;
    ga.summary = nullptr;
    ga.one_plain = gd + lay.one_off;
    ga.r2 = gd + lay.r2_off;
    ga.inv_exp = gd + lay.exp_off;
    ga.scales = (uint32_t*)dsc.p;
    launch_gao(impl, ga, n, 1, s);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t res[2] = {0, 0};
    std::vector<uint8_t> co((k ? k : 1) * eb);
    HIP_TRY(ctx, hipMemcpyAsync(co.data(), dout.p, co.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(res, dn.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    const uint8_t st = (uint8_t)(res[1] & 0xff);
    if (st != 1) return fail(ctx, (ShareErrorCode)st, "Failed to recover message polynomial from g(x)/v(x)");
    const size_t len = res[0] < k ? res[0] : k;
    memcpy(coeffs_out, co.data(), len * eb);
    *ncoeffs_out = res[0];
    return ShareSuccess;
}

// ---- NonRobustShare::recover_secret (common/share/shamir.rs:199-239) ---------------------------
template <class H>
static std::vector<uint32_t> lagrange_rows_t(const size_t* ids, size_t S, size_t n, int impl) {
    std::vector<H> el = domain_elements<H>(n, n), xs(S);
    for (size_t i = 0; i < S; ++i) xs[i] = el[ids[i]];
    auto basis = lagrange_basis(xs);
    std::vector<uint32_t> lb;
    for (size_t k = 0; k < S; ++k)
        for (size_t j = 0; j < S; ++j) put_const(lb, basis[j][k], impl);
    return lb;
}
static ShareErrorCode nonrobust_recover_any(hbmpc_ctx* ctx, const size_t* ids, const size_t* degrees, const void* vals,
                                            size_t S, size_t n, void* coeffs_out, size_t* ncoeffs_out, void* secret_out) {
    if (!ctx) return InvalidInput;
    if (S == 0) return fail(ctx, InvalidInput, "no shares");  // :204
    if (!ids || !degrees || !vals || !coeffs_out || !ncoeffs_out || !secret_out) return fail(ctx, InvalidInput, "null");
    {
        std::vector<size_t> srt(ids, ids + S);
        std::sort(srt.begin(), srt.end());
        for (size_t i = 1; i < S; ++i)
            if (srt[i] == srt[i - 1]) return fail(ctx, InvalidInput, "duplicate ids");  // :207
    }
    const size_t deg = degrees[0];
    for (size_t i = 0; i < S; ++i)
        if (degrees[i] != deg) return fail(ctx, DegreeMismatch, "mismatch degree between shares");  // :212
    if (S < deg + 1) return fail(ctx, InsufficientShares, "insufficient shares");                   // :215
    if (n == 0 || domain_size(n) > ((size_t)1 << 32)) return fail(ctx, NoSuitableDomain, "no domain");
    for (size_t i = 0; i < S; ++i)
        if (ids[i] >= n) return fail(ctx, InvalidInput, "id out of range");  // :224
    if (S > 4096) return fail(ctx, InvalidInput, "too many shares");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int impl = ctx->impl;
    const size_t eb = ebytes(ctx);
    const std::vector<uint32_t> lb = impl == IMPL_GOLD ? lagrange_rows_t<HGl>(ids, S, n, impl) : lagrange_rows_t<HFr>(ids, S, n, impl);
    Stage stg(ctx, lb.size() * 4 + 2 * S * eb, 3);
    void *dl, *dy, *dout;
    hipStream_t s = ctx->stream;
    HIP_TRY(ctx, stg.in(lb.data(), lb.size() * 4, &dl));
    HIP_TRY(ctx, stg.in(vals, S * eb, &dy));
    HIP_TRY(ctx, stg.alloc(S * eb, &dout));
    launch_matvec(impl, (const uint32_t*)dl, (const uint32_t*)dy, (int)S, (uint32_t*)dout, s);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint8_t> co(S * eb);
    HIP_TRY(ctx, stg.out(co.data(), dout, S * eb));
    HIP_TRY(ctx, stg.finish());
    size_t len = S;
    while (len > 0 && elem_is_zero(co.data() + (len - 1) * eb, eb)) --len;
    const size_t degree = len == 0 ? 0 : len - 1;  // DensePolynomial::degree()
    if (degree > deg) return fail(ctx, DegreeMismatch, "interpolated degree exceeds the share degree");  // :235
    // the reference indexes result_poly[0] (a panic for the zero polynomial): zero is returned here
    *ncoeffs_out = emit_trimmed(co, len, eb, coeffs_out, secret_out);
    return ShareSuccess;
}

#define TYPED_SINGLE(T, REQ, PFX)                                                                                         \
    extern "C" ShareErrorCode PFX##dev_batch_interpolate(hbmpc_ctx* ctx, const size_t* ids, size_t S, const T* evals_dev, \
                                                         size_t row_stride, size_t G, size_t n, T* coeffs_out_dev,        \
                                                         uint32_t* degree_out_dev, void* stream) {                        \
        REQ(ctx);                                                                                                         \
        return batch_interpolate_dev(ctx, ids, S, evals_dev, row_stride, G, n, coeffs_out_dev, degree_out_dev, stream);   \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##dev_batch_interpolate_c0(hbmpc_ctx* ctx, const size_t* ids, size_t S, const T* evals_dev, \
                                                            size_t row_stride, size_t G, size_t n, T* tmp_coeffs_dev, T* c0_out_dev, \
                                                            uint32_t* degree_out_dev, void* stream) {                          \
        REQ(ctx);                                                                                                         \
        if (!c0_out_dev || !degree_out_dev) return fail(ctx, InvalidInput, "null buffer");                                \
        return batch_interpolate_dev(ctx, ids, S, evals_dev, row_stride, G, n, tmp_coeffs_dev, degree_out_dev, stream, c0_out_dev); \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##dev_interpolate_degree_check_strided(                                                  \
        hbmpc_ctx* ctx, const size_t* ids, size_t S, const T* evals_dev, size_t row_stride, size_t G, size_t n, size_t d, \
        size_t groups, size_t group_stride, T* ws_dev, T* sel_out_dev, uint8_t* status_out_dev, void* stream) {           \
        REQ(ctx);                                                                                                         \
        if (!ws_dev || !sel_out_dev || !status_out_dev || groups == 0) return fail(ctx, InvalidInput, "null buffer or no group"); \
        if (S == 0 || d >= S) return fail(ctx, InvalidInput, "the degree must be below the number of points");            \
        if (groups > 1) { /* group q's results at sel_out_dev + q G 2, status_out_dev + q G */                            \
            if (ctx->list_rows_in_kernel) {                                                                               \
                /* groups that follow each other inside the sender rows (group_stride == G) are one plain call of groups * G chunks */ \
                const bool dense = group_stride == G;                                                                     \
                const ShareErrorCode rc = batch_recover_dev(                                                              \
                    ctx, {.sender_ids = ids, .S = S, .evals = evals_dev, .row_stride = row_stride, .G = groups * G, .n = n, .d = d, \
                          .t = S - d - 1, .out = sel_out_dev, .status = status_out_dev, .stream = stream, .second_coeff = (int)d, \
                          .group = dense ? 0 : G, .group_stride = dense ? 0 : group_stride});                             \
                if (rc != HBMPC_NOT_FUSED) return rc;                                                                     \
            }                                                                                                             \
            for (size_t q = 0; q < groups; ++q) {                                                                         \
                const ShareErrorCode rc = PFX##dev_interpolate_degree_check_strided(ctx, ids, S, evals_dev + q * group_stride, row_stride, \
                                                                                    G, n, d, 1, 0, ws_dev, sel_out_dev + q * G * 2, \
                                                                                    status_out_dev + q * G, stream);       \
                if (rc != ShareSuccess) return rc;                                                                        \
            }                                                                                                             \
            return ShareSuccess;                                                                                          \
        }                                                                                                                 \
        /* the S points on a polynomial of degree <= d?  d + 1 of them interpolate, the others verify; coefficients 0, d */ \
        if (ctx->list_rows_in_kernel) {                                                                                   \
            const ShareErrorCode rc = batch_recover_dev(ctx, {.sender_ids = ids, .S = S, .evals = evals_dev, .row_stride = row_stride, \
                                                              .G = G, .n = n, .d = d, .t = S - d - 1, .out = sel_out_dev,        \
                                                              .status = status_out_dev, .stream = stream, .second_coeff = (int)d}); \
            if (rc != HBMPC_NOT_FUSED) return rc;                                                                         \
        }                                                                                                                 \
        /* other shapes: the full interpolation through all S points, then the same two coefficients and the verdict */   \
        const ShareErrorCode rc = batch_interpolate_dev(ctx, ids, S, evals_dev, row_stride, G, n, ws_dev, nullptr, stream); \
        if (rc != ShareSuccess) return rc;                                                                                \
        launch_pick_two((int)(ebytes(ctx) / 8), (const uint64_t*)ws_dev, G, (int)S, (int)d, (uint64_t*)sel_out_dev,       \
                        status_out_dev, pick(ctx, stream));                                                               \
        HIP_TRY(ctx, hipGetLastError());                                                                                  \
        return ShareSuccess;                                                                                              \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##batch_interpolate(hbmpc_ctx* ctx, const size_t* ids, size_t S, const T* evals, size_t G, \
                                                     size_t n, T* coeffs_out, uint32_t* degree_out) {                     \
        REQ(ctx);                                                                                                         \
        return batch_interpolate_host(ctx, ids, S, evals, G, n, coeffs_out, degree_out);                                  \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##recover_secret(hbmpc_ctx* ctx, const size_t* ids, const size_t* degrees, const T* vals, \
                                                  size_t S, size_t n, size_t t, T* coeffs_out, size_t* ncoeffs_out,       \
                                                  T* secret_out) {                                                        \
        REQ(ctx);                                                                                                         \
        return recover_secret_any(ctx, ids, degrees, vals, S, n, t, coeffs_out, ncoeffs_out, secret_out);                 \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##gao_rs_decode(hbmpc_ctx* ctx, const T* received, size_t k, size_t n,                   \
                                                 const size_t* erasure_positions, size_t n_erasures, T* coeffs_out,       \
                                                 size_t* ncoeffs_out) {                                                   \
        REQ(ctx);                                                                                                         \
        return gao_rs_decode_any(ctx, received, k, n, erasure_positions, n_erasures, coeffs_out, ncoeffs_out);            \
    }                                                                                                                     \
    extern "C" ShareErrorCode PFX##nonrobust_recover_secret(hbmpc_ctx* ctx, const size_t* ids, const size_t* degrees,     \
                                                            const T* vals, size_t S, size_t n, T* coeffs_out,             \
                                                            size_t* ncoeffs_out, T* secret_out) {                         \
        REQ(ctx);                                                                                                         \
        return nonrobust_recover_any(ctx, ids, degrees, vals, S, n, coeffs_out, ncoeffs_out, secret_out);                 \
    }
TYPED_SINGLE(U256, REQ_FR, hbmpc_)
TYPED_SINGLE(uint64_t, REQ_GL, hbmpc_gl_)

// test aid (tests/test_gpu_device_tables.py): the matrix-core table of a sender set as the library builds it -- expanded on
// the device (on_device != 0) or by the host reference (tables_mfma.hpp::build_mfma_table) -- copied to the host
extern "C" ShareErrorCode hbmpc_debug_mfma_table(hbmpc_ctx* ctx, const size_t* sorted_ids, size_t S, size_t n, size_t d, size_t t,
                                                 int on_device, uint8_t* out, size_t cap, size_t* bytes_out) {
    REQ_FR(ctx);
    if (!ctx) return InvalidInput;
    const size_t m = d + 1, needed = d + t + 1;
    if (!sorted_ids || !bytes_out || S < needed || m < 2 || m > MF_MAX_M || n > 255 || n < S) return fail(ctx, InvalidInput, "bad shape");
    for (size_t i = 0; i < S; ++i)
        if (sorted_ids[i] >= n || (i && sorted_ids[i] <= sorted_ids[i - 1])) return fail(ctx, InvalidInput, "ids must ascend");
    const std::vector<size_t> ids(sorted_ids, sorted_ids + S);
    const auto dom = domain_inv<HFr>(ctx, n);
    const auto rows = recover_coeff_rows<HFr>(*dom, ids, d, t);
    const size_t bytes = rows.size() * mf_row_bytes(m);
    *bytes_out = bytes;
    if (!out || cap < bytes) return ShareSuccess;
    if (!on_device) {
        const std::vector<uint32_t> tab = build_mfma_table(rows, m);
        memcpy(out, tab.data(), bytes);
        return ShareSuccess;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> seed = mf_coeff_words(rows, m);
    seed.resize(2 * seed.size());
    uint32_t* dev = nullptr;
    HIP_TRY(ctx, hipMalloc(&dev, bytes + seed.size() * 4));
    uint32_t* dseed = dev + bytes / 4;
    uint64_t e[4];
    mf_bias_e(m, e);
    hipError_t err = hipMemcpy(dseed, seed.data(), seed.size() * 4, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        launch_mfma_table((const uint64_t*)dseed, (int)m, (int)rows.size(), e, mf_bias_mag(m), (uint8_t*)dev, (uint64_t*)dseed + rows.size() * m * 4,
                          ctx->stream);
        err = hipStreamSynchronize(ctx->stream);
    }
    if (err == hipSuccess) err = hipMemcpy(out, dev, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(dev);
    HIP_TRY(ctx, err);
    return ShareSuccess;
}
