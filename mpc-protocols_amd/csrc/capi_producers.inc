// capi_producers.inc -- RanSha and DouSha + RanDouSha for all parties on this device (share_gen/share_gen.rs:232-289, 401-454, 516-530,
// 199-203; double_share/double_share_generation.rs:151-215, ran_dou_sha/mod.rs:371-449, 569-602, 314-331)
// (included at the end of hbmpc_capi.hip).  A layer beside the handles of capi_pipelines.hip, for a caller with buffers of its own: the
// calls of the handles' together form (producer_route.hpp), or ONE launch (kernels_producers_wg.hpp).

namespace {

const uint32_t kBadInit[2] = {0u, 0xffffffffu};  // static: a captured copy reads it again at every replay

struct ProducersCall {
    const void *coeffs[2];          // [dealer][K][deg + 1]; null: dealt is the input
    void *dealt[2], *out[2], *yv[2], *sel[2], *st[2];
    void* ws;
    uint8_t* status;                // RanSha
    hbmpc_recover_summary* summary; // RanSha
    uint32_t* bad;
    size_t K, n, t, S;
    void* stream;
};

// what every refusal of both calls shares; all of it comes before the first launch or copy: a call that is refused has written nothing
ShareErrorCode producers_refusal(hbmpc_ctx* ctx, const ProducersCall& c, bool dou) {
    const size_t n = c.n, t = c.t, K = c.K, eb = ebytes(ctx);
    if (K == 0) return fail(ctx, InvalidInput, "K must be >= 1");
    if (t > 127 || n > 255 || n <= 2 * t) return fail(ctx, InvalidInput, "n must be in 2t + 1 .. 255");  // t first: 2 * t cannot wrap
    if (!dou && (c.S < 2 * t + 1 || c.S > n)) return fail(ctx, InvalidInput, "verify_senders must be in 2t + 1 .. n");
    const size_t nver = dou ? n - t - 1 : 2 * t;
    for (int s = 0; s < (dou ? 2 : 1); ++s) {
        if (!c.dealt[s] || !c.out[s] || (nver && !c.yv[s])) return fail(ctx, InvalidInput, "null buffer");
        if (dou && nver && (!c.sel[s] || !c.st[s])) return fail(ctx, InvalidInput, "null buffer");
    }
    if (!c.ws || !c.bad) return fail(ctx, InvalidInput, "null buffer");
    if (dou && (c.coeffs[0] == nullptr) != (c.coeffs[1] == nullptr)) return fail(ctx, InvalidInput, "both sharings from coefficients or both from dealt shares");
    // the sizes at which the together form's single calls do not exist (producer_route.hpp): the handles are the path there
    if (K >= ((size_t)1 << 19) || n * n * K * eb >= ((size_t)1 << 32)) return fail(ctx, InvalidInput, "batch beyond the single calls: use the handle");
    // a guard, not a case of its own: below the two limits above plan_deal never splits a deal (kDealersTogetherMax is above 2^19, and its
    // 32-bit limits on a call's outputs and inputs go below n only from a dealt block of 4 GiB on, deg + 1 <= n); it keeps this call and
    // the handles' rule from drifting apart
    if (c.coeffs[0])
        for (int s = 0; s < (dou ? 2 : 1); ++s)
            if (plan_deal(eb, n, K, (size_t)(s + 1) * t) != (n >= 2 ? n : 1)) return fail(ctx, InvalidInput, "the deal would be split: use the handle");
    return ShareSuccess;
}

// the deal and the mixing call of one sharing: rows [row0, row0 + rows) to the parties' lists, the others party-major to yv
ShareErrorCode producers_deal_mix(hbmpc_ctx* ctx, const ProducersCall& c, int s, size_t deg, size_t row0, size_t rows) {
    const size_t n = c.n, K = c.K, eb = ebytes(ctx);
    unsigned char *x = (unsigned char*)c.ws, *y = x + n * n * K * eb;
    if (c.coeffs[s]) {
        const ShareErrorCode rc = eval_dev(ctx, c.coeffs[s], K, n, deg, c.dealt[s], c.stream, n);
        if (rc != ShareSuccess) return rc;
    }
    const hbmpc_list_slice slice{c.out[s], rows * K, 0, K};
    const bool others = rows < n;
    return eval_rows_lists_any(ctx, c.dealt[s], n * K, n * K, n, n - 1, x, y, row0, rows, K, &slice, 1, c.stream, others ? c.yv[s] : nullptr, others);
}

// the fields of the one-launch form that both calls fill the same way; false: the kernel does not run here (nothing is enqueued)
template <class H>
ShareErrorCode producers_one_launch(hbmpc_ctx* ctx, const ProducersCall& c, bool dou, bool* ran) {
    *ran = false;
    const size_t n = c.n, t = c.t;
    const bool gold = is_gold(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, c.stream);
    const int impl = ctx->impl;
    ProducersWgArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.K = c.K, pa.n = (int)n, pa.t = (int)t;
    pa.row0 = dou ? 0 : (int)(2 * t), pa.rows = dou ? (int)(t + 1) : (int)(n - 2 * t);
    pa.nver = dou ? (int)(n - t - 1) : (int)(2 * t), pa.ver0 = dou ? (int)(t + 1) : 0;
    for (int i = 0; i < (dou ? 2 : 1); ++i) {
        ProducersWgSharing& sh = pa.sh[i];
        sh.deg = (int)((i + 1) * t);
        // the verifiers' decode: RanSha from senders 0 .. 2t (degree t, t verify rows); RanDouSha through all n points, selectively over
        // Fr (degree deg, n - deg - 1 verify rows), the full interpolation over Goldilocks
        sh.M = !dou ? (int)(t + 1) : gold ? (int)n : sh.deg + 1;
        sh.nv = !dou ? (int)t : (int)n - sh.M;
    }
    if (!launch_producers_wg(impl, dou, pa, ctx->device, s, true)) return ShareSuccess;
    const auto dom = domain_inv<H>(ctx, n);
    ShareErrorCode rc = vmat_table<H>(ctx, n, n - 1, &pa.vmat);
    if (rc != ShareSuccess) return rc;
    for (int i = 0; i < (dou ? 2 : 1); ++i) {
        ProducersWgSharing& sh = pa.sh[i];
        rc = rec_table<H>(ctx, *dom, first_ids(sh.M + sh.nv), n, sh.M - 1, sh.nv, &sh.tab);
        if (rc != ShareSuccess) return rc;
        sh.coeffs = as_words(c.coeffs[i]), sh.dealt = as_words(c.dealt[i]), sh.out = as_words(c.out[i]), sh.yv = as_words(c.yv[i]);
        sh.sel = as_words(c.sel[i]), sh.st = dou ? c.st[i] : c.status;
    }
    pa.bad = c.bad;
    *ran = true;
    return enqueue_one_launch(ctx, s, &pa.counters, {{&pa.summary, c.summary}}, [&] { launch_producers_wg(impl, dou, pa, ctx->device, s, false); });
}

template <class H, class T>
ShareErrorCode ransha_parties_any(hbmpc_ctx* ctx, const ProducersCall& c) {
    ShareErrorCode rc = producers_refusal(ctx, c, false);
    if (rc != ShareSuccess) return rc;
    const size_t n = c.n, t = c.t, K = c.K, nver = 2 * t, eb = ebytes(ctx);
    if (plan_producers(protocol_knobs(ctx), ctx->fused_producers_max, {ProducerCall::RanSha, K, n, t, c.S}).one_launch) {
        bool ran = false;
        rc = producers_one_launch<H>(ctx, c, false, &ran);
        if (ran || rc != ShareSuccess) return rc;
    }
    rc = producers_deal_mix(ctx, c, 0, t, 2 * t, n - 2 * t);  // rows 2t .. n - 1 are the output (share_gen.rs:199-203)
    if (rc != ShareSuccess) return rc;
    hipStream_t s = pick(ctx, c.stream);
    if (nver == 0 || n >= 3 * t + 1) {
        rc = hbmpc_memcpy_h2d(ctx, c.bad, kBadInit, sizeof kBadInit, c.stream);
        if (rc != ShareSuccess || nver == 0) return rc;  // t = 0: no verifier
        T* poly = (T*)((unsigned char*)c.ws + 2 * n * n * K * eb);
        return recover_check_degree_dev<T>(ctx, first_ids(c.S).data(), c.S, (const T*)c.yv[0], nver * K, K, n, t, nver, K, poly, c.status, c.summary, c.bad, c.stream);
    }
    // below n = 3t + 1 recover_secret refuses every column (robust_interpolate.rs:290): every verifier fails every column, by value (a
    // captured call keeps no host pointer)
    const uint32_t all = (uint32_t)(nver * K);
    if (c.status) HIP_TRY(ctx, hipMemsetAsync(c.status, (int)InvalidInput, nver * K, s));
    const uint32_t sm[4] = {all, all, 0u, (uint32_t)InvalidInput}, bd[2] = {all, 0u};
    for (int i = 0; i < 4 && c.summary; ++i) HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)((uint32_t*)c.summary + i), (int)sm[i], 1, s));
    for (int i = 0; i < 2; ++i) HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(c.bad + i), (int)bd[i], 1, s));
    return ShareSuccess;
}

template <class H, class T>
ShareErrorCode randousha_parties_any(hbmpc_ctx* ctx, const ProducersCall& c, bool gold) {
    ShareErrorCode rc = producers_refusal(ctx, c, true);
    if (rc != ShareSuccess) return rc;
    const size_t n = c.n, t = c.t, K = c.K, nver = n - t - 1, eb = ebytes(ctx);
    if (plan_producers(protocol_knobs(ctx), ctx->fused_producers_max, {ProducerCall::RanDouSha, K, n, t, n}).one_launch) {
        bool ran = false;
        rc = producers_one_launch<H>(ctx, c, true, &ran);
        if (ran || rc != ShareSuccess) return rc;
    }
    // DouShaNode::init_batch: both sharings of every secret; RanDouShaNode::init_batch: rows 0 .. t are the output (ran_dou_sha/mod.rs:314-331)
    if (c.coeffs[0]) {
        for (int s = 0; s < 2; ++s) {
            rc = eval_dev(ctx, c.coeffs[s], K, n, (size_t)(s + 1) * t, c.dealt[s], c.stream, n);
            if (rc != ShareSuccess) return rc;
        }
    }
    ProducersCall mixes = c;
    mixes.coeffs[0] = mixes.coeffs[1] = nullptr;
    for (int s = 0; s < 2; ++s) {
        rc = producers_deal_mix(ctx, mixes, s, 0, 0, t + 1);
        if (rc != ShareSuccess) return rc;
    }
    rc = hbmpc_memcpy_h2d(ctx, c.bad, kBadInit, sizeof kBadInit, c.stream);
    if (rc != ShareSuccess || nver == 0) return rc;
    // verifiers t + 1 .. n - 1 interpolate both sharings through all n shares and test the degrees and the constant terms (:586-602)
    const std::vector<size_t> ids = first_ids(n);
    T* poly = (T*)((unsigned char*)c.ws + 2 * n * n * K * eb);
    for (int s = 0; s < 2; ++s) {
        if constexpr (std::is_same<T, uint64_t>::value)
            rc = hbmpc_gl_dev_batch_interpolate_c0(ctx, ids.data(), n, (const T*)c.yv[s], nver * K, nver * K, n, poly, (T*)c.sel[s], (uint32_t*)c.st[s], c.stream);
        else
            rc = hbmpc_dev_interpolate_degree_check_strided(ctx, ids.data(), n, (const T*)c.yv[s], nver * K, K, n, (size_t)(s + 1) * t, nver, K, poly, (T*)c.sel[s],
                                                            (uint8_t*)c.st[s], c.stream);
        if (rc != ShareSuccess) return rc;
    }
    if (gold) return hbmpc_dev_check_double_share_c0_columns(ctx, c.sel[0], (const uint32_t*)c.st[0], c.sel[1], (const uint32_t*)c.st[1], nver * K, K, t, c.bad, c.stream);
    return hbmpc_dev_check_double_share_sel(ctx, c.sel[0], (const uint8_t*)c.st[0], c.sel[1], (const uint8_t*)c.st[1], nver * K, K, t, c.bad, c.stream);
}

}  // namespace

// Each call is ONE launch (kernels_producers_wg.hpp) or the calls of the handles' together form -- the same bytes in every output
// buffer.  Which: plan_producers (protocol_route.hpp).
#define TYPED_PRODUCERS(T, H, REQ, PFX, GOLD)                                                                                                        \
    extern "C" ShareErrorCode PFX##dev_ransha_parties(hbmpc_ctx* ctx, const T* coeffs, T* dealt, size_t K, size_t n, size_t t, size_t verify_senders, \
                                                      T* out, T* yv_out, T* ws_dev, uint8_t* status_out, hbmpc_recover_summary* summary_dev,        \
                                                      uint32_t* bad_dev, void* stream) {                                                             \
        if (!ctx) return InvalidInput;                                                                                                               \
        REQ(ctx);                                                                                                                                    \
        ProducersCall c{};                                                                                                                           \
        c.coeffs[0] = coeffs, c.dealt[0] = dealt, c.out[0] = out, c.yv[0] = yv_out, c.ws = ws_dev, c.status = status_out, c.summary = summary_dev;    \
        c.bad = bad_dev, c.K = K, c.n = n, c.t = t, c.S = verify_senders, c.stream = stream;                                                          \
        return ransha_parties_any<H, T>(ctx, c);                                                                                                     \
    }                                                                                                                                                \
    extern "C" ShareErrorCode PFX##dev_randousha_parties(hbmpc_ctx* ctx, const T* coeffs_t, const T* coeffs_2t, T* dealt_t, T* dealt_2t, size_t K,   \
                                                         size_t n, size_t t, T* out_t, T* out_2t, T* yv_t_out, T* yv_2t_out, T* ws_dev, T* sel_t_out, \
                                                         T* sel_2t_out, void* st_t_out, void* st_2t_out, uint32_t* bad_dev, void* stream) {          \
        if (!ctx) return InvalidInput;                                                                                                               \
        REQ(ctx);                                                                                                                                    \
        ProducersCall c{};                                                                                                                           \
        c.coeffs[0] = coeffs_t, c.coeffs[1] = coeffs_2t, c.dealt[0] = dealt_t, c.dealt[1] = dealt_2t, c.out[0] = out_t, c.out[1] = out_2t;            \
        c.yv[0] = yv_t_out, c.yv[1] = yv_2t_out, c.ws = ws_dev, c.sel[0] = sel_t_out, c.sel[1] = sel_2t_out, c.st[0] = st_t_out, c.st[1] = st_2t_out; \
        c.bad = bad_dev, c.K = K, c.n = n, c.t = t, c.S = n, c.stream = stream;                                                                       \
        return randousha_parties_any<H, T>(ctx, c, GOLD);                                                                                            \
    }
TYPED_PRODUCERS(U256, HFr, REQ_FR, hbmpc_, false)
TYPED_PRODUCERS(uint64_t, HGl, REQ_GL, hbmpc_gl_, true)
#undef TYPED_PRODUCERS
