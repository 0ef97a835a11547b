// capi_batchrecon.inc -- BatchReconNode for all parties on this device (honeybadger/batch_recon/batch_recon.rs:144-185, 371-391, 451-467)
// (included at the end of hbmpc_capi.hip, ahead of capi_randbit.inc, whose two opens are calls of batchrecon_launches).

namespace {

// ids are 0 .. S - 1 in this order: the decode reads row s as sender s's without a slots list
bool is_prefix(const size_t* ids, size_t S) {
    for (size_t i = 0; i < S; ++i)
        if (ids[i] != i) return false;
    return true;
}

// The three launches.  BatchRecon (degree d) of x [party][G (d + 1)] -> opened [G (d + 1)]: every party's encode of its chunks of
// d + 1 (:157-165), the recipients' P(0) decodes from ids1 (:384-391: the row of sender p for "chunk" j G + g is Y + p (n G) + (j G + g)),
// the coefficient decode of the revealed values from ids2 (:457-467).  Y and Z are [party][..] and [recipient][..], so a sender set
// that is not a prefix reads every sender's row in place at its id (the slots form).
ShareErrorCode batchrecon_launches(hbmpc_ctx* ctx, const size_t* ids1, size_t S1, const size_t* ids2, size_t S2, const void* x, size_t G, size_t n,
                                   size_t d, size_t t, void* Y, void* Z, void* opened, uint8_t* rstatus, uint8_t* status,
                                   hbmpc_recover_summary* summary_first, hbmpc_recover_summary* summary, void* stream, bool honest_majority) {
    ShareErrorCode rc = eval_dev(ctx, x, G, n, d, Y, stream, n);
    if (rc != ShareSuccess) return rc;
    rc = batch_recover_dev(ctx, {.sender_ids = ids1, .S = S1, .evals = Y, .row_stride = n * G, .G = n * G, .n = n, .d = d, .t = t, .out = Z,
                                 .status = rstatus, .summary = summary_first, .p0 = true, .stream = stream,
                                 .slots = is_prefix(ids1, S1) ? nullptr : ids1, .honest_majority = honest_majority});
    if (rc != ShareSuccess) return rc;
    return batch_recover_dev(ctx, {.sender_ids = ids2, .S = S2, .evals = Z, .G = G, .n = n, .d = d, .t = t, .out = opened, .status = status,
                                   .summary = summary, .stream = stream, .slots = is_prefix(ids2, S2) ? nullptr : ids2,
                                   .honest_majority = honest_majority});
}

// H: HFr or HGl.  All of the validation comes before the first launch or memset: a call that is refused has written nothing.
template <class H>
ShareErrorCode batchrecon_parties_any(hbmpc_ctx* ctx, const size_t* ids1, size_t S1, const size_t* ids2, size_t S2, const void* x, size_t N, size_t n,
                                      size_t d, size_t t, void* Y, void* Z, void* opened, uint8_t* rstatus, uint8_t* status,
                                      hbmpc_recover_summary* summary_first, hbmpc_recover_summary* summary, void* stream) {
    if (!ids1 || !ids2 || !x || !Y || !Z || !opened) return fail(ctx, InvalidInput, "null buffer");
    if (d == 0 || d >= 255) return fail(ctx, InvalidInput, "d must be in 1 .. 254");
    if (!batch_in_range(ctx, N, n)) return InvalidInput;
    if (N % (d + 1) != 0) return fail(ctx, InvalidInput, "N must be a multiple of d + 1");  // batch_recon.rs:144-185 pads; the caller does here
    const size_t G = N / (d + 1);
    SortedSenders ss1, ss2;
    ShareErrorCode rc = validate_senders(ctx, ids1, S1, n * G, n, d, t, &ss1);
    if (rc != ShareSuccess) return rc;
    rc = validate_senders(ctx, ids2, S2, G, n, d, t, &ss2);
    if (rc != ShareSuccess) return rc;
    const BatchReconPlan plan = plan_batchrecon(protocol_knobs(ctx), ctx->fused_batchrecon_max, {N, n, t, d, S1, S2});
    if (plan.one_launch) {  // a workgroup per chunk (kernels_batchrecon_wg.hpp)
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick(ctx, stream);
        const int impl = ctx->impl;
        BatchReconWgArgs ba;
        memset(&ba, 0, sizeof ba);
        ba.n = (int)n, ba.t = (int)t, ba.d = (int)d, ba.G = G, ba.N = N, ba.lk1 = plan.lk_eval;
        ba.same = ss1.ids == ss2.ids;
        if (launch_batchrecon_wg(impl, ba, ctx->device, s, true)) {
            rc = rec_table<H>(ctx, *domain_inv<H>(ctx, n), ss1.ids, n, d, t, &ba.tab1);
            if (rc != ShareSuccess) return rc;
            rc = rec_table<H>(ctx, *domain_inv<H>(ctx, n), ss2.ids, n, d, t, &ba.tab2);
            if (rc != ShareSuccess) return rc;
            rc = vmat_table<H>(ctx, n, d, &ba.vmat);
            if (rc != ShareSuccess) return rc;
            for (size_t i = 0; i < S1; ++i) ba.ids1[i] = (uint8_t)ss1.ids[i], ba.ids2[i] = (uint8_t)ss2.ids[i];
            ba.x = as_words(x), ba.Y = as_words(Y), ba.Z = as_words(Z), ba.opened = as_words(opened), ba.rstatus = rstatus, ba.status = status;
            return enqueue_one_launch(ctx, s, &ba.counters, {{&ba.summary_first, summary_first}, {&ba.summary, summary}},
                                      [&] { launch_batchrecon_wg(impl, ba, ctx->device, s, false); });
        }
    }
    return batchrecon_launches(ctx, ids1, S1, ids2, S2, x, G, n, d, t, Y, Z, opened, rstatus, status, summary_first, summary, stream, false);
}

}  // namespace

// The call is ONE launch (kernels_batchrecon_wg.hpp), or hbmpc_dev_vandermonde_apply_parties and hbmpc_dev_batch_recover_slots twice
// (the P(0) form over the n G recipients' chunks, the coefficient form over the G revealed ones) -- the same bytes in every output
// buffer.  Which: plan_batchrecon (protocol_route.hpp).
#define TYPED_BATCHRECON(T, H, REQ, PFX)                                                                                                             \
    extern "C" ShareErrorCode PFX##dev_batchrecon_parties(hbmpc_ctx* ctx, const size_t* eval_senders, size_t S1, const size_t* reveal_senders,       \
                                                          size_t S2, const T* x, size_t N, size_t n, size_t d, size_t t, T* y_ws, T* z_out,          \
                                                          T* opened_out, uint8_t* rstatus_out, uint8_t* status_out,                                  \
                                                          hbmpc_recover_summary* summary_first_dev, hbmpc_recover_summary* summary_dev, void* stream) { \
        if (!ctx) return InvalidInput;                                                                                                               \
        REQ(ctx);                                                                                                                                    \
        return batchrecon_parties_any<H>(ctx, eval_senders, S1, reveal_senders, S2, x, N, n, d, t, y_ws, z_out, opened_out, rstatus_out, status_out,  \
                                         summary_first_dev, summary_dev, stream);                                                                    \
    }
TYPED_BATCHRECON(U256, HFr, REQ_FR, hbmpc_)
TYPED_BATCHRECON(uint64_t, HGl, REQ_GL, hbmpc_gl_)
#undef TYPED_BATCHRECON
