// capi_prandbit.inc -- PRandBit / PRandInt for all parties on this device (fpmul/prandbitd.rs; honeybadger/mod.rs:1951-2150)
// (included at the end of hbmpc_capi.hip).

namespace {

// every buffer of the call
struct PRandBitCall {
    const uint64_t *contrib, *b_q;
    size_t n, t, B, lk_bits;
    uint64_t* sums;
    uint8_t* bad;
    U256* r_p;
    uint8_t* r_2;
    uint64_t *r_q, *rb, *Y, *Z, *opened;
    U256* b_p;
    uint8_t *b_2, *rstatus;
    hbmpc_recover_summary *sm_first, *sm;
    void* stream;
};

// What both calls check before the first launch or memset: the shape (riss_shape), the GF(2^8) domain, the fold's capacity rule and its
// and the conversion's ranges.  *tn: C(n, t).
ShareErrorCode prand_shape(hbmpc_ctx* ctx, size_t n, size_t t, size_t B, size_t lk_bits, size_t* tn) {
    const ShareErrorCode rc = riss_shape(ctx, n, t, tn);
    if (rc != ShareSuccess) return rc;
    if (n > 255) return fail(ctx, InvalidInput, "the GF(2^8) domain holds at most 255 parties");  // Gf256Domain::new
    if (lk_bits >= 64 || lk_bits + 2 + (size_t)ilog2(n) >= 64) return fail(ctx, HBMPC_FIELD_CAPACITY, "k + l + 2 + ceil(log2 n) reaches 64 bits");
    if (B > ((size_t)1 << 32) || *tn * ((B + 255) / 256) > 0x7fffffffu) return fail(ctx, InvalidInput, "B beyond the supported range");
    return ShareSuccess;
}

// the Fr half of the one-launch kernel's arguments: the coefficient table of (ctx_fr, n, t)
ShareErrorCode prand_fr_args(hbmpc_ctx* ctx_fr, size_t n, size_t t, size_t tn, PRandBitWgArgs* a) {
    RissTab tab;
    size_t Tn = 0;
    const ShareErrorCode rc = riss_tab(ctx_fr, n, t, tn, -1, &tab, &Tn);
    if (rc != ShareSuccess) return rc;
    a->coefF = tab.coef, a->coef2 = tab.coef2, a->red = tab.red;
    a->n = (int)n, a->t = (int)t, a->Tn = (int)Tn;
    return ShareSuccess;
}

// The eight launches: today's sequence (pipelines.py:PRandBit).  The open is BatchRecon of degree t from senders 0 .. S - 1: with
// S = 2t + 1 a decode with no OEC round, a failed chunk final and opened to zero (as randbit_launches); a larger S takes the decodes' OEC path.
// prandbit_tail: the seven after the fold, shared with the seeded call (capi_riss_seeded.inc), whose fold draws the contributions itself.
ShareErrorCode prandbit_tail(hbmpc_ctx* ctx_fr, hbmpc_ctx* ctx_gl, const PRandBitCall& c, size_t S, void* s) {
    const size_t n = c.n, t = c.t, B = c.B, G = B / (t + 1);
    ShareErrorCode rc = riss_convert_any(ctx_fr, c.sums, n, t, B, nullptr, n, 0, c.r_p, c.r_2, s);
    if (rc != ShareSuccess) return rc;
    rc = riss_convert_any(ctx_gl, c.sums, n, t, B, nullptr, n, 0, c.r_q, nullptr, s);
    if (rc != ShareSuccess) return rc;
    rc = fr_op_any(ctx_gl, 0, c.r_q, c.b_q, n * B, c.rb, s);
    if (rc != ShareSuccess) return rc;
    rc = eval_dev(ctx_gl, c.rb, G, n, t, c.Y, s, n);  // batch_recon.rs:157-165: Y [party][recipient][chunk]
    if (rc != ShareSuccess) return rc;
    const std::vector<size_t> ids = first_ids(S);
    rc = batch_recover_dev(ctx_gl, {.sender_ids = ids.data(), .S = S, .evals = c.Y, .row_stride = n * G, .G = n * G, .n = n, .d = t, .t = t, .out = c.Z,
                                    .status = c.rstatus, .summary = c.sm_first, .p0 = true, .stream = s});
    if (rc != ShareSuccess) return rc;
    rc = batch_recover_dev(ctx_gl, {.sender_ids = ids.data(), .S = S, .evals = c.Z, .G = G, .n = n, .d = t, .t = t, .out = c.opened, .status = c.rstatus,
                                    .summary = c.sm, .stream = s});
    if (rc != ShareSuccess) return rc;
    return hbmpc_dev_prandbit_finalize_parties(ctx_fr, c.opened, c.r_p, c.r_2, B, n, c.b_p, c.b_2, s);
}
ShareErrorCode prandbit_launches(hbmpc_ctx* ctx_fr, hbmpc_ctx* ctx_gl, const PRandBitCall& c, size_t tn, size_t S, void* s) {
    const ShareErrorCode rc = hbmpc_dev_riss_fold(ctx_fr, c.contrib, c.n, tn, c.B, c.lk_bits, c.sums, c.bad, s);
    return rc != ShareSuccess ? rc : prandbit_tail(ctx_fr, ctx_gl, c, S, s);
}
// PRandInt after the fold: the conversion over Fr
ShareErrorCode prandint_tail(hbmpc_ctx* ctx_fr, size_t n, size_t t, size_t B, const uint64_t* sums, U256* r_p, void* s) {
    return riss_convert_any(ctx_fr, sums, n, t, B, nullptr, n, 0, r_p, nullptr, s);
}

}  // namespace

// The call is ONE launch (kernels_prandbit_wg.hpp), or hbmpc_dev_riss_fold, the two conversions, the add, the encode, the two decodes
// and hbmpc_dev_prandbit_finalize_parties -- the same bytes in every output buffer (y_ws, z_ws: workspaces).  Which: plan_prandbit
// (prandbit_route.hpp).  All of the validation comes before the first launch or memset: a call that is refused has written nothing.
extern "C" ShareErrorCode hbmpc_dev_prandbit_parties(hbmpc_ctx* ctx_fr, hbmpc_ctx* ctx_gl, const uint64_t* contrib, const uint64_t* b_q, size_t n, size_t t,
                                                     size_t B, size_t lk_bits, size_t open_senders, uint64_t* sums, uint8_t* bad, U256* r_p, uint8_t* r_2,
                                                     uint64_t* r_q, uint64_t* rb, uint64_t* y_ws, uint64_t* z_ws, uint64_t* opened, U256* b_p, uint8_t* b_2,
                                                     uint8_t* rstatus, hbmpc_recover_summary* summary_first, hbmpc_recover_summary* summary,
                                                     void* stream) {
    if (!ctx_fr || !ctx_gl) return InvalidInput;
    REQ_FR(ctx_fr);
    REQ_GL(ctx_gl);
    if (ctx_fr->device != ctx_gl->device) return fail(ctx_fr, InvalidInput, "the two contexts are on different devices");
    size_t tn = 0;
    ShareErrorCode rc = prand_shape(ctx_fr, n, t, B, lk_bits, &tn);
    if (rc != ShareSuccess) return rc;
    if (B % (t + 1) != 0) return fail(ctx_fr, InvalidInput, "B must be a multiple of t + 1");  // prandbitd.rs:472-476
    const PRandBitKnobs knobs{ctx_fr->impl, ctx_fr->force_generic, ctx_gl->direct_fail, ctx_fr->fused_prandbit_max};
    const PRandBitPlan plan = plan_prandbit(knobs, {true, B, n, t, tn, open_senders});
    if (plan.senders < 2 * t + 1 || plan.senders > n) return fail(ctx_fr, InvalidInput, "open_senders must be 0 or in 2t + 1 .. n");
    if (B == 0) return ShareSuccess;
    if (!contrib || !b_q || !sums || !bad || !r_p || !r_2 || !r_q || !rb || !y_ws || !z_ws || !opened || !b_p || !b_2 || !rstatus)
        return fail(ctx_fr, InvalidInput, "null buffer");
    HIP_TRY(ctx_fr, hipSetDevice(ctx_fr->device));
    hipStream_t s = pick(ctx_fr, stream);  // the Goldilocks context's calls run on it too
    const PRandBitCall c{contrib, b_q, n, t, B, lk_bits, sums, bad, r_p, r_2, r_q, rb, y_ws, z_ws, opened, b_p, b_2, rstatus, summary_first, summary, s};
    if (plan.one_launch) {
        PRandBitWgArgs a;
        memset(&a, 0, sizeof a);
        rc = prand_fr_args(ctx_fr, n, t, tn, &a);
        if (rc != ShareSuccess) return rc;
        if (launch_prandbit_wg(true, a, ctx_fr->device, s, true)) {
            RissTab tg;
            size_t Tn = 0;
            rc = riss_tab(ctx_gl, n, t, tn, -1, &tg, &Tn);
            if (rc != ShareSuccess) return rc;
            a.coefG = tg.coef;
            rc = rec_table<HGl>(ctx_gl, *domain_inv<HGl>(ctx_gl, n), first_ids(2 * t + 1), n, t, t, &a.tab);
            if (rc != ShareSuccess) return rc;
            rc = vmat_table<HGl>(ctx_gl, n, t, &a.vmat);
            if (rc != ShareSuccess) return rc;
            a.contrib = contrib, a.b_q = b_q, a.sums = sums, a.bad = bad, a.r_p = as_words(r_p), a.r_2 = r_2, a.r_q = r_q, a.rb = rb, a.opened = opened;
            a.b_p = as_words(b_p), a.b_2 = b_2, a.rstatus = rstatus, a.B = B, a.bound = (uint64_t)1 << lk_bits;
            return enqueue_one_launch(ctx_gl, s, &a.counters, {{&a.sm_first, summary_first}, {&a.sm, summary}}, [&]() -> ShareErrorCode {
                HIP_TRY(ctx_fr, hipMemsetAsync(bad, 0, n * tn, s));
                launch_prandbit_wg(true, a, ctx_fr->device, s, false);
                return ShareSuccess;
            });
        }
    }
    return prandbit_launches(ctx_fr, ctx_gl, c, tn, plan.senders, s);
}

// PRandInt: the fold and the Fr conversion (any B) as ONE launch, or as hbmpc_dev_riss_fold and hbmpc_dev_riss_convert_parties
extern "C" ShareErrorCode hbmpc_dev_prandint_parties(hbmpc_ctx* ctx_fr, const uint64_t* contrib, size_t n, size_t t, size_t B, size_t lk_bits,
                                                     uint64_t* sums, uint8_t* bad, U256* r_p, void* stream) {
    if (!ctx_fr) return InvalidInput;
    REQ_FR(ctx_fr);
    size_t tn = 0;
    ShareErrorCode rc = prand_shape(ctx_fr, n, t, B, lk_bits, &tn);
    if (rc != ShareSuccess) return rc;
    if (B == 0) return ShareSuccess;
    if (!contrib || !sums || !bad || !r_p) return fail(ctx_fr, InvalidInput, "null buffer");
    HIP_TRY(ctx_fr, hipSetDevice(ctx_fr->device));
    hipStream_t s = pick(ctx_fr, stream);
    const PRandBitKnobs knobs{ctx_fr->impl, ctx_fr->force_generic, true, ctx_fr->fused_prandbit_max};
    if (plan_prandbit(knobs, {false, B, n, t, tn, 0}).one_launch) {
        PRandBitWgArgs a;
        memset(&a, 0, sizeof a);
        rc = prand_fr_args(ctx_fr, n, t, tn, &a);
        if (rc != ShareSuccess) return rc;
        a.contrib = contrib, a.sums = sums, a.bad = bad, a.r_p = as_words(r_p), a.B = B, a.bound = (uint64_t)1 << lk_bits;
        if (launch_prandbit_wg(false, a, ctx_fr->device, s, true)) {
            HIP_TRY(ctx_fr, hipMemsetAsync(bad, 0, n * tn, s));
            launch_prandbit_wg(false, a, ctx_fr->device, s, false);
            HIP_TRY(ctx_fr, hipGetLastError());
            return ShareSuccess;
        }
    }
    rc = hbmpc_dev_riss_fold(ctx_fr, contrib, n, tn, B, lk_bits, sums, bad, s);
    if (rc != ShareSuccess) return rc;
    return prandint_tail(ctx_fr, n, t, B, sums, r_p, s);
}
