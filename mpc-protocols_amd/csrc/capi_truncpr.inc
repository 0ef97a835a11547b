// capi_truncpr.inc -- TruncPrNode and FPDivConstNode for all parties on this device (fpmul/truncpr.rs:185-318,
// fpdiv/fpdiv_const.rs:61-99) and the host helper that turns denominators into the public multipliers
// (included at the end of hbmpc_capi.hip).

// fpdiv/mod.rs:8-60.  Host arithmetic only: no context, no device.
extern "C" ShareErrorCode hbmpc_fixed_point_reciprocal_scaled(const U256* denom, size_t N, size_t f, U256* w_out, size_t* first_bad_out) {
    if (first_bad_out) *first_bad_out = SIZE_MAX;
    if (N == 0) return ShareSuccess;
    if (!denom || !w_out) return fail(nullptr, InvalidInput, "null buffer");
    if (f >= 64) return fail(nullptr, InvalidInput, "f: 1u128 << (2 f) overflows in the reference");
    typedef unsigned __int128 u128;
    for (size_t i = 0; i < N; ++i)  // :18-20, :32-34 InvalidDivisor; checked for the whole batch before anything is written
        if ((denom[i].data[0] | denom[i].data[1]) == 0) {
            if (first_bad_out) *first_bad_out = i;
            return fail(nullptr, InvalidInput, "InvalidDivisor: a denominator is zero in its low 128 bits");
        }
    const u128 num = (u128)1 << (2 * f);
    for (size_t i = 0; i < N; ++i) {
        const u128 b = ((u128)denom[i].data[1] << 64) | denom[i].data[0];  // :23-30 the lowest 16 bytes
        const u128 w = (num + (b >> 1)) / b;                               // :44; num + b / 2 < 2^126 + 2^127
        w_out[i] = U256{{(uint64_t)w, (uint64_t)(w >> 64), 0, 0}};         // :49-57; < 2^128 < r
    }
    return ShareSuccess;
}

// The call is ONE launch, a wave per element (kernels_truncpr_wave.hpp), or k_truncpr_front, hbmpc_dev_batch_recover_p0 and
// hbmpc_dev_truncpr_finalize_parties -- the same bytes in every output buffer.  Which: plan_protocol (protocol_route.hpp).
extern "C" ShareErrorCode hbmpc_dev_truncpr_parties(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const U256* a, const U256* w_dev,
                                                    const U256* r_bits, const U256* r_int, size_t k, size_t m, size_t N, size_t n, size_t t,
                                                    U256* c_out, U256* r_dash_out, U256* open_sh_out, U256* c_open_out, U256* d_out,
                                                    uint8_t* status_out, hbmpc_recover_summary* summary_dev, void* stream) {
    if (!ctx) return InvalidInput;
    REQ_FR(ctx);
    if (!truncpr_params_ok(ctx, TP_ALL, k, m)) return InvalidInput;
    if (!sender_ids || !a || !r_int || (m && !r_bits) || !r_dash_out || !open_sh_out || !c_open_out || !d_out) return fail(ctx, InvalidInput, "null buffer");
    if (w_dev && !c_out) return fail(ctx, InvalidInput, "a multiplier needs c_out for the products");
    if (!batch_in_range(ctx, N, n)) return InvalidInput;
    SortedSenders ss;  // before the first launch: a call that is refused has written nothing
    ShareErrorCode rc = validate_senders(ctx, sender_ids, S, N, n, t, t, &ss);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    const int impl = ctx->impl;
    const ProtocolPlan plan = plan_protocol(protocol_knobs(ctx), {ProtocolCall::TruncPr, N, n, t, S, 0});
    TruncprConsts tc;  // 2^-m only for the one launch: the separate launches' last step fetches its own
    rc = truncpr_consts(ctx, k, m, plan.one_launch, &tc);
    if (rc != ShareSuccess) return rc;
    if (plan.one_launch) {
        TruncprWaveArgs ta;
        memset(&ta, 0, sizeof ta);
        ta.N = N, ta.parties = (int)n, ta.m = (int)m, ta.needed = (int)(2 * t + 1), ta.M = (int)(t + 1), ta.mask_bits = (int)(m > 256 ? 256 : m);
        ta.w = (const uint32_t*)w_dev, ta.lk = plan.lk_wave;
        if (launch_truncpr_wave(ta, ctx->device, s, true)) {
            rc = fpmul_wave_table(ctx, ss, n, t, &ta.tab);  // its first t + 1 rows: the verify rows and the P(0) row
            if (rc != ShareSuccess) return rc;
            memcpy(ta.c0, tc.cs.c0, sizeof ta.c0), memcpy(ta.c1, tc.cs.c1, sizeof ta.c1), memcpy(ta.cinv, tc.ci.c0, sizeof ta.cinv), memcpy(ta.r2, tc.cs.r2, sizeof ta.r2);
            ta.a = (const uint32_t*)a, ta.r_bits = (const uint32_t*)r_bits, ta.r_int = (const uint32_t*)r_int, ta.pow2 = tc.pow2;
            ta.c = (uint32_t*)c_out, ta.r_dash = (uint32_t*)r_dash_out, ta.open_sh = (uint32_t*)open_sh_out;
            ta.out = (uint32_t*)d_out, ta.c_open = (uint32_t*)c_open_out, ta.status = status_out;
            for (size_t i = 0; i < S; ++i) ta.rows.set(i, (unsigned)ss.rows[i]);  // row s of the arrays is sender_ids[s]'s, as the decode call reads them
            return enqueue_one_launch(ctx, s, &ta.counters, {{&ta.summary, summary_dev}}, [&] { launch_truncpr_wave(ta, ctx->device, s, false); });
        }
    }
    // a grid row per party at every size.  k_fpmul_middle's rule (one thread for all parties from 2^16 elements, so that the public
    // operand is converted once) loses here: a thread's n rounds of m + 2 dependent loads cost more than n - 1 conversions of w
    // save (profiles/fpdiv_bench.txt: 0.285 against 0.185 ms at 2^16, level at 2^18); the kernel itself serves any gridDim.y
    const unsigned grid_parties = (unsigned)n;
    launch_truncpr_front(impl, as_words(a), as_words(w_dev), as_words(r_bits), as_words(r_int), (int)m, N, tc.cs, tc.pow2, as_words(c_out),
                         as_words(r_dash_out), as_words(open_sh_out), (unsigned)n, grid_parties, s);
    HIP_TRY(ctx, hipGetLastError());
    rc = hbmpc_dev_batch_recover_p0(ctx, sender_ids, S, open_sh_out, N, n, t, t, c_open_out, status_out, summary_dev, stream);
    if (rc != ShareSuccess) return rc;
    return hbmpc_dev_truncpr_finalize_parties(ctx, w_dev ? c_out : a, r_dash_out, c_open_out, m, N, n, d_out, stream);
}
