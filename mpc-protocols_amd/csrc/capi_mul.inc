// capi_mul.inc -- Multiply (Beaver) for all parties on this device (mul/multiplication.rs:417-426,102-139,57-100;
// honeybadger/mod.rs:543-628)
// (included at the end of hbmpc_capi.hip).

extern "C" ShareErrorCode hbmpc_set_fused_mul(hbmpc_ctx* ctx, size_t max_elements) {
    if (!ctx) return InvalidInput;
    ctx->fused_mul_max = max_elements;
    return ShareSuccess;
}

namespace {

// The separate launches: the shares Multiply opens, ONE P(0) decode over the 2 N values of a sender row, finalize_mul.  sender_ids
// are party ids and de_sh_ws is [party][2][N], so the decode reads every sender's row in place at its id (the slots form).
ShareErrorCode mul_launches(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const U256* a, const U256* b, const U256* c, const U256* x,
                            const U256* y, size_t N, size_t n, size_t t, U256* de_sh_ws, U256* de_out, U256* z_out, uint8_t* status_out,
                            hbmpc_recover_summary* summary_dev, void* stream) {
    // Large batches: the shares are formed as the matrix-core decode loads them, as in hbmpc_dev_fpmul_parties
    ShareErrorCode rc = HBMPC_NOT_FUSED;
    if (N >= ctx->pair_decode_min) {
        PairInput pi = {(const uint32_t*)a, (const uint32_t*)b, (const uint32_t*)x, (const uint32_t*)y, N};
        rc = batch_recover_dev(ctx, {.sender_ids = sender_ids, .S = S, .G = 2 * N, .n = n, .d = t, .t = t, .out = de_out, .status = status_out,
                                     .summary = summary_dev, .p0 = true, .stream = stream, .pair = &pi});
    }
    if (rc == HBMPC_NOT_FUSED) {
        rc = hbmpc_dev_beaver_open_shares_paired(ctx, a, b, x, y, N, n, de_sh_ws, stream);
        if (rc != ShareSuccess) return rc;
        rc = hbmpc_dev_batch_recover_slots(ctx, sender_ids, sender_ids, S, de_sh_ws, 2 * N, 2 * N, n, t, t, 1, de_out, nullptr, status_out,
                                           summary_dev, stream);
    }
    if (rc != ShareSuccess) return rc;
    return hbmpc_dev_beaver_finalize_parties(ctx, c, x, y, de_out, de_out + N, N, n, z_out, stream);
}
ShareErrorCode mul_launches(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const uint64_t* a, const uint64_t* b, const uint64_t* c,
                            const uint64_t* x, const uint64_t* y, size_t N, size_t n, size_t t, uint64_t* de_sh_ws, uint64_t* de_out,
                            uint64_t* z_out, uint8_t* status_out, hbmpc_recover_summary* summary_dev, void* stream) {
    ShareErrorCode rc = hbmpc_gl_dev_beaver_open_shares_paired(ctx, a, b, x, y, N, n, de_sh_ws, stream);
    if (rc != ShareSuccess) return rc;
    rc = hbmpc_gl_dev_batch_recover_slots(ctx, sender_ids, sender_ids, S, de_sh_ws, 2 * N, 2 * N, n, t, t, 1, de_out, nullptr, status_out,
                                          summary_dev, stream);
    if (rc != ShareSuccess) return rc;
    return hbmpc_gl_dev_beaver_finalize_parties(ctx, c, x, y, de_out, de_out + N, N, n, z_out, stream);
}

// what both fields check, all of it before the first launch: a call that is refused has written nothing
template <class T>
ShareErrorCode mul_validate(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const T* a, const T* b, const T* c, const T* x, const T* y, size_t N,
                            size_t n, size_t t, const T* de_sh_ws, const T* de_out, const T* z_out, SortedSenders* ss) {
    if (!sender_ids || !a || !b || !c || !x || !y || !de_sh_ws || !de_out || !z_out) return fail(ctx, InvalidInput, "null buffer");
    if (N == 0 || n == 0 || n > 255) return fail(ctx, InvalidInput, "N, n out of range");
    return validate_senders(ctx, sender_ids, S, 2 * N, n, t, t, ss);
}

}  // namespace

// The call is ONE launch for a small batch opened from exactly 2t + 1 senders (kernels_mul_wave.hpp), and otherwise
// hbmpc_dev_beaver_open_shares_paired, the P(0) decode of the 2 N values and hbmpc_dev_beaver_finalize_parties -- the same bytes
// in every output buffer.
extern "C" ShareErrorCode hbmpc_dev_mul_parties(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const U256* a, const U256* b, const U256* c,
                                                const U256* x, const U256* y, size_t N, size_t n, size_t t, U256* de_sh_ws, U256* de_out,
                                                U256* z_out, uint8_t* status_out, hbmpc_recover_summary* summary_dev, void* stream) {
    if (!ctx) return InvalidInput;
    REQ_FR(ctx);
    SortedSenders ss;
    ShareErrorCode rc = mul_validate(ctx, sender_ids, S, a, b, c, x, y, N, n, t, de_sh_ws, de_out, z_out, &ss);
    if (rc != ShareSuccess) return rc;
    if (N <= ctx->fused_mul_max && S == 2 * t + 1 && ctx->impl == IMPL_U29 && !ctx->force_generic && ctx->direct_fail && n <= 64 && t <= 30) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick(ctx, stream);
        MulWaveArgs ma;
        memset(&ma, 0, sizeof ma);
        ma.N = N, ma.parties = (int)n, ma.needed = (int)(2 * t + 1), ma.M = (int)(t + 1);
        // the products of a table row are shared by up to four adjacent lanes (a DPP quad) while the t + 2 rows still fit half a wave
        while (ma.lk < 2 && ((t + 2) << (ma.lk + 1)) <= 32 && ((size_t)2 << ma.lk) <= t + 1) ++ma.lk;
        if (launch_mul_wave(ma, ctx->device, s, true)) {
            rc = fpmul_wave_table(ctx, ss, n, t, &ma.tab);
            if (rc != ShareSuccess) return rc;
            ma.ta = (const uint32_t*)a, ma.tb = (const uint32_t*)b, ma.tc = (const uint32_t*)c, ma.x = (const uint32_t*)x, ma.y = (const uint32_t*)y;
            ma.de_out = (uint32_t*)de_out, ma.z = (uint32_t*)z_out, ma.status = status_out;
            for (size_t i = 0; i < S; ++i) ma.rows.set(i, (unsigned)ss.ids[i]);  // the per-party arrays are indexed by party id
            return with_decode_counters(ctx, s, 2048, [&](uint32_t* counters) -> ShareErrorCode {
                ma.counters = counters;
                ma.summary = summary_dev ? (uint32_t*)summary_dev : counters + 4;  // the scratch's local summary slot
                launch_mul_wave(ma, ctx->device, s, false);
                HIP_TRY(ctx, hipGetLastError());
                return ShareSuccess;  // the kernel's last workgroup leaves the counters at zero
            });
        }
    }
    return mul_launches(ctx, sender_ids, S, a, b, c, x, y, N, n, t, de_sh_ws, de_out, z_out, status_out, summary_dev, stream);
}

// Goldilocks: always the three hbmpc_gl_* launches
extern "C" ShareErrorCode hbmpc_gl_dev_mul_parties(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const uint64_t* a, const uint64_t* b,
                                                   const uint64_t* c, const uint64_t* x, const uint64_t* y, size_t N, size_t n, size_t t,
                                                   uint64_t* de_sh_ws, uint64_t* de_out, uint64_t* z_out, uint8_t* status_out,
                                                   hbmpc_recover_summary* summary_dev, void* stream) {
    if (!ctx) return InvalidInput;
    REQ_GL(ctx);
    SortedSenders ss;
    const ShareErrorCode rc = mul_validate(ctx, sender_ids, S, a, b, c, x, y, N, n, t, de_sh_ws, de_out, z_out, &ss);
    if (rc != ShareSuccess) return rc;
    return mul_launches(ctx, sender_ids, S, a, b, c, x, y, N, n, t, de_sh_ws, de_out, z_out, status_out, summary_dev, stream);
}
