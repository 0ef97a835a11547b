// capi_mul.inc -- Multiply (Beaver) for all parties on this device (mul/multiplication.rs:417-426,102-139,57-100;
// honeybadger/mod.rs:543-628)
// (included at the end of hbmpc_capi.hip).

namespace {

// Either field.  The call is ONE launch, a wave per element (kernels_mul_wave.hpp: Fr only), or the open of a - x and b - y
// (open_beaver_pair) and finalize_mul -- the same bytes in every output buffer.  Which: plan_protocol (protocol_route.hpp).
// All of the validation comes before the first launch: a call that is refused has written nothing.
ShareErrorCode mul_parties_any(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const void* a, const void* b, const void* c, const void* x,
                               const void* y, size_t N, size_t n, size_t t, void* de_sh_ws, void* de_out, void* z_out, uint8_t* status_out,
                               hbmpc_recover_summary* summary_dev, void* stream) {
    if (!sender_ids || !a || !b || !c || !x || !y || !de_sh_ws || !de_out || !z_out) return fail(ctx, InvalidInput, "null buffer");
    if (!batch_in_range(ctx, N, n)) return InvalidInput;
    SortedSenders ss;
    ShareErrorCode rc = validate_senders(ctx, sender_ids, S, 2 * N, n, t, t, &ss);
    if (rc != ShareSuccess) return rc;
    const ProtocolPlan plan = plan_protocol(protocol_knobs(ctx), {ProtocolCall::Mul, N, n, t, S, 0});
    if (plan.one_launch) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick(ctx, stream);
        MulWaveArgs ma;
        memset(&ma, 0, sizeof ma);
        ma.N = N, ma.parties = (int)n, ma.needed = (int)(2 * t + 1), ma.M = (int)(t + 1);
        ma.lk = plan.lk_row;
        if (launch_mul_wave(ma, ctx->device, s, true)) {
            rc = fpmul_wave_table(ctx, ss, n, t, &ma.tab);
            if (rc != ShareSuccess) return rc;
            ma.ta = as_words(a), ma.tb = as_words(b), ma.tc = as_words(c), ma.x = as_words(x), ma.y = as_words(y);
            ma.de_out = as_words(de_out), ma.z = as_words(z_out), ma.status = status_out;
            for (size_t i = 0; i < S; ++i) ma.rows.set(i, (unsigned)ss.ids[i]);  // the per-party arrays are indexed by party id
            return enqueue_one_launch(ctx, s, &ma.counters, {{&ma.summary, summary_dev}}, [&] { launch_mul_wave(ma, ctx->device, s, false); });
        }
    }
    // sender_ids are party ids and de_sh_ws is [party][2][N], so the decode reads every sender's row in place at its id (the slots form)
    rc = open_beaver_pair(ctx, plan.pair_first, true, sender_ids, S, a, b, x, y, N, n, t, de_sh_ws, de_out, status_out, summary_dev, stream);
    if (rc != ShareSuccess) return rc;
    return beaver_finalize_any(ctx, c, x, y, de_out, (const unsigned char*)de_out + N * ebytes(ctx), N, z_out, stream, n);
}

}  // namespace

#define TYPED_MUL(T, REQ, PFX)                                                                                                               \
    extern "C" ShareErrorCode PFX##dev_mul_parties(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const T* a, const T* b, const T* c,    \
                                                   const T* x, const T* y, size_t N, size_t n, size_t t, T* de_sh_ws, T* de_out, T* z_out,    \
                                                   uint8_t* status_out, hbmpc_recover_summary* summary_dev, void* stream) {                  \
        if (!ctx) return InvalidInput;                                                                                                       \
        REQ(ctx);                                                                                                                            \
        return mul_parties_any(ctx, sender_ids, S, a, b, c, x, y, N, n, t, de_sh_ws, de_out, z_out, status_out, summary_dev, stream);        \
    }
TYPED_MUL(U256, REQ_FR, hbmpc_)
TYPED_MUL(uint64_t, REQ_GL, hbmpc_gl_)
#undef TYPED_MUL
