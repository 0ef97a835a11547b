// capi_input.inc -- Input and Output for all parties on this device (honeybadger/input/input.rs:489-506, 85-100, 300-301;
// honeybadger/output/output.rs:157-177)
// (included at the end of hbmpc_capi.hip).
//
// Input: the client opens a mask per value from the servers' shares of it (recover_secret per element; the first error aborts),
// broadcasts masked = x + mask, and server p keeps masked - r_p as its share of x.  Output: the client opens the result shares.
// Not here: sessions, RBC and the InputMessage / OutputMessage envelopes; the 48-byte Vec<RobustShare> and Vec<F> payloads
// (hbmpc_dev_unpack_shares / hbmpc_dev_pack_fvec convert them); sampling the masks (they are RanSha's outputs).

namespace {

// Either field.  The call is ONE launch, a wave per element (kernels_input_wave.hpp: Fr only), or the P(0) decode of the masks
// with every sender's row read in place and k_input_finish -- the same bytes in every output buffer.  Which: plan_protocol
// (protocol_route.hpp).  An element whose mask does not open (status >= 2) is refused in either form: zeros in mask_out,
// masked_out and in_sh_out, never x + 0.  All of the validation comes before the first launch: a call that is refused has
// written nothing.
ShareErrorCode input_parties_any(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const void* x, const void* r_sh, size_t N, size_t n, size_t t,
                                 void* mask_out, void* masked_out, void* in_sh_out, uint8_t* status_out, hbmpc_recover_summary* summary_dev,
                                 void* stream) {
    if (!sender_ids || !x || !r_sh || !mask_out || !masked_out || !in_sh_out) return fail(ctx, InvalidInput, "null buffer");
    if (!status_out) return fail(ctx, InvalidInput, "status_out is required: it decides which elements are refused");
    if (!batch_in_range(ctx, N, n)) return InvalidInput;
    SortedSenders ss;
    ShareErrorCode rc = validate_senders(ctx, sender_ids, S, N, n, t, t, &ss);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    const ProtocolPlan plan = plan_protocol(protocol_knobs(ctx), {ProtocolCall::Input, N, n, t, S, 0});
    if (plan.one_launch) {
        InputWaveArgs ia;
        memset(&ia, 0, sizeof ia);
        ia.N = N, ia.parties = (int)n, ia.needed = (int)(2 * t + 1), ia.M = (int)(t + 1);
        ia.lk = plan.lk_wave;
        if (launch_input_wave(ia, ctx->device, s, true)) {
            rc = fpmul_wave_table(ctx, ss, n, t, &ia.tab);  // its first t + 1 rows: the verify rows and the P(0) row
            if (rc != ShareSuccess) return rc;
            ia.x = as_words(x), ia.r_sh = as_words(r_sh), ia.mask = as_words(mask_out), ia.masked = as_words(masked_out);
            ia.in_sh = as_words(in_sh_out), ia.status = status_out;
            for (size_t i = 0; i < S; ++i) ia.rows.set(i, (unsigned)ss.ids[i]);  // the per-party arrays are indexed by party id
            return enqueue_one_launch(ctx, s, &ia.counters, {{&ia.summary, summary_dev}}, [&] { launch_input_wave(ia, ctx->device, s, false); });
        }
    }
    // sender_ids are party ids and r_sh is [party][N], so the decode reads every sender's row in place at its id (the slots form)
    rc = batch_recover_dev(ctx, {.sender_ids = sender_ids, .S = S, .evals = r_sh, .G = N, .n = n, .d = t, .t = t, .out = mask_out, .status = status_out,
                                 .summary = summary_dev, .p0 = true, .stream = stream, .slots = sender_ids});
    if (rc != ShareSuccess) return rc;
    launch_input_finish(ctx->impl, status_out, as_words(mask_out), as_words(x), as_words(r_sh), N, (unsigned)n, as_words(masked_out), as_words(in_sh_out), s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}

// output.rs:157-177: recover_secret(.., n, t) per element from the servers' rows, read in place at their party ids
ShareErrorCode output_parties_any(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const void* sh, size_t N, size_t n, size_t t, void* out,
                                  uint8_t* status_out, hbmpc_recover_summary* summary_dev, void* stream) {
    if (!sender_ids || !sh || !out) return fail(ctx, InvalidInput, "null buffer");
    if (!batch_in_range(ctx, N, n)) return InvalidInput;
    return batch_recover_dev(ctx, {.sender_ids = sender_ids, .S = S, .evals = sh, .G = N, .n = n, .d = t, .t = t, .out = out, .status = status_out,
                                   .summary = summary_dev, .p0 = true, .stream = stream, .slots = sender_ids});
}

}  // namespace

#define TYPED_IO(T, REQ, PFX)                                                                                                                  \
    extern "C" ShareErrorCode PFX##dev_input_parties(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const T* x, const T* r_sh, size_t N,   \
                                                     size_t n, size_t t, T* mask_out, T* masked_out, T* in_sh_out, uint8_t* status_out,         \
                                                     hbmpc_recover_summary* summary_dev, void* stream) {                                       \
        if (!ctx) return InvalidInput;                                                                                                         \
        REQ(ctx);                                                                                                                              \
        return input_parties_any(ctx, sender_ids, S, x, r_sh, N, n, t, mask_out, masked_out, in_sh_out, status_out, summary_dev, stream);      \
    }                                                                                                                                          \
    extern "C" ShareErrorCode PFX##dev_output_parties(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const T* sh, size_t N, size_t n,      \
                                                      size_t t, T* out, uint8_t* status_out, hbmpc_recover_summary* summary_dev, void* stream) { \
        if (!ctx) return InvalidInput;                                                                                                         \
        REQ(ctx);                                                                                                                              \
        return output_parties_any(ctx, sender_ids, S, sh, N, n, t, out, status_out, summary_dev, stream);                                      \
    }
TYPED_IO(U256, REQ_FR, hbmpc_)
TYPED_IO(uint64_t, REQ_GL, hbmpc_gl_)
#undef TYPED_IO
