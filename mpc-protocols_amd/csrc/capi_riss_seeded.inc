// capi_riss_seeded.inc -- seeded RISS dealing (kernels_riss_sample.hpp, contract "hbmpc-riss-chacha20-v1"): one sender's contributions,
// all n senders' folded sums, and the seeded forms of PRandBit / PRandInt for all parties (included after capi_prandbit.inc, whose
// checks and tails they share).  Every check comes before the first launch or memset: a call that is refused has written nothing.

namespace {

// what every seeded call checks after the shape: the domain tag's 16 bits and the index range [first_index, first_index + B)
ShareErrorCode riss_stream_range(hbmpc_ctx* ctx, size_t domain, size_t B, uint64_t first_index) {
    if (domain > 65535) return fail(ctx, InvalidInput, "the stream's domain tag has 16 bits");
    if (first_index + (uint64_t)B < first_index) return fail(ctx, InvalidInput, "first_index + B passes 2^64");
    return ShareSuccess;
}
// riss_shape, the fold's capacity rule and the grid's ranges for a context of either field (the protocol calls use prand_shape)
ShareErrorCode riss_seeded_shape(hbmpc_ctx* ctx, size_t n, size_t t, size_t domain, size_t B, uint64_t first_index, size_t lk_bits, size_t* tn) {
    ShareErrorCode rc = riss_shape(ctx, n, t, tn);
    if (rc != ShareSuccess) return rc;
    if (lk_bits >= 64 || lk_bits + 2 + (size_t)ilog2(n) >= 64) return fail(ctx, HBMPC_FIELD_CAPACITY, "k + l + 2 + ceil(log2 n) reaches 64 bits");
    if (B > ((size_t)1 << 32) || *tn * ((B + 255) / 256) > 0x7fffffffu) return fail(ctx, InvalidInput, "B beyond the supported range");
    return riss_stream_range(ctx, domain, B, first_index);
}
// the two launches that stand where hbmpc_dev_riss_fold stands in the unseeded calls: drawn values are within the bound, so no verdict
ShareErrorCode riss_sample_fold_launches(hbmpc_ctx* ctx, const uint32_t* seeds_dev, size_t n, size_t tn, size_t domain, size_t B, uint64_t first_index,
                                         size_t lk_bits, uint64_t* sums, uint8_t* bad_or_null, hipStream_t s) {
    if (bad_or_null) HIP_TRY(ctx, hipMemsetAsync(bad_or_null, 0, n * tn, s));
    launch_riss_sample_fold(seeds_dev, (unsigned)n, (uint32_t)domain, tn, B, first_index, (uint64_t)1 << lk_bits, sums, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}

}  // namespace

extern "C" ShareErrorCode hbmpc_dev_riss_sample(hbmpc_ctx* ctx, const uint8_t seed[32], size_t n, size_t t, size_t domain, size_t B,
                                                uint64_t first_index, size_t lk_bits, uint64_t* out_dev, void* stream) {
    if (!ctx) return InvalidInput;
    size_t tn = 0;
    const ShareErrorCode rc = riss_seeded_shape(ctx, n, t, domain, B, first_index, lk_bits, &tn);
    if (rc != ShareSuccess) return rc;
    if (B == 0) return ShareSuccess;
    if (!seed || !out_dev) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t k[8];
    memcpy(k, seed, 32);  // little-endian words
    launch_riss_sample(k, (uint32_t)domain, tn, B, first_index, (uint64_t)1 << lk_bits, out_dev, pick(ctx, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
// host-pointer form: nothing goes in but the seed, the rows come back
extern "C" ShareErrorCode hbmpc_riss_sample(hbmpc_ctx* ctx, const uint8_t seed[32], size_t n, size_t t, size_t domain, size_t B, uint64_t first_index,
                                            size_t lk_bits, uint64_t* out) {
    if (!ctx) return InvalidInput;
    size_t tn = 0;
    ShareErrorCode rc = riss_seeded_shape(ctx, n, t, domain, B, first_index, lk_bits, &tn);
    if (rc != ShareSuccess) return rc;
    if (B == 0) return ShareSuccess;
    if (!seed || !out) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Stage st(ctx, tn * B * 8, 1);
    void* po = nullptr;
    HIP_TRY(ctx, st.alloc(tn * B * 8, &po));
    rc = hbmpc_dev_riss_sample(ctx, seed, n, t, domain, B, first_index, lk_bits, (uint64_t*)po, nullptr);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, st.out(out, po, tn * B * 8));
    HIP_TRY(ctx, st.finish());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_riss_sample_fold(hbmpc_ctx* ctx, const uint32_t* seeds_dev, size_t n, size_t t, size_t domain, size_t B,
                                                     uint64_t first_index, size_t lk_bits, uint64_t* sums_out, void* stream) {
    if (!ctx) return InvalidInput;
    size_t tn = 0;
    const ShareErrorCode rc = riss_seeded_shape(ctx, n, t, domain, B, first_index, lk_bits, &tn);
    if (rc != ShareSuccess) return rc;
    if (B == 0) return ShareSuccess;
    if (!seeds_dev || !sums_out) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return riss_sample_fold_launches(ctx, seeds_dev, n, tn, domain, B, first_index, lk_bits, sums_out, nullptr, pick(ctx, stream));
}

// PRandBit from the senders' seeds: sample_fold (domain 0), bad = zeros, then exactly the launches hbmpc_dev_prandbit_parties runs after
// its fold (prandbit_tail).  There is no one-launch form (k_prandbit_wg reads contrib): plan_prandbit is not consulted.
extern "C" ShareErrorCode hbmpc_dev_prandbit_parties_seeded(hbmpc_ctx* ctx_fr, hbmpc_ctx* ctx_gl, const uint32_t* seeds_dev, uint64_t first_index,
                                                            const uint64_t* b_q, size_t n, size_t t, size_t B, size_t lk_bits, size_t open_senders,
                                                            uint64_t* sums, uint8_t* bad, U256* r_p, uint8_t* r_2, uint64_t* r_q, uint64_t* rb,
                                                            uint64_t* y_ws, uint64_t* z_ws, uint64_t* opened, U256* b_p, uint8_t* b_2, uint8_t* rstatus,
                                                            hbmpc_recover_summary* summary_first, hbmpc_recover_summary* summary, void* stream) {
    if (!ctx_fr || !ctx_gl) return InvalidInput;
    REQ_FR(ctx_fr);
    REQ_GL(ctx_gl);
    if (ctx_fr->device != ctx_gl->device) return fail(ctx_fr, InvalidInput, "the two contexts are on different devices");
    size_t tn = 0;
    ShareErrorCode rc = prand_shape(ctx_fr, n, t, B, lk_bits, &tn);
    if (rc != ShareSuccess) return rc;
    if (B % (t + 1) != 0) return fail(ctx_fr, InvalidInput, "B must be a multiple of t + 1");  // prandbitd.rs:472-476
    const size_t S = open_senders ? open_senders : 2 * t + 1;
    if (S < 2 * t + 1 || S > n) return fail(ctx_fr, InvalidInput, "open_senders must be 0 or in 2t + 1 .. n");
    rc = riss_stream_range(ctx_fr, 0, B, first_index);
    if (rc != ShareSuccess) return rc;
    if (B == 0) return ShareSuccess;
    if (!seeds_dev || !b_q || !sums || !bad || !r_p || !r_2 || !r_q || !rb || !y_ws || !z_ws || !opened || !b_p || !b_2 || !rstatus)
        return fail(ctx_fr, InvalidInput, "null buffer");
    HIP_TRY(ctx_fr, hipSetDevice(ctx_fr->device));
    hipStream_t s = pick(ctx_fr, stream);  // the Goldilocks context's calls run on it too
    const PRandBitCall c{nullptr, b_q, n, t, B, lk_bits, sums, bad, r_p, r_2, r_q, rb, y_ws, z_ws, opened, b_p, b_2, rstatus, summary_first, summary, s};
    rc = riss_sample_fold_launches(ctx_fr, seeds_dev, n, tn, 0, B, first_index, lk_bits, sums, bad, s);
    return rc != ShareSuccess ? rc : prandbit_tail(ctx_fr, ctx_gl, c, S, s);
}
// PRandInt from the senders' seeds (domain 1): sample_fold, bad = zeros, the conversion over Fr
extern "C" ShareErrorCode hbmpc_dev_prandint_parties_seeded(hbmpc_ctx* ctx_fr, const uint32_t* seeds_dev, uint64_t first_index, size_t n, size_t t,
                                                            size_t B, size_t lk_bits, uint64_t* sums, uint8_t* bad, U256* r_p, void* stream) {
    if (!ctx_fr) return InvalidInput;
    REQ_FR(ctx_fr);
    size_t tn = 0;
    ShareErrorCode rc = prand_shape(ctx_fr, n, t, B, lk_bits, &tn);
    if (rc != ShareSuccess) return rc;
    rc = riss_stream_range(ctx_fr, 1, B, first_index);
    if (rc != ShareSuccess) return rc;
    if (B == 0) return ShareSuccess;
    if (!seeds_dev || !sums || !bad || !r_p) return fail(ctx_fr, InvalidInput, "null buffer");
    HIP_TRY(ctx_fr, hipSetDevice(ctx_fr->device));
    hipStream_t s = pick(ctx_fr, stream);
    rc = riss_sample_fold_launches(ctx_fr, seeds_dev, n, tn, 1, B, first_index, lk_bits, sums, bad, s);
    return rc != ShareSuccess ? rc : prandint_tail(ctx_fr, n, t, B, sums, r_p, s);
}
