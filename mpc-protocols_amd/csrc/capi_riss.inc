// capi_riss.inc -- PRandBit / PRandInt entry points (kernels_riss.hpp, tables_riss.hpp); included by hbmpc_capi.hip.

// (n, t) of a supported shape: n >= 3t + 1, C(n, t) <= 8192 (the reference materialises every set too), table within RISS_MAX_ENTRIES
static ShareErrorCode riss_shape(hbmpc_ctx* ctx, size_t n, size_t t, size_t* tn_all) {
    if (n == 0 || n > (1u << 20) || t > n || n < 3 * t + 1) return fail(ctx, InvalidInput, "PRandBit needs n >= 3t + 1");
    const size_t c = riss_binomial(n, t, RISS_MAX_TSETS);
    if (c == SIZE_MAX) return fail(ctx, InvalidInput, "more than 8192 maximal unqualified sets: shape not supported");
    if (c * n > RISS_MAX_ENTRIES) return fail(ctx, InvalidInput, "coefficient table of C(n, t) n entries beyond the supported size");
    *tn_all = c;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_riss_tsets(size_t n, size_t t, size_t* ids_out, size_t* count_out) {
    if (!count_out || t > n) return InvalidInput;
    const size_t c = riss_binomial(n, t, RISS_MAX_TSETS);
    if (c == SIZE_MAX) return InvalidInput;
    *count_out = c;
    if (!ids_out) return ShareSuccess;
    size_t k = 0;
    for (const auto& T : riss_tsets(n, t))
        for (uint32_t m : T) ids_out[k++] = m;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_set_riss_form(hbmpc_ctx* ctx, int form) {
    if (!ctx || form < 0 || form > 2) return InvalidInput;
    ctx->riss_form = form;
    return ShareSuccess;
}

extern "C" ShareErrorCode hbmpc_dev_riss_fold(hbmpc_ctx* ctx, const uint64_t* contrib, size_t n, size_t Tn, size_t B, size_t lk_bits,
                                              uint64_t* sums_out, uint8_t* bad_out, void* stream) {
    if (!ctx) return InvalidInput;
    if (n == 0 || n > (1u << 20)) return fail(ctx, InvalidInput, "n beyond the supported range");
    // prandbitd.rs:506-517: k + l + 2 bits for b + ceil(log2 n) must stay below the smaller modulus' 64 bits
    if (lk_bits >= 64 || lk_bits + 2 + (size_t)ilog2(n) >= 64) return fail(ctx, HBMPC_FIELD_CAPACITY, "k + l + 2 + ceil(log2 n) reaches 64 bits");
    if (Tn == 0 || B == 0) return ShareSuccess;
    if (!contrib || !sums_out || !bad_out) return fail(ctx, InvalidInput, "null buffer");
    if (Tn > ((size_t)1 << 24) || Tn * ((B + 255) / 256) > 0x7fffffffu) return fail(ctx, InvalidInput, "Tn, B beyond the supported range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, hipMemsetAsync(bad_out, 0, n * Tn, s));
    launch_riss_fold(contrib, (unsigned)n, Tn, B, (uint64_t)1 << lk_bits, sums_out, bad_out, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}

// the coefficient table of (context, n, t) -- every set, a column per party -- or of one party's own sets
static ShareErrorCode riss_tab(hbmpc_ctx* ctx, size_t n, size_t t, size_t tn_all, long own, RissTab* tab, size_t* tn_out) {
    const int impl = ctx->impl;
    const size_t tn_own = own < 0 ? 0 : riss_binomial(n - 1, t, RISS_MAX_TSETS);
    const uint32_t* p = nullptr;
    ShareErrorCode rc;
    try {
        rc = get_table(ctx, key("riss", {n, t, (size_t)(own + 1)}, impl), [&] {
            RissLayout L;
            return impl == IMPL_GOLD ? build_riss_table<HGl>(n, t, own, impl, &L) : build_riss_table<HFr>(n, t, own, impl, &L);
        }, &p);
    } catch (const std::exception& e) {
        return fail(ctx, HBMPC_NO_DEVICE, e.what());
    }
    if (rc != ShareSuccess) return rc;
    const RissLayout L = riss_layout(impl, n, tn_all, tn_own, own);
    tab->coef = p + L.coef, tab->red = p + L.red, tab->coef2 = L.has2 ? p + L.coef2 : nullptr;
    tab->ncols = (unsigned)L.ncols;
    *tn_out = L.Tn;
    return ShareSuccess;
}
static ShareErrorCode riss_convert_any(hbmpc_ctx* ctx, const uint64_t* r, size_t n, size_t t, size_t B, const size_t* party_ids, size_t parties,
                                       int own_sets_only, void* out, uint8_t* out2, void* stream) {
    if (!ctx) return InvalidInput;
    size_t tn_all = 0;
    ShareErrorCode rc = riss_shape(ctx, n, t, &tn_all);
    if (rc != ShareSuccess) return rc;
    if (out2 && n > 255) return fail(ctx, InvalidInput, "the GF(2^8) domain holds at most 255 parties");  // Gf256Domain::new
    if (own_sets_only) {
        if (parties != 1 || !party_ids) return fail(ctx, InvalidInput, "the one-party form takes exactly one party id");
    } else if (!party_ids && parties != n) {
        return fail(ctx, InvalidInput, "party_ids == NULL means all n parties");
    }
    CHECK_PARTIES(parties);
    if (party_ids)
        for (size_t i = 0; i < parties; ++i)
            if (party_ids[i] >= n) return fail(ctx, InvalidInput, "party id out of range");
    if (B == 0) return ShareSuccess;
    if (!r || !out) return fail(ctx, InvalidInput, "null buffer");
    if ((B + 63) / 64 > 0x7fffffffu) return fail(ctx, InvalidInput, "B beyond the supported range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    RissTab tab;
    size_t Tn = 0;
    rc = riss_tab(ctx, n, t, tn_all, own_sets_only ? (long)party_ids[0] : -1, &tab, &Tn);
    if (rc != ShareSuccess) return rc;
    const uint32_t* cols = nullptr;
    if (party_ids && !own_sets_only) {  // the columns of a party subset: a small table of its own, keyed by the ids
        std::string k = "risscols:" + std::to_string(n);
        for (size_t i = 0; i < parties; ++i) k += ":" + std::to_string(party_ids[i]);
        rc = get_table(ctx, k, [&] {
            std::vector<uint32_t> w(parties);
            for (size_t i = 0; i < parties; ++i) w[i] = (uint32_t)party_ids[i];
            return w;
        }, &cols);
        if (rc != ShareSuccess) return rc;
    }
    if (Tn == 0) {  // t = 0 has the single empty set; Tn is never 0 for a valid shape
        return fail(ctx, InvalidInput, "no sets");
    }
    // A workgroup per 64 elements and party, its four waves each a slice of the sets, measured faster than a workgroup that serves 16
    // parties from one read of r at every size with many sets (n = 16, t = 5, 2^14 elements: 1.5-1.7 ms against 4.1 ms over Fr; the other
    // waves' reads of r hit the cache, and 16 parties per workgroup leave one wave per SIMD).  With only a few sets there is nothing to
    // slice: Goldilocks then takes the 16-party form (n = 4, t = 1, 2^20 elements: 0.038 ms against 0.072 ms; DESIGN.md section 4).
    const bool wide = ctx->riss_form == 1 || (ctx->riss_form == 0 && parties > 1 && ctx->impl == IMPL_GOLD && Tn < 64);
    launch_riss_convert(ctx->impl, wide, r, B, (unsigned)Tn, tab, cols, (unsigned)parties, as_words(out), out2, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_riss_convert_parties(hbmpc_ctx* ctx, const uint64_t* r, size_t n, size_t t, size_t B, const size_t* party_ids,
                                                         size_t parties, int own_sets_only, U256* out, uint8_t* out2_or_null, void* stream) {
    REQ_FR(ctx);
    return riss_convert_any(ctx, r, n, t, B, party_ids, parties, own_sets_only, out, out2_or_null, stream);
}
extern "C" ShareErrorCode hbmpc_gl_dev_riss_convert_parties(hbmpc_ctx* ctx, const uint64_t* r, size_t n, size_t t, size_t B, const size_t* party_ids,
                                                            size_t parties, int own_sets_only, uint64_t* out, uint8_t* out2_or_null, void* stream) {
    REQ_GL(ctx);
    return riss_convert_any(ctx, r, n, t, B, party_ids, parties, own_sets_only, out, out2_or_null, stream);
}
extern "C" ShareErrorCode hbmpc_dev_prandbit_finalize_parties(hbmpc_ctx* ctx, const uint64_t* opened, const U256* r_p, const uint8_t* r_2, size_t B,
                                                              size_t parties, U256* bp_out, uint8_t* b2_out, void* stream) {
    if (!ctx) return InvalidInput;
    REQ_FR(ctx);
    CHECK_PARTIES(parties);
    if (B == 0) return ShareSuccess;
    if (!opened || !r_p || !r_2 || !bp_out || !b2_out) return fail(ctx, InvalidInput, "null buffer");
    if ((B + 255) / 256 > 0x7fffffffu) return fail(ctx, InvalidInput, "B beyond the supported range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    launch_prandbit_finalize(ctx->impl, opened, as_words(r_p), r_2, B, (unsigned)parties, as_words(bp_out), b2_out, pick(ctx, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}

// host-pointer forms: inputs staged, outputs copied back
static ShareErrorCode riss_convert_host(hbmpc_ctx* ctx, const uint64_t* r, size_t n, size_t t, size_t B, const size_t* party_ids, size_t parties,
                                        int own_sets_only, void* out, uint8_t* out2) {
    if (!ctx) return InvalidInput;
    size_t tn = 0;
    ShareErrorCode rc = riss_shape(ctx, n, t, &tn);
    if (rc != ShareSuccess) return rc;
    if (own_sets_only) tn = riss_binomial(n - 1, t, RISS_MAX_TSETS);
    CHECK_PARTIES(parties);
    if (B == 0) return ShareSuccess;
    if (!r || !out) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t eb = ebytes(ctx);
    Stage st(ctx, tn * B * 8 + parties * B * (eb + 1), 3);
    void *pr = nullptr, *po = nullptr, *p2 = nullptr;
    HIP_TRY(ctx, st.in(r, tn * B * 8, &pr));
    HIP_TRY(ctx, st.alloc(parties * B * eb, &po));
    if (out2) HIP_TRY(ctx, st.alloc(parties * B, &p2));
    rc = riss_convert_any(ctx, (const uint64_t*)pr, n, t, B, party_ids, parties, own_sets_only, po, (uint8_t*)p2, nullptr);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, st.out(out, po, parties * B * eb));
    if (out2) HIP_TRY(ctx, st.out(out2, p2, parties * B));
    HIP_TRY(ctx, st.finish());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_riss_convert_parties(hbmpc_ctx* ctx, const uint64_t* r, size_t n, size_t t, size_t B, const size_t* party_ids,
                                                     size_t parties, int own_sets_only, U256* out, uint8_t* out2_or_null) {
    REQ_FR(ctx);
    return riss_convert_host(ctx, r, n, t, B, party_ids, parties, own_sets_only, out, out2_or_null);
}
extern "C" ShareErrorCode hbmpc_gl_riss_convert_parties(hbmpc_ctx* ctx, const uint64_t* r, size_t n, size_t t, size_t B, const size_t* party_ids,
                                                        size_t parties, int own_sets_only, uint64_t* out, uint8_t* out2_or_null) {
    REQ_GL(ctx);
    return riss_convert_host(ctx, r, n, t, B, party_ids, parties, own_sets_only, out, out2_or_null);
}
extern "C" ShareErrorCode hbmpc_prandbit_finalize_parties(hbmpc_ctx* ctx, const uint64_t* opened, const U256* r_p, const uint8_t* r_2, size_t B,
                                                          size_t parties, U256* bp_out, uint8_t* b2_out) {
    if (!ctx) return InvalidInput;
    REQ_FR(ctx);
    CHECK_PARTIES(parties);
    if (B == 0) return ShareSuccess;
    if (!opened || !r_p || !r_2 || !bp_out || !b2_out) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Stage st(ctx, B * 8 + 2 * parties * B * 33, 5);
    void *pv = nullptr, *prp = nullptr, *pr2 = nullptr, *pbp = nullptr, *pb2 = nullptr;
    HIP_TRY(ctx, st.in(opened, B * 8, &pv));
    HIP_TRY(ctx, st.in(r_p, parties * B * 32, &prp));
    HIP_TRY(ctx, st.in(r_2, parties * B, &pr2));
    HIP_TRY(ctx, st.alloc(parties * B * 32, &pbp));
    HIP_TRY(ctx, st.alloc(parties * B, &pb2));
    const ShareErrorCode rc = hbmpc_dev_prandbit_finalize_parties(ctx, (const uint64_t*)pv, (const U256*)prp, (const uint8_t*)pr2, B, parties,
                                                                  (U256*)pbp, (uint8_t*)pb2, nullptr);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, st.out(bp_out, pbp, parties * B * 32));
    HIP_TRY(ctx, st.out(b2_out, pb2, parties * B));
    HIP_TRY(ctx, st.finish());
    return ShareSuccess;
}
