// capi_shamir.inc -- the integer-point Shamir scheme (Shamirshare, common/share/shamir.rs:13-126): shares at the field elements
// F::from(id), recovery by plain Lagrange (included at the end of hbmpc_capi.hip).  The encode's route is decided in
// shamir_route.hpp; the interpolation feeds the batch decode's kernels a table built over the points (capi_recover.inc).

namespace {

bool shamir_point_is_zero(const hbmpc_ctx* ctx, uint64_t id) { return id == 0 || (is_gold(ctx) && id == HGl::P); }  // F::from(id) == 0
uint64_t shamir_point_field(const hbmpc_ctx* ctx, uint64_t id) { return is_gold(ctx) ? id % HGl::P : id; }         // below p over Fr already
bool shamir_has_duplicates(std::vector<uint64_t> v) {
    std::sort(v.begin(), v.end());
    return std::adjacent_find(v.begin(), v.end()) != v.end();
}
ShamirKnobs shamir_knobs(const hbmpc_ctx* ctx) { return ShamirKnobs{is_gold(ctx) ? 2 : 8, ctx->shamir_route, ctx->wide_max_chunks}; }
std::string shamir_key(const char* kind, const uint64_t* points, size_t m, size_t d, int impl) {
    std::string k = kind;
    k += ":" + std::to_string(d) + ":";
    for (size_t i = 0; i < m; ++i) k += std::to_string(points[i]) + ",";
    return k + "#" + std::to_string(impl);
}

// compute_shares' checks in the reference's order (shamir.rs:51-70)
ShareErrorCode shamir_check_encode(hbmpc_ctx* ctx, const uint64_t* points, size_t m, size_t d) {
    if (!points) return fail(ctx, InvalidInput, "no ids");                                                 // :51-54
    if (m < d + 1) return fail(ctx, InsufficientShares, "fewer ids than degree + 1");                      // :57-59
    for (size_t i = 0; i < m; ++i)
        if (shamir_point_is_zero(ctx, points[i])) return fail(ctx, InvalidInput, "an id maps to the zero field element");  // :62-64
    if (shamir_has_duplicates(std::vector<uint64_t>(points, points + m))) return fail(ctx, InvalidInput, "duplicate ids");  // :67-70
    if (m > (1u << 20) || d > (1u << 20)) return fail(ctx, InvalidInput, "m, d beyond the supported range");
    return ShareSuccess;
}

ShareErrorCode shamir_encode_dev(hbmpc_ctx* ctx, const void* coeffs, size_t B, const uint64_t* points, size_t m, size_t d, void* out,
                                 void* stream) {
    if (!ctx) return InvalidInput;
    ShareErrorCode rc = shamir_check_encode(ctx, points, m, d);
    if (rc != ShareSuccess) return rc;
    if (B == 0) return ShareSuccess;
    if (!coeffs || !out) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    const int impl = ctx->impl;
    const ShamirPlan plan = plan_shamir_encode(shamir_knobs(ctx), m, d, B, points);
    if (plan.kernel == ShamirKernel::SmallWeight) {
        const uint32_t* w;
        rc = get_table(ctx, shamir_key("shamir-w", points, m, d, impl), [&] {
            std::vector<uint32_t> words;  // w[i][k] = points[i]^k, 64-bit little-endian
            for (size_t i = 0; i < m; ++i) {
                uint64_t p = 1;
                for (size_t k = 0; k <= d; ++k) {
                    words.push_back((uint32_t)p);
                    words.push_back((uint32_t)(p >> 32));
                    if (k < d) p *= points[i];  // below 2^64 up to points[i]^d: the route's condition
                }
            }
            return words;
        }, &w);
        if (rc != ShareSuccess) return rc;
        launch_shamir_encode(is_gold(ctx) ? 2 : 8, plan.w32, coeffs, B, (int)m, (int)(d + 1), (const uint64_t*)w, out, plan.waves, plan.lds_bytes,
                             (int)plan.row_units, s);
    } else {
        const uint32_t* alpha;  // the points in device-constant form, where the domain encode has omega^j
        rc = get_table(ctx, shamir_key("shamir-alpha", points, m, 0, impl), [&] {
            std::vector<uint32_t> words;
            for (size_t i = 0; i < m; ++i) {
                if (is_gold(ctx)) put_const(words, HGl::from_u64(points[i]), impl);
                else put_const(words, HFr::from_u64(points[i]), impl);
            }
            return words;
        }, &alpha);
        if (rc != ShareSuccess) return rc;
        const EvalOut y{(uint32_t*)out, 0, 1};
        if (plan.kernel == ShamirKernel::Wide) launch_eval_wide(impl, (const uint32_t*)coeffs, B, (int)m, (int)(d + 1), alpha, y, s);
        else launch_eval_generic(impl, (const uint32_t*)coeffs, B, (int)m, (int)(d + 1), alpha, y, s);
    }
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}

ShareErrorCode shamir_encode_host(hbmpc_ctx* ctx, const void* coeffs, size_t B, const uint64_t* points, size_t m, size_t d, void* out) {
    if (!ctx) return InvalidInput;
    ShareErrorCode rc = shamir_check_encode(ctx, points, m, d);
    if (rc != ShareSuccess) return rc;
    if (B == 0) return ShareSuccess;
    if (!coeffs || !out) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t eb = ebytes(ctx);
    Stage st(ctx, B * (d + 1 + m) * eb, 2);
    void *dx, *dy;
    HIP_TRY(ctx, st.in(coeffs, B * (d + 1) * eb, &dx));
    HIP_TRY(ctx, st.alloc(B * m * eb, &dy));
    rc = shamir_encode_dev(ctx, dx, B, points, m, d, dy, nullptr);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, st.out(out, dy, B * m * eb));
    HIP_TRY(ctx, st.finish());
    return ShareSuccess;
}

// the point checks of an interpolation: the reference's (shamir.rs:94-110 and common/mod.rs:141-144, without the degree checks, which
// the batched form leaves to the caller), then this library's bound on S
ShareErrorCode shamir_check_points(hbmpc_ctx* ctx, const uint64_t* points, size_t S) {
    std::vector<uint64_t> v(points, points + S);
    if (shamir_has_duplicates(v)) return fail(ctx, InvalidInput, "duplicate ids");                                              // :97-100
    for (size_t i = 0; i < S; ++i)
        if (shamir_point_is_zero(ctx, points[i])) return fail(ctx, InvalidInput, "an id maps to the zero field element");        // :108-113
    for (uint64_t& x : v) x = shamir_point_field(ctx, x);
    if (shamir_has_duplicates(v)) return fail(ctx, InvalidInput, "two ids map to the same field element");                       // mod.rs:141-144
    if (S > 255) return fail(ctx, InvalidInput, "more than 255 points");
    return ShareSuccess;
}

ShareErrorCode shamir_interpolate_dev(hbmpc_ctx* ctx, const uint64_t* points, size_t S, const void* evals_dev, size_t row_stride, size_t G,
                                      void* coeffs_out_dev, uint32_t* degree_out_dev, void* stream, void* c0_out_dev = nullptr) {
    if (!ctx) return InvalidInput;
    if (S == 0 || G == 0) return fail(ctx, InvalidInput, "empty input");  // :91-93
    if (!points || !evals_dev || !coeffs_out_dev) return fail(ctx, InvalidInput, "null buffer");
    const ShareErrorCode rc = shamir_check_points(ctx, points, S);
    if (rc != ShareSuccess) return rc;
    return batch_interpolate_dev(ctx, nullptr, S, evals_dev, row_stride, G, S, coeffs_out_dev, degree_out_dev, stream, c0_out_dev, points);
}

ShareErrorCode shamir_interpolate_host(hbmpc_ctx* ctx, const uint64_t* points, size_t S, const void* evals, size_t G, void* coeffs_out,
                                       uint32_t* degree_out) {
    if (!ctx) return InvalidInput;
    if (S == 0 || G == 0) return fail(ctx, InvalidInput, "empty input");
    if (!points || !evals || !coeffs_out) return fail(ctx, InvalidInput, "null buffer");
    ShareErrorCode rc = shamir_check_points(ctx, points, S);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t eb = ebytes(ctx);
    Stage stg(ctx, 2 * S * G * eb + G * 4, 3);
    void *de, *dc, *dd;
    HIP_TRY(ctx, stg.in(evals, S * G * eb, &de));
    HIP_TRY(ctx, stg.alloc(S * G * eb, &dc));
    HIP_TRY(ctx, stg.alloc(G * 4, &dd));
    rc = shamir_interpolate_dev(ctx, points, S, de, G, G, dc, (uint32_t*)dd, nullptr);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, stg.out(coeffs_out, dc, S * G * eb));
    HIP_TRY(ctx, stg.out(degree_out, dd, G * 4));
    HIP_TRY(ctx, stg.finish());
    return ShareSuccess;
}

template <class H>
std::vector<uint32_t> shamir_lagrange_rows(const uint64_t* ids, size_t S, int impl) {
    std::vector<H> xs(S);
    for (size_t i = 0; i < S; ++i) xs[i] = H::from_u64(ids[i]);
    const auto basis = lagrange_basis(xs);
    std::vector<uint32_t> lb;
    for (size_t k = 0; k < S; ++k)
        for (size_t j = 0; j < S; ++j) put_const(lb, basis[j][k], impl);
    return lb;
}

// Shamirshare::recover_secret for one polynomial (shamir.rs:90-125), the checks in its order
ShareErrorCode shamir_recover_any(hbmpc_ctx* ctx, const uint64_t* ids, const size_t* degrees, const void* vals, size_t S, void* coeffs_out,
                                  size_t* ncoeffs_out, void* secret_out) {
    if (!ctx) return InvalidInput;
    if (S == 0) return fail(ctx, InvalidInput, "no shares");  // :91-93
    if (!ids || !degrees || !vals || !coeffs_out || !ncoeffs_out || !secret_out) return fail(ctx, InvalidInput, "null");
    std::vector<uint64_t> v(ids, ids + S);
    if (shamir_has_duplicates(v)) return fail(ctx, InvalidInput, "duplicate ids");  // :94-97
    const size_t deg = degrees[0];
    for (size_t i = 0; i < S; ++i)
        if (degrees[i] != deg) return fail(ctx, DegreeMismatch, "mismatch degree between shares");  // :98-101
    if (S < deg + 1) return fail(ctx, InsufficientShares, "insufficient shares");                   // :102-104
    for (size_t i = 0; i < S; ++i)
        if (shamir_point_is_zero(ctx, ids[i])) return fail(ctx, InvalidInput, "an id maps to the zero field element");  // :105-110
    for (uint64_t& x : v) x = shamir_point_field(ctx, x);
    if (shamir_has_duplicates(v)) return fail(ctx, InvalidInput, "two ids map to the same field element");  // mod.rs:141-144
    if (S > 4096) return fail(ctx, InvalidInput, "too many shares");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int impl = ctx->impl;
    const size_t eb = ebytes(ctx);
    const std::vector<uint32_t> lb = impl == IMPL_GOLD ? shamir_lagrange_rows<HGl>(ids, S, impl) : shamir_lagrange_rows<HFr>(ids, S, impl);
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
    if (degree > deg) return fail(ctx, DegreeMismatch, "interpolated degree exceeds the share degree");  // :120-122
    // the reference indexes result_poly[0] (a panic for the zero polynomial): zero is returned here
    *ncoeffs_out = emit_trimmed(co, len, eb, coeffs_out, secret_out);
    return ShareSuccess;
}

}  // namespace

#define TYPED_SHAMIR(T, REQ, PFX)                                                                                                  \
    extern "C" ShareErrorCode PFX##dev_shamir_compute_shares(hbmpc_ctx* ctx, const T* coeffs_dev, size_t B, const uint64_t* points, \
                                                             size_t m, size_t d, T* shares_out_dev, void* stream) {                \
        REQ(ctx);                                                                                                                  \
        return shamir_encode_dev(ctx, coeffs_dev, B, points, m, d, shares_out_dev, stream);                                        \
    }                                                                                                                              \
    extern "C" ShareErrorCode PFX##shamir_compute_shares(hbmpc_ctx* ctx, const T* coeffs, size_t B, const uint64_t* points, size_t m, \
                                                         size_t d, T* shares_out) {                                                \
        REQ(ctx);                                                                                                                  \
        return shamir_encode_host(ctx, coeffs, B, points, m, d, shares_out);                                                       \
    }                                                                                                                              \
    extern "C" ShareErrorCode PFX##shamir_recover_secret(hbmpc_ctx* ctx, const uint64_t* ids, const size_t* degrees, const T* vals, \
                                                         size_t S, T* coeffs_out, size_t* ncoeffs_out, T* secret_out) {            \
        REQ(ctx);                                                                                                                  \
        return shamir_recover_any(ctx, ids, degrees, vals, S, coeffs_out, ncoeffs_out, secret_out);                                \
    }                                                                                                                              \
    extern "C" ShareErrorCode PFX##shamir_batch_interpolate(hbmpc_ctx* ctx, const uint64_t* points, size_t S, const T* evals, size_t G, \
                                                            T* coeffs_out, uint32_t* degree_out) {                                 \
        REQ(ctx);                                                                                                                  \
        return shamir_interpolate_host(ctx, points, S, evals, G, coeffs_out, degree_out);                                          \
    }                                                                                                                              \
    extern "C" ShareErrorCode PFX##dev_shamir_batch_interpolate(hbmpc_ctx* ctx, const uint64_t* points, size_t S, const T* evals_dev, \
                                                                size_t row_stride, size_t G, T* coeffs_out_dev,                    \
                                                                uint32_t* degree_out_dev, void* stream) {                          \
        REQ(ctx);                                                                                                                  \
        return shamir_interpolate_dev(ctx, points, S, evals_dev, row_stride, G, coeffs_out_dev, degree_out_dev, stream);           \
    }                                                                                                                              \
    extern "C" ShareErrorCode PFX##dev_shamir_batch_interpolate_c0(hbmpc_ctx* ctx, const uint64_t* points, size_t S, const T* evals_dev, \
                                                                   size_t row_stride, size_t G, T* tmp_coeffs_dev, T* c0_out_dev,  \
                                                                   uint32_t* degree_out_dev, void* stream) {                       \
        REQ(ctx);                                                                                                                  \
        if (ctx && (!c0_out_dev || !degree_out_dev)) return fail(ctx, InvalidInput, "null buffer");                                \
        return shamir_interpolate_dev(ctx, points, S, evals_dev, row_stride, G, tmp_coeffs_dev, degree_out_dev, stream, c0_out_dev); \
    }
TYPED_SHAMIR(U256, REQ_FR, hbmpc_)
TYPED_SHAMIR(uint64_t, REQ_GL, hbmpc_gl_)

// test and sweep aid: SHAMIR_ROUTE_* (0 = the planner's rule, 1 = the small-weight kernel wherever it covers the call, 2 = never)
extern "C" ShareErrorCode hbmpc_set_shamir_route(hbmpc_ctx* ctx, int route) {
    if (!ctx) return InvalidInput;
    if (route < 0 || route > 2) return fail(ctx, InvalidInput, "route must be 0, 1 or 2");
    ctx->shamir_route = route;
    return ShareSuccess;
}
// test aid: the kernel plan_shamir_encode picks for a call on this context (1 small-weight, 2 wave per secret, 3 lane per secret)
extern "C" ShareErrorCode hbmpc_shamir_route(hbmpc_ctx* ctx, const uint64_t* points, size_t m, size_t d, size_t B, int* kernel_out) {
    if (!ctx) return InvalidInput;
    if (!kernel_out) return fail(ctx, InvalidInput, "null buffer");
    const ShareErrorCode rc = shamir_check_encode(ctx, points, m, d);
    if (rc != ShareSuccess) return rc;
    *kernel_out = (int)plan_shamir_encode(shamir_knobs(ctx), m, d, B, points).kernel;
    return ShareSuccess;
}
