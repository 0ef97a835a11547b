// capi_randbit.inc -- RandBit for all parties on this device (fpmul/rand_bit.rs:242-293, 197-220; honeybadger/mod.rs:1951-2086)
// (included at the end of hbmpc_capi.hip).

namespace {

// every buffer of the call, typed per field by the two entry points
struct RandBitCall {
    const void *a, *ta, *tb, *tc;
    size_t N, n, t;
    void *desh, *Y, *Z, *deop, *sq, *sqop, *out;
    uint8_t *status, *rst_de, *rst_sq;
    hbmpc_recover_summary *sm_de_first, *sm_de, *sm_sq_first, *sm_sq;
    hbmpc_randbit_summary* rb;
    void* stream;
};

// The nine launches.  Both opens are BatchRecon of degree t (N is a multiple of t + 1, so Multiply never takes the RBC path:
// mul/multiplication.rs:417-462): every party's encode of its chunks of t + 1, the recipients' P(0) decodes from senders 0 .. 2t, the
// coefficient decode of the revealed values from the same.
ShareErrorCode randbit_launches(hbmpc_ctx* ctx, const RandBitCall& c) {
    const size_t N = c.N, n = c.n, t = c.t, Gde = 2 * N / (t + 1), Gsq = N / (t + 1), eb = ebytes(ctx);
    const std::vector<size_t> ids = first_ids(2 * t + 1);
    // BatchRecon (degree t) of x [party][G (t + 1)] -> opened [G (t + 1)]: the three launches of capi_batchrecon.inc from senders 0 .. 2t
    auto open = [&](const void* x, size_t G, void* opened, uint8_t* st, hbmpc_recover_summary* first, hbmpc_recover_summary* second) -> ShareErrorCode {
        return batchrecon_launches(ctx, ids.data(), ids.size(), ids.data(), ids.size(), x, G, n, t, t, c.Y, c.Z, opened, st, st, first, second, c.stream, true);
    };
    // Multiply::init(a, a, triples): d = ta - a, e = tb - a (multiplication.rs:417-426), opened together
    ShareErrorCode rc = beaver_open_pair_any(ctx, c.ta, c.tb, c.a, c.a, N, n, c.desh, c.stream);
    if (rc != ShareSuccess) return rc;
    rc = open(c.desh, Gde, c.deop, c.rst_de, c.sm_de_first, c.sm_de);
    if (rc != ShareSuccess) return rc;
    // finalize_mul (multiplication.rs:57-100): [a^2] = tc - d e - d a - e a
    rc = beaver_finalize_any(ctx, c.tc, c.a, c.a, c.deop, (const unsigned char*)c.deop + N * eb, N, c.sq, c.stream, n);
    if (rc != ShareSuccess) return rc;
    rc = open(c.sq, Gsq, c.sqop, c.rst_sq, c.sm_sq_first, c.sm_sq);  // rand_bit.rs:281-290
    if (rc != ShareSuccess) return rc;
    return randbit_finalize_any(ctx, c.a, c.sqop, N, n, c.out, c.status, c.rb, c.stream);
}

// H: HFr or HGl.  All of the validation comes before the first launch or memset: a call that is refused has written nothing.
template <class H>
ShareErrorCode randbit_parties_any(hbmpc_ctx* ctx, const RandBitCall& c) {
    const size_t N = c.N, n = c.n, t = c.t;
    if (!c.a || !c.ta || !c.tb || !c.tc || !c.desh || !c.Y || !c.Z || !c.deop || !c.sq || !c.sqop || !c.out || !c.status || !c.rst_de || !c.rst_sq || !c.rb)
        return fail(ctx, InvalidInput, "null buffer");
    if (!batch_in_range(ctx, N, n)) return InvalidInput;
    if (t >= n || N % (t + 1) != 0) return fail(ctx, InvalidInput, "N must be a multiple of t + 1");  // rand_bit.rs:253-255
    if (n < 2 * t + 1) return fail(ctx, InvalidInput, "n must be >= 2t + 1");
    if (plan_protocol(protocol_knobs(ctx), {ProtocolCall::RandBit, N, n, t, 0, 0}).one_launch) {  // a workgroup per chunk of t + 1 elements (kernels_randbit_wg.hpp)
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick(ctx, c.stream);
        const int impl = ctx->impl;
        RandBitWgArgs ra;
        memset(&ra, 0, sizeof ra);
        ShareErrorCode rc = rec_table<H>(ctx, *domain_inv<H>(ctx, n), first_ids(2 * t + 1), n, t, t, &ra.tab);
        if (rc != ShareSuccess) return rc;
        rc = vmat_table<H>(ctx, n, t, &ra.vmat);
        if (rc != ShareSuccess) return rc;
        rc = sqrt_tab(ctx, &ra.st);
        if (rc != ShareSuccess) return rc;
        const ElemConsts cs = elem_consts(impl);
        memcpy(ra.r2, cs.r2, sizeof ra.r2);
        ra.a = as_words(c.a), ra.ta = as_words(c.ta), ra.tb = as_words(c.tb), ra.tc = as_words(c.tc);
        ra.desh = as_words(c.desh), ra.deop = as_words(c.deop), ra.sq = as_words(c.sq), ra.sqop = as_words(c.sqop), ra.out = as_words(c.out);
        ra.status = c.status, ra.rst_de = c.rst_de, ra.rst_sq = c.rst_sq, ra.rb = reinterpret_cast<RandBitSummaryDev*>(c.rb);
        ra.N = N, ra.n = (int)n, ra.t = (int)t;
        return enqueue_one_launch(ctx, s, &ra.counters, {{&ra.sm_de_first, c.sm_de_first}, {&ra.sm_de, c.sm_de}, {&ra.sm_sq_first, c.sm_sq_first}, {&ra.sm_sq, c.sm_sq}},
                                  [&]() -> ShareErrorCode {
                                      HIP_TRY(ctx, hipMemsetAsync(c.rb, 0xff, 8, s));  // first = all ones
                                      HIP_TRY(ctx, hipMemsetAsync((char*)c.rb + 8, 0, 8, s));
                                      launch_randbit_wg(impl, ra, s);
                                      return ShareSuccess;
                                  });
    }
    return randbit_launches(ctx, c);
}

}  // namespace

// The call is ONE launch (kernels_randbit_wg.hpp), or hbmpc_dev_beaver_open_shares_paired, the encode and the two decodes of d and
// e, hbmpc_dev_beaver_finalize_parties, the same three of a^2 and hbmpc_dev_randbit_finalize_parties -- the same bytes in every
// output buffer.  Which: plan_protocol (protocol_route.hpp).
#define TYPED_RANDBIT(T, H, REQ, PFX)                                                                                                          \
    extern "C" ShareErrorCode PFX##dev_randbit_parties(hbmpc_ctx* ctx, const T* a, const T* ta, const T* tb, const T* tc, size_t N, size_t n,   \
                                                       size_t t, T* desh_ws, T* y_ws, T* z_ws, T* de_opened, T* sq_out, T* sq_opened, T* out,   \
                                                       uint8_t* status, uint8_t* rstatus_de, uint8_t* rstatus_sq,                               \
                                                       hbmpc_recover_summary* summary_de_first, hbmpc_recover_summary* summary_de,              \
                                                       hbmpc_recover_summary* summary_sq_first, hbmpc_recover_summary* summary_sq,              \
                                                       hbmpc_randbit_summary* summary, void* stream) {                                          \
        if (!ctx) return InvalidInput;                                                                                                         \
        REQ(ctx);                                                                                                                              \
        return randbit_parties_any<H>(ctx, RandBitCall{a, ta, tb, tc, N, n, t, desh_ws, y_ws, z_ws, de_opened, sq_out, sq_opened, out, status, \
                                                       rstatus_de, rstatus_sq, summary_de_first, summary_de, summary_sq_first, summary_sq,     \
                                                       summary, stream});                                                                      \
    }
TYPED_RANDBIT(U256, HFr, REQ_FR, hbmpc_)
TYPED_RANDBIT(uint64_t, HGl, REQ_GL, hbmpc_gl_)
#undef TYPED_RANDBIT
