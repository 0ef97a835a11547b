// capi_pipelines_riss.hip -- the PRandBit / PRandInt handles behind the C ABI (hbmpc_pipe_prandbit_create, hbmpc_pipe_prandint_create):
// the arena, the buffers by name and the capture rules of hbmpc_dev_prandbit_parties / hbmpc_dev_prandint_parties, so that a Rust
// node or any C caller gets them from the library.
//
//   prandbit   the fold, the RISS-to-Shamir conversion over Fr, GF(2^8) and Goldilocks, r + b, BatchRecon of degree t, try_finalize_bit
//              fpmul/prandbitd.rs:638-647, 667-684, 311-356, 437-446, 189-211 (driven by honeybadger/mod.rs:1951-2150)
//   prandint   the fold and the conversion over Fr                                fpmul/prandbitd.rs:667-684, 311-356
//
// A file of its own: capi_pipelines.hip is linked alone against stubs of every entry point it calls (tests/cpp/pipeline_calls_dump.cpp).
// Like it, this file is a CLIENT of the public header only (pipe_internal.hpp: struct hbmpc_pipe) and compiles with a host C++ compiler.
// The other hbmpc_pipe_* functions (buffer, upload, download, run, capture, replay, summary, destroy) are capi_pipelines.hip's and serve
// these handles too: a buffer here has an element size of its own (8, 32 or 1 byte), which upload / download count in.
//
// The seeded forms (hbmpc_pipe_prandbit_create_seeded, hbmpc_pipe_prandint_create_seeded; contract "hbmpc-riss-chacha20-v1") are the same
// handles with a buffer `seeds` ([n][32] bytes) where `contrib` was -- nothing of contrib's size is allocated -- and a stream index that
// run() uses and then advances by B (hbmpc_pipe_set_stream_index); they refuse capture().
#include "pipe_internal.hpp"

namespace {

size_t binomial(size_t n, size_t t) {  // C(n, t) of a shape hbmpc_riss_tsets accepts
    size_t c = 0;
    if (hbmpc_riss_tsets(n, t, nullptr, &c) != ShareSuccess) throw PipeError{InvalidInput};
    return c;
}

// PRandBit of B bits for n parties.  The handle's context is the Goldilocks one: the open's decode counters, which a replayed graph
// expects at zero, live in its scratch (hbmpc_graph_launch); g_capturing is per thread, so a capture covers both contexts.
struct PRandBit : hbmpc_pipe {
    hbmpc_ctx* fr;
    size_t n, t, B, lk, S, Tn, G;
    unsigned char *contrib, *b_q, *sums, *bad, *r_p, *r_2, *r_q, *rb, *Y, *Z, *opened, *b_p, *b_2, *rstatus;
    hbmpc_recover_summary* summ_first;  // the recipients' decodes' (summ: the revealed values')
    bool own_stream = false;
    const bool seeded;
    unsigned char* seeds = nullptr;
    uint64_t index = 0;  // seeded: the stream position of the next run()
    ~PRandBit() override {
        if (!own_stream) return;
        (void)hbmpc_stream_sync(ctx, stream);
        hbmpc_graph_destroy(graph), graph = nullptr;
        (void)hbmpc_stream_destroy(ctx, stream);  // through the Goldilocks context: the stream's scratch (the decode counters) is its
    }
    PRandBit(hbmpc_ctx* gl, hbmpc_ctx* fr_, size_t n_, size_t t_, size_t B_, size_t lk_, size_t S_, void* s, bool seeded_)
        : hbmpc_pipe(gl, s), fr(fr_), n(n_), t(t_), B(B_), lk(lk_), S(S_), seeded(seeded_) {
        if (!fr || hbmpc_field_of(fr) != Bls12_381Fr || hbmpc_field_of(gl) != Goldilocks64) throw PipeError{TypeMismatch};
        if (n == 0 || n > 255 || t >= n || n < 3 * t + 1 || B == 0 || B % (t + 1) != 0) throw PipeError{InvalidInput};  // prandbitd.rs:472-476
        if (S != 0 && (S < 2 * t + 1 || S > n)) throw PipeError{InvalidInput};
        // the call's own checks of the shape, the capacity rule and the two contexts' devices, now and not at the first run(): with
        // B = 0 it validates, enqueues nothing and touches no buffer
        PL(hbmpc_dev_prandbit_parties(fr, gl, nullptr, nullptr, n, t, 0, lk, S, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s));
        Tn = binomial(n, t), G = B / (t + 1);
        arena(((seeded ? 4 * n : n * Tn * B) + Tn * B + 3 * n * B + n * n * G + n * G + B) * 8 + 2 * n * B * 32 + n * Tn + 2 * n * B + n * G + (1 << 14));
        if (seeded) seeds = take_typed("seeds", n * 32, 1), contrib = nullptr;
        else contrib = take_typed("contrib", n * Tn * B, 8);
        b_q = take_typed("b_q", n * B, 8);
        sums = take_typed("sums", Tn * B, 8), bad = take_typed("bad", n * Tn, 1);
        r_p = take_typed("r_p", n * B, 32), r_2 = take_typed("r_2", n * B, 1), r_q = take_typed("r_q", n * B, 8), rb = take_typed("rb", n * B, 8);
        Y = take_typed("Y", n * n * G, 8);  // [party][recipient][chunk]: the encoded messages (the separate launches' workspace)
        Z = take_typed("Z", n * G, 8);      // [recipient][chunk]: the revealed values
        opened = take_typed("opened", B, 8), b_p = take_typed("b_p", n * B, 32), b_2 = take_typed("b_2", n * B, 1);
        rstatus = take_typed("rstatus", n * G, 1);
        take_bytes("summary", 64, 16), take_bytes("summary_first", 64, 16);
        buffers["summary"].eb = buffers["summary_first"].eb = 1;
        summ = reinterpret_cast<hbmpc_recover_summary*>(buffers["summary"].p);
        summ_first = reinterpret_cast<hbmpc_recover_summary*>(buffers["summary_first"].p);
        if (!stream) {  // the two contexts' own streams differ: without a caller's stream the handle works on one of its own (last: nothing below throws)
            PL(hbmpc_stream_create(ctx, &stream));
            own_stream = true;
        }
    }
    void before_capture() override {
        if (seeded) refuse_seeded_capture();
    }
    void set_stream_index(uint64_t i) override {
        if (!seeded) throw PipeError{InvalidInput};
        index = i;
    }
    void run() override {
        if (seeded) {  // the contributions are drawn at [index, index + B) of the senders' streams; a refused call leaves the index where it was
            PL(hbmpc_dev_prandbit_parties_seeded(fr, ctx, (const uint32_t*)seeds, index, (const uint64_t*)b_q, n, t, B, lk, S, (uint64_t*)sums, bad,
                                                 (U256*)r_p, r_2, (uint64_t*)r_q, (uint64_t*)rb, (uint64_t*)Y, (uint64_t*)Z, (uint64_t*)opened, (U256*)b_p,
                                                 b_2, rstatus, summ_first, summ, stream));
            index += B;
        } else {
            // one call for the whole protocol: one launch for a small batch, eight otherwise (hbmpc_dev_prandbit_parties)
            PL(hbmpc_dev_prandbit_parties(fr, ctx, (const uint64_t*)contrib, (const uint64_t*)b_q, n, t, B, lk, S, (uint64_t*)sums, bad, (U256*)r_p,
                                          r_2, (uint64_t*)r_q, (uint64_t*)rb, (uint64_t*)Y, (uint64_t*)Z, (uint64_t*)opened, (U256*)b_p, b_2, rstatus,
                                          summ_first, summ, stream));
        }
        check_summary(summ_first);
        check_summary(summ);
    }
};

// PRandInt of B integers for n parties (any B)
struct PRandInt : hbmpc_pipe {
    size_t n, t, B, lk, Tn;
    unsigned char *contrib, *sums, *bad, *r_p;
    const bool seeded;
    unsigned char* seeds = nullptr;
    uint64_t index = 0;  // seeded: the stream position of the next run()
    PRandInt(hbmpc_ctx* fr, size_t n_, size_t t_, size_t B_, size_t lk_, void* s, bool seeded_)
        : hbmpc_pipe(fr, s), n(n_), t(t_), B(B_), lk(lk_), seeded(seeded_) {
        if (hbmpc_field_of(fr) != Bls12_381Fr) throw PipeError{TypeMismatch};
        if (n == 0 || n > 255 || t >= n || n < 3 * t + 1 || B == 0) throw PipeError{InvalidInput};
        PL(hbmpc_dev_prandint_parties(fr, nullptr, n, t, 0, lk, nullptr, nullptr, nullptr, s));  // the call's own checks, now (B = 0: nothing runs)
        Tn = binomial(n, t);
        arena(((seeded ? 4 * n : n * Tn * B) + Tn * B) * 8 + n * B * 32 + n * Tn + (1 << 12));
        if (seeded) seeds = take_typed("seeds", n * 32, 1), contrib = nullptr;
        else contrib = take_typed("contrib", n * Tn * B, 8);
        sums = take_typed("sums", Tn * B, 8), bad = take_typed("bad", n * Tn, 1);
        r_p = take_typed("r_p", n * B, 32);
    }
    void before_capture() override {
        if (seeded) refuse_seeded_capture();
    }
    void set_stream_index(uint64_t i) override {
        if (!seeded) throw PipeError{InvalidInput};
        index = i;
    }
    void run() override {
        if (!seeded) {
            PL(hbmpc_dev_prandint_parties(ctx, (const uint64_t*)contrib, n, t, B, lk, (uint64_t*)sums, bad, (U256*)r_p, stream));
            return;
        }
        PL(hbmpc_dev_prandint_parties_seeded(ctx, (const uint32_t*)seeds, index, n, t, B, lk, (uint64_t*)sums, bad, (U256*)r_p, stream));
        index += B;
    }
};

}  // namespace

extern "C" ShareErrorCode hbmpc_pipe_prandbit_create(hbmpc_ctx* ctx_fr, hbmpc_ctx* ctx_gl, size_t n, size_t t, size_t B, size_t lk_bits,
                                                     size_t open_senders, void* stream, hbmpc_pipe** pipe_out) {
    if (pipe_out) *pipe_out = nullptr;
    if (!ctx_fr) return InvalidInput;
    return create<PRandBit>(ctx_gl, pipe_out, ctx_fr, n, t, B, lk_bits, open_senders, stream, false);
}
extern "C" ShareErrorCode hbmpc_pipe_prandbit_create_seeded(hbmpc_ctx* ctx_fr, hbmpc_ctx* ctx_gl, size_t n, size_t t, size_t B, size_t lk_bits,
                                                            size_t open_senders, void* stream, hbmpc_pipe** pipe_out) {
    if (pipe_out) *pipe_out = nullptr;
    if (!ctx_fr) return InvalidInput;
    return create<PRandBit>(ctx_gl, pipe_out, ctx_fr, n, t, B, lk_bits, open_senders, stream, true);
}
extern "C" ShareErrorCode hbmpc_pipe_prandint_create(hbmpc_ctx* ctx_fr, size_t n, size_t t, size_t B, size_t lk_bits, void* stream,
                                                     hbmpc_pipe** pipe_out) {
    if (pipe_out) *pipe_out = nullptr;
    return create<PRandInt>(ctx_fr, pipe_out, n, t, B, lk_bits, stream, false);
}
extern "C" ShareErrorCode hbmpc_pipe_prandint_create_seeded(hbmpc_ctx* ctx_fr, size_t n, size_t t, size_t B, size_t lk_bits, void* stream,
                                                            hbmpc_pipe** pipe_out) {
    if (pipe_out) *pipe_out = nullptr;
    return create<PRandInt>(ctx_fr, pipe_out, n, t, B, lk_bits, stream, true);
}
extern "C" ShareErrorCode hbmpc_pipe_set_stream_index(hbmpc_pipe* pipe, uint64_t index) {
    if (!pipe) return InvalidInput;
    return guarded([&] { pipe->set_stream_index(index); });
}
