// capi_pipelines_io.hip -- the Input, Output and BatchRecon handles behind the C ABI (hbmpc_pipe_input_create, hbmpc_pipe_output_create,
// hbmpc_pipe_batchrecon_create): the arena, the buffers by name and the capture rules of hbmpc_[gl_]dev_input_parties /
// hbmpc_[gl_]dev_output_parties / hbmpc_[gl_]dev_batchrecon_parties, so that a Rust node or any C caller gets them from the library.
//
//   input       the client's open of the masks, masked = x + mask, the servers' masked - r   honeybadger/input/input.rs:489-506, 85-100, 300-301
//   output      the client's open of the result shares                                        honeybadger/output/output.rs:157-177
//   batchrecon  the public open of a vector of shared values through both arms                honeybadger/batch_recon/batch_recon.rs:144-185, 371-391, 451-467
//
// Not here: sessions, RBC and the InputMessage / OutputMessage envelopes; the 48-byte Vec<RobustShare> and Vec<F> payloads
// (hbmpc_dev_unpack_shares / hbmpc_dev_pack_fvec convert them); sampling the masks (they are RanSha's outputs).
//
// A file of its own: capi_pipelines.hip is linked alone against stubs of every entry point it calls (tests/cpp/pipeline_calls_dump.cpp).
// Like it, this file is a CLIENT of the public header only (pipe_internal.hpp: struct hbmpc_pipe) and compiles with a host C++ compiler.
// The other hbmpc_pipe_* functions (buffer, upload, download, run, capture, replay, summary, destroy) are capi_pipelines.hip's and serve
// these handles too.
#include "pipe_internal.hpp"

namespace {

// what the two handles share: n parties, t faults, N values, parties 0 .. open_senders - 1 as the senders (0: 2t + 1)
struct ClientIo : hbmpc_pipe {
    size_t n, t, N;
    uint8_t* status = nullptr;
    std::vector<size_t> ids;
    ClientIo(hbmpc_ctx* cx, size_t n_, size_t t_, size_t N_, size_t open_senders, void* s) : hbmpc_pipe(cx, s), n(n_), t(t_), N(N_) {
        if (open_senders == 0) open_senders = 2 * t + 1;
        if (n == 0 || N == 0 || open_senders < 2 * t + 1 || open_senders > n) throw PipeError{InvalidInput};
        for (size_t i = 0; i < open_senders; ++i) ids.push_back(i);
    }
    void tail() {  // the status bytes and the summary close every arena
        status = take_bytes("status", N, N);
        summ = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary", 64, 16));
    }
};

// Input of N client values.  A mask that does not open refuses its element (zeros, never x + 0: hbmpc_dev_input_parties); checked
// mode then ends the run with the summary's error, where the reference's `?` would (input.rs:499-502).
struct Input : ClientIo {
    unsigned char *x, *r, *mask, *masked, *out;
    Input(hbmpc_ctx* cx, size_t n_, size_t t_, size_t N_, size_t open_senders, void* s) : ClientIo(cx, n_, t_, N_, open_senders, s) {
        arena((2 * n * N + 3 * N) * f.eb + N + (1 << 12));
        x = take("x", N), r = take("r", n * N);
        mask = take("mask", N), masked = take("masked", N), out = take("out", n * N);
        tail();
    }
    void run() override {
        // one launch for a small batch over Fr, two otherwise; checked mode looks at the open's summary afterwards
        if (f.gl)
            PL(hbmpc_gl_dev_input_parties(ctx, ids.data(), ids.size(), (const uint64_t*)x, (const uint64_t*)r, N, n, t, (uint64_t*)mask, (uint64_t*)masked,
                                          (uint64_t*)out, status, summ, stream));
        else
            PL(hbmpc_dev_input_parties(ctx, ids.data(), ids.size(), (const U256*)x, (const U256*)r, N, n, t, (U256*)mask, (U256*)masked, (U256*)out, status,
                                       summ, stream));
        check_summary(summ);
    }
};

// Output of N result values
struct Output : ClientIo {
    unsigned char *sh, *out;
    Output(hbmpc_ctx* cx, size_t n_, size_t t_, size_t N_, size_t open_senders, void* s) : ClientIo(cx, n_, t_, N_, open_senders, s) {
        arena((n * N + N) * f.eb + N + (1 << 12));
        sh = take("sh", n * N), out = take("out", N);
        tail();
    }
    void run() override {
        if (f.gl) PL(hbmpc_gl_dev_output_parties(ctx, ids.data(), ids.size(), (const uint64_t*)sh, N, n, t, (uint64_t*)out, status, summ, stream));
        else PL(hbmpc_dev_output_parties(ctx, ids.data(), ids.size(), (const U256*)sh, N, n, t, (U256*)out, status, summ, stream));
        check_summary(summ);
    }
};

// BatchRecon of N = G (d + 1) shared values of degree d.  run() is the device call; deal() and finish() are its two arms as separate
// launches (the encode and the recipients' decodes up to Z; the decode of Z), so that a caller can rewrite rows of Z in between.
// Checked mode ends at the first failing decode with its error.
struct BatchRecon : hbmpc_pipe {
    size_t n, t, d, N, G;
    unsigned char *x, *Y, *Z, *opened;
    uint8_t *rstatus, *status;
    hbmpc_recover_summary* summ_first;
    std::vector<size_t> ids1, ids2;
    BatchRecon(hbmpc_ctx* cx, size_t n_, size_t t_, size_t d_, size_t N_, size_t eval_senders, size_t reveal_senders, void* s)
        : hbmpc_pipe(cx, s), n(n_), t(t_), d(d_), N(N_) {
        if (eval_senders == 0) eval_senders = d + t + 1;
        if (reveal_senders == 0) reveal_senders = d + t + 1;
        if (n == 0 || n > 255 || d == 0 || N == 0 || N % (d + 1) != 0 || n < 3 * t + 1 || eval_senders < d + t + 1 || eval_senders > n ||
            reveal_senders < d + t + 1 || reveal_senders > n)
            throw PipeError{InvalidInput};
        G = N / (d + 1);
        for (size_t i = 0; i < eval_senders; ++i) ids1.push_back(i);
        for (size_t i = 0; i < reveal_senders; ++i) ids2.push_back(i);
        arena((n * N + n * n * G + n * G + N) * f.eb + n * G + G + (1 << 12));
        x = take("x", n * N), Y = take("Y", n * n * G), Z = take("Z", n * G), opened = take("opened", N);
        rstatus = take_bytes("rstatus", n * G, n * G), status = take_bytes("status", G, G);
        summ_first = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary_first", 64, 16));
        summ = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary", 64, 16));
    }
    void run() override {
        PL(f.batchrecon_parties(ctx, ids1.data(), ids1.size(), ids2.data(), ids2.size(), x, N, n, d, t, Y, Z, opened, rstatus, status, summ_first, summ,
                                stream));
        check_summary(summ_first);
        check_summary(summ);
    }
    void deal() override {
        PL(f.apply_parties(ctx, x, G, n, d, n, Y, stream));
        PL(f.recover_slots(ctx, ids1.data(), ids1.size(), Y, n * G, n * G, n, d, t, 1, Z, rstatus, summ_first, stream));
        check_summary(summ_first);
    }
    void finish() override {
        PL(f.recover_slots(ctx, ids2.data(), ids2.size(), Z, G, G, n, d, t, 0, opened, status, summ, stream));
        check_summary(summ);
    }
};

}  // namespace

extern "C" ShareErrorCode hbmpc_pipe_input_create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t open_senders, void* stream,
                                                  hbmpc_pipe** pipe_out) {
    return create<Input>(ctx, pipe_out, n, t, N, open_senders, stream);
}
extern "C" ShareErrorCode hbmpc_pipe_output_create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t open_senders, void* stream,
                                                   hbmpc_pipe** pipe_out) {
    return create<Output>(ctx, pipe_out, n, t, N, open_senders, stream);
}
extern "C" ShareErrorCode hbmpc_pipe_batchrecon_create(hbmpc_ctx* ctx, size_t n, size_t t, size_t d, size_t N, size_t eval_senders,
                                                       size_t reveal_senders, void* stream, hbmpc_pipe** pipe_out) {
    return create<BatchRecon>(ctx, pipe_out, n, t, d, N, eval_senders, reveal_senders, stream);
}
