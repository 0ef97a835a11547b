// hbmpc_pipelines.hpp -- C++ convenience over the hbmpc_pipe_* handles of hbmpc_hip.h (csrc/capi_pipelines.hip): device-resident
// replays of the reference's arithmetic pipelines for ALL n simulated parties on one GPU (how every reference test and bench
// runs: n parties in one process on FakeNetwork).  The call sequencing, the arena layout and the capture rules live in the
// LIBRARY, behind the C ABI; this header only gives the handles RAII, exceptions and typed buffer access.  The same wrappers
// exist in Python (mpc-protocols_amd/pipelines.py) and for Rust (rust/gpu_shares.rs).
//
//   TripleGen      TripleGenNode::init_batch + BatchReconNode (degree 2t) + try_finalize_triple_gen
//                  triple_gen/triple_generation.rs:304-364,164-232; batch_recon/batch_recon.rs:144-185,332-481
//   FpMul          FPMulNode::init = Multiply (Beaver, RBC path) + TruncPrNode
//                  fpmul/fpmul.rs:61-110, mul/multiplication.rs:417-426,57-139, fpmul/truncpr.rs:185-318
//   Mul            Multiply (Beaver, RBC path): the opened shares, the open, finalize_mul
//                  honeybadger/mod.rs:543-628, mul/multiplication.rs:417-426,102-139,57-100
//   Input          the client's open of the masks, masked = x + mask, the servers' masked - r
//                  honeybadger/input/input.rs:489-506, 85-100, 300-301
//   BatchRecon     the public open of a vector of shared values through both arms  batch_recon/batch_recon.rs:144-185, 371-391, 451-467
//   Output         the client's open of the result shares                           honeybadger/output/output.rs:157-177
//   TruncPr        TruncPrNode on its own                                           fpmul/truncpr.rs:185-318
//   FpDivConst     FPDivConstNode: a * w for a public reciprocal w, then TruncPr    fpdiv/fpdiv_const.rs:61-99, fpdiv/mod.rs:8-60
//   RanSha         RanShaNode: deal, n x n Vandermonde, verifier reconstruction + degree test, output slice
//                  share_gen/share_gen.rs:232-289,401-454,516-530,199-203
//   RanDouSha      DouShaNode deal + RanDouShaNode: both Vandermonde products, verifier interpolations + tests, output slice
//                  double_share/double_share_generation.rs:151-215, ran_dou_sha/mod.rs:371-449,569-602,314-331
//   Preprocessing  run_preprocessing's triple part (honeybadger/mod.rs:1239-1393): RanSha -> a, b; RanDouSha -> r; TripleGen
//   PRandIntPipe   fold of the RISS contributions, conversion to Fr shares      fpmul/prandbitd.rs:667-684,311-356
//   PRandBitPipe   ... and to Goldilocks and GF(2^8), open r + b, finalize      fpmul/prandbitd.rs:311-356,437-446,189-211
//                  (handles of csrc/capi_pipelines_riss.hip over an Fr and a Goldilocks context; PRandInt / PRandBit below are the
//                  compositions of eight device calls with the prepare() / finish() seam)
//   FixedPrep      run_preprocessing's steps 5 and 6: the PRandBit / PRandInt pools and take()   honeybadger/mod.rs:1396-1410,1951-2150
//                  (the handle of csrc/capi_pipelines_fixedprep.hip over the same two contexts)
//
// run() only ENQUEUES on the stream; capture() records the same call sequence into a HIP graph after two eager runs and
// replay() launches it -- at the batch sizes the protocols really use that removes the launch overhead that dominates.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "hbmpc_hip.h"

namespace hbmpc {

inline void pl_check(ShareErrorCode rc, hbmpc_ctx* ctx, const char* what) {
    if (rc != ShareSuccess) throw std::runtime_error(std::string(what) + " -> " + std::to_string((int)rc) + ": " + hbmpc_last_error(ctx));
}

class Pipeline {
  public:
    Pipeline(const Pipeline&) = delete;
    Pipeline& operator=(const Pipeline&) = delete;
    virtual ~Pipeline() {
        if (owned_) hbmpc_pipe_destroy(h_);
    }
    // a named device buffer of the pipeline (see the list in hbmpc_hip.h), e.g. buffer("a"), buffer("out")
    U256* buffer(const char* name, size_t* elements = nullptr) const {
        void* p = nullptr;
        pl_check(hbmpc_pipe_buffer(h_, name, &p, elements), ctx_, name);
        return static_cast<U256*>(p);
    }
    void upload(const char* name, const U256* src, size_t elements) { pl_check(hbmpc_pipe_upload(h_, name, src, elements), ctx_, name); }
    void download(const char* name, U256* dst, size_t elements) { pl_check(hbmpc_pipe_download(h_, name, dst, elements), ctx_, name); }
    // the same by device pointer (any position inside a buffer), on the pipeline's stream; download synchronises
    void upload(U256* dst_dev, const U256* src, size_t elements) {
        pl_check(hbmpc_memcpy_h2d(ctx_, dst_dev, src, elements * sizeof(U256), stream_), ctx_, "h2d");
    }
    void download(U256* dst, const U256* src_dev, size_t elements) {
        pl_check(hbmpc_memcpy_d2h(ctx_, dst, src_dev, elements * sizeof(U256), stream_), ctx_, "d2h");
        sync();
    }
    void run(bool checked = false) {  // enqueue only; checked: the summary is read back after every decode
        pl_check(hbmpc_pipe_set_checked(h_, checked ? 1 : 0), ctx_, "set_checked");
        pl_check(hbmpc_pipe_run(h_), ctx_, "run");
    }
    void capture() { pl_check(hbmpc_pipe_capture(h_), ctx_, "capture"); }
    void replay() { pl_check(hbmpc_pipe_replay(h_), ctx_, "replay"); }
    void sync() { pl_check(hbmpc_pipe_sync(h_), ctx_, "sync"); }
    hbmpc_recover_summary last_summary() {  // of the last decode: {n_fallback, n_failed, first_failed, first_error}
        hbmpc_recover_summary s;
        pl_check(hbmpc_pipe_summary(h_, &s), ctx_, "summary");
        return s;
    }
    hbmpc_pipe* handle() const { return h_; }

  protected:
    Pipeline(hbmpc_ctx* ctx, hbmpc_pipe* h, void* stream, bool owned = true) : ctx_(ctx), h_(h), stream_(stream), owned_(owned) {}
    hbmpc_ctx* ctx_;
    hbmpc_pipe* h_;
    void* stream_;
    bool owned_;
};

// n parties, threshold t, N triples (a multiple of 2t+1).  Buffers a, b, r2t, rt (inputs), c (output): [party][N].
class TripleGen : public Pipeline {
  public:
    TripleGen(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream) : Pipeline(ctx, create(ctx, n, t, N, stream), stream) { bind(); }
    TripleGen(hbmpc_ctx* ctx, hbmpc_pipe* borrowed, void* stream) : Pipeline(ctx, borrowed, stream, false) { bind(); }
    U256 *a, *b, *r2t, *rt, *c;

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream) {
        hbmpc_pipe* h = nullptr;
        pl_check(hbmpc_pipe_triplegen_create(ctx, n, t, N, stream, &h), ctx, "hbmpc_pipe_triplegen_create");
        return h;
    }
    void bind() { a = buffer("a"), b = buffer("b"), r2t = buffer("r2t"), rt = buffer("rt"), c = buffer("c"); }
};

// Fixed-point multiplication of N element pairs for n parties: Beaver mul + TruncPr with k-bit values and m fractional bits.
// open_senders: how many parties' shares an open interpolates from (0 = the reference's 2t+1).
class FpMul : public Pipeline {
  public:
    FpMul(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t k, size_t m, void* stream, size_t open_senders = 0)
        : Pipeline(ctx, create(ctx, n, t, N, k, m, open_senders, stream), stream) {
        x = buffer("x"), y = buffer("y"), ta = buffer("ta"), tb = buffer("tb"), tc = buffer("tc"), rint = buffer("rint"), rbits = buffer("rbits");
        z = buffer("z"), out = buffer("out");
    }
    U256 *x, *y, *ta, *tb, *tc, *rint, *rbits, *z, *out;  // [party][N] (rbits: [party][bit][N])

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t k, size_t m, size_t open_senders, void* stream) {
        hbmpc_pipe* h = nullptr;
        pl_check(hbmpc_pipe_fpmul_create(ctx, n, t, N, k, m, open_senders, stream, &h), ctx, "hbmpc_pipe_fpmul_create");
        return h;
    }
};

// Multiply (Beaver; honeybadger/mod.rs:543-628) of N element pairs for n parties over Fr: out = the parties' shares of x * y from one
// triple (ta, tb, tc) per pair.  open_senders as in FpMul.  (A Goldilocks context takes the same handle through the C ABI; this
// class names its buffers as U256.)
class Mul : public Pipeline {
  public:
    Mul(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream, size_t open_senders = 0)
        : Pipeline(ctx, create(ctx, n, t, N, open_senders, stream), stream) {
        x = buffer("x"), y = buffer("y"), ta = buffer("ta"), tb = buffer("tb"), tc = buffer("tc"), out = buffer("out");
        desh = buffer("desh"), deop = buffer("deop"), dop = buffer("dop"), eop = buffer("eop");
    }
    U256 *x, *y, *ta, *tb, *tc, *out;  // [party][N]
    U256 *desh, *deop, *dop, *eop;     // [party][2][N]; [2 N] the opened ta - x then tb - y; dop, eop: its halves

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t open_senders, void* stream) {
        hbmpc_pipe* h = nullptr;
        pl_check(hbmpc_pipe_mul_create(ctx, n, t, N, open_senders, stream, &h), ctx, "hbmpc_pipe_mul_create");
        return h;
    }
};

// Input (honeybadger/input/input.rs:489-506, 85-100, 300-301) of N client values for n parties over Fr: out = the parties' shares of
// x from one random mask per value, whose shares r the caller uploads.  An element whose mask does not open is refused (zeros in
// mask, masked and out); a checked run() then throws.  open_senders as in FpMul.  (A Goldilocks context takes the same handle through
// the C ABI; this class names its buffers as U256.)
class Input : public Pipeline {
  public:
    Input(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream, size_t open_senders = 0)
        : Pipeline(ctx, create(ctx, n, t, N, open_senders, stream), stream) {
        x = buffer("x"), r = buffer("r"), mask = buffer("mask"), masked = buffer("masked"), out = buffer("out");
    }
    U256 *x, *mask, *masked;  // [N]
    U256 *r, *out;            // [party][N]

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t open_senders, void* stream) {
        hbmpc_pipe* h = nullptr;
        pl_check(hbmpc_pipe_input_create(ctx, n, t, N, open_senders, stream, &h), ctx, "hbmpc_pipe_input_create");
        return h;
    }
};

// Output (honeybadger/output/output.rs:157-177) of N result values from the n parties' shares sh over Fr: out = what they open to.
class Output : public Pipeline {
  public:
    Output(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream, size_t open_senders = 0)
        : Pipeline(ctx, create(ctx, n, t, N, open_senders, stream), stream) {
        sh = buffer("sh"), out = buffer("out");
    }
    U256* sh;   // [party][N]
    U256* out;  // [N]

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t open_senders, void* stream) {
        hbmpc_pipe* h = nullptr;
        pl_check(hbmpc_pipe_output_create(ctx, n, t, N, open_senders, stream, &h), ctx, "hbmpc_pipe_output_create");
        return h;
    }
};

// BatchRecon (honeybadger/batch_recon/batch_recon.rs:144-185, 371-391, 451-467) of N = G (d + 1) shared values of degree d for n parties
// over Fr: opened = the N values, through the reference's two arms.  eval_senders / reveal_senders: parties 0 .. S - 1 whose messages
// everyone decodes from (0 = d + t + 1).  deal() / finish() are the two arms as separate launches: rows of Z may be rewritten in
// between.  A checked run() throws at the first failing decode.  (A Goldilocks context takes the same handle through the C ABI; this
// class names its buffers as U256.)
class BatchRecon : public Pipeline {
  public:
    BatchRecon(hbmpc_ctx* ctx, size_t n, size_t t, size_t d, size_t N, void* stream, size_t eval_senders = 0, size_t reveal_senders = 0)
        : Pipeline(ctx, create(ctx, n, t, d, N, eval_senders, reveal_senders, stream), stream) {
        x = buffer("x"), Y = buffer("Y"), Z = buffer("Z"), opened = buffer("opened");
        rstatus = reinterpret_cast<uint8_t*>(buffer("rstatus")), status = reinterpret_cast<uint8_t*>(buffer("status"));
    }
    U256* x;                    // [party][N]
    U256 *Y, *Z, *opened;       // [party][recipient][G]; [recipient][G]; [N]
    uint8_t *rstatus, *status;  // [n G], [G]
    void deal(bool checked = false) {
        pl_check(hbmpc_pipe_set_checked(h_, checked ? 1 : 0), ctx_, "set_checked");
        pl_check(hbmpc_pipe_deal(h_), ctx_, "deal");
    }
    void finish(bool checked = false) {
        pl_check(hbmpc_pipe_set_checked(h_, checked ? 1 : 0), ctx_, "set_checked");
        pl_check(hbmpc_pipe_finish(h_), ctx_, "finish");
    }

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t d, size_t N, size_t eval_senders, size_t reveal_senders, void* stream) {
        hbmpc_pipe* h = nullptr;
        pl_check(hbmpc_pipe_batchrecon_create(ctx, n, t, d, N, eval_senders, reveal_senders, stream, &h), ctx, "hbmpc_pipe_batchrecon_create");
        return h;
    }
};

// TruncPr (fpmul/truncpr.rs:185-318) of N values for n parties: k-bit values, m fractional bits dropped.  The caller uploads rbits
// and rint (what PRandBit / PRandInt produce).  open_senders as in FpMul.
class TruncPr : public Pipeline {
  public:
    TruncPr(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t k, size_t m, void* stream, size_t open_senders = 0)
        : TruncPr(ctx, n, t, N, k, m, stream, open_senders, 0) {}
    U256 *a, *rint, *rbits, *rdash, *osh, *cop, *out;  // [party][N] (rbits: [party][bit][N]; cop: [N], the opened value)

  protected:
    TruncPr(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t k, size_t m, void* stream, size_t open_senders, int with_multiplier)
        : Pipeline(ctx, create(ctx, n, t, N, k, m, open_senders, with_multiplier, stream), stream) {
        a = buffer("a"), rint = buffer("rint"), rbits = buffer("rbits"), rdash = buffer("rdash"), osh = buffer("osh"), cop = buffer("cop");
        out = buffer("out");
    }

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t k, size_t m, size_t open_senders, int with_multiplier, void* stream) {
        hbmpc_pipe* h = nullptr;
        pl_check(hbmpc_pipe_truncpr_create(ctx, n, t, N, k, m, open_senders, with_multiplier, stream, &h), ctx, "hbmpc_pipe_truncpr_create");
        return h;
    }
};

// FPDivConstNode (fpdiv/fpdiv_const.rs:61-99) for n parties: N fixed-point values of k bits with f fractional bits, each divided by a
// PUBLIC denominator: c = a * w with w = fixed_point_reciprocal_scaled(denominator) (fpdiv/mod.rs:8-60), then TruncPr of c with 2 k
// bits and m = f.
class FpDivConst : public TruncPr {
  public:
    FpDivConst(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t k, size_t f, void* stream, size_t open_senders = 0)
        : TruncPr(ctx, n, t, N, 2 * k, f, stream, open_senders, 1), f_(f) {
        w = buffer("w"), c = buffer("c");
    }
    // denom[count], count <= N: the ClearFixedPoint integers; runs the host helper (throws on an invalid divisor), then uploads w
    void set_denominators(const U256* denom, size_t count) {
        std::vector<U256> host(count);
        size_t bad = SIZE_MAX;
        const ShareErrorCode rc = hbmpc_fixed_point_reciprocal_scaled(denom, count, f_, host.data(), &bad);
        if (rc != ShareSuccess && bad != SIZE_MAX)
            throw std::runtime_error("hbmpc_fixed_point_reciprocal_scaled -> " + std::to_string((int)rc) + ": invalid divisor at index " + std::to_string(bad));
        pl_check(rc, ctx_, "hbmpc_fixed_point_reciprocal_scaled");
        upload("w", host.data(), count);
        sync();  // the copy reads `host`
    }
    U256 *w, *c;  // [N] the public multipliers; [party][N] = a * w

  private:
    size_t f_;
};

class Producer : public Pipeline {
  public:
    void deal() { pl_check(hbmpc_pipe_deal(h_), ctx_, "deal"); }      // the dealers' compute_shares
    void finish() { pl_check(hbmpc_pipe_finish(h_), ctx_, "finish"); }  // everything after the dealers' messages have arrived
    // {number of verifier checks that failed, first failing batch element}: zero means every verifier says OK (synchronises)
    void verdict(uint32_t out[2]) { pl_check(hbmpc_pipe_verdict(h_, out), ctx_, "verdict"); }

  protected:
    using Pipeline::Pipeline;
};

// K batch elements per dealer -> (n - 2t) K random degree-t sharings per party ("out": [party][K][n - 2t]), verified by parties
// 0 .. 2t - 1 from the shares of the first verify_senders parties (0 = the reference's 2t + 1)
class RanSha : public Producer {
  public:
    RanSha(hbmpc_ctx* ctx, size_t n, size_t t, size_t K, void* stream, size_t verify_senders = 0)
        : Producer(ctx, create(ctx, n, t, K, verify_senders, stream), stream), nout((n - 2 * t) * K) {
        bind();
    }
    RanSha(hbmpc_ctx* ctx, hbmpc_pipe* borrowed, void* stream, size_t n, size_t t, size_t K) : Producer(ctx, borrowed, stream, false), nout((n - 2 * t) * K) { bind(); }
    const size_t nout;       // output shares per party
    U256 *coeffs, *S, *out;  // [dealer][K][t + 1]; [dealer][recipient][K]; [party][K][n - 2t]

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t K, size_t verify_senders, void* stream) {
        hbmpc_pipe* h = nullptr;
        pl_check(hbmpc_pipe_ransha_create(ctx, n, t, K, verify_senders, stream, &h), ctx, "hbmpc_pipe_ransha_create");
        return h;
    }
    void bind() { coeffs = buffer("coeffs"), S = buffer("S"), out = buffer("out"); }
};

// K batch elements per dealer -> (t + 1) K double sharings per party, verified by parties t + 1 .. n - 1
class RanDouSha : public Producer {
  public:
    RanDouSha(hbmpc_ctx* ctx, size_t n, size_t t, size_t K, void* stream) : Producer(ctx, create(ctx, n, t, K, stream), stream), nout((t + 1) * K) { bind(); }
    RanDouSha(hbmpc_ctx* ctx, hbmpc_pipe* borrowed, void* stream, size_t t, size_t K) : Producer(ctx, borrowed, stream, false), nout((t + 1) * K) { bind(); }
    const size_t nout;
    U256 *coeffs_t, *coeffs_2t, *S_t, *S_2t, *out_t, *out_2t;

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t K, void* stream) {
        hbmpc_pipe* h = nullptr;
        pl_check(hbmpc_pipe_randousha_create(ctx, n, t, K, stream, &h), ctx, "hbmpc_pipe_randousha_create");
        return h;
    }
    void bind() {
        coeffs_t = buffer("coeffs_t"), coeffs_2t = buffer("coeffs_2t"), S_t = buffer("S_t"), S_2t = buffer("S_2t");
        out_t = buffer("out_t"), out_2t = buffer("out_2t");
    }
};

// The producers as ONE device call each for a caller with buffers of its own (hbmpc_dev_ransha_parties / hbmpc_dev_randousha_parties: one
// launch for a small batch, the handles' together form otherwise), over Fr.  The two functions own what the caller does not keep: what the
// parties send the verifiers, the verifiers' results and the workspace live in a DevBlock for the call and are freed after the
// stream has been waited for; verdict_out = {failing (verifier, column) pairs, lowest failing column}.
class DevBlock {
  public:
    DevBlock(hbmpc_ctx* ctx, size_t bytes) : ctx_(ctx) { pl_check(hbmpc_dev_alloc(ctx, bytes ? bytes : 16, &p_), ctx, "hbmpc_dev_alloc"); }
    DevBlock(const DevBlock&) = delete;
    DevBlock& operator=(const DevBlock&) = delete;
    ~DevBlock() { hbmpc_dev_free(ctx_, p_); }
    template <class T>
    T* at(size_t byte_offset) const { return reinterpret_cast<T*>(static_cast<unsigned char*>(p_) + byte_offset); }

  private:
    hbmpc_ctx* ctx_;
    void* p_ = nullptr;
};
// coeffs [dealer][K][t + 1] (or null: dealt is the input) -> dealt [dealer][recipient][K], out [party][K][n - 2t]
inline void ransha_parties(hbmpc_ctx* ctx, const U256* coeffs, U256* dealt, size_t K, size_t n, size_t t, U256* out, uint32_t verdict_out[2],
                           void* stream, size_t verify_senders = 0) {
    const size_t eb = sizeof(U256), yv = n * 2 * t * K * eb, ws = (2 * n * n + (2 * t > t + 1 ? 2 * t : t + 1)) * K * eb;
    DevBlock blk(ctx, yv + ws + 16);
    uint32_t* bad = blk.at<uint32_t>(yv + ws);
    pl_check(hbmpc_dev_ransha_parties(ctx, coeffs, dealt, K, n, t, verify_senders ? verify_senders : 2 * t + 1, out, blk.at<U256>(0), blk.at<U256>(yv), nullptr,
                                      nullptr, bad, stream),
             ctx, "hbmpc_dev_ransha_parties");
    pl_check(hbmpc_memcpy_d2h(ctx, verdict_out, bad, 8, stream), ctx, "d2h");
    pl_check(hbmpc_stream_sync(ctx, stream), ctx, "sync");
}
// both coefficient arrays (or both null) -> dealt_t, dealt_2t, out_t, out_2t [party][K][t + 1]
inline void randousha_parties(hbmpc_ctx* ctx, const U256* coeffs_t, const U256* coeffs_2t, U256* dealt_t, U256* dealt_2t, size_t K, size_t n, size_t t,
                              U256* out_t, U256* out_2t, uint32_t verdict_out[2], void* stream) {
    const size_t eb = sizeof(U256), nver = n - t - 1, G = nver * K, yv = n * G * eb, sel = 2 * G * eb, st = (G + 15) / 16 * 16;
    const size_t ws = (2 * n * n + nver * n) * K * eb;
    DevBlock blk(ctx, 2 * yv + 2 * sel + ws + 2 * st + 16);
    uint32_t* bad = blk.at<uint32_t>(2 * yv + 2 * sel + ws + 2 * st);
    pl_check(hbmpc_dev_randousha_parties(ctx, coeffs_t, coeffs_2t, dealt_t, dealt_2t, K, n, t, out_t, out_2t, blk.at<U256>(0), blk.at<U256>(yv),
                                         blk.at<U256>(2 * yv + 2 * sel), blk.at<U256>(2 * yv), blk.at<U256>(2 * yv + sel), blk.at<void>(2 * yv + 2 * sel + ws),
                                         blk.at<void>(2 * yv + 2 * sel + ws + st), bad, stream),
             ctx, "hbmpc_dev_randousha_parties");
    pl_check(hbmpc_memcpy_d2h(ctx, verdict_out, bad, 8, stream), ctx, "d2h");
    pl_check(hbmpc_stream_sync(ctx, stream), ctx, "sync");
}

// RandBit of N shared values for n parties (N a multiple of t + 1): Beaver square of a, BatchRecon of a^2, phase 2
// (fpmul/rand_bit.rs:242-293,197-220).  Buffers a, ta, tb, tc (inputs), out (output), sq: [party][N]; sqop: [N].  Elements are
// those of the context's field (U256, or 8-byte Goldilocks values: cast the pointers).  run(true) fails with HBMPC_ZERO_SQUARE /
// HBMPC_NO_SQUARE_ROOT where phase 2's `?` returns; summary() gives the finalize's verdict.
class RandBit : public Pipeline {
  public:
    RandBit(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream) : Pipeline(ctx, create(ctx, n, t, N, stream), stream) { bind(); }
    U256 *a, *ta, *tb, *tc, *out, *sq, *sqop;
    uint8_t* status;                        // [N]: 0 ok, 1 zero square, 2 no root
    hbmpc_randbit_summary* summary_dev;     // device memory
    hbmpc_randbit_summary summary() {
        hbmpc_randbit_summary s;
        pl_check(hbmpc_memcpy_d2h(ctx_, &s, summary_dev, sizeof s, stream_), ctx_, "summary");
        pl_check(hbmpc_stream_sync(ctx_, stream_), ctx_, "sync");
        return s;
    }

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream) {
        hbmpc_pipe* h = nullptr;
        pl_check(hbmpc_pipe_randbit_create(ctx, n, t, N, stream, &h), ctx, "hbmpc_pipe_randbit_create");
        return h;
    }
    void bind() {
        a = buffer("a"), ta = buffer("ta"), tb = buffer("tb"), tc = buffer("tc"), out = buffer("out"), sq = buffer("sq"), sqop = buffer("sqop");
        status = reinterpret_cast<uint8_t*>(buffer("status"));
        summary_dev = reinterpret_cast<hbmpc_randbit_summary*>(buffer("summary"));
    }
};

// run_preprocessing's triple part for all n parties, device-resident from the dealers' polynomials to [c]_t
class Preprocessing : public Pipeline {
  public:
    Preprocessing(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream)
        : Pipeline(ctx, create(ctx, n, t, N, stream), stream), rs(ctx, part("ransha"), stream, n, t, (2 * N + (n - 2 * t) - 1) / (n - 2 * t)),
          rd(ctx, part("randousha"), stream, t, (N + t) / (t + 1)), tg(ctx, part("triplegen"), stream) {}
    RanSha rs;     // borrowed parts: they live as long as this object
    RanDouSha rd;
    TripleGen tg;
    void verdict(uint32_t out[2]) { pl_check(hbmpc_pipe_verdict(h_, out), ctx_, "verdict"); }  // both producers

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream) {
        hbmpc_pipe* h = nullptr;
        pl_check(hbmpc_pipe_preprocessing_create(ctx, n, t, N, stream, &h), ctx, "hbmpc_pipe_preprocessing_create");
        return h;
    }
    hbmpc_pipe* part(const char* name) {
        hbmpc_pipe* p = nullptr;
        pl_check(hbmpc_pipe_part(h_, name, &p), ctx_, name);
        return p;
    }
};

// PRandInt and PRandBit (fpmul/prandbitd.rs) for all n parties.  They span two fields -- a Goldilocks context and an Fr context on
// the same device -- so they are compositions of device calls on one stream, not hbmpc_pipe handles (no graph replay here).
// Buffers are device memory owned by the object; inputs: contrib [n][C(n,t)][B] uint64_t the senders' RISS values (and, PRandBit,
// b_q [n][B] the Goldilocks shares of the bits).
class PRandInt {
  public:
    // fold -> sums [C(n,t)][B], bad [n][C(n,t)] verdict bytes; convert over Fr -> r_p [n][B] (prandbitd.rs:667-684, 311-356).  Any B.
    PRandInt(hbmpc_ctx* ctx_fr, size_t n, size_t t, size_t B, void* stream) : n(n), t(t), B(B), fr_(ctx_fr), stream_(stream) {
        pl_check(stream ? ShareSuccess : InvalidInput, fr_, "PRandInt needs an explicit stream");
        pl_check(hbmpc_riss_tsets(n, t, nullptr, &tsets), fr_, "hbmpc_riss_tsets");
        contrib = alloc<uint64_t>(n * tsets * B), sums = alloc<uint64_t>(tsets * B), bad = alloc<uint8_t>(n * tsets), r_p = alloc<U256>(n * B);
    }
    virtual ~PRandInt() {
        for (void* p : owned_) hbmpc_dev_free(fr_, p);
    }
    PRandInt(const PRandInt&) = delete;
    PRandInt& operator=(const PRandInt&) = delete;
    void run(size_t lk_bits) { fold_and_fr(lk_bits, nullptr); }
    void sync() { pl_check(hbmpc_stream_sync(fr_, stream_), fr_, "sync"); }
    const size_t n, t, B;
    size_t tsets = 0;
    uint64_t *contrib, *sums;
    uint8_t* bad;
    U256* r_p;

  protected:
    template <class T>
    T* alloc(size_t count) {
        void* p = nullptr;
        pl_check(hbmpc_dev_alloc(fr_, (count ? count : 1) * sizeof(T), &p), fr_, "hbmpc_dev_alloc");
        owned_.push_back(p);
        return static_cast<T*>(p);
    }
    void fold_and_fr(size_t lk_bits, uint8_t* r_2) {
        pl_check(hbmpc_dev_riss_fold(fr_, contrib, n, tsets, B, lk_bits, sums, bad, stream_), fr_, "hbmpc_dev_riss_fold");
        pl_check(hbmpc_dev_riss_convert_parties(fr_, sums, n, t, B, nullptr, n, 0, r_p, r_2, stream_), fr_, "hbmpc_dev_riss_convert_parties");
    }
    hbmpc_ctx* fr_;
    void* stream_;
    std::vector<void*> owned_;
};

// fold; convert over Fr -> r_p, r_2 (GF(2^8)) and over Goldilocks -> r_q; rb = r_q + b_q; BatchRecon of rb in chunks of t + 1 from all
// n senders (prandbitd.rs:437-446: the encode, the recipients' P(0) decodes, the coefficient decode; up to t wrong senders are
// corrected) -> opened [B]; finalize -> b_p [n][B] Fr, b_2 [n][B] bytes (prandbitd.rs:189-211).  B a multiple of t + 1
// (PRandError::Incompatible; here InvalidInput).
class PRandBit : public PRandInt {
  public:
    PRandBit(hbmpc_ctx* ctx_gl, hbmpc_ctx* ctx_fr, size_t n, size_t t, size_t B, void* stream) : PRandInt(ctx_fr, n, t, B, stream), gl_(ctx_gl) {
        pl_check(B % (t + 1) == 0 ? ShareSuccess : InvalidInput, fr_, "B must be a multiple of t + 1");
        G = B / (t + 1);
        b_q = alloc<uint64_t>(n * B), r_q = alloc<uint64_t>(n * B), rb = alloc<uint64_t>(n * B), Y = alloc<uint64_t>(n * n * G);
        Z = alloc<uint64_t>(n * G), opened = alloc<uint64_t>(B), r_2 = alloc<uint8_t>(n * B), b_2 = alloc<uint8_t>(n * B), b_p = alloc<U256>(n * B);
        rstatus = alloc<uint8_t>(n * G), summary_first = alloc<hbmpc_recover_summary>(1), summary = alloc<hbmpc_recover_summary>(1);
        for (size_t i = 0; i < n; ++i) ids_.push_back(i);
    }
    void prepare(size_t lk_bits) {  // everything before the messages of the open are exchanged
        fold_and_fr(lk_bits, r_2);
        pl_check(hbmpc_gl_dev_riss_convert_parties(gl_, sums, n, t, B, nullptr, n, 0, r_q, nullptr, stream_), gl_, "hbmpc_gl_dev_riss_convert_parties");
        pl_check(hbmpc_gl_dev_fr_op(gl_, 0, r_q, b_q, n * B, rb, stream_), gl_, "r + b");
        pl_check(hbmpc_gl_dev_vandermonde_apply_parties(gl_, rb, G, n, t, n, Y, stream_), gl_, "open: encode");
    }
    void finish() {
        pl_check(hbmpc_gl_dev_batch_recover_strided(gl_, ids_.data(), n, Y, n * G, n * G, n, t, t, 1, Z, nullptr, rstatus, summary_first, stream_), gl_,
                 "open: P(0) decodes");
        pl_check(hbmpc_gl_dev_batch_recover(gl_, ids_.data(), n, Z, G, n, t, t, opened, nullptr, rstatus, summary, stream_), gl_,
                 "open: coefficient decode");
        pl_check(hbmpc_dev_prandbit_finalize_parties(fr_, opened, r_p, r_2, B, n, b_p, b_2, stream_), fr_, "hbmpc_dev_prandbit_finalize_parties");
    }
    void run(size_t lk_bits) {
        prepare(lk_bits);
        finish();
    }
    size_t G = 0;  // chunks of the open
    uint64_t *b_q, *r_q, *rb, *Y, *Z, *opened;
    uint8_t *r_2, *b_2, *rstatus;
    U256* b_p;
    hbmpc_recover_summary *summary_first, *summary;  // device memory: the two decodes of the open

  private:
    hbmpc_ctx* gl_;
    std::vector<size_t> ids_;
};

// The same two as hbmpc_pipe handles (csrc/capi_pipelines_riss.hip): run() is ONE device call (hbmpc_dev_prandint_parties /
// hbmpc_dev_prandbit_parties: one launch for a small batch), capture() / replay() work as for the other handles.  Every buffer has an
// element type of its own, which the typed accessors below count in.
// seeded = true (hbmpc_pipe_*_create_seeded; contract "hbmpc-riss-chacha20-v1", include/hbmpc_hip.h): the handle has seeds ([n][32]
// bytes, one seed per sender) and no contrib (the pointer is null); run() draws the contributions on the device at the handle's stream
// index and advances it (set_stream_index); capture() throws: a replayed graph would reuse the same stream positions.
class RissPipeline : public Pipeline {
  public:
    template <class T>
    T* typed(const char* name, size_t* elements = nullptr) const {
        return reinterpret_cast<T*>(buffer(name, elements));
    }
    template <class T>
    void upload_typed(const char* name, const T* src, size_t elements) { pl_check(hbmpc_pipe_upload(h_, name, src, elements), ctx_, name); }
    template <class T>
    void download_typed(const char* name, T* dst, size_t elements) { pl_check(hbmpc_pipe_download(h_, name, dst, elements), ctx_, name); }
    void set_stream_index(uint64_t index) { pl_check(hbmpc_pipe_set_stream_index(h_, index), ctx_, "set_stream_index"); }  // seeded handles

  protected:
    using Pipeline::Pipeline;
};

// contrib [n][C(n,t)][B] -> sums [C(n,t)][B], bad [n][C(n,t)] bytes, r_p [n][B] (prandbitd.rs:667-684, 311-356).  Any B.
class PRandIntPipe : public RissPipeline {
  public:
    PRandIntPipe(hbmpc_ctx* ctx_fr, size_t n, size_t t, size_t B, size_t lk_bits, void* stream, bool seeded = false)
        : RissPipeline(ctx_fr, create(ctx_fr, n, t, B, lk_bits, stream, seeded), stream) {
        contrib = seeded ? nullptr : typed<uint64_t>("contrib"), seeds = seeded ? typed<uint8_t>("seeds") : nullptr;
        sums = typed<uint64_t>("sums"), bad = typed<uint8_t>("bad"), r_p = typed<U256>("r_p");
    }
    uint64_t *contrib, *sums;
    uint8_t *bad, *seeds;
    U256* r_p;

  private:
    static hbmpc_pipe* create(hbmpc_ctx* ctx, size_t n, size_t t, size_t B, size_t lk_bits, void* stream, bool seeded) {
        hbmpc_pipe* h = nullptr;
        if (seeded) pl_check(hbmpc_pipe_prandint_create_seeded(ctx, n, t, B, lk_bits, stream, &h), ctx, "hbmpc_pipe_prandint_create_seeded");
        else pl_check(hbmpc_pipe_prandint_create(ctx, n, t, B, lk_bits, stream, &h), ctx, "hbmpc_pipe_prandint_create");
        return h;
    }
};

// ... and b_q [n][B] -> r_2, r_q, rb, opened [B], b_p [n][B] Fr, b_2 [n][B] bytes (prandbitd.rs:437-446, 189-211).  B a multiple of
// t + 1; open_senders: 0 = the reference's 2t + 1 (no OEC round).  last_summary() is the revealed values' decode's.
class PRandBitPipe : public RissPipeline {
  public:
    PRandBitPipe(hbmpc_ctx* ctx_gl, hbmpc_ctx* ctx_fr, size_t n, size_t t, size_t B, size_t lk_bits, void* stream, size_t open_senders = 0,
                 bool seeded = false)
        : RissPipeline(ctx_gl, create(ctx_fr, ctx_gl, n, t, B, lk_bits, open_senders, stream, seeded), stream) {
        contrib = seeded ? nullptr : typed<uint64_t>("contrib"), seeds = seeded ? typed<uint8_t>("seeds") : nullptr;
        b_q = typed<uint64_t>("b_q"), sums = typed<uint64_t>("sums"), r_q = typed<uint64_t>("r_q");
        rb = typed<uint64_t>("rb"), opened = typed<uint64_t>("opened"), bad = typed<uint8_t>("bad"), r_2 = typed<uint8_t>("r_2");
        b_2 = typed<uint8_t>("b_2"), rstatus = typed<uint8_t>("rstatus"), r_p = typed<U256>("r_p"), b_p = typed<U256>("b_p");
    }
    uint64_t *contrib, *b_q, *sums, *r_q, *rb, *opened;
    uint8_t *bad, *r_2, *b_2, *rstatus, *seeds;
    U256 *r_p, *b_p;

  private:
    static hbmpc_pipe* create(hbmpc_ctx* fr, hbmpc_ctx* gl, size_t n, size_t t, size_t B, size_t lk_bits, size_t open_senders, void* stream,
                              bool seeded) {
        hbmpc_pipe* h = nullptr;
        if (seeded)
            pl_check(hbmpc_pipe_prandbit_create_seeded(fr, gl, n, t, B, lk_bits, open_senders, stream, &h), fr, "hbmpc_pipe_prandbit_create_seeded");
        else pl_check(hbmpc_pipe_prandbit_create(fr, gl, n, t, B, lk_bits, open_senders, stream, &h), fr, "hbmpc_pipe_prandbit_create");
        return h;
    }
};

// FixedPrep (csrc/capi_pipelines_fixedprep.hip): run_preprocessing's steps 5 and 6 for all n parties -- one refill of the r_bits / r_int
// pools that mul_fixed drains (honeybadger/mod.rs:1396-1410, 1951-2150, 1031-1045).  R = n_prandbit up to a multiple of t + 1 bits,
// n_prandint integers; one of the two may be 0 and that half is then absent.  Inputs are the parts' (part("ransha") ... : borrowed
// handles for hbmpc_pipe_buffer / _upload): coeffs, coeffs_t, coeffs_2t over Goldilocks and contrib of "prandbit" and "prandint".
// take(): N multiplications' worth from the front of the pools into a consumer's rbits [n][m][N] / rint [n][N].
class FixedPrep : public RissPipeline {
  public:
    // seeded: "prandbit" and "prandint" are seeded handles fed from this handle's own seeds and stream index; no contrib anywhere
    FixedPrep(hbmpc_ctx* ctx_gl, hbmpc_ctx* ctx_fr, size_t n, size_t t, size_t n_prandbit, size_t n_prandint, size_t lk_bits, void* stream,
              bool seeded = false)
        : RissPipeline(ctx_gl, create(ctx_fr, ctx_gl, n, t, n_prandbit, n_prandint, lk_bits, stream, seeded), stream) {
        if (n_prandbit) r_bits = typed<U256>("r_bits"), r_bits2 = typed<uint8_t>("r_bits2");
        if (n_prandint) r_int = typed<U256>("r_int");
        if (seeded) seeds = typed<uint8_t>("seeds");
    }
    uint8_t* seeds = nullptr;  // [n][32] (seeded)
    U256 *r_bits = nullptr, *r_int = nullptr;  // [n][R], [n][n_prandint]
    uint8_t* r_bits2 = nullptr;                // [n][R]
    hbmpc_pipe* part(const char* name) const {  // "ransha", "randousha", "triplegen", "randbit", "prandbit", "prandint"
        hbmpc_pipe* p = nullptr;
        pl_check(hbmpc_pipe_part(h_, name, &p), ctx_, name);
        return p;
    }
    void deal() { pl_check(hbmpc_pipe_deal(h_), ctx_, "deal"); }      // the dealers' encodes of both producers
    void finish() { pl_check(hbmpc_pipe_finish(h_), ctx_, "finish"); }  // everything after
    void verdict(uint32_t out[2]) { pl_check(hbmpc_pipe_verdict(h_, out), ctx_, "verdict"); }  // both producers
    // InsufficientShares (nothing written, the cursors unchanged) when a pool is short: returned, not thrown
    ShareErrorCode take(size_t m, size_t N, U256* rbits_dst, U256* rint_dst) { return hbmpc_pipe_fixedprep_take(h_, m, N, rbits_dst, rint_dst); }
    ShareErrorCode take(FpMul& consumer, size_t m, size_t N) { return take(m, N, consumer.buffer("rbits"), consumer.buffer("rint")); }
    void available(size_t out[2]) { pl_check(hbmpc_pipe_fixedprep_available(h_, out), ctx_, "available"); }  // bits, integers left

  private:
    static hbmpc_pipe* create(hbmpc_ctx* fr, hbmpc_ctx* gl, size_t n, size_t t, size_t nb, size_t ni, size_t lk_bits, void* stream, bool seeded) {
        hbmpc_pipe* h = nullptr;
        if (seeded) pl_check(hbmpc_pipe_fixedprep_create_seeded(fr, gl, n, t, nb, ni, lk_bits, stream, &h), fr, "hbmpc_pipe_fixedprep_create_seeded");
        else pl_check(hbmpc_pipe_fixedprep_create(fr, gl, n, t, nb, ni, lk_bits, stream, &h), fr, "hbmpc_pipe_fixedprep_create");
        return h;
    }
};

}  // namespace hbmpc
