// capi_pipelines.hip -- the device-resident pipelines behind the C ABI (hbmpc_pipe_* of include/hbmpc_hip.h): replays of the
// reference's arithmetic pipelines for ALL n simulated parties on one GPU -- how every reference test and bench runs (n
// parties in one process on FakeNetwork) -- so that a Rust node (or any C caller) gets the call sequencing, the arena
// layout and the capture rules from the library instead of re-deriving them.
//
//   triplegen      TripleGenNode::init_batch + BatchReconNode (degree 2t) + try_finalize_triple_gen
//                  triple_gen/triple_generation.rs:304-364,164-232; batch_recon/batch_recon.rs:144-185,332-481
//   fpmul          FPMulNode::init = Multiply (Beaver, RBC path) + TruncPrNode
//                  fpmul/fpmul.rs:61-110, mul/multiplication.rs:417-426,57-139, fpmul/truncpr.rs:185-318
//   ransha         RanShaNode: deal, n x n Vandermonde, verifier reconstruction + degree test, output slice
//                  share_gen/share_gen.rs:232-289,401-454,516-530,199-203
//   randousha      DouShaNode deal + RanDouShaNode: both Vandermonde products, verifier interpolations + tests, output slice
//                  double_share/double_share_generation.rs:151-215, ran_dou_sha/mod.rs:371-449,569-602,314-331
//   preprocessing  run_preprocessing's triple part (honeybadger/mod.rs:1239-1393): ransha -> a, b; randousha -> r; triplegen
//   randbit        RandBit: Beaver square of a, BatchRecon of a^2, phase 2   fpmul/rand_bit.rs:242-293,197-220
//   truncpr        TruncPrNode alone, or FPDivConstNode = a local product with a public reciprocal + TruncPrNode
//                  fpmul/truncpr.rs:185-318, fpdiv/fpdiv_const.rs:61-99
//   mul            Multiply (Beaver, RBC path): the opened shares, the open, finalize_mul
//                  honeybadger/mod.rs:543-628, mul/multiplication.rs:417-426,102-139,57-100
//
// Host-side orchestration only: this file is a CLIENT of the hbmpc_dev_* entry points (it includes nothing but the public
// header, pipe_internal.hpp -- struct hbmpc_pipe, shared with capi_pipelines_riss.hip, which holds the PRandBit / PRandInt handles --
// and producer_route.hpp, the plain-C++ rule for the form the producers' calls take) and compiles with a host C++ compiler,
// which is how tests/cpp/pipeline_calls_dump.cpp records its calls; every arithmetic step is a device call, buffers never leave HBM,
// the parties' all-to-all is a layout.
#include "pipe_internal.hpp"
#include "producer_route.hpp"

namespace {

// n parties, threshold t, N triples (a multiple of 2t+1); buffers [party][N]
struct TripleGen : hbmpc_pipe {
    size_t n, t, N, G;
    unsigned char *a, *b, *r2t, *rt, *c, *Y, *Z, *opened;
    uint8_t* status;
    hbmpc_recover_summary* summ_first;  // the recipients' decodes' (summ: the revealed values')
    std::vector<size_t> ids;
    TripleGen(hbmpc_ctx* cx, size_t n_, size_t t_, size_t N_, void* s) : hbmpc_pipe(cx, s), n(n_), t(t_), N(N_), G(N_ / (2 * t_ + 1)) {
        if (n == 0 || N == 0 || N % (2 * t + 1) != 0) throw PipeError{InvalidInput};
        arena((5 * n * N + n * n * G + n * G + N) * f.eb + (n + 2) * G + (1 << 14));
        a = take("a", n * N), b = take("b", n * N), r2t = take("r2t", n * N), rt = take("rt", n * N), c = take("c", n * N);
        Y = take("Y", n * n * G);   // Y[p][j][g]: party p's evaluation for recipient j
        Z = take("Z", n * G);       // Z[j][g]: recipient j's opened y_j (the broadcast RevealBatch)
        opened = take("opened", N); // [G][2t+1] == flat [N]
        status = take_bytes("status", n * G, n * G);
        summ = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary", 64, 16));
        summ_first = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary_first", 64, 16));
        for (size_t i = 0; i < n; ++i) ids.push_back(i);
    }
    void run() override {
        // one call for the whole step: one launch for a small batch, four otherwise (hbmpc_[gl_]dev_triplegen_parties)
        PL(f.triplegen_parties(ctx, a, b, r2t, rt, N, n, t, Y, Z, opened, c, status, summ_first, summ, stream));
        check_summary(summ_first);
        check_summary(summ);
    }
};

// Fixed-point multiplication of N element pairs for n parties: Beaver mul (a-x, b-y opened by direct robust interpolation,
// the RBC path FPMulNode always takes) followed by TruncPr with k-bit values and m fractional bits.  open_senders: how many
// parties' shares an open interpolates from (0 = the default 2t+1: the reference opens as soon as that many have arrived,
// multiplication.rs:388,617, truncpr.rs:202 -- with d = t a decode with no OEC round, one launch).  Fr only, as in the reference.
struct FpMul : hbmpc_pipe {
    size_t n, t, N, k, m;
    U256 *x, *y, *ta, *tb, *tc, *rint, *z, *rdash, *osh, *out, *desh, *rbits, *dop, *eop, *cop;
    uint8_t* status;
    hbmpc_recover_summary* summ_first;  // the first open's (summ: the second's)
    std::vector<size_t> ids;
    FpMul(hbmpc_ctx* cx, size_t n_, size_t t_, size_t N_, size_t k_, size_t m_, size_t open_senders, void* s)
        : hbmpc_pipe(cx, s), n(n_), t(t_), N(N_), k(k_), m(m_) {
        if (f.gl) throw PipeError{TypeMismatch};
        if (open_senders == 0) open_senders = 2 * t + 1;
        if (n == 0 || N == 0 || open_senders < 2 * t + 1 || open_senders > n) throw PipeError{InvalidInput};
        arena(((12 + m) * n * N + 4 * N) * 32 + 8 * N + (1 << 14));
        const char* names[] = {"x", "y", "ta", "tb", "tc", "rint", "z", "rdash", "osh", "out"};
        U256** per_party[] = {&x, &y, &ta, &tb, &tc, &rint, &z, &rdash, &osh, &out};
        for (int i = 0; i < 10; ++i) *per_party[i] = reinterpret_cast<U256*>(take(names[i], n * N));
        desh = reinterpret_cast<U256*>(take("desh", 2 * n * N));    // [party][2][N]: a party's shares of a - x and of b - y side by side
        rbits = reinterpret_cast<U256*>(take("rbits", n * m * N));  // [party][bit][N]
        dop = reinterpret_cast<U256*>(take("deop", 2 * N)), eop = dop + N;  // the opened a - x [N], then the opened b - y [N]
        buffers["dop"] = Buffer{(unsigned char*)dop, N}, buffers["eop"] = Buffer{(unsigned char*)eop, N};
        cop = reinterpret_cast<U256*>(take("cop", N));
        status = take_bytes("status", 2 * N, 2 * N);
        summ = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary", 64, 16));
        summ_first = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary_first", 64, 16));
        for (size_t i = 0; i < open_senders; ++i) ids.push_back(i);
    }
    void run() override {
        // all parties at once (the [party][N] arrays are contiguous; opened values are broadcast): one launch for a small batch,
        // one per step otherwise (hbmpc_dev_fpmul_parties).  Checked mode looks at the two opens' summaries afterwards, in order.
        PL(hbmpc_dev_fpmul_parties(ctx, ids.data(), ids.size(), ta, tb, tc, x, y, rbits, rint, k, m, N, n, t, desh, dop, z, rdash, osh, cop, out,
                                   status, summ_first, summ, stream));
        check_summary(summ_first);
        check_summary(summ);
    }
};

// TruncPr of N values for n parties (fpmul/truncpr.rs:185-318) and, with a multiplier, FPDivConstNode (fpdiv/fpdiv_const.rs:61-99:
// c = a * w with the public reciprocal w of the element's denominator, then TruncPr of c with k = 2 k_fixed, m = f).  The
// caller uploads rbits and rint (PRandBit / PRandInt produce them) and, with a multiplier, w.  open_senders as in FpMul.  Fr only.
struct TruncPr : hbmpc_pipe {
    size_t n, t, N, k, m;
    U256 *a, *rint, *rbits, *rdash, *osh, *out, *c = nullptr, *w = nullptr, *cop;
    uint8_t* status;
    std::vector<size_t> ids;
    TruncPr(hbmpc_ctx* cx, size_t n_, size_t t_, size_t N_, size_t k_, size_t m_, size_t open_senders, int with_multiplier, void* s)
        : hbmpc_pipe(cx, s), n(n_), t(t_), N(N_), k(k_), m(m_) {
        if (f.gl) throw PipeError{TypeMismatch};
        if (open_senders == 0) open_senders = 2 * t + 1;
        if (n == 0 || N == 0 || open_senders < 2 * t + 1 || open_senders > n) throw PipeError{InvalidInput};
        arena(((6 + m) * n * N + 2 * N) * 32 + N + (1 << 14));
        a = reinterpret_cast<U256*>(take("a", n * N)), rint = reinterpret_cast<U256*>(take("rint", n * N));
        rbits = reinterpret_cast<U256*>(take("rbits", n * m * N));  // [party][bit][N]
        rdash = reinterpret_cast<U256*>(take("rdash", n * N)), osh = reinterpret_cast<U256*>(take("osh", n * N));
        out = reinterpret_cast<U256*>(take("out", n * N));
        if (with_multiplier) c = reinterpret_cast<U256*>(take("c", n * N)), w = reinterpret_cast<U256*>(take("w", N));
        cop = reinterpret_cast<U256*>(take("cop", N));
        status = take_bytes("status", N, N);
        summ = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary", 64, 16));
        for (size_t i = 0; i < open_senders; ++i) ids.push_back(i);
    }
    void run() override {
        // one launch for a small batch, three otherwise (hbmpc_dev_truncpr_parties); checked mode looks at the open's summary afterwards
        PL(hbmpc_dev_truncpr_parties(ctx, ids.data(), ids.size(), a, w, rbits, rint, k, m, N, n, t, c, rdash, osh, cop, out, status, summ, stream));
        check_summary(summ);
    }
};

// Multiply (Beaver) of N element pairs for n parties (honeybadger/mod.rs:543-628, mul/multiplication.rs:417-426,102-139,57-100):
// a - x and b - y opened by direct robust interpolation, then finalize_mul.  open_senders as in FpMul.  Either field.
struct Mul : hbmpc_pipe {
    size_t n, t, N;
    unsigned char *x, *y, *ta, *tb, *tc, *out, *desh, *deop;
    uint8_t* status;
    std::vector<size_t> ids;
    Mul(hbmpc_ctx* cx, size_t n_, size_t t_, size_t N_, size_t open_senders, void* s) : hbmpc_pipe(cx, s), n(n_), t(t_), N(N_) {
        if (open_senders == 0) open_senders = 2 * t + 1;
        if (n == 0 || N == 0 || open_senders < 2 * t + 1 || open_senders > n) throw PipeError{InvalidInput};
        arena((8 * n * N + 2 * N) * f.eb + 2 * N + (1 << 14));
        x = take("x", n * N), y = take("y", n * N), ta = take("ta", n * N), tb = take("tb", n * N), tc = take("tc", n * N);
        out = take("out", n * N);
        desh = take("desh", 2 * n * N);  // [party][2][N]: a party's shares of a - x and of b - y side by side
        deop = take("deop", 2 * N);      // the opened a - x [N], then the opened b - y [N]
        buffers["dop"] = Buffer{deop, N}, buffers["eop"] = Buffer{deop + N * f.eb, N};
        status = take_bytes("status", 2 * N, 2 * N);
        summ = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary", 64, 16));
        for (size_t i = 0; i < open_senders; ++i) ids.push_back(i);
    }
    void run() override {
        // one launch for a small batch over Fr, three otherwise (hbmpc_[gl_]dev_mul_parties); checked mode looks at the open's summary afterwards
        PL(f.mul_parties(ctx, ids.data(), ids.size(), ta, tb, tc, x, y, N, n, t, desh, deop, out, status, summ, stream));
        check_summary(summ);
    }
};

// What RanSha and RanDouSha share.  The dealers' polynomials are the INPUT (coefficient rows [dealer][K][deg + 1], column 0 the
// secret: uploaded by the host or filled on the device by hbmpc_dev_fill_coeffs -- the reference draws them from each party's
// rng).  Layouts (all n parties on one device): dealt S[p][j, k] --n x n Vandermonde over the rows p--> y[i][j, k]; what party j
// sends verifier i is y[i][j K .. j K + K): a strided sender row, nothing is copied.
struct Producer : hbmpc_pipe {
    size_t n, t, K;
    bool lists_in_kernel;  // does the mixing step write its lists from the kernel that computes them?  (a fact of the context: asked once)
    hbmpc::VerifyPlan v;   // the form of the verifiers' calls and the workspace it needs: what the arena is sized from and what finish() enqueues
    Producer(hbmpc_ctx* cx, size_t n_, size_t t_, size_t K_, void* s) : hbmpc_pipe(cx, s), n(n_), t(t_), K(K_) {
        // the degree-2t sharing (RanDouSha) and the 2t verifiers (RanSha) need 2t + 1 <= n points; before anything is sized from n - 2t
        if (n <= 2 * t || K == 0) throw PipeError{InvalidInput};
        int yes = 0;
        PL(hbmpc_dev_apply_rows_lists_in_kernel(ctx, n * K, n, n - 1, &yes));
        lists_in_kernel = yes != 0;
    }
    // compute_shares of every dealer's K polynomials: coeffs [dealer][K][deg + 1] -> S [dealer][recipient][K], `per` dealers to a call (plan_deal)
    void deal_one(const unsigned char* coeffs, size_t deg, size_t per, unsigned char* S) {
        for (size_t p = 0; p < n; p += per) {
            const unsigned char* co = coeffs + p * K * (deg + 1) * f.eb;
            unsigned char* out = S + p * n * K * f.eb;
            if (per == 1) PL(f.compute_shares(ctx, co, K, n, deg, out, stream));
            else PL(f.apply_parties(ctx, co, K, n, deg, n - p < per ? n - p : per, out, stream));
        }
    }
    // The share of dealer p for (recipient, element) is row p of S: the n x n map reads the dealers' outputs in place (x is the
    // workspace of the shapes that have to be transposed first).  Rows [row0, row0 + rows) of the result are the parties' OUTPUT:
    // they are written as the per-party lists [k][row] the reference returns, where `lists` says; the other rows -- what the
    // parties send the verifiers -- to y[row][party, k]
    // with `others`: the verifiers' rows party-major (hbmpc_dev_vandermonde_apply_rows_split): others[(party (n - rows) + r') K + k]
    void mix(const unsigned char* S, unsigned char* x, unsigned char* y, size_t row0, size_t rows, const std::vector<Slice>& lists,
             unsigned char* others = nullptr) {
        if (others) PL(f.apply_rows_split(ctx, S, n * K, n * K, n, n - 1, x, y, row0, rows, K, lists.data(), lists.size(), others, stream));
        else PL(f.apply_rows_lists(ctx, S, n * K, n * K, n, n - 1, x, y, row0, rows, K, lists.data(), lists.size(), stream));
    }
    // call i's source: the party-major block where the form has one, the mixing call's rows otherwise
    const unsigned char* source(size_t i, const unsigned char* y, const unsigned char* yv) const {
        return (v.party_major ? yv : y) + (v.src0 + i * v.call_stride) * f.eb;
    }
    void run() override {
        deal();
        finish();
    }
};

// K batch elements per dealer -> (n - 2t) K random degree-t sharings per party, verified by parties 0 .. 2t - 1 from the
// shares of the first verify_senders parties (0 = the default 2t + 1: the handler fires when that many have arrived,
// share_gen.rs:497 -- with degree t a decode with no OEC round)
struct RanSha : Producer {
    size_t nout, per;
    unsigned char *coeffs, *S, *x, *y, *yv = nullptr, *poly, *out;
    uint8_t* status;
    std::vector<size_t> ids;
    std::vector<Slice> split;  // set by Preprocessing: where the output slices go instead of `out`
    RanSha(hbmpc_ctx* cx, size_t n_, size_t t_, size_t K_, size_t verify_senders, void* s)
        : Producer(cx, n_, t_, K_, s), nout((n_ - 2 * t_) * K_), per(hbmpc::plan_deal(f.eb, n_, K_, t_)) {
        if (verify_senders == 0) verify_senders = 2 * t + 1;
        if (verify_senders < 2 * t + 1 || verify_senders > n) throw PipeError{InvalidInput};
        v = hbmpc::plan_ransha(f.eb, n, t, K, verify_senders, lists_in_kernel);
        arena((n * K * (t + 1) + 3 * n * n * K + v.yv_el + v.poly_el + n * nout) * f.eb + v.status_b + (1 << 14));
        coeffs = take("coeffs", n * K * (t + 1));  // [dealer][K][t + 1]
        S = take("S", n * n * K);                  // [dealer][recipient][K]
        x = take("x", n * n * K);
        y = take("y", n * n * K);                  // [row i][party][K]
        if (v.yv_el) yv = take("yv", v.yv_el);     // [party][verifier i][K]
        poly = take("poly", v.poly_el);
        status = take_bytes("status", v.status_b, K);
        summ = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary", 64, 16));
        bad = reinterpret_cast<uint32_t*>(take_bytes("bad", 64, 16));
        out = take("out", n * nout);               // [party][K][n - 2t]: the reference's output order (share_gen.rs:199-203)
        for (size_t i = 0; i < verify_senders; ++i) ids.push_back(i);
    }
    void deal() override { deal_one(coeffs, t, per, S); }
    void finish() override {  // everything after the dealers' messages have arrived
        // rows 2t .. n - 1 of every batch element are the output, per party in the order [k][i - 2t]  (share_gen.rs:199-203)
        mix(S, x, y, 2 * t, n - 2 * t, split.empty() ? std::vector<Slice>{{out, nout, 0, K}} : split, yv);
        clear_bad();
        // verifiers 0 .. 2t - 1: recover_secret of the K columns + exact-degree test (share_gen.rs:516-530), in the calls the plan lays out
        for (size_t i = 0; i < v.calls; ++i)
            PL(f.recover_check_degree(ctx, ids.data(), ids.size(), source(i, y, yv), v.row_stride, v.columns, n, t, v.groups, v.group_stride, poly, status,
                                      summ, bad, stream));
    }
};

// K batch elements per dealer -> (t + 1) K double sharings per party, verified by parties t + 1 .. n - 1, each of which
// interpolates both polynomials through ALL n shares (ran_dou_sha/mod.rs:557-602)
struct RanDouSha : Producer {
    size_t nout, per_t, per_2t;
    unsigned char *coeffs_t, *coeffs_2t, *S_t, *S_2t, *x, *y_t, *y_2t, *poly, *c0_t, *c0_2t, *out_t, *out_2t, *sel_t, *sel_2t, *st_t, *st_2t;
    unsigned char *yv_t = nullptr, *yv_2t = nullptr;
    uint32_t *deg_t, *deg_2t;
    std::vector<size_t> ids;
    std::vector<Slice> split_t, split_2t;
    RanDouSha(hbmpc_ctx* cx, size_t n_, size_t t_, size_t K_, void* s)
        : Producer(cx, n_, t_, K_, s), nout((t_ + 1) * K_), per_t(hbmpc::plan_deal(f.eb, n_, K_, t_)), per_2t(hbmpc::plan_deal(f.eb, n_, K_, 2 * t_)) {
        v = hbmpc::plan_randousha(f.eb, n, t, K, lists_in_kernel);
        const size_t vr = v.vr, vc = v.vc;
        arena((n * K * (3 * t + 2) + 5 * n * n * K + 2 * v.yv_el + vc * K * n + (2 * vc + 4 * vr) * K + 2 * n * nout) * f.eb + (8 * vc + 2 * vr) * K +
              (1 << 14));
        coeffs_t = take("coeffs_t", n * K * (t + 1)), coeffs_2t = take("coeffs_2t", n * K * (2 * t + 1));
        S_t = take("S_t", n * n * K), S_2t = take("S_2t", n * n * K);
        x = take("x", n * n * K), y_t = take("y_t", n * n * K), y_2t = take("y_2t", n * n * K);
        if (v.yv_el) yv_t = take("yv_t", v.yv_el), yv_2t = take("yv_2t", v.yv_el);  // [party][verifier][K]
        poly = take("poly", vc * K * n);  // workspace of the verifier interpolations that have no c0-only kernel
        c0_t = take("c0_t", vc * K), c0_2t = take("c0_2t", vc * K);
        deg_t = reinterpret_cast<uint32_t*>(take_bytes("deg_t", 4 * vc * K, K)), deg_2t = reinterpret_cast<uint32_t*>(take_bytes("deg_2t", 4 * vc * K, K));
        sel_t = take("sel_t", 2 * K * vr), sel_2t = take("sel_2t", 2 * K * vr);  // (constant term, top coefficient) of a verifier's two polynomials
        st_t = take_bytes("st_t", K * vr, K), st_2t = take_bytes("st_2t", K * vr, K);
        bad = reinterpret_cast<uint32_t*>(take_bytes("bad", 64, 16));
        out_t = take("out_t", n * nout), out_2t = take("out_2t", n * nout);  // [party][K][t + 1]  (ran_dou_sha/mod.rs:314-331)
        for (size_t i = 0; i < n; ++i) ids.push_back(i);
    }
    void deal() override {  // DouShaNode::init_batch: both sharings of every secret
        deal_one(coeffs_t, t, per_t, S_t);
        deal_one(coeffs_2t, 2 * t, per_2t, S_2t);
    }
    void finish() override {
        // RanDouShaNode::init_batch steps 1, 2, 4-5: rows 0 .. t are the output, per party in the order [k][i]  (ran_dou_sha/mod.rs:314-331)
        mix(S_t, x, y_t, 0, t + 1, split_t.empty() ? std::vector<Slice>{{out_t, nout, 0, K}} : split_t, yv_t);
        mix(S_2t, x, y_2t, 0, t + 1, split_2t.empty() ? std::vector<Slice>{{out_2t, nout, 0, K}} : split_2t, yv_2t);
        clear_bad();
        // step 3: verifiers t + 1 .. n - 1 interpolate both sharings through all n shares and test the degrees and the constant terms
        // (:586-602) -- they keep nothing else of them.  Each call of the plan: both interpolations, then the verdict on their results
        for (size_t i = 0; i < v.calls; ++i) {
            const unsigned char *ev_t = source(i, y_t, yv_t), *ev_2t = source(i, y_2t, yv_2t);
            if (v.check == hbmpc::VerifyCheck::Selected) {  // the two questions answered without the full interpolation
                PL(f.interpolate_degree_check(ctx, ids.data(), n, ev_t, v.row_stride, v.columns, n, t, v.groups, v.group_stride, poly, sel_t, st_t, stream));
                PL(f.interpolate_degree_check(ctx, ids.data(), n, ev_2t, v.row_stride, v.columns, n, 2 * t, v.groups, v.group_stride, poly, sel_2t, st_2t,
                                              stream));
                PL(hbmpc_dev_check_double_share_sel(ctx, sel_t, st_t, sel_2t, st_2t, v.verdict_G, v.verdict_columns, t, bad, stream));
            } else {
                PL(f.interpolate_c0(ctx, ids.data(), n, ev_t, v.row_stride, v.columns, n, poly, c0_t, deg_t, stream));
                PL(f.interpolate_c0(ctx, ids.data(), n, ev_2t, v.row_stride, v.columns, n, poly, c0_2t, deg_2t, stream));
                PL(hbmpc_dev_check_double_share_c0_columns(ctx, c0_t, deg_t, c0_2t, deg_2t, v.verdict_G, v.verdict_columns, t, bad, stream));
            }
        }
    }
};

// run_preprocessing's triple part for all n parties, device-resident from the dealers' polynomials to [c]_t: RanSha produces
// 2 N random sharings per party (a = the first N, b = the next N: take_random_shares twice, honeybadger/mod.rs:1307-1316),
// RanDouSha the N double sharings, TripleGen consumes them where they lie.
struct Preprocessing : hbmpc_pipe {
    size_t n, t, N;
    std::unique_ptr<RanSha> rs;
    std::unique_ptr<RanDouSha> rd;
    std::unique_ptr<TripleGen> tg;
    bool in_place;
    Preprocessing(hbmpc_ctx* cx, size_t n_, size_t t_, size_t N_, void* s) : hbmpc_pipe(cx, s), n(n_), t(t_), N(N_) {
        if (n <= 2 * t || N == 0) throw PipeError{InvalidInput};
        rs.reset(new RanSha(cx, n, t, (2 * N + (n - 2 * t) - 1) / (n - 2 * t), 0, s));  // (n - 2t) K >= 2 N
        rd.reset(new RanDouSha(cx, n, t, (N + t) / (t + 1), s));                          // (t + 1) K >= N
        tg.reset(new TripleGen(cx, n, t, N, s));
        // whole batch elements on both sides of every cut: the producers' output slices go straight into TripleGen's
        // [party][N] arrays and nothing is copied
        in_place = N % (n - 2 * t) == 0 && N % (t + 1) == 0;
        if (in_place) {
            const size_t k1 = N / (n - 2 * t), k2 = N / (t + 1);
            rs->split = {Slice{tg->a, N, 0, k1}, Slice{tg->b, N, k1, k1}};
            rd->split_t = {Slice{tg->rt, N, 0, k2}};
            rd->split_2t = {Slice{tg->r2t, N, 0, k2}};
        }
        summ = tg->summ;
    }
    hbmpc_pipe* part(const std::string& name) override {
        return name == "ransha" ? (hbmpc_pipe*)rs.get() : name == "randousha" ? (hbmpc_pipe*)rd.get() : name == "triplegen" ? (hbmpc_pipe*)tg.get() : nullptr;
    }
    void run() override {
        rs->checked = rd->checked = tg->checked = checked;
        rs->run();
        rd->run();
        if (!in_place) {
            // the parties' lists, in the reference's order, become TripleGen's [party][N] inputs: one copy per array for all parties
            const size_t eb = f.eb;
            PL(hbmpc_memcpy_d2d_rows(ctx, tg->a, N * eb, rs->out, rs->nout * eb, N * eb, n, stream));
            PL(hbmpc_memcpy_d2d_rows(ctx, tg->b, N * eb, rs->out + N * eb, rs->nout * eb, N * eb, n, stream));
            PL(hbmpc_memcpy_d2d_rows(ctx, tg->rt, N * eb, rd->out_t, rd->nout * eb, N * eb, n, stream));
            PL(hbmpc_memcpy_d2d_rows(ctx, tg->r2t, N * eb, rd->out_2t, rd->nout * eb, N * eb, n, stream));
        }
        tg->run();
    }
    void verdict(uint32_t out[2]) override {  // both producers: the sum of the failed checks, the first failing element of the first that failed
        uint32_t a[2], b[2];
        rs->verdict(a);
        rd->verdict(b);
        out[0] = a[0] + b[0];
        out[1] = a[0] ? a[1] : b[1];
    }
};

// RandBit of N shared values for n parties (fpmul/rand_bit.rs:242-293, 197-220; either field).  Both opens are BatchRecon of
// degree t (N is a multiple of t + 1, so Multiply never takes the RBC path: mul/multiplication.rs:417-462): every party's encode of its
// chunks of t + 1, the recipients' P(0) decodes from senders 0 .. 2t, the coefficient decode of the revealed values from the same.
struct RandBit : hbmpc_pipe {
    size_t n, t, N, Gde, Gsq;
    unsigned char *a, *ta, *tb, *tc, *out, *sq, *sqop, *desh, *Y, *Z, *deop;
    uint8_t *status, *rst_de, *rst_sq;
    hbmpc_recover_summary *sm_de_first, *sm_de, *sm_sq_first;  // summ: summary_sq
    hbmpc_randbit_summary* rb;
    RandBit(hbmpc_ctx* cx, size_t n_, size_t t_, size_t N_, void* s) : hbmpc_pipe(cx, s), n(n_), t(t_), N(N_) {
        if (n == 0 || N == 0 || N % (t + 1) != 0 || n < 2 * t + 1) throw PipeError{InvalidInput};  // rand_bit.rs:253-255
        Gde = 2 * N / (t + 1), Gsq = N / (t + 1);
        arena((8 * n * N + n * n * Gde + n * Gde + 3 * N) * f.eb + N + 2 * n * Gde + (1 << 14));
        a = take("a", n * N), ta = take("ta", n * N), tb = take("tb", n * N), tc = take("tc", n * N);
        out = take("out", n * N), sq = take("sq", n * N);
        desh = take("desh", 2 * n * N);  // [party][2][N]: ta - a, then tb - a
        Y = take("Y", n * n * Gde);      // [party][recipient][chunk]: the encoded messages (both opens)
        Z = take("Z", n * Gde);          // [recipient][chunk]: the revealed values
        deop = take("deop", 2 * N);      // the opened d [N], then e [N]
        sqop = take("sqop", N);
        status = take_bytes("status", N, N);
        rst_de = take_bytes("rstatus_de", n * Gde, n * Gde);
        rst_sq = take_bytes("rstatus_sq", n * Gsq, n * Gsq);
        rb = reinterpret_cast<hbmpc_randbit_summary*>(take_bytes("summary", 64, 16));
        sm_de_first = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary_de_first", 64, 16));
        sm_de = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary_de", 64, 16));
        sm_sq_first = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary_sq_first", 64, 16));
        summ = reinterpret_cast<hbmpc_recover_summary*>(take_bytes("summary_sq", 64, 16));
    }
    void run() override {
        // one call for the whole protocol: one launch for a small batch, nine otherwise (hbmpc_[gl_]dev_randbit_parties)
        PL(f.randbit_parties(ctx, a, ta, tb, tc, N, n, t, desh, Y, Z, deop, sq, sqop, out, status, rst_de, rst_sq, sm_de_first, sm_de, sm_sq_first, summ,
                             rb, stream));
        if (!checked) return;
        // the opens' `?` in their order, then phase 2's (rand_bit.rs:198-207): the first summary that failed decides, read after ONE
        // synchronisation (the later steps have run by then)
        hbmpc_recover_summary v[4];
        hbmpc_randbit_summary r;
        hbmpc_recover_summary* const order[4] = {sm_de_first, sm_de, sm_sq_first, summ};
        for (int i = 0; i < 4; ++i) PL(hbmpc_memcpy_d2h(ctx, &v[i], order[i], sizeof v[i], stream));
        PL(hbmpc_memcpy_d2h(ctx, &r, rb, sizeof r, stream));
        PL(hbmpc_stream_sync(ctx, stream));
        for (int i = 0; i < 4; ++i)
            if (v[i].n_failed != 0) throw PipeError{(ShareErrorCode)v[i].first_error};
        if (r.n_failed != 0) throw PipeError{(r.first >> 32) == 1 ? HBMPC_ZERO_SQUARE : HBMPC_NO_SQUARE_ROOT};
    }
};

}  // namespace

extern "C" ShareErrorCode hbmpc_pipe_triplegen_create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream, hbmpc_pipe** pipe_out) {
    return create<TripleGen>(ctx, pipe_out, n, t, N, stream);
}
extern "C" ShareErrorCode hbmpc_pipe_fpmul_create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t k, size_t m, size_t open_senders,
                                                  void* stream, hbmpc_pipe** pipe_out) {
    return create<FpMul>(ctx, pipe_out, n, t, N, k, m, open_senders, stream);
}
extern "C" ShareErrorCode hbmpc_pipe_truncpr_create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t k, size_t m, size_t open_senders,
                                                    int with_multiplier, void* stream, hbmpc_pipe** pipe_out) {
    return create<TruncPr>(ctx, pipe_out, n, t, N, k, m, open_senders, with_multiplier, stream);
}
extern "C" ShareErrorCode hbmpc_pipe_mul_create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, size_t open_senders, void* stream,
                                                hbmpc_pipe** pipe_out) {
    return create<Mul>(ctx, pipe_out, n, t, N, open_senders, stream);
}
extern "C" ShareErrorCode hbmpc_pipe_ransha_create(hbmpc_ctx* ctx, size_t n, size_t t, size_t K, size_t verify_senders, void* stream,
                                                   hbmpc_pipe** pipe_out) {
    return create<RanSha>(ctx, pipe_out, n, t, K, verify_senders, stream);
}
extern "C" ShareErrorCode hbmpc_pipe_randousha_create(hbmpc_ctx* ctx, size_t n, size_t t, size_t K, void* stream, hbmpc_pipe** pipe_out) {
    return create<RanDouSha>(ctx, pipe_out, n, t, K, stream);
}
extern "C" ShareErrorCode hbmpc_pipe_preprocessing_create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream, hbmpc_pipe** pipe_out) {
    return create<Preprocessing>(ctx, pipe_out, n, t, N, stream);
}
extern "C" ShareErrorCode hbmpc_pipe_randbit_create(hbmpc_ctx* ctx, size_t n, size_t t, size_t N, void* stream, hbmpc_pipe** pipe_out) {
    return create<RandBit>(ctx, pipe_out, n, t, N, stream);
}
extern "C" void hbmpc_pipe_destroy(hbmpc_pipe* pipe) { delete pipe; }
extern "C" ShareErrorCode hbmpc_pipe_part(hbmpc_pipe* pipe, const char* name, hbmpc_pipe** part_out) {
    if (!pipe || !name || !part_out) return InvalidInput;
    *part_out = pipe->part(name);
    return *part_out ? ShareSuccess : InvalidInput;
}
extern "C" ShareErrorCode hbmpc_pipe_buffer(hbmpc_pipe* pipe, const char* name, void** dev_out, size_t* elements_out) {
    if (!pipe || !name) return InvalidInput;
    const auto it = pipe->buffers.find(name);
    if (it == pipe->buffers.end()) return InvalidInput;
    if (dev_out) *dev_out = it->second.p;
    if (elements_out) *elements_out = it->second.elements;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_pipe_upload(hbmpc_pipe* pipe, const char* name, const void* host, size_t elements) {
    if (!pipe || !name || !host) return InvalidInput;
    const auto it = pipe->buffers.find(name);
    if (it == pipe->buffers.end() || elements > it->second.elements) return InvalidInput;
    return hbmpc_memcpy_h2d(pipe->ctx, it->second.p, host, elements * pipe->ebytes_of(it->second), pipe->stream);
}
extern "C" ShareErrorCode hbmpc_pipe_download(hbmpc_pipe* pipe, const char* name, void* host, size_t elements) {
    if (!pipe || !name || !host) return InvalidInput;
    const auto it = pipe->buffers.find(name);
    if (it == pipe->buffers.end() || elements > it->second.elements) return InvalidInput;
    const ShareErrorCode rc = hbmpc_memcpy_d2h(pipe->ctx, host, it->second.p, elements * pipe->ebytes_of(it->second), pipe->stream);
    return rc != ShareSuccess ? rc : hbmpc_stream_sync(pipe->ctx, pipe->stream);
}
extern "C" ShareErrorCode hbmpc_pipe_set_checked(hbmpc_pipe* pipe, int on) {
    if (!pipe) return InvalidInput;
    pipe->checked = on != 0;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_pipe_run(hbmpc_pipe* pipe) {
    if (!pipe) return InvalidInput;
    return guarded([&] { pipe->run(); });
}
extern "C" ShareErrorCode hbmpc_pipe_deal(hbmpc_pipe* pipe) {
    if (!pipe) return InvalidInput;
    return guarded([&] { pipe->deal(); });
}
extern "C" ShareErrorCode hbmpc_pipe_finish(hbmpc_pipe* pipe) {
    if (!pipe) return InvalidInput;
    return guarded([&] { pipe->finish(); });
}
// Two eager runs, then the same calls are recorded: nothing can be built during capture, and a mid-size decode builds its
// matrix-core table when it first sees a sender set -- the recorded launches are the ones an eager caller gets from then on.
extern "C" ShareErrorCode hbmpc_pipe_capture(hbmpc_pipe* pipe) {
    if (!pipe || !pipe->stream) return InvalidInput;  // capture needs an explicit stream
    return guarded([&] {
        pipe->before_capture();
        const bool was_checked = pipe->checked;
        pipe->checked = false;  // a captured run only enqueues
        struct Restore {
            hbmpc_pipe* p;
            bool v;
            ~Restore() { p->checked = v; }
        } restore{pipe, was_checked};
        pipe->run();
        pipe->run();
        PL(hbmpc_stream_sync(pipe->ctx, pipe->stream));
        PL(hbmpc_graph_begin_capture(pipe->ctx, pipe->stream));
        try {
            pipe->run();
        } catch (...) {
            hbmpc_graph* g = nullptr;
            (void)hbmpc_graph_end_capture(pipe->ctx, pipe->stream, &g);
            hbmpc_graph_destroy(g);
            throw;
        }
        hbmpc_graph_destroy(pipe->graph);
        pipe->graph = nullptr;
        PL(hbmpc_graph_end_capture(pipe->ctx, pipe->stream, &pipe->graph));
    });
}
extern "C" ShareErrorCode hbmpc_pipe_replay(hbmpc_pipe* pipe) {
    if (!pipe || !pipe->graph) return InvalidInput;
    const ShareErrorCode rc = hbmpc_graph_launch(pipe->ctx, pipe->graph, pipe->stream);
    if (rc == ShareSuccess) pipe->replayed();
    return rc;
}
extern "C" ShareErrorCode hbmpc_pipe_sync(hbmpc_pipe* pipe) {
    if (!pipe) return InvalidInput;
    return hbmpc_stream_sync(pipe->ctx, pipe->stream);
}
extern "C" ShareErrorCode hbmpc_pipe_summary(hbmpc_pipe* pipe, hbmpc_recover_summary* summary_out) {
    if (!pipe || !summary_out || !pipe->summ) return InvalidInput;
    const ShareErrorCode rc = hbmpc_memcpy_d2h(pipe->ctx, summary_out, pipe->summ, sizeof *summary_out, pipe->stream);
    return rc != ShareSuccess ? rc : hbmpc_stream_sync(pipe->ctx, pipe->stream);
}
extern "C" ShareErrorCode hbmpc_pipe_verdict(hbmpc_pipe* pipe, uint32_t verdict_out[2]) {
    if (!pipe || !verdict_out) return InvalidInput;
    return guarded([&] { pipe->verdict(verdict_out); });
}
