// capi_pipelines_fixedprep.hip -- the FixedPrep handle behind the C ABI (hbmpc_pipe_fixedprep_create, _take, _available): the second
// half of run_preprocessing for all n parties, i.e. one refill of the r_bits / r_int pools that mul_fixed drains.
//
//   fixedprep   RanSha -> DouSha / RanDouSha -> TripleGen -> RandBit over Goldilocks, then PRandBit and PRandInt over Fr
//               honeybadger/mod.rs:1396-1410, ensure_prandbit_shares :1951-2086, ensure_prandint_shares :2088-2150; the pools' order
//               preprocessing.rs:126-163; the consumer's takes mod.rs:1031-1045
//
// A file of its own for the reason capi_pipelines_riss.hip is one, and a CLIENT of the public header only (pipe_internal.hpp: struct
// hbmpc_pipe): the six parts are the handles hbmpc_pipe_*_create makes, reached through hbmpc_pipe_buffer / _deal / _finish / _run like
// any caller's; the two producers run as hbmpc_gl_dev_ransha_parties / _randousha_parties on the parts' buffers (ONE launch each for a
// small batch), and the moves between the parts are hbmpc_dev_take_rows -- one per cut.  It compiles with a host C++ compiler.
#include "pipe_internal.hpp"

namespace {

size_t round_up(size_t x, size_t to) { return (x + to - 1) / to * to; }

struct FixedPrep : hbmpc_pipe {
    struct Part {  // an owned handle: destroyed with this one (also when the constructor throws half-way)
        hbmpc_pipe* p = nullptr;
        ~Part() { hbmpc_pipe_destroy(p); }
        unsigned char* buf(const char* name) const {
            void* d = nullptr;
            PL(hbmpc_pipe_buffer(p, name, &d, nullptr));
            return static_cast<unsigned char*>(d);
        }
    };
    struct OwnStream {  // declared before the parts, so destroyed after them
        hbmpc_ctx* ctx = nullptr;
        void* s = nullptr;
        ~OwnStream() {
            if (s) (void)hbmpc_stream_destroy(ctx, s);  // through the Goldilocks context: the stream's scratch (the decode counters) is its
        }
    };
    hbmpc_ctx* fr;
    size_t n, t, nbit, nint, R = 0, T = 0, K1 = 0, K2 = 0;
    OwnStream own;
    Part rs, rd, tg, rb, pb, pi;
    std::vector<hbmpc_take_slice> cut_producers, cut_triples, cut_bits;
    unsigned char *r_bits = nullptr, *r_int = nullptr;
    // the producers as ONE device call each (hbmpc_gl_dev_ransha_parties / _randousha_parties: one launch for a small batch) on the
    // parts' coeffs, S, out and bad and on workspace of this handle -- below the sizes at which those calls send a caller to the handles
    bool calls = false;
    uint64_t *yv = nullptr, *ws1 = nullptr, *yv_t = nullptr, *yv_2t = nullptr, *ws2 = nullptr, *sel_t = nullptr, *sel_2t = nullptr;
    unsigned char *st_t = nullptr, *st_2t = nullptr;
    size_t cur_bits = 0, cur_ints = 0;
    bool filled = false;
    // seeded (hbmpc_pipe_fixedprep_create_seeded): both RISS parts are seeded handles; this handle's own `seeds` and index go to both
    // before they run (PRandBit draws in domain 0, PRandInt in domain 1), and the index then advances past the longer of the two ranges
    const bool seeded;
    unsigned char* seeds = nullptr;
    uint64_t index = 0;

    ~FixedPrep() override {
        (void)hbmpc_stream_sync(ctx, stream);
        hbmpc_graph_destroy(graph), graph = nullptr;  // before the stream it was recorded on
    }
    FixedPrep(hbmpc_ctx* gl, hbmpc_ctx* fr_, size_t n_, size_t t_, size_t nbit_, size_t nint_, size_t lk, void* s, bool seeded_)
        : hbmpc_pipe(gl, s), fr(fr_), n(n_), t(t_), nbit(nbit_), nint(nint_), seeded(seeded_) {
        if (hbmpc_field_of(fr) != Bls12_381Fr || hbmpc_field_of(gl) != Goldilocks64) throw PipeError{TypeMismatch};
        if ((nbit == 0 && nint == 0) || n <= 2 * t) throw PipeError{InvalidInput};
        if (!stream) {  // the two contexts' own streams differ: without a caller's stream every part works on one of the handle's
            PL(hbmpc_stream_create(ctx, &stream));
            own.ctx = ctx, own.s = stream;
        }
        if (nbit) {
            R = round_up(nbit, t + 1);                      // mod.rs:1973-1974
            T = round_up(R, 2 * t + 1);                     // :1998-2001
            K1 = (R + 2 * T + (n - 2 * t) - 1) / (n - 2 * t);  // :2004-2008, :1618-1619
            K2 = (T + t) / (t + 1);                         // :1816-1817
            PL(hbmpc_pipe_ransha_create(gl, n, t, K1, 0, stream, &rs.p));
            PL(hbmpc_pipe_randousha_create(gl, n, t, K2, stream, &rd.p));
            PL(hbmpc_pipe_triplegen_create(gl, n, t, T, stream, &tg.p));
            PL(hbmpc_pipe_randbit_create(gl, n, t, R, stream, &rb.p));
            PL((seeded ? hbmpc_pipe_prandbit_create_seeded : hbmpc_pipe_prandbit_create)(fr, gl, n, t, R, lk, 0, stream, &pb.p));
            calls = K1 < ((size_t)1 << 19) && n * n * K1 * 8 < ((size_t)1 << 32);  // K2 <= K1
            if (calls) {
                const size_t v2 = n - t - 1, w1 = 2 * n * n * K1 + (2 * t > t + 1 ? 2 * t : t + 1) * K1, w2 = 2 * n * n * K2 + v2 * n * K2;
                arena((n * 2 * t * K1 + w1 + 2 * n * v2 * K2 + w2 + 2 * v2 * K2) * 8 + 2 * 4 * v2 * K2 + (1 << 13) + (seeded ? n * 32 : 0));
                yv = (uint64_t*)take(nullptr, n * 2 * t * K1), ws1 = (uint64_t*)take(nullptr, w1);
                yv_t = (uint64_t*)take(nullptr, n * v2 * K2), yv_2t = (uint64_t*)take(nullptr, n * v2 * K2), ws2 = (uint64_t*)take(nullptr, w2);
                sel_t = (uint64_t*)take(nullptr, v2 * K2), sel_2t = (uint64_t*)take(nullptr, v2 * K2);
                st_t = take_bytes(nullptr, 4 * v2 * K2, 0), st_2t = take_bytes(nullptr, 4 * v2 * K2, 0);
            }
            // every take from the front (preprocessing.rs:126-163): a party's RanSha list is RandBit's a, then the triples' a, then their b
            const size_t l1 = (n - 2 * t) * K1, l2 = (t + 1) * K2;
            unsigned char* const out = rs.buf("out");
            cut_producers = {{out, l1, rb.buf("a"), R, R, 1},
                             {out + R * 8, l1, tg.buf("a"), T, T, 1},
                             {out + (R + T) * 8, l1, tg.buf("b"), T, T, 1},
                             {rd.buf("out_t"), l2, tg.buf("rt"), T, T, 1},
                             {rd.buf("out_2t"), l2, tg.buf("r2t"), T, T, 1}};
            cut_triples = {{tg.buf("a"), T, rb.buf("ta"), R, R, 1}, {tg.buf("b"), T, rb.buf("tb"), R, R, 1}, {tg.buf("c"), T, rb.buf("tc"), R, R, 1}};
            cut_bits = {{rb.buf("out"), R, pb.buf("b_q"), R, R, 1}};
            r_bits = pb.buf("b_p");
            buffers["r_bits"] = Buffer{r_bits, n * R, 32};
            buffers["r_bits2"] = Buffer{pb.buf("b_2"), n * R, 1};
            summ = reinterpret_cast<hbmpc_recover_summary*>(pb.buf("summary"));
        }
        if (nint) {
            PL((seeded ? hbmpc_pipe_prandint_create_seeded : hbmpc_pipe_prandint_create)(fr, n, t, nint, lk, stream, &pi.p));
            r_int = pi.buf("r_p");
            buffers["r_int"] = Buffer{r_int, n * nint, 32};
        }
        if (seeded) {
            if (!base) arena(n * 32 + 256);
            seeds = take_typed("seeds", n * 32, 1);
        }
    }
    hbmpc_pipe* part(const std::string& name) override {
        return name == "ransha" ? rs.p : name == "randousha" ? rd.p : name == "triplegen" ? tg.p : name == "randbit" ? rb.p : name == "prandbit" ? pb.p
               : name == "prandint" ? pi.p : nullptr;
    }
    void take_cut(const std::vector<hbmpc_take_slice>& cut) { PL(hbmpc_dev_take_rows(ctx, cut.data(), cut.size(), n, stream)); }
    void deal() override {  // the dealers' encodes of both producers
        if (!nbit) return;
        PL(hbmpc_pipe_deal(rs.p));
        PL(hbmpc_pipe_deal(rd.p));
    }
    // both producers: from the polynomials (run(): the dealt shares S are an output) or from the dealt shares (finish())
    void producers(bool from_coeffs) {
        if (!calls) {
            if (from_coeffs) deal();
            PL(hbmpc_pipe_finish(rs.p));
            PL(hbmpc_pipe_finish(rd.p));
            return;
        }
        auto u = [](unsigned char* p) { return reinterpret_cast<uint64_t*>(p); };
        PL(hbmpc_gl_dev_ransha_parties(ctx, from_coeffs ? u(rs.buf("coeffs")) : nullptr, u(rs.buf("S")), K1, n, t, 2 * t + 1, u(rs.buf("out")), yv, ws1,
                                       nullptr, nullptr, reinterpret_cast<uint32_t*>(rs.buf("bad")), stream));
        PL(hbmpc_gl_dev_randousha_parties(ctx, from_coeffs ? u(rd.buf("coeffs_t")) : nullptr, from_coeffs ? u(rd.buf("coeffs_2t")) : nullptr,
                                          u(rd.buf("S_t")), u(rd.buf("S_2t")), K2, n, t, u(rd.buf("out_t")), u(rd.buf("out_2t")), yv_t, yv_2t, ws2, sel_t,
                                          sel_2t, st_t, st_2t, reinterpret_cast<uint32_t*>(rd.buf("bad")), stream));
    }
    void finish() override { rest(false); }  // everything after the dealers' messages have arrived
    void rest(bool from_coeffs) {
        if (nbit) {
            producers(from_coeffs);
            take_cut(cut_producers);
            PL(hbmpc_pipe_run(tg.p));
            take_cut(cut_triples);  // the first R triples (mod.rs:2022-2026); T - R stay in TripleGen's buffers
            PL(hbmpc_pipe_run(rb.p));
            take_cut(cut_bits);
            seed_part(pb);
            PL(hbmpc_pipe_run(pb.p));
        }
        if (nint) {
            seed_part(pi);
            PL(hbmpc_pipe_run(pi.p));
        }
        if (seeded) index += R > nint ? R : nint;
        replayed();
        if (checked) check();
    }
    void seed_part(const Part& part) {
        if (!seeded) return;
        PL(hbmpc_memcpy_d2d(fr, part.buf("seeds"), seeds, n * 32, stream));
        PL(hbmpc_pipe_set_stream_index(part.p, index));
    }
    void before_capture() override {
        if (seeded) refuse_seeded_capture();
    }
    void set_stream_index(uint64_t i) override {
        if (!seeded) throw PipeError{InvalidInput};
        index = i;
    }
    void run() override { rest(true); }
    void replayed() override { cur_bits = cur_ints = 0, filled = true; }
    // The reference's `?`s in their order, read after ONE synchronisation (everything has run by then): a producer's verifier that says
    // no (the reference aborts there), TripleGen's two decodes, RandBit's four and its finalize, PRandBit's two.
    void check() {
        if (!nbit) {
            PL(hbmpc_stream_sync(ctx, stream));
            return;
        }
        uint32_t bad_rs[2], bad_rd[2];
        hbmpc_recover_summary v[8];
        hbmpc_randbit_summary r;
        const unsigned char* const order[8] = {tg.buf("summary_first"),    tg.buf("summary"),          rb.buf("summary_de_first"), rb.buf("summary_de"),
                                               rb.buf("summary_sq_first"), rb.buf("summary_sq"),       pb.buf("summary_first"),    pb.buf("summary")};
        PL(hbmpc_memcpy_d2h(ctx, bad_rs, rs.buf("bad"), sizeof bad_rs, stream));
        PL(hbmpc_memcpy_d2h(ctx, bad_rd, rd.buf("bad"), sizeof bad_rd, stream));
        for (int i = 0; i < 8; ++i) PL(hbmpc_memcpy_d2h(ctx, &v[i], order[i], sizeof v[i], stream));
        PL(hbmpc_memcpy_d2h(ctx, &r, rb.buf("summary"), sizeof r, stream));
        PL(hbmpc_stream_sync(ctx, stream));
        if (bad_rs[0] || bad_rd[0]) throw PipeError{DecodingError};
        for (int i = 0; i < 6; ++i)
            if (v[i].n_failed != 0) throw PipeError{(ShareErrorCode)v[i].first_error};
        if (r.n_failed != 0) throw PipeError{(r.first >> 32) == 1 ? HBMPC_ZERO_SQUARE : HBMPC_NO_SQUARE_ROOT};  // as hbmpc_pipe_randbit_create's handle
        for (int i = 6; i < 8; ++i)
            if (v[i].n_failed != 0) throw PipeError{(ShareErrorCode)v[i].first_error};
    }
    void verdict(uint32_t out[2]) override {  // both producers, combined as the preprocessing handle combines them
        if (!nbit) throw PipeError{InvalidInput};
        uint32_t a[2], b[2];
        PL(hbmpc_pipe_verdict(rs.p, a));
        PL(hbmpc_pipe_verdict(rd.p, b));
        out[0] = a[0] + b[0];
        out[1] = a[0] ? a[1] : b[1];
    }
    size_t bits_left() const { return filled ? R - cur_bits : 0; }
    size_t ints_left() const { return filled ? nint - cur_ints : 0; }
    ShareErrorCode take_front(size_t m, size_t N, void* rbits_dst, void* rint_dst) {
        if ((!rbits_dst && !rint_dst) || m == 0 || N == 0) return InvalidInput;
        if (rbits_dst && (m > bits_left() || N > bits_left() / m)) return InsufficientShares;
        if (rint_dst && N > ints_left()) return InsufficientShares;
        hbmpc_take_slice sl[2];
        size_t c = 0;
        if (rbits_dst) sl[c++] = {r_bits + cur_bits * 32, R, rbits_dst, m * N, m * N, m};  // element i owns bits i m .. i m + m - 1
        if (rint_dst) sl[c++] = {r_int + cur_ints * 32, nint, rint_dst, N, N, 1};
        const ShareErrorCode rc = hbmpc_dev_take_rows(fr, sl, c, n, stream);
        if (rc != ShareSuccess) return rc;
        if (rbits_dst) cur_bits += m * N;
        if (rint_dst) cur_ints += N;
        return ShareSuccess;
    }
};

}  // namespace

extern "C" ShareErrorCode hbmpc_pipe_fixedprep_create(hbmpc_ctx* ctx_fr, hbmpc_ctx* ctx_gl, size_t n, size_t t, size_t n_prandbit, size_t n_prandint,
                                                      size_t lk_bits, void* stream, hbmpc_pipe** pipe_out) {
    if (pipe_out) *pipe_out = nullptr;
    if (!ctx_fr) return InvalidInput;
    return create<FixedPrep>(ctx_gl, pipe_out, ctx_fr, n, t, n_prandbit, n_prandint, lk_bits, stream, false);
}
extern "C" ShareErrorCode hbmpc_pipe_fixedprep_create_seeded(hbmpc_ctx* ctx_fr, hbmpc_ctx* ctx_gl, size_t n, size_t t, size_t n_prandbit,
                                                             size_t n_prandint, size_t lk_bits, void* stream, hbmpc_pipe** pipe_out) {
    if (pipe_out) *pipe_out = nullptr;
    if (!ctx_fr) return InvalidInput;
    return create<FixedPrep>(ctx_gl, pipe_out, ctx_fr, n, t, n_prandbit, n_prandint, lk_bits, stream, true);
}
extern "C" ShareErrorCode hbmpc_pipe_fixedprep_take(hbmpc_pipe* prep, size_t m, size_t N, void* rbits_dst, void* rint_dst) {
    FixedPrep* const p = dynamic_cast<FixedPrep*>(prep);
    return p ? p->take_front(m, N, rbits_dst, rint_dst) : InvalidInput;
}
extern "C" ShareErrorCode hbmpc_pipe_fixedprep_available(hbmpc_pipe* prep, size_t out[2]) {
    FixedPrep* const p = dynamic_cast<FixedPrep*>(prep);
    if (!p || !out) return InvalidInput;
    out[0] = p->bits_left(), out[1] = p->ints_left();
    return ShareSuccess;
}
