// pipe_internal.hpp -- struct hbmpc_pipe and its helpers: what the files that implement hbmpc_pipe_* handles share
// (capi_pipelines.hip, capi_pipelines_riss.hip, capi_pipelines_io.hip, capi_pipelines_fixedprep.hip).  Like them it is a CLIENT of the public header only and compiles with a host C++ compiler.
#pragma once
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hbmpc_hip.h"

namespace hbmpc_pipes {  // named: struct hbmpc_pipe has members of these types and is defined in two translation units

struct PipeError {
    ShareErrorCode rc;
};
#define PL(call)                              \
    do {                                      \
        const ShareErrorCode rc_ = (call);    \
        if (rc_ != ShareSuccess) throw PipeError{rc_}; \
    } while (0)

// the two fields' entry points behind one signature (elements are 32-byte U256 or 8-byte uint64_t): every cast of a two-field buffer is here
struct Calls {
    bool gl;
    size_t eb;  // bytes per element
    using G = uint64_t;
    using F = U256;
    ShareErrorCode compute_shares(hbmpc_ctx* c, const void* co, size_t B, size_t n, size_t d, void* out, void* s) const {
        return gl ? hbmpc_gl_dev_compute_shares(c, (const G*)co, B, n, d, (G*)out, s) : hbmpc_dev_compute_shares(c, (const F*)co, B, n, d, (F*)out, s);
    }
    ShareErrorCode apply_parties(hbmpc_ctx* c, const void* x, size_t B, size_t n, size_t d, size_t parties, void* y, void* s) const {
        return gl ? hbmpc_gl_dev_vandermonde_apply_parties(c, (const G*)x, B, n, d, parties, (G*)y, s)
                  : hbmpc_dev_vandermonde_apply_parties(c, (const F*)x, B, n, d, parties, (F*)y, s);
    }
    ShareErrorCode apply_rows_lists(hbmpc_ctx* c, const void* x, size_t stride, size_t B, size_t n, size_t d, void* tmp, void* y, size_t row0,
                                    size_t rows, size_t K, const hbmpc_list_slice* sl, size_t nsl, void* s) const {
        return gl ? hbmpc_gl_dev_vandermonde_apply_rows_lists(c, (const G*)x, stride, B, n, d, (G*)tmp, (G*)y, row0, rows, K, sl, nsl, s)
                  : hbmpc_dev_vandermonde_apply_rows_lists(c, (const F*)x, stride, B, n, d, (F*)tmp, (F*)y, row0, rows, K, sl, nsl, s);
    }
    ShareErrorCode apply_rows_split(hbmpc_ctx* c, const void* x, size_t stride, size_t B, size_t n, size_t d, void* tmp, void* y, size_t row0,
                                    size_t rows, size_t K, const hbmpc_list_slice* sl, size_t nsl, void* others, void* s) const {
        return gl ? hbmpc_gl_dev_vandermonde_apply_rows_split(c, (const G*)x, stride, B, n, d, (G*)tmp, (G*)y, row0, rows, K, sl, nsl, (G*)others, s)
                  : hbmpc_dev_vandermonde_apply_rows_split(c, (const F*)x, stride, B, n, d, (F*)tmp, (F*)y, row0, rows, K, sl, nsl, (F*)others, s);
    }
    ShareErrorCode interpolate_c0(hbmpc_ctx* c, const size_t* ids, size_t S, const void* ev, size_t stride, size_t B, size_t n, void* tmp,
                                  void* c0, uint32_t* deg, void* s) const {
        return gl ? hbmpc_gl_dev_batch_interpolate_c0(c, ids, S, (const G*)ev, stride, B, n, (G*)tmp, (G*)c0, deg, s)
                  : hbmpc_dev_batch_interpolate_c0(c, ids, S, (const F*)ev, stride, B, n, (F*)tmp, (F*)c0, deg, s);
    }
    // Fr only: Goldilocks has no selective decode
    ShareErrorCode interpolate_degree_check(hbmpc_ctx* c, const size_t* ids, size_t S, const void* ev, size_t stride, size_t B, size_t n, size_t d,
                                            size_t groups, size_t group_stride, void* ws, void* sel, uint8_t* st, void* s) const {
        return gl ? TypeMismatch
                  : hbmpc_dev_interpolate_degree_check_strided(c, ids, S, (const F*)ev, stride, B, n, d, groups, group_stride, (F*)ws, (F*)sel, st, s);
    }
    ShareErrorCode recover_check_degree(hbmpc_ctx* c, const size_t* ids, size_t S, const void* ev, size_t stride, size_t B, size_t n, size_t t,
                                        size_t groups, size_t group_stride, void* ws, uint8_t* st, hbmpc_recover_summary* sm, uint32_t* bad,
                                        void* s) const {
        return gl ? hbmpc_gl_dev_recover_check_degree_strided(c, ids, S, (const G*)ev, stride, B, n, t, groups, group_stride, (G*)ws, st, sm, bad, s)
                  : hbmpc_dev_recover_check_degree_strided(c, ids, S, (const F*)ev, stride, B, n, t, groups, group_stride, (F*)ws, st, sm, bad, s);
    }
    ShareErrorCode triplegen_parties(hbmpc_ctx* c, const void* a, const void* b, const void* r2t, const void* rt, size_t N, size_t n, size_t t, void* Y,
                                     void* Z, void* opened, void* out, uint8_t* st, hbmpc_recover_summary* sf, hbmpc_recover_summary* sm, void* s) const {
        return gl ? hbmpc_gl_dev_triplegen_parties(c, (const G*)a, (const G*)b, (const G*)r2t, (const G*)rt, N, n, t, (G*)Y, (G*)Z, (G*)opened, (G*)out, st,
                                                   sf, sm, s)
                  : hbmpc_dev_triplegen_parties(c, (const F*)a, (const F*)b, (const F*)r2t, (const F*)rt, N, n, t, (F*)Y, (F*)Z, (F*)opened, (F*)out, st, sf,
                                                sm, s);
    }
    ShareErrorCode mul_parties(hbmpc_ctx* c, const size_t* ids, size_t S, const void* ta, const void* tb, const void* tc, const void* x, const void* y,
                               size_t N, size_t n, size_t t, void* desh, void* deop, void* out, uint8_t* st, hbmpc_recover_summary* sm, void* s) const {
        return gl ? hbmpc_gl_dev_mul_parties(c, ids, S, (const G*)ta, (const G*)tb, (const G*)tc, (const G*)x, (const G*)y, N, n, t, (G*)desh, (G*)deop,
                                             (G*)out, st, sm, s)
                  : hbmpc_dev_mul_parties(c, ids, S, (const F*)ta, (const F*)tb, (const F*)tc, (const F*)x, (const F*)y, N, n, t, (F*)desh, (F*)deop,
                                          (F*)out, st, sm, s);
    }
    ShareErrorCode batchrecon_parties(hbmpc_ctx* c, const size_t* ids1, size_t S1, const size_t* ids2, size_t S2, const void* x, size_t N, size_t n,
                                      size_t d, size_t t, void* Y, void* Z, void* opened, uint8_t* rst, uint8_t* st, hbmpc_recover_summary* sf,
                                      hbmpc_recover_summary* sm, void* s) const {
        return gl ? hbmpc_gl_dev_batchrecon_parties(c, ids1, S1, ids2, S2, (const G*)x, N, n, d, t, (G*)Y, (G*)Z, (G*)opened, rst, st, sf, sm, s)
                  : hbmpc_dev_batchrecon_parties(c, ids1, S1, ids2, S2, (const F*)x, N, n, d, t, (F*)Y, (F*)Z, (F*)opened, rst, st, sf, sm, s);
    }
    ShareErrorCode recover_slots(hbmpc_ctx* c, const size_t* ids, size_t S, const void* ev, size_t stride, size_t B, size_t n, size_t d, size_t t,
                                 int p0_only, void* out, uint8_t* st, hbmpc_recover_summary* sm, void* s) const {
        return gl ? hbmpc_gl_dev_batch_recover_slots(c, ids, ids, S, (const G*)ev, stride, B, n, d, t, p0_only, (G*)out, nullptr, st, sm, s)
                  : hbmpc_dev_batch_recover_slots(c, ids, ids, S, (const F*)ev, stride, B, n, d, t, p0_only, (F*)out, nullptr, st, sm, s);
    }
    ShareErrorCode randbit_parties(hbmpc_ctx* c, const void* a, const void* ta, const void* tb, const void* tc, size_t N, size_t n, size_t t, void* desh,
                                   void* Y, void* Z, void* deop, void* sq, void* sqop, void* out, uint8_t* st, uint8_t* rde, uint8_t* rsq,
                                   hbmpc_recover_summary* s1, hbmpc_recover_summary* s2, hbmpc_recover_summary* s3, hbmpc_recover_summary* s4,
                                   hbmpc_randbit_summary* rb, void* s) const {
        return gl ? hbmpc_gl_dev_randbit_parties(c, (const G*)a, (const G*)ta, (const G*)tb, (const G*)tc, N, n, t, (G*)desh, (G*)Y, (G*)Z, (G*)deop, (G*)sq,
                                                 (G*)sqop, (G*)out, st, rde, rsq, s1, s2, s3, s4, rb, s)
                  : hbmpc_dev_randbit_parties(c, (const F*)a, (const F*)ta, (const F*)tb, (const F*)tc, N, n, t, (F*)desh, (F*)Y, (F*)Z, (F*)deop, (F*)sq,
                                              (F*)sqop, (F*)out, st, rde, rsq, s1, s2, s3, s4, rb, s);
    }
};

struct Buffer {
    unsigned char* p;
    size_t elements;  // of the context's field (status / verdict buffers: bytes)
    size_t eb = 0;    // bytes per element where the buffer has a type of its own (the two-field handles: 8, 32 or 1); 0: the context's field
};
// where a slice of every party's output list goes instead of the producer's own buffer: hbmpc_list_slice {dst, party stride,
// k0, count} = batch elements [k0, k0 + count) of party p to dst + p * stride (elements)
using Slice = hbmpc_list_slice;

// the one thing a handle takes from the library that the public header does not offer: the calling thread's hbmpc_last_error text, for
// a refusal that is the handle's own (defined beside that text, hbmpc_capi.hip)
void set_last_error(const char* msg);
// a seeded RISS handle refuses hbmpc_pipe_capture: every replay of the recording would draw the same stream positions again
[[noreturn]] inline void refuse_seeded_capture() {
    set_last_error("a seeded handle cannot be captured: a replayed graph would reuse the same stream positions");
    throw PipeError{InvalidInput};
}

}  // namespace hbmpc_pipes
using namespace hbmpc_pipes;

struct hbmpc_pipe {
    hbmpc_ctx* ctx;
    void* stream;
    Calls f;
    bool checked = false;
    hbmpc_graph* graph = nullptr;
    unsigned char* base = nullptr;  // one hbmpc_dev_alloc block, bump-allocated (no per-step allocations)
    size_t size = 0, off = 0;
    std::map<std::string, Buffer> buffers;
    hbmpc_recover_summary* summ = nullptr;  // the summary of the last decode
    uint32_t* bad = nullptr;                // producers: {verifier checks that failed, first failing batch element}

    hbmpc_pipe(hbmpc_ctx* c, void* s) : ctx(c), stream(s) {
        const bool gl = hbmpc_field_of(c) == Goldilocks64;
        f = Calls{gl, (size_t)(gl ? 8 : 32)};
    }
    virtual ~hbmpc_pipe() {
        hbmpc_graph_destroy(graph);
        if (base) (void)hbmpc_dev_free(ctx, base);
    }
    void arena(size_t bytes) {
        void* p = nullptr;
        PL(hbmpc_dev_alloc(ctx, bytes, &p));
        base = static_cast<unsigned char*>(p), size = bytes;
    }
    unsigned char* take_bytes(const char* name, size_t bytes, size_t elements) {
        const size_t padded = (bytes + 255) & ~(size_t)255;
        if (off + padded > size) throw PipeError{InvalidInput};
        unsigned char* p = base + off;
        off += padded;
        if (name) buffers[name] = Buffer{p, elements};
        return p;
    }
    unsigned char* take(const char* name, size_t elements) { return take_bytes(name, elements * f.eb, elements); }
    // a buffer with an element size of its own: hbmpc_pipe_upload / _download count its elements
    unsigned char* take_typed(const char* name, size_t elements, size_t eb) {
        unsigned char* p = take_bytes(name, elements * eb, elements);
        buffers[name].eb = eb;
        return p;
    }
    size_t ebytes_of(const Buffer& b) const { return b.eb ? b.eb : f.eb; }
    virtual void run() = 0;  // enqueue only (checked: summaries are read back after every decode)
    virtual void deal() { throw PipeError{InvalidInput}; }
    virtual void finish() { throw PipeError{InvalidInput}; }
    virtual hbmpc_pipe* part(const std::string&) { return nullptr; }
    virtual void replayed() {}  // hbmpc_pipe_replay has enqueued the recording: host-side state that run() resets (fixedprep's cursors)
    virtual void before_capture() {}  // hbmpc_pipe_capture, before anything runs: a handle that cannot be recorded throws (the seeded RISS handles)
    virtual void set_stream_index(uint64_t) { throw PipeError{InvalidInput}; }  // hbmpc_pipe_set_stream_index: the seeded RISS handles
    virtual void verdict(uint32_t out[2]) {
        if (!bad) throw PipeError{InvalidInput};
        PL(hbmpc_memcpy_d2h(ctx, out, bad, 8, stream));
        PL(hbmpc_stream_sync(ctx, stream));
    }
    void check_summary(const hbmpc_recover_summary* which = nullptr) {  // checked mode: a failed chunk ends the run where the reference's `?` would
        if (!checked) return;
        hbmpc_recover_summary s;
        PL(hbmpc_memcpy_d2h(ctx, &s, which ? which : summ, sizeof s, stream));
        PL(hbmpc_stream_sync(ctx, stream));
        if (s.n_failed != 0) throw PipeError{(ShareErrorCode)s.first_error};
    }
    void clear_bad() {
        static const uint32_t init[2] = {0u, 0xffffffffu};
        PL(hbmpc_memcpy_h2d(ctx, bad, init, sizeof init, stream));
    }
};

namespace {

template <class F>
ShareErrorCode guarded(F&& fn) {
    try {
        fn();
        return ShareSuccess;
    } catch (const PipeError& e) {
        return e.rc;
    } catch (const std::bad_alloc&) {
        return InvalidInput;
    }
}
template <class P, class... A>
ShareErrorCode create(hbmpc_ctx* ctx, hbmpc_pipe** out, A... args) {
    if (!ctx || !out) return InvalidInput;
    *out = nullptr;
    return guarded([&] { *out = new P(ctx, args...); });
}

}  // namespace
