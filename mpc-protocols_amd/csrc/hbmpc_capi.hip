// hbmpc_capi.hip -- the C ABI of include/hbmpc_hip.h: context, table cache, kernel dispatch.
// There is no CPU data path here and no device code either: host code validates arguments, builds the small constant
// tables (tables.hpp) and calls the launchers of launchers.hpp (the kernels and their launches are in tu_*.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hbmpc_hip.h"
#include "fr_gold.hpp"
#include "elem_args.hpp"
#include "kernels_fpmul_wave.hpp"
#include "kernels_truncpr_wave.hpp"
#include "kernels_mul_wave.hpp"
#include "kernels_input_wave.hpp"
#include "kernels_triplegen_wg.hpp"
#include "kernels_randbit_wg.hpp"
#include "kernels_batchrecon_wg.hpp"
#include "kernels_producers_wg.hpp"
#include "kernels_prandbit_wg.hpp"
#include "bfly_ring_plan.hpp"
#include "launchers.hpp"
#include "tables.hpp"
#include "tables_mfma.hpp"
#include "tables_mfma_gl.hpp"
#include "kernels_mfma.hpp"
#include "kernels_mfma_gl.hpp"
#include "encode_route.hpp"
#include "recover_route.hpp"
#include "protocol_route.hpp"
#include "producer_route.hpp"
#include "prandbit_route.hpp"
#include "take_plan.hpp"
#include "shamir_route.hpp"
#include "tables_sqrt.hpp"
#include "tables_riss.hpp"

using namespace hbmpc;

// hbmpc_[gl_]dev_randbit_parties as one launch: the defaults of hbmpc_set_fused_randbit per field, in chunks of t + 1 elements -- the
// largest swept size at which one launch measured ahead of or level with the nine, eager and replayed, at n = 16 and at n = 4
// (profiles/fused_randbit_sweep.txt; over Fr each element's 255-bit exponentiation runs on a single lane in either form)
constexpr size_t FUSED_RANDBIT_FR = 256, FUSED_RANDBIT_GL = 1024;
// hbmpc_dev_prandbit_parties / hbmpc_dev_prandint_parties as one launch: the default of hbmpc_set_fused_prandbit, in chunks of t + 1
// elements -- the largest swept count at which one launch was not slower than the composition of eight calls at (7,2) and at (10,3)
// (profiles/fused_prandbit_sweep.txt)
constexpr size_t FUSED_PRANDBIT = 256;
// hbmpc_[gl_]dev_batchrecon_parties as one launch: the defaults of hbmpc_set_fused_batchrecon per field, in chunks of d + 1 elements --
// the largest swept count at which one launch was not slower than the three launches at (4, 1, d = 1), (16, 5, d = 5) and
// (16, 5, d = 10), eager and replayed (profiles/fused_batchrecon_sweep.txt)
constexpr size_t FUSED_BATCHRECON_FR = 512, FUSED_BATCHRECON_GL = 256;
// hbmpc_[gl_]dev_ransha_parties / _randousha_parties as one launch: the defaults of hbmpc_set_fused_producers per field, in columns per
// dealer -- the largest swept count at which one launch was not slower than the separate launches at (4, 1), (7, 2) and (16, 5), both
// producers, both input modes, eager and replayed (profiles/fused_producers_sweep.txt)
constexpr size_t FUSED_PRODUCERS_FR = 256, FUSED_PRODUCERS_GL = 256;
constexpr size_t STAGE_PIN_BLOCK = (size_t)2048 << 10;  // pinned host block of the small-call staging path (Stage, hbmpc_scrub_staging)
struct hbmpc_ctx {
    int device = 0;
    int impl = IMPL_U29;
    bool force_generic = false;                    // tests: route every shape through the generic kernels
    hipStream_t stream = nullptr;
    std::mutex mu;                                 // guards the table cache, the scratch map and the staging pool
    std::mutex enqueue_mu;                         // keeps multi-launch sequences that share scratch contiguous on a stream
    struct Tab {
        uint32_t* p = nullptr;
        bool pinned = false;  // referenced by a captured HIP graph: never evicted
        std::array<size_t, 5> aux = {0, 0, 0, 0, 0};  // offsets inside the buffer (OEC/Gao tables): one unit with the table
    };
    struct Scratch {
        void* p = nullptr;
        size_t cap = 0;
        bool pinned = false;  // referenced by a captured HIP graph: never freed before hbmpc_destroy
        bool dirty = true;    // the batch_recover counters at its start are not known to be zero (fresh, or a failed call)
    };
    std::map<std::string, Tab> tables;             // device-resident constant tables
    std::vector<uint32_t*> retired_tables;         // evicted one flush ago; freed at the next flush (see get_table)
    std::vector<void*> retired_scratch;            // outgrown scratch that a graph may still reference
    size_t evictions = 0;                          // flushes of the table cache so far
    std::vector<void*> pin_free;                   // pinned, device-mapped staging blocks of small host-pointer calls (Stage)
    size_t wide_max_chunks = 8192;                 // batch_recover calls up to this many chunks (evaluations: a quarter of it) use the wave-per-chunk kernels
    bool second_chance = true;                     // flagged chunks try two cheap interpolation candidates before OEC/Gao
    bool direct_fail = true;                       // a decode with no OEC round (S == d + t + 1) is ONE launch: failures are written by the first kernel
    bool zero_copy = true;                         // small host-pointer calls stage through mapped host memory
    bool matrix_cores = true;                      // large Fr decodes run the int8 MFMA formulation (kernels_mfma.hpp)
    size_t mfma_min_cached = 4096;                 // Fr decodes take the matrix cores from this many chunks on (the crossover with the wave-per-chunk kernels)
    size_t mfma_min_direct = 2048;                 // ... and from this many when the call has no OEC round (one launch)
    size_t mfma_min_encode = 2049;                 // encodes (one table per (n, d), never rebuilt): right above the wave-per-chunk range
    int lazy_fallback_tables = 1;                  // a new sender set's OEC / Gao and second-chance tables are built when a chunk needs them: 1 = host-pointer calls, 2 = all
    bool device_tables = true;                     // the matrix-core table of a new sender set is expanded on the device (kernels_tables.hpp)
    size_t pair_decode_min = 8192;                // hbmpc_dev_fpmul_parties: from this many elements the first open forms its shares at load time
    size_t fused_triplegen_max = 1024;             // hbmpc_dev_triplegen_parties: one launch (a workgroup per chunk of 2t + 1 triples) up to this many chunks (0: never)
    size_t fused_fpmul_max = 2048;                 // hbmpc_dev_fpmul_parties: one launch (a wave per element) up to this many elements (0: never)
    size_t fused_truncpr_max = 768;                // hbmpc_dev_truncpr_parties: the same (profiles/fused_truncpr_sweep.txt: ahead or level, eager and replayed)
    size_t fused_mul_max = 1024;                   // hbmpc_dev_mul_parties: the same (profiles/fused_mul_sweep.txt: ahead both eager and replayed)
    size_t fused_input_max = 768;                  // hbmpc_dev_input_parties: the same (profiles/fused_input_sweep.txt)
    size_t fused_randbit_max = FUSED_RANDBIT_FR;   // hbmpc_dev_randbit_parties: one launch (a workgroup per chunk of t + 1 elements) up to this many chunks (0: never); per field, hbmpc_create
    size_t fused_batchrecon_max = FUSED_BATCHRECON_FR;  // hbmpc_dev_batchrecon_parties: one launch (a workgroup per chunk of d + 1 elements) up to this many chunks (0: never); per field, hbmpc_create
    size_t fused_producers_max = FUSED_PRODUCERS_FR;    // hbmpc_dev_ransha_parties / _randousha_parties: one launch (a workgroup per column) up to this many columns per dealer (0: never); per field, hbmpc_create
    size_t fused_prandbit_max = FUSED_PRANDBIT;    // hbmpc_dev_prandbit_parties / _prandint_parties (read from the Fr context): the same, in chunks of t + 1 elements
    bool gather_row_copies = false;                // hbmpc_dev_gather_party_major: take the per-row peer copies even where the 2-D copy applies (A/B aid)
    bool list_rows_in_kernel = true;               // the producers' mixing step writes the parties' lists itself (k_mfma_bfly<.., LISTS>)
    bool mfma_bfly = true;                         // large encodes take the domain points in pairs (kernels_mfma_bfly.hpp)
    int mfma_ring = 1;                             // the plain chunk-major point-pair encode reads through a loader wave and an LDS ring (kernels_mfma_bfly_ring.hpp):
                                                   // 1 = from bfly_ring_min_tiles on, 0 = never, 2 = at every size (hbmpc_set_matrix_cores 4 / 5)
    bool mfma_team = true;                         // batches with fewer tiles than waves: a workgroup per tile (kernels_mfma_team.hpp)
    size_t mfma_min_gold = 4096;                   // Goldilocks encodes (tiny tables, one workgroup kind): from this many chunks
    size_t mfma_min_gold_direct = 2048;            // Goldilocks decodes without OEC rounds (one launch): flat ~7 us against a wave-per-chunk kernel that grows
    size_t mfma_min_gold_oec = 8193;               // Goldilocks decodes with OEC rounds (four launches against the small-batch path's two): beyond its range
    std::map<size_t, HFr> inv_pow2;                // (2^m)^-1 per m: a field inversion is ~20 us of host time, more than a small launch
    std::map<size_t, std::shared_ptr<DomainInv<HFr>>> dom_fr;  // per n: domain elements + inverse differences (tables.hpp), built once
    std::map<size_t, std::shared_ptr<DomainInv<HGl>>> dom_gl;
    int n_cus = 256;
    int riss_form = 0;                             // RISS conversion (kernels_riss.hpp): 0 = by size, 1 = always 16 parties per workgroup, 2 = always one (A/B aid)
    int mfma_wgs = 0;                              // test aid: workgroups of a matrix-core launch (0 = one per CU)
    int shamir_route = 0;                          // test and sweep aid: the integer-point encode's forced route (shamir_route.hpp: SHAMIR_ROUTE_*)
    std::map<hipStream_t, Scratch> scratch;        // per-stream scratch (calls on one stream are ordered)
    std::vector<std::pair<void*, size_t>> stage_free;  // device staging buffers of the host-pointer API, kept between calls
    size_t stage_bytes = 0;
};

// the calling thread's last failure message (hbmpc_last_error): thread-local, so concurrent callers of one
// context never write the same string
static thread_local std::string g_err;
namespace hbmpc_pipes {
void set_last_error(const char* msg) { g_err = msg; }  // for a handle's own refusals (pipe_internal.hpp)
}
// > 0 while the calling thread is between hbmpc_graph_begin_capture and _end_capture (capture mode is thread-local):
// tables and scratch it looks up are then pinned for the graph's lifetime, and nothing may be allocated
static thread_local int g_capturing = 0;
static const ShareErrorCode HBMPC_NOT_FUSED = (ShareErrorCode)9999;  // internal: a fused form does not cover the call (nothing was enqueued)
// internal: batch_recover_dev was asked to form the senders' values at load time and the call cannot take that form

#define HIP_TRY(ctx, call)                                                                              \
    do {                                                                                                \
        hipError_t e__ = (call);                                                                        \
        if (e__ != hipSuccess) {                                                                        \
            (void)(ctx);                                                                                \
            g_err = std::string(#call) + ": " + hipGetErrorString(e__);                            \
            return e__ == hipErrorOutOfMemory ? HBMPC_OUT_OF_MEMORY : HBMPC_NO_DEVICE;                  \
        }                                                                                               \
    } while (0)

static ShareErrorCode fail(hbmpc_ctx* ctx, ShareErrorCode rc, const char* msg) {
    (void)ctx;
    g_err = msg;
    return rc;
}

static bool is_gold(const hbmpc_ctx* ctx) { return ctx->impl == IMPL_GOLD; }
static size_t ebytes(const hbmpc_ctx* ctx) { return impl_ebytes(ctx->impl); }
// entry points are typed per field (U256* vs uint64_t*): a context only serves the field it was created for
#define REQ_FR(ctx) do { if ((ctx) && is_gold(ctx)) return fail((ctx), TypeMismatch, "this context was created for Goldilocks: use the hbmpc_gl_* entry points"); } while (0)
#define REQ_GL(ctx) do { if ((ctx) && !is_gold(ctx)) return fail((ctx), TypeMismatch, "this context was created for bls12-381 Fr: hbmpc_gl_* needs a Goldilocks64 context"); } while (0)

// ---- table cache -------------------------------------------------------------------------------
// Looks the table up or builds it, all under ctx->mu.  `aux` (optional): in = what the builder computed alongside the
// words (read after build() returns), out = what is stored with the table -- a table and its offsets are published
// together, so a second thread that finds the table cached also finds its layout.
// frees a fresh device block unless it was published (the HIP_TRY early returns between hipMalloc and the cache entry)
struct DevBlockGuard {
    uint32_t* p = nullptr;
    ~DevBlockGuard() {
        if (p) (void)hipFree(p);
    }
    uint32_t* release() {
        uint32_t* q = p;
        p = nullptr;
        return q;
    }
};
// Bound the cache in a long-running node (every new sender set is a new table); ctx->mu is held.  Eviction is two-phase so
// that a concurrent call which has looked a table up but not launched yet never sees it freed: tables
// evicted now are only unlinked, and freed at the NEXT flush (>= 512 table builds later), after a device
// synchronise for kernels still running on caller streams.  Tables a captured graph references stay.
static void flush_tables_if_full(hbmpc_ctx* ctx) {
    if (ctx->tables.size() < 512) return;
    ++ctx->evictions;
    (void)hipDeviceSynchronize();
    for (uint32_t* q : ctx->retired_tables) (void)hipFree(q);
    ctx->retired_tables.clear();
    for (auto t = ctx->tables.begin(); t != ctx->tables.end();) {
        if (t->second.pinned) {
            ++t;
            continue;
        }
        ctx->retired_tables.push_back(t->second.p);
        t = ctx->tables.erase(t);
    }
}
template <class Build>
static ShareErrorCode get_table(hbmpc_ctx* ctx, const std::string& key, Build build, const uint32_t** out,
                                std::array<size_t, 5>* aux = nullptr) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->tables.find(key);
    if (it != ctx->tables.end()) {
        if (g_capturing) it->second.pinned = true;
        *out = it->second.p;
        if (aux) *aux = it->second.aux;
        return ShareSuccess;
    }
    if (g_capturing) return fail(ctx, HBMPC_NO_DEVICE, "a table would have to be built during graph capture: run the call sequence once eagerly first");
    flush_tables_if_full(ctx);
    std::vector<uint32_t> host = build();
    if (host.empty()) host.push_back(0);
    DevBlockGuard blk;
    HIP_TRY(ctx, hipMalloc(&blk.p, host.size() * 4));
    HIP_TRY(ctx, hipMemcpy(blk.p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    hbmpc_ctx::Tab& tab = ctx->tables[key];
    tab.p = blk.release();
    if (aux) tab.aux = *aux;
    *out = tab.p;
    return ShareSuccess;
}
// A table whose bulk is EXPANDED ON THE DEVICE from a small host-built seed (the matrix-core byte-digit table: a few KB of
// coefficients -> hundreds of KB): the entry is dev_words of table followed by the seed; `expand` enqueues the kernels on
// the context's own stream, which is drained before the entry is published -- so whichever stream or thread uses the
// entry next is ordered behind the build by the host, and the caller's stream is never waited for.
template <class Build, class Expand>
static ShareErrorCode get_table_expanded(hbmpc_ctx* ctx, const std::string& key, size_t dev_words, Build build_seed, Expand expand,
                                         const uint32_t** out) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->tables.find(key);
    if (it != ctx->tables.end()) {
        if (g_capturing) it->second.pinned = true;
        *out = it->second.p;
        return ShareSuccess;
    }
    if (g_capturing) return fail(ctx, HBMPC_NO_DEVICE, "a table would have to be built during graph capture: run the call sequence once eagerly first");
    flush_tables_if_full(ctx);
    // (ctx->mu is held across the build and the drain of the context's own stream: a second thread that wants the SAME new table
    // must find it finished, and builds are rare -- one per new sender set -- and short, two launches of a few microseconds)
    std::vector<uint32_t> seed = build_seed();
    DevBlockGuard blk;
    HIP_TRY(ctx, hipMalloc(&blk.p, (dev_words + seed.size() + 16) * 4));
    HIP_TRY(ctx, hipMemcpyAsync(blk.p + dev_words, seed.data(), seed.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    expand(blk.p, blk.p + dev_words, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // also keeps `seed` (pageable host memory) alive until the copy has run
    hbmpc_ctx::Tab& tab = ctx->tables[key];
    tab.p = blk.release();
    *out = tab.p;
    return ShareSuccess;
}
static bool table_cached(hbmpc_ctx* ctx, const std::string& key) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ctx->tables.find(key) != ctx->tables.end();
}
// Per-stream scratch from plain hipMalloc.  NOT hipMallocAsync: data written to stream-ordered-pool memory by
// one kernel was observed stale for workgroups of the NEXT kernel that run on other XCDs (their L2 kept the
// value an earlier memset/kernel had left there), which silently dropped flagged chunks; ordinary hipMalloc
// memory is coherent at kernel boundaries.  Calls on one stream are ordered, so they can share a buffer; it
// only grows (after draining the stream).
static ShareErrorCode get_scratch(hbmpc_ctx* ctx, hipStream_t s, size_t bytes, void** out, bool* dirty = nullptr) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto& slot = ctx->scratch[s];
    if (slot.cap < bytes) {
        if (g_capturing) return fail(ctx, HBMPC_NO_DEVICE, "scratch would have to grow during graph capture: run the call sequence once eagerly first");
        if (slot.p) {
            HIP_TRY(ctx, hipStreamSynchronize(s));
            if (slot.pinned) ctx->retired_scratch.push_back(slot.p);  // a graph replays kernels that point into it
            else HIP_TRY(ctx, hipFree(slot.p));
            slot = hbmpc_ctx::Scratch();
        }
        const size_t want = bytes < (1u << 16) ? (1u << 16) : bytes + bytes / 2;
        HIP_TRY(ctx, hipMalloc(&slot.p, want));
        slot.cap = want;
    }
    if (g_capturing) slot.pinned = true;
    if (dirty) *dirty = slot.dirty;
    *out = slot.p;
    return ShareSuccess;
}
static void set_scratch_dirty(hbmpc_ctx* ctx, hipStream_t s, bool dirty) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->scratch.find(s);
    if (it != ctx->scratch.end()) it->second.dirty = dirty;
}
// The decodes (batch_recover_dev and the one-launch protocol kernels) share the counters at the start of the stream's scratch
// (`bytes` of it; [0, 32) u32: counters[0..4), the local summary, the sub-tickets of finish_direct).  They are zero because the last
// kernel of the previous call on this stream left them so (k_unscale, or the last block of a one-launch kernel).  Fresh scratch,
// or a call that failed between its first and last launch, is the exception: then they are cleared here.  A graph capture records
// the clear under the same condition (as a node it costs ~4 us per decode and replay, more than a small decode itself): a replay
// finds the counters at zero because whatever ran before it on the stream left them so, and hbmpc_graph_launch clears them itself
// when a call has failed since (the scratch is then marked dirty).
// Two threads may drive one context (and so one stream): the launches of `enqueue(counters)` reach the stream as one uninterrupted
// sequence.  When it returns ShareSuccess its last kernel has left the counters at zero, and the scratch is marked clean again.
template <class Enqueue>
static ShareErrorCode with_decode_counters(hbmpc_ctx* ctx, hipStream_t s, size_t bytes, Enqueue enqueue) {
    std::lock_guard<std::mutex> enqueue_lock(ctx->enqueue_mu);
    void* scratch;
    bool dirty = false;
    ShareErrorCode rc = get_scratch(ctx, s, bytes, &scratch, &dirty);
    if (rc != ShareSuccess) return rc;
    uint32_t* counters = (uint32_t*)scratch;
    if (dirty) HIP_TRY(ctx, hipMemsetAsync(counters, 0, 128, s));
    set_scratch_dirty(ctx, s, true);
    rc = enqueue(counters);
    if (rc == ShareSuccess) set_scratch_dirty(ctx, s, false);
    return rc;
}
static std::string key(const char* kind, std::initializer_list<size_t> v, int impl) {
    std::string k = kind;
    for (size_t x : v) k += ":" + std::to_string(x);
    return k + "#" + std::to_string(impl);
}

static HFr rdev_value(int impl) {  // Rdev mod r as a field value: 2^256 (sat32) or 2^261 (u29)
    HFr two = HFr::from_u64(2), p = HFr::one();
    const int bits = impl == IMPL_U29 ? 261 : 256;
    for (int i = 0; i < bits; ++i) p = p * two;
    return p;
}
// r2: mont(x, r2) = x * Rdev (canonical -> Montgomery).  c0: a constant in device-constant form.
// c1_plain: a canonical value in plain limb form (for load_const).
static ElemConsts elem_consts(int impl, const HFr* c0 = nullptr, const HFr* c1_plain = nullptr) {
    ElemConsts cs = {};
    std::vector<uint32_t> v;
    if (impl == IMPL_GOLD) {  // no Montgomery form: mont(x, 1) = x
        cs.r2[0] = 1;
        return cs;
    }
    put_const(v, rdev_value(impl), impl);
    for (int i = 0; i < impl_nl(impl); ++i) cs.r2[i] = v[i];
    if (c0) {
        v.clear();
        put_const(v, *c0, impl);
        for (int i = 0; i < impl_nl(impl); ++i) cs.c0[i] = v[i];
    }
    if (c1_plain) {
        v.clear();
        put_plain(v, *c1_plain, impl);
        for (int i = 0; i < impl_nl(impl); ++i) cs.c1[i] = v[i];
    }
    return cs;
}

// (2^m)^-1, computed once per m and context (TruncPr's last step, truncpr.rs:216-220)
static HFr inv_pow2(hbmpc_ctx* ctx, size_t m) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->inv_pow2.find(m);
    if (it != ctx->inv_pow2.end()) return it->second;
    if (ctx->inv_pow2.size() > 4096) ctx->inv_pow2.clear();
    const HFr v = HFr::from_u64(2).pow_u64(m).inv();
    ctx->inv_pow2.emplace(m, v);
    return v;
}
// TruncPr's constants (truncpr.rs:277-297, 216-220): the table of 2^i, cs.c0 = 2^m, cs.c1 = 2^(k-1) in plain limbs and, for the
// one-launch kernels (the separate launches' last step fetches its own), ci.c0 = 2^-m
struct TruncprConsts {
    const uint32_t* pow2;
    ElemConsts cs, ci;
};
static ShareErrorCode truncpr_consts(hbmpc_ctx* ctx, size_t k, size_t m, bool inv, TruncprConsts* out) {
    const int impl = ctx->impl;
    const ShareErrorCode rc = get_table(ctx, key("pow2", {m}, impl), [&] { return build_pow2(m, impl); }, &out->pow2);
    if (rc != ShareSuccess) return rc;
    const HFr two = HFr::from_u64(2);
    const HFr p2m = two.pow_u64(m), p2k = two.pow_u64(k - 1);
    out->cs = elem_consts(impl, &p2m, &p2k);
    if (inv) {
        const HFr i2m = inv_pow2(ctx, m);
        out->ci = elem_consts(impl, &i2m);
    }
    return ShareSuccess;
}
// TruncPr's parameter checks, each asked for by its bit.  False: the message is set and the call answers InvalidInput.
enum { TP_K = 1, TP_M = 2, TP_BYTES = 4, TP_ALL = 7 };
static bool truncpr_params_ok(hbmpc_ctx* ctx, int which, size_t k, size_t m) {
    if ((which & TP_K) && k == 0) return fail(ctx, InvalidInput, "k must be >= 1 (2^(k-1))"), false;
    if ((which & TP_M) && m > 4096) return fail(ctx, InvalidInput, "m beyond the supported range"), false;
    // fpmul/mod.rs:381-406 indexes bytes[m/8] when m % 8 != 0: out of bounds (a panic) from m = 257 on
    if ((which & TP_BYTES) && m % 8 != 0 && m / 8 >= 32) return fail(ctx, InvalidInput, "m: bytes[m/8] out of bounds in the reference"), false;
    return true;
}
static bool batch_in_range(hbmpc_ctx* ctx, size_t N, size_t n) {  // N elements of each of n <= 255 parties; false as above
    return (N != 0 && n != 0 && n <= 255) || (fail(ctx, InvalidInput, "N, n out of range"), false);
}
// ---- context -----------------------------------------------------------------------------------
extern "C" const char* hbmpc_version(void) { return "hbmpc-hip 0.1 (gfx950)"; }

extern "C" ShareErrorCode hbmpc_create(int device, FieldKind field_kind, hbmpc_ctx** ctx_out) {
    if (!ctx_out) return InvalidInput;
    *ctx_out = nullptr;
    if (field_kind != Bls12_381Fr && field_kind != Goldilocks64) return TypeMismatch;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) {
        g_err = "hbmpc_create: no HIP device " + std::to_string(device) + " (this library has no CPU path)";
        return HBMPC_NO_DEVICE;
    }
    hbmpc_ctx* ctx = new hbmpc_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        g_err = "hbmpc_create: hipSetDevice/hipStreamCreate failed";
        delete ctx;
        return HBMPC_NO_DEVICE;
    }
    const char* env = getenv("HBMPC_FIELD_IMPL");
    if (env && std::string(env) == "sat32") ctx->impl = IMPL_SAT32;
    if (field_kind == Goldilocks64) ctx->impl = IMPL_GOLD, ctx->fused_randbit_max = FUSED_RANDBIT_GL, ctx->fused_batchrecon_max = FUSED_BATCHRECON_GL, ctx->fused_producers_max = FUSED_PRODUCERS_GL;
    env = getenv("HBMPC_MATRIX_CORES");
    if (env && std::string(env) == "0") ctx->matrix_cores = false;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ctx->n_cus = prop.multiProcessorCount;
    *ctx_out = ctx;
    return ShareSuccess;
}
// Staging memory of the host-pointer API holds copies of what callers passed in (polynomial coefficients, i.e. secrets,
// shares) until a later call overwrites it: zero what the pools hold.
extern "C" ShareErrorCode hbmpc_scrub_staging(hbmpc_ctx* ctx) {
    // (blocks checked out by a host-pointer call running on another thread, and the per-stream scratch, are not in the
    // pools and are not touched)
    if (!ctx) return InvalidInput;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (auto& b : ctx->stage_free) HIP_TRY(ctx, hipMemsetAsync(b.first, 0, b.second, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (void* q : ctx->pin_free) memset(q, 0, STAGE_PIN_BLOCK);
    return ShareSuccess;
}
extern "C" void hbmpc_destroy(hbmpc_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hbmpc_scrub_staging(ctx);
    for (auto& kv : ctx->tables) (void)hipFree(kv.second.p);
    for (uint32_t* q : ctx->retired_tables) (void)hipFree(q);
    for (auto& kv : ctx->scratch) (void)hipFree(kv.second.p);
    for (void* q : ctx->retired_scratch) (void)hipFree(q);
    for (void* q : ctx->pin_free) (void)hipHostFree(q);
    for (auto& b : ctx->stage_free) (void)hipFree(b.first);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}
extern "C" const char* hbmpc_last_error(const hbmpc_ctx*) { return g_err.c_str(); }
extern "C" FieldKind hbmpc_field_of(const hbmpc_ctx* ctx) { return ctx && is_gold(ctx) ? Goldilocks64 : Bls12_381Fr; }
extern "C" ShareErrorCode hbmpc_set_field_impl(hbmpc_ctx* ctx, int impl) {
    if (!ctx || (impl != IMPL_U29 && impl != IMPL_SAT32)) return InvalidInput;
    REQ_FR(ctx);
    ctx->impl = impl;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_set_matrix_cores(hbmpc_ctx* ctx, int on, size_t min_chunks) {  // either field
    if (!ctx) return InvalidInput;
    ctx->matrix_cores = on != 0;
    ctx->mfma_team = on != 2;  // 2: without the workgroup-per-tile kernel of small batches (A/B aid)
    ctx->mfma_bfly = on != 3;  // 3: large encodes with one table row per point instead of per point pair (A/B aid)
    // 4: the point-pair encode without the loader wave and its LDS ring, every wave gathering its own inputs (A/B aid); 5: with them at
    // every batch size, not only where they pay (test aid: a few tiles then reach every state of the ring)
    ctx->mfma_ring = on == 4 ? 0 : on == 5 ? 2 : 1;
    if (min_chunks) {
        ctx->mfma_min_gold = std::min<size_t>(min_chunks, 4096);
        ctx->mfma_min_gold_direct = std::min<size_t>(min_chunks, 2048);
        ctx->mfma_min_gold_oec = std::min<size_t>(min_chunks, 8193);
        ctx->mfma_min_cached = std::min<size_t>(min_chunks, 4096);
        ctx->mfma_min_direct = std::min<size_t>(min_chunks, 2048);
        ctx->mfma_min_encode = std::min<size_t>(min_chunks, 2049);
    }
    return ShareSuccess;
}
// the thresholds of the protocol calls' rule (protocol_route.hpp)
#define KNOB_SETTER(NAME, FIELD)                                   \
    extern "C" ShareErrorCode NAME(hbmpc_ctx* ctx, size_t value) { \
        if (!ctx) return InvalidInput;                             \
        ctx->FIELD = value;                                        \
        return ShareSuccess;                                       \
    }
KNOB_SETTER(hbmpc_set_fused_fpmul, fused_fpmul_max)
KNOB_SETTER(hbmpc_set_fused_truncpr, fused_truncpr_max)
KNOB_SETTER(hbmpc_set_fused_triplegen, fused_triplegen_max)
KNOB_SETTER(hbmpc_set_fused_mul, fused_mul_max)
KNOB_SETTER(hbmpc_set_fused_input, fused_input_max)
KNOB_SETTER(hbmpc_set_fused_randbit, fused_randbit_max)
KNOB_SETTER(hbmpc_set_fused_batchrecon, fused_batchrecon_max)
KNOB_SETTER(hbmpc_set_fused_producers, fused_producers_max)
KNOB_SETTER(hbmpc_set_fused_prandbit, fused_prandbit_max)
KNOB_SETTER(hbmpc_set_fpmul_pair_decode, pair_decode_min)
#undef KNOB_SETTER
extern "C" ShareErrorCode hbmpc_set_gather_row_copies(hbmpc_ctx* ctx, int on) {  // either field
    if (!ctx) return InvalidInput;
    ctx->gather_row_copies = on != 0;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_set_producer_fusion(hbmpc_ctx* ctx, int on) {  // either field
    if (!ctx) return InvalidInput;
    ctx->list_rows_in_kernel = on != 0;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_set_lazy_fallback_tables(hbmpc_ctx* ctx, int on) {  // either field
    if (!ctx) return InvalidInput;
    if (on < 0 || on > 2) return InvalidInput;
    ctx->lazy_fallback_tables = on;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_set_single_launch_decode(hbmpc_ctx* ctx, int on) {  // either field
    if (!ctx) return InvalidInput;
    ctx->direct_fail = on != 0;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_set_matrix_core_workgroups(hbmpc_ctx* ctx, int workgroups) {
    if (!ctx || workgroups < 0) return InvalidInput;
    ctx->mfma_wgs = workgroups;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_set_small_batch_chunks(hbmpc_ctx* ctx, size_t max_chunks) {
    if (!ctx) return InvalidInput;
    ctx->wide_max_chunks = max_chunks;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_set_second_chance(hbmpc_ctx* ctx, int on) {
    if (!ctx) return InvalidInput;
    ctx->second_chance = on != 0;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_cache_stats(hbmpc_ctx* ctx, size_t stats_out[4]) {
    if (!ctx || !stats_out) return InvalidInput;
    std::lock_guard<std::mutex> lk(ctx->mu);
    size_t pinned = 0;
    for (auto& kv : ctx->tables) pinned += kv.second.pinned;
    stats_out[0] = ctx->tables.size(), stats_out[1] = pinned, stats_out[2] = ctx->retired_tables.size(), stats_out[3] = ctx->evictions;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_set_force_generic(hbmpc_ctx* ctx, int on) {  // either field
    if (!ctx) return InvalidInput;
    ctx->force_generic = on != 0;
    return ShareSuccess;
}

extern "C" ShareErrorCode hbmpc_dev_alloc(hbmpc_ctx* ctx, size_t bytes, void** dptr_out) {
    if (!ctx || !dptr_out) return InvalidInput;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMalloc(dptr_out, bytes ? bytes : 1));
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_free(hbmpc_ctx* ctx, void* dptr) {
    if (!ctx) return InvalidInput;
    HIP_TRY(ctx, hipFree(dptr));
    return ShareSuccess;
}
// The stream-ordered pool of the context's device (hipMallocAsync): caller buffers from it are safe only while the pool retains its
// freed blocks (include/hbmpc_hip.h, "Device buffers").  Pointer attributes do not say which allocator a buffer came from
// (HIP_POINTER_ATTRIBUTE_MEMPOOL_HANDLE: hipErrorNotSupported on ROCm 7.2, tools/probe_pool_attr.hip), so the check is on the pool.
extern "C" ShareErrorCode hbmpc_stream_pool_release_threshold(hbmpc_ctx* ctx, uint64_t* threshold_out) {
    if (!ctx || !threshold_out) return InvalidInput;
    hipMemPool_t pool = nullptr;
    HIP_TRY(ctx, hipDeviceGetMemPool(&pool, ctx->device));
    HIP_TRY(ctx, hipMemPoolGetAttribute(pool, hipMemPoolAttrReleaseThreshold, threshold_out));
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_stream_pool_retain(hbmpc_ctx* ctx) {
    if (!ctx) return InvalidInput;
    hipMemPool_t pool = nullptr;
    uint64_t keep = ~0ull;
    HIP_TRY(ctx, hipDeviceGetMemPool(&pool, ctx->device));
    HIP_TRY(ctx, hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep));
    return ShareSuccess;
}
static hipStream_t pick(hbmpc_ctx* ctx, void* stream) { return stream ? (hipStream_t)stream : ctx->stream; }
extern "C" ShareErrorCode hbmpc_memcpy_h2d(hbmpc_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream) {
    if (!ctx) return InvalidInput;
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, pick(ctx, stream)));
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_memcpy_d2h(hbmpc_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream) {
    if (!ctx) return InvalidInput;
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, pick(ctx, stream)));
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_memcpy_d2d_rows(hbmpc_ctx* ctx, void* dst, size_t dst_pitch_bytes, const void* src, size_t src_pitch_bytes,
                                                size_t row_bytes, size_t rows, void* stream) {
    if (!ctx) return InvalidInput;
    if ((rows && row_bytes && (!dst || !src)) || dst_pitch_bytes < row_bytes || src_pitch_bytes < row_bytes) return fail(ctx, InvalidInput, "null buffer or pitch below the row");
    if (rows == 0 || row_bytes == 0) return ShareSuccess;
    HIP_TRY(ctx, hipMemcpy2DAsync(dst, dst_pitch_bytes, src, src_pitch_bytes, row_bytes, rows, hipMemcpyDeviceToDevice, pick(ctx, stream)));
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_memcpy_d2d(hbmpc_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream) {
    if (!ctx) return InvalidInput;
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, pick(ctx, stream)));
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_stream_sync(hbmpc_ctx* ctx, void* stream) {
    if (!ctx) return InvalidInput;
    HIP_TRY(ctx, hipStreamSynchronize(pick(ctx, stream)));
    return ShareSuccess;
}

extern "C" ShareErrorCode hbmpc_stream_create(hbmpc_ctx* ctx, void** stream_out) {
    if (!ctx || !stream_out) return InvalidInput;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = nullptr;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream_out = s;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_gather_party_major(hbmpc_ctx* const* ctxs, size_t n_shards, size_t root,
                                                       const void* const* shards_dev, const size_t* counts,
                                                       const size_t* strides, size_t n_rows, void* out_dev, size_t out_stride,
                                                       int sync_sources, void* stream) {
    if (!ctxs || n_shards == 0 || root >= n_shards || !ctxs[root]) return InvalidInput;
    hbmpc_ctx* rc_ctx = ctxs[root];
    if (!shards_dev || !counts || !strides || !out_dev) return fail(rc_ctx, InvalidInput, "null argument");
    size_t total = 0;
    for (size_t r = 0; r < n_shards; ++r) {
        if (!ctxs[r]) return fail(rc_ctx, InvalidInput, "null context in the shard list");
        if (is_gold(ctxs[r]) != is_gold(rc_ctx)) return fail(rc_ctx, TypeMismatch, "contexts of different fields");
        if (strides[r] < counts[r]) return fail(rc_ctx, InvalidInput, "shard row stride below its column count");
        if (counts[r] && !shards_dev[r]) return fail(rc_ctx, InvalidInput, "null shard");
        total += counts[r];
    }
    if (out_stride < total) return fail(rc_ctx, InvalidInput, "output row stride below the total column count");
    const size_t eb = ebytes(rc_ctx);
    if (sync_sources) {
        for (size_t r = 0; r < n_shards; ++r) {
            HIP_TRY(rc_ctx, hipSetDevice(ctxs[r]->device));
            HIP_TRY(rc_ctx, hipStreamSynchronize(ctxs[r]->stream));
        }
    }
    HIP_TRY(rc_ctx, hipSetDevice(rc_ctx->device));
    hipStream_t s = pick(rc_ctx, stream);
    size_t col = 0;
    for (size_t r = 0; r < n_shards; ++r) {
        const int src_dev = ctxs[r]->device;
        bool direct = src_dev == rc_ctx->device;
        if (rc_ctx->gather_row_copies) direct = false;  // A/B aid: the branch a pair of devices without peer access takes
        else if (!direct) {
            int can = 0;
            HIP_TRY(rc_ctx, hipDeviceCanAccessPeer(&can, rc_ctx->device, src_dev));
            if (can) {
                const hipError_t e = hipDeviceEnablePeerAccess(src_dev, 0);  // idempotent across calls
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_TRY(rc_ctx, e);
                (void)hipGetLastError();
                direct = true;
            }
        }
        if (counts[r] && n_rows) {
            char* dst = (char*)out_dev + col * eb;
            const char* src = (const char*)shards_dev[r];
            if (direct) {
                // ONE strided copy per shard: n_rows row segments of counts[r] elements (the destination reads the source
                // over xGMI when the devices differ)
                HIP_TRY(rc_ctx, hipMemcpy2DAsync(dst, out_stride * eb, src, strides[r] * eb, counts[r] * eb, n_rows, hipMemcpyDeviceToDevice, s));
            } else {
                // no peer access between the two devices: the runtime stages every row through the host
                for (size_t j = 0; j < n_rows; ++j)
                    HIP_TRY(rc_ctx, hipMemcpyPeerAsync(dst + j * out_stride * eb, rc_ctx->device, src + j * strides[r] * eb, src_dev, counts[r] * eb, s));
            }
        }
        col += counts[r];
    }
    return ShareSuccess;
}
// 1: the root's device reads the source's memory directly (same device, or peer access over xGMI, enabled here);
// 0: hbmpc_dev_gather_party_major falls back to copies the runtime stages through the host
extern "C" ShareErrorCode hbmpc_dev_peer_access(hbmpc_ctx* root, hbmpc_ctx* source, int* direct_out) {
    if (!root || !source || !direct_out) return InvalidInput;
    *direct_out = 0;
    if (root->device == source->device) {
        *direct_out = 1;
        return ShareSuccess;
    }
    int can = 0;
    HIP_TRY(root, hipSetDevice(root->device));
    HIP_TRY(root, hipDeviceCanAccessPeer(&can, root->device, source->device));
    if (can) {
        const hipError_t e = hipDeviceEnablePeerAccess(source->device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_TRY(root, e);
        (void)hipGetLastError();
        *direct_out = 1;
    }
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_stream_destroy(hbmpc_ctx* ctx, void* stream) {
    if (!ctx || !stream) return InvalidInput;
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    {
        std::lock_guard<std::mutex> lk(ctx->mu);  // the stream's scratch goes with it
        auto it = ctx->scratch.find((hipStream_t)stream);
        if (it != ctx->scratch.end()) {
            if (it->second.pinned) ctx->retired_scratch.push_back(it->second.p);  // a graph may be replayed elsewhere
            else (void)hipFree(it->second.p);
            ctx->scratch.erase(it);
        }
    }
    HIP_TRY(ctx, hipStreamDestroy((hipStream_t)stream));
    return ShareSuccess;
}

// ---- HIP graphs ----------------------------------------------------------------------------------
struct hbmpc_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipStream_t captured_on = nullptr;  // the stream whose scratch (decode counters) the recorded kernels point into
    void* scratch = nullptr;
};
extern "C" ShareErrorCode hbmpc_graph_begin_capture(hbmpc_ctx* ctx, void* stream) {
    if (!ctx) return InvalidInput;
    if (!stream) return fail(ctx, InvalidInput, "graph capture needs an explicit stream");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
    ++g_capturing;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_graph_end_capture(hbmpc_ctx* ctx, void* stream, hbmpc_graph** graph_out) {
    if (!ctx || !graph_out) return InvalidInput;
    *graph_out = nullptr;
    if (!stream) return fail(ctx, InvalidInput, "graph capture needs an explicit stream");
    if (g_capturing > 0) --g_capturing;
    hbmpc_graph* g = new hbmpc_graph();
    hipError_t e = hipStreamEndCapture((hipStream_t)stream, &g->graph);
    if (e == hipSuccess) e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        g_err = std::string("graph capture failed: ") + hipGetErrorString(e);
        hbmpc_graph_destroy(g);
        return HBMPC_NO_DEVICE;
    }
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        auto it = ctx->scratch.find((hipStream_t)stream);
        g->captured_on = (hipStream_t)stream;
        g->scratch = it != ctx->scratch.end() ? it->second.p : nullptr;
    }
    *graph_out = g;
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_graph_launch(hbmpc_ctx* ctx, hbmpc_graph* graph, void* stream) {
    if (!ctx || !graph || !graph->exec) return InvalidInput;
    hipStream_t s = pick(ctx, stream);
    {
        // the recorded decodes expect their counters at zero and carry no clear of their own (batch_recover_dev): a call that
        // failed between its launches since the capture is the one case in which they are not
        std::lock_guard<std::mutex> lk(ctx->mu);
        auto it = ctx->scratch.find(graph->captured_on);
        if (graph->scratch && it != ctx->scratch.end() && it->second.p == graph->scratch && it->second.dirty) {
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            HIP_TRY(ctx, hipMemsetAsync(graph->scratch, 0, 128, s));
            it->second.dirty = false;
        }
    }
    HIP_TRY(ctx, hipGraphLaunch(graph->exec, s));
    return ShareSuccess;
}
extern "C" void hbmpc_graph_destroy(hbmpc_graph* graph) {
    if (!graph) return;
    if (graph->exec) (void)hipGraphExecDestroy(graph->exec);
    if (graph->graph) (void)hipGraphDestroy(graph->graph);
    delete graph;
}

// ---- a3 / a5: evaluation on the domain ---------------------------------------------------------
// Which kernel an encode takes is decided in one place, plan_encode (encode_route.hpp); the functions below build the tables,
// fill the kernel arguments and walk its candidates.
// the producers' lists of a rows call (hbmpc_dev_vandermonde_apply_rows_lists / _split, MfmaRowsArgs::list)
struct ListSpec {
    size_t row0, rows, K;
    const hbmpc_list_slice* slices;
    size_t n_slices;
    void* others = nullptr;  // non-null: the rows outside the lists go here, party-major: others[(j (n - rows) + r') K + k] (hbmpc_dev_vandermonde_apply_rows_split)
};
static EncodeKnobs encode_knobs(const hbmpc_ctx* ctx) {
    return EncodeKnobs{ctx->impl, ctx->force_generic, ctx->matrix_cores, ctx->mfma_team, ctx->mfma_bfly, ctx->list_rows_in_kernel,
                       ctx->wide_max_chunks, ctx->mfma_min_encode, ctx->mfma_min_gold, ctx->mfma_wgs, ctx->n_cus};
}
// rows alpha_j^k (j < n, k < dp1) of the encode's matrix-core tables, times `scale`
template <class H>
static std::vector<std::vector<H>> vandermonde(size_t n, size_t dp1, H scale = H::one()) {
    std::vector<H> el = domain_elements<H>(n, n);
    std::vector<std::vector<H>> V(n, std::vector<H>(dp1));
    for (size_t j = 0; j < n; ++j) {
        H p = scale;
        for (size_t k = 0; k < dp1; ++k) V[j][k] = p, p = p * el[j];
    }
    return V;
}
// the matrix-core routes of plan_mfma (encode_route.hpp) as int8 MFMA tiles (kernels_mfma.hpp, kernels_mfma_bfly.hpp).  Returns false
// when the route does not run (its launcher declines, or the point-pair table's digit-sum bound does not hold: tables_mfma.hpp) and
// nothing was enqueued; true when it ran or *rc_out holds an error.
// x_row_stride != 0: x is given as d + 1 ROWS of G elements, x_row_stride elements apart (the point-pair kernel only)
static bool run_mfma(hbmpc_ctx* ctx, const EncodeRoute& r, const uint32_t* x, size_t G, size_t n, size_t dp1, EvalOut y, hipStream_t s,
                     ShareErrorCode* rc_out, size_t x_row_stride = 0, const ListSpec* lists = nullptr) {
    *rc_out = ShareSuccess;
    mf::MfmaRowsArgs a;
    memset(&a, 0, sizeof a);
    mf::mf_take_plan(r.plan, &a);
    a.G = G;
    a.in_chunk_major = 1;
    a.nv = 0;
    a.out_party_major = 1;
    a.out_stride = y.ys ? y.ys : G;
    const int mi = (int)dp1;
    const uint32_t* tab;
    if (r.kernel == EncodeKernel::MfmaRows || r.kernel == EncodeKernel::MfmaRowsTeam) {
        *rc_out = get_table(ctx, key("mfvand", {n, dp1}, ctx->impl), [&] { return build_mfma_table(vandermonde<HFr>(n, dp1), dp1); }, &tab);
        if (*rc_out != ShareSuccess) return true;
        a.table = (const uint8_t*)tab;
        // party-batched calls (x[P][G][d+1] -> y[P][n][G]): one launch per party (each is >= tens of microseconds)
        for (unsigned p = 0; p < y.parties; ++p) {
            a.in = (const uint8_t*)x + (size_t)p * G * dp1 * 32;
            a.out = (uint8_t*)y.y + (size_t)p * n * a.out_stride * 32;
            if (!launch_mfma_rows(mi, a, ctx->device, s, r.kernel == EncodeKernel::MfmaRowsTeam)) return false;
        }
        return true;
    }
    const size_t half = domain_size(n) / 2;
    std::array<size_t, 5> aux = {0, 0, 0, 0, 0};  // aux[0]: the table's words (0: its digit-sum bound does not hold, tables_mfma.hpp)
    *rc_out = get_table(ctx, key("mfbfly", {n, dp1}, ctx->impl), [&] {
        std::vector<uint32_t> tbl = build_mfma_bfly_table(vandermonde<HFr>(n, dp1), dp1, half);
        aux[0] = tbl.size();
        return tbl;
    }, &tab, &aux);
    if (*rc_out != ShareSuccess) return true;
    if (aux[0] == 0) return false;
    a.table = (const uint8_t*)tab;
    a.half = (int)half, a.nout = (int)n;
    if (x_row_stride) {
        a.in_chunk_major = 0, a.row_stride = x_row_stride;
        for (size_t i = 0; i < dp1; ++i) a.rows.set(i, (unsigned)i);
    }
    if (lists) {
        a.list_row0 = (int)lists->row0, a.list_rows = (int)lists->rows, a.list_K = (uint32_t)lists->K;
        if (lists->others) a.other_stride = (uint32_t)((n - lists->rows) * lists->K);
        for (size_t k = 0; k < 2; ++k) {
            const bool have = k < lists->n_slices;
            a.list[k].dst = have ? (uint8_t*)lists->slices[k].dst_dev : nullptr;
            a.list[k].stride = have ? lists->slices[k].party_stride : 0;
            a.list[k].k0 = have ? (uint32_t)lists->slices[k].k0 : 0u;
            a.list[k].count = have ? (uint32_t)lists->slices[k].count : 0u;
        }
    }
    // party-batched calls x[P][G][M] -> y[P][n][G]: ONE launch over the P G chunks where the instance with party-major "other" rows
    // covers the shape (MfmaRowsArgs::other_stride with no list rows: chunk (p, g) of row k goes to ((p n + k) G + g)) -- the
    // dealers' encodes of the producers; otherwise a launch per party
    if (r.kernel == EncodeKernel::BflyParties) {
        a.G = (size_t)y.parties * G, a.list_K = (uint32_t)G, a.other_stride = (uint32_t)(n * G), a.list_row0 = 0, a.list_rows = 0;
        a.in = (const uint8_t*)x, a.out = (uint8_t*)y.y;
        return launch_mfma_bfly(mi, a, ctx->device, s);  // the plan does not depend on the number of chunks (workgroups stride over the tiles)
    }
    for (unsigned p = 0; p < y.parties; ++p) {
        a.in = (const uint8_t*)x + (size_t)p * G * dp1 * 32;
        a.out = lists && lists->others ? (uint8_t*)lists->others : (uint8_t*)y.y + (size_t)p * n * a.out_stride * 32;
        // the shape and the batch size decide (bfly_ring_plan.hpp), the same for every party
        const bool ring = ctx->mfma_ring == 2 || (ctx->mfma_ring == 1 && a.nroles == 1 && mf::bfly_ring_ntiles(G) >= mf::bfly_ring_min_tiles((size_t)a.role_nwg[0]));
        if (ring && launch_mfma_bfly_ring(mi, a, ctx->device, s)) continue;
        if (!launch_mfma_bfly(mi, a, ctx->device, s)) return false;  // only the first party's launch can decline: the shape decides
    }
    return true;
}

// the same over Goldilocks (kernels_mfma_gl.hpp): all n rows in every workgroup's LDS
static bool run_mfma_gl(hbmpc_ctx* ctx, const uint32_t* x, size_t G, size_t n, size_t dp1, EvalOut y, hipStream_t s, ShareErrorCode* rc_out) {
    *rc_out = ShareSuccess;
    const uint32_t* tab;
    *rc_out = get_table(ctx, key("mfvandgl", {n, dp1}, ctx->impl), [&] { return build_mfma_table_gl(vandermonde<HGl>(n, dp1), dp1); }, &tab);
    if (*rc_out != ShareSuccess) return true;
    mf::MfmaGlArgs a;
    memset(&a, 0, sizeof a);
    a.G = G;
    a.in_chunk_major = 1;
    a.table = (const uint8_t*)tab;
    a.m = (int)dp1, a.nrows = (int)n, a.nv = 0;
    a.out_party_major = 1;
    a.out_stride = y.ys ? y.ys : G;
    const size_t ntiles = (G + 31) / 32;
    const unsigned grid = (unsigned)std::min<size_t>((ntiles + 3) / 4, (size_t)(ctx->mfma_wgs ? ctx->mfma_wgs : ctx->n_cus * 4));
    for (unsigned p = 0; p < y.parties; ++p) {  // party-batched calls: one launch per party
        a.in = (const uint8_t*)x + (size_t)p * G * dp1 * 8;
        a.out = (uint8_t*)y.y + (size_t)p * n * a.out_stride * 8;
        if (!launch_mfma_rows_gl(a, grid, ctx->device, s)) return false;
    }
    return true;
}

// alpha_j^k, j < n, k <= d, as constants [n][d + 1] (k_eval_wide_dot, k_triplegen_wg)
template <class H = HFr>
static ShareErrorCode vmat_table(hbmpc_ctx* ctx, size_t n, size_t d, const uint32_t** out) {
    const int impl = ctx->impl;
    return get_table(ctx, key("vmat", {n, d}, impl), [&] {
        std::vector<uint32_t> w;
        for (const H& al : domain_elements<H>(n, n)) {
            H p = H::one();
            for (size_t k = 0; k <= d; ++k) {
                put_const(w, p, impl);
                p = p * al;
            }
        }
        return w;
    }, out);
}
// the chunk-major encode: the candidates of plan_encode in order, the first that runs does the call
static ShareErrorCode eval_impl(hbmpc_ctx* ctx, const uint32_t* x, size_t G, size_t n, size_t d, EvalOut y,
                                hipStream_t s) {
    const size_t size = domain_size(n), dp1 = d + 1;
    const int impl = ctx->impl;
    const bool gold = impl == IMPL_GOLD;
    const EncodePlan plan = plan_encode(encode_knobs(ctx), EncodeShape{EncodeKind::ChunkMajor, G, n, d, y.parties, y.ys});
    for (int i = 0; i < plan.count; ++i) {
        const EncodeRoute& r = plan.route[i];
        ShareErrorCode rc = ShareSuccess;
        switch (r.kernel) {
        case EncodeKernel::WideDot: {
            const uint32_t* vmat;
            rc = vmat_table(ctx, n, d, &vmat);
            if (rc != ShareSuccess) return rc;
            launch_eval_wide_dot(x, G, (int)n, (int)dp1, vmat, y, s);
            return ShareSuccess;
        }
        case EncodeKernel::Wide:
        case EncodeKernel::Generic: {
            const uint32_t* alpha;
            rc = get_table(ctx, key("alpha", {n}, impl), [&] { return gold ? build_alpha<HGl>(n, impl) : build_alpha<HFr>(n, impl); }, &alpha);
            if (rc != ShareSuccess) return rc;
            if (r.kernel == EncodeKernel::Wide) launch_eval_wide(impl, x, G, (int)n, (int)dp1, alpha, y, s);
            else launch_eval_generic(impl, x, G, (int)n, (int)dp1, alpha, y, s);
            return ShareSuccess;
        }
        case EncodeKernel::MfmaRowsTeam:
        case EncodeKernel::MfmaRows:
        case EncodeKernel::Bfly:
        case EncodeKernel::BflyParties:
            if (run_mfma(ctx, r, x, G, n, dp1, y, s, &rc)) return rc;
            break;
        case EncodeKernel::MfmaRowsGl:
            if (run_mfma_gl(ctx, x, G, n, dp1, y, s, &rc)) return rc;
            break;
        case EncodeKernel::Fft1: {
            const uint32_t* tw;
            rc = get_table(ctx, key("tw", {size}, impl), [&] { return gold ? build_twiddles<HGl>(size, impl) : build_twiddles<HFr>(size, impl); }, &tw);
            if (rc != ShareSuccess) return rc;
            const int lg = ilog2(size), c = (int)dp1, nn = (int)n;
            if (gold ? launch_gold_fft1(lg, c, x, G, nn, tw, y, s)
                     : lg < 4 ? launch_fft1_lo(lg, c, x, G, nn, tw, y, s) : launch_fft1_16(c, x, G, nn, tw, y, s))
                return ShareSuccess;
            break;
        }
        case EncodeKernel::FftP: {
            const size_t P = size / 16;
            const uint32_t *tw16, *twist;
            rc = get_table(ctx, key("tw", {16}, impl), [&] { return gold ? build_twiddles<HGl>(16, impl) : build_twiddles<HFr>(16, impl); }, &tw16);
            if (rc != ShareSuccess) return rc;
            rc = get_table(ctx, key("twist", {size, dp1}, impl), [&] {
                return gold ? build_twist<HGl>(size, P, dp1, impl) : build_twist<HFr>(size, P, dp1, impl);
            }, &twist);
            if (rc != ShareSuccess) return rc;
            const int c = (int)dp1, nn = (int)n, pp = (int)P;
            if (gold ? launch_gold_fftP(c, x, G, nn, pp, tw16, twist, y, s) : launch_fftP(c, x, G, nn, pp, tw16, twist, y, s)) return ShareSuccess;
            break;
        }
        default:
            break;
        }
    }
    return fail(ctx, InvalidInput, "no encode kernel for this shape");  // not reached: the generic kernel ends every plan
}

static ShareErrorCode eval_dev(hbmpc_ctx* ctx, const void* x, size_t G, size_t n, size_t d, void* y, void* stream,
                               size_t parties = 1, size_t ystride = 0) {
    if (!ctx) return InvalidInput;
    if (parties == 0 || parties > 65535) return fail(ctx, InvalidInput, "parties must be in 1..65535");
    if (n <= d) return fail(ctx, InvalidInput, "number of shares must be greater than the degree");  // :59-64
    if (n == 0 || n > ((size_t)1 << 32)) return fail(ctx, NoSuitableDomain, "no radix-2 domain of that size");
    if (n > (1u << 20) || d > (1u << 20)) return fail(ctx, InvalidInput, "n, d beyond the supported range");
    if (ystride != 0 && ystride < G) return fail(ctx, InvalidInput, "output row stride must be >= G");
    if (G == 0) return ShareSuccess;
    if (!x || !y) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    ShareErrorCode rc = eval_impl(ctx, (const uint32_t*)x, G, n, d, EvalOut{(uint32_t*)y, ystride, (unsigned)parties}, s);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}

extern "C" ShareErrorCode hbmpc_dev_compute_shares(hbmpc_ctx* ctx, const U256* coeffs, size_t B, size_t n, size_t d,
                                                   U256* shares_out, void* stream) {
    REQ_FR(ctx);
    return eval_dev(ctx, coeffs, B, n, d, shares_out, stream);
}
extern "C" ShareErrorCode hbmpc_dev_vandermonde_apply(hbmpc_ctx* ctx, const U256* x, size_t G, size_t n, size_t d,
                                                      U256* y_out, void* stream) {
    REQ_FR(ctx);
    return eval_dev(ctx, x, G, n, d, y_out, stream);
}
// x[parties][G][d+1] -> y[parties][n][G]: the encodes of several parties in one launch
extern "C" ShareErrorCode hbmpc_dev_vandermonde_apply_parties(hbmpc_ctx* ctx, const U256* x, size_t G, size_t n, size_t d,
                                                              size_t parties, U256* y_out, void* stream) {
    REQ_FR(ctx);
    return eval_dev(ctx, x, G, n, d, y_out, stream, parties);
}
extern "C" ShareErrorCode hbmpc_gl_dev_vandermonde_apply_parties(hbmpc_ctx* ctx, const uint64_t* x, size_t G, size_t n,
                                                                 size_t d, size_t parties, uint64_t* y_out, void* stream) {
    REQ_GL(ctx);
    return eval_dev(ctx, x, G, n, d, y_out, stream, parties);
}
extern "C" ShareErrorCode hbmpc_gl_dev_compute_shares(hbmpc_ctx* ctx, const uint64_t* coeffs, size_t B, size_t n, size_t d,
                                                      uint64_t* shares_out, void* stream) {
    REQ_GL(ctx);
    return eval_dev(ctx, coeffs, B, n, d, shares_out, stream);
}
extern "C" ShareErrorCode hbmpc_gl_dev_vandermonde_apply(hbmpc_ctx* ctx, const uint64_t* x, size_t G, size_t n, size_t d,
                                                         uint64_t* y_out, void* stream) {
    REQ_GL(ctx);
    return eval_dev(ctx, x, G, n, d, y_out, stream);
}

// host wrapper helper: RAII device staging buffers for the host-pointer API.  They are recycled through a small
// per-context pool: hipMalloc + hipFree (which synchronises the device) cost ~0.45 ms per call, half the time of
// a 2^14-secret hbmpc_compute_shares.  Every user of a buffer runs on the context's own stream, so a recycled
// buffer is ordered behind its previous use.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hbmpc_ctx* owner = nullptr;
    ~DevBuf() {
        if (!p) return;
        std::lock_guard<std::mutex> lk(owner->mu);
        if (owner->stage_free.size() < 16 && owner->stage_bytes + cap <= ((size_t)2 << 30)) {
            owner->stage_free.emplace_back(p, cap);
            owner->stage_bytes += cap;
        } else {
            (void)hipFree(p);
        }
    }
    hipError_t alloc(hbmpc_ctx* ctx, size_t bytes) {
        owner = ctx;
        if (bytes == 0) bytes = 1;
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            int best = -1;
            for (int i = 0; i < (int)ctx->stage_free.size(); ++i) {
                const size_t c = ctx->stage_free[i].second;
                if (c >= bytes && c <= 4 * bytes + (1u << 20) && (best < 0 || c < ctx->stage_free[best].second)) best = i;
            }
            if (best >= 0) {
                p = ctx->stage_free[best].first;
                cap = ctx->stage_free[best].second;
                ctx->stage_bytes -= cap;
                ctx->stage_free.erase(ctx->stage_free.begin() + best);
                return hipSuccess;
            }
        }
        cap = bytes < (1u << 16) ? (1u << 16) : bytes + bytes / 4;
        return hipMalloc(&p, cap);
    }
};


// ---- staging of one host-pointer call -------------------------------------------------------------------------
// Large calls: device buffers from the DevBuf pool + async copies on the context stream.  Small calls (everything
// fits one 2 MiB block) stage through pinned host memory that is mapped into the device: inputs are memcpy'd in,
// the kernels read and write that block over PCIe, outputs are memcpy'd out after the stream sync -- no DMA commands
// at all.  On this box one 512-byte hipMemcpy + sync costs 16-27 us and a kernel launch + sync 25 us, so a
// one-polynomial recover_secret (1 upload, 3 launches, 4 downloads) drops from 111 us to about 45 us
// (tools/time_small_calls.py).  Only plain loads/stores touch the mapped block (the kernels' atomics -- flag lists,
// counters -- live in device scratch; the host path derives its summary from the status bytes instead).
struct Stage {
    static constexpr size_t BLOCK = STAGE_PIN_BLOCK;
    hbmpc_ctx* ctx;
    bool mapped = false, finished = false;
    char* hblk = nullptr;  // host view of the block
    char* dblk = nullptr;  // device view
    size_t off = 0;
    std::deque<DevBuf> bufs;
    struct Out {
        void* dst;
        const void* src;
        size_t bytes;
    };
    std::vector<Out> outs;

    Stage(hbmpc_ctx* c, size_t total_bytes, size_t n_bufs) : ctx(c) {
        if (!c->zero_copy || total_bytes + 256 * n_bufs > BLOCK) return;
        {
            std::lock_guard<std::mutex> lk(c->mu);
            if (!c->pin_free.empty()) {
                hblk = (char*)c->pin_free.back();
                c->pin_free.pop_back();
            }
        }
        if (!hblk && hipHostMalloc((void**)&hblk, BLOCK, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            (void)hipGetLastError();
            hblk = nullptr;
            return;  // no pinned memory to be had: the device-buffer path serves the call
        }
        if (hipHostGetDevicePointer((void**)&dblk, hblk, 0) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipHostFree(hblk);
            hblk = nullptr;
            return;
        }
        mapped = true;
    }
    ~Stage() {
        if (!hblk) return;
        if (!finished) (void)hipStreamSynchronize(ctx->stream);  // an error path: kernels may still be writing the block
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (ctx->pin_free.size() < 16) ctx->pin_free.push_back(hblk);
        else (void)hipHostFree(hblk);
    }
    Stage(const Stage&) = delete;
    Stage& operator=(const Stage&) = delete;

    hipError_t alloc(size_t bytes, void** p) {
        if (mapped) {
            *p = dblk + off;
            off += (bytes + 255) & ~(size_t)255;
            return off <= BLOCK ? hipSuccess : hipErrorOutOfMemory;  // cannot happen: sized in the constructor
        }
        bufs.emplace_back();
        hipError_t e = bufs.back().alloc(ctx, bytes);
        *p = bufs.back().p;
        return e;
    }
    hipError_t in(const void* src, size_t bytes, void** p) {
        hipError_t e = alloc(bytes, p);
        if (e != hipSuccess || bytes == 0) return e;
        if (mapped) {
            memcpy(hblk + ((char*)*p - dblk), src, bytes);
            return hipSuccess;
        }
        return hipMemcpyAsync(*p, src, bytes, hipMemcpyHostToDevice, ctx->stream);
    }
    hipError_t out(void* dst, const void* p, size_t bytes) {  // p: a pointer returned by alloc()/in()
        if (!dst || bytes == 0) return hipSuccess;
        if (mapped) {
            outs.push_back({dst, hblk + ((const char*)p - dblk), bytes});
            return hipSuccess;
        }
        return hipMemcpyAsync(dst, p, bytes, hipMemcpyDeviceToHost, ctx->stream);
    }
    hipError_t finish() {
        hipError_t e = hipStreamSynchronize(ctx->stream);
        finished = true;
        if (e != hipSuccess) return e;
        for (const Out& o : outs) memcpy(o.dst, o.src, o.bytes);
        return hipSuccess;
    }
};
extern "C" ShareErrorCode hbmpc_set_small_call_staging(hbmpc_ctx* ctx, int zero_copy) {
    if (!ctx) return InvalidInput;
    ctx->zero_copy = zero_copy != 0;
    return ShareSuccess;
}

static ShareErrorCode eval_host(hbmpc_ctx* ctx, const void* x, size_t G, size_t n, size_t d, void* y) {
    if (!ctx) return InvalidInput;
    if (n <= d) return fail(ctx, InvalidInput, "number of shares must be greater than the degree");
    // the range checks of eval_dev, before any size arithmetic with n and d
    if (n == 0 || n > ((size_t)1 << 32)) return fail(ctx, NoSuitableDomain, "no radix-2 domain of that size");
    if (n > (1u << 20) || d > (1u << 20)) return fail(ctx, InvalidInput, "n, d beyond the supported range");
    if (G == 0) return ShareSuccess;
    if (!x || !y) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t eb = ebytes(ctx);
    Stage st(ctx, G * (d + 1 + n) * eb, 2);
    void *dx, *dy;
    HIP_TRY(ctx, st.in(x, G * (d + 1) * eb, &dx));
    HIP_TRY(ctx, st.alloc(G * n * eb, &dy));
    ShareErrorCode rc = eval_dev(ctx, dx, G, n, d, dy, nullptr);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, st.out(y, dy, G * n * eb));
    HIP_TRY(ctx, st.finish());
    return ShareSuccess;
}
// ---- seeded compute_shares: the random coefficients are generated on the device ("hbmpc-chacha20-v1") ---------
static ShareErrorCode fill_coeffs_dev(hbmpc_ctx* ctx, const uint8_t seed[32], const void* secrets, size_t B,
                                      uint64_t first_index, size_t d, void* coeffs_out, void* stream) {
    if (!ctx) return InvalidInput;
    if (!seed) return fail(ctx, InvalidInput, "null seed");
    if (d > (1u << 20)) return fail(ctx, InvalidInput, "degree beyond the supported range");
    if (B == 0) return ShareSuccess;
    if (!coeffs_out) return fail(ctx, InvalidInput, "null buffer");  // secrets may be null: they are drawn too
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t k[8];
    memcpy(k, seed, 32);  // little-endian words
    launch_fill_coeffs((int)(ebytes(ctx) / 4), k, (const uint32_t*)secrets, B, first_index, (int)(d + 1), (uint32_t*)coeffs_out,
                       pick(ctx, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
static ShareErrorCode compute_shares_seeded_dev(hbmpc_ctx* ctx, const uint8_t seed[32], const void* secrets, size_t B,
                                                uint64_t first_index, size_t n, size_t d, void* coeffs_ws, void* shares_out,
                                                void* stream) {
    if (ctx && n <= d) return fail(ctx, InvalidInput, "number of shares must be greater than the degree");
    ShareErrorCode rc = fill_coeffs_dev(ctx, seed, secrets, B, first_index, d, coeffs_ws, stream);
    if (rc != ShareSuccess) return rc;
    return eval_dev(ctx, coeffs_ws, B, n, d, shares_out, stream);
}
static ShareErrorCode compute_shares_seeded_host(hbmpc_ctx* ctx, const uint8_t seed[32], const void* secrets, size_t B,
                                                 uint64_t first_index, size_t n, size_t d, void* shares_out) {
    if (!ctx) return InvalidInput;
    if (n <= d) return fail(ctx, InvalidInput, "number of shares must be greater than the degree");
    if (B == 0) return ShareSuccess;
    if (!shares_out || !seed) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t eb = ebytes(ctx);
    Stage st(ctx, B * (1 + d + 1 + n) * eb, 3);  // only the SECRETS cross the bus on the way in: 1/(d+1) of what hbmpc_compute_shares uploads
    void *ds = nullptr, *dc, *dy;
    if (secrets) HIP_TRY(ctx, st.in(secrets, B * eb, &ds));
    HIP_TRY(ctx, st.alloc(B * (d + 1) * eb, &dc));
    HIP_TRY(ctx, st.alloc(B * n * eb, &dy));
    ShareErrorCode rc = compute_shares_seeded_dev(ctx, seed, ds, B, first_index, n, d, dc, dy, nullptr);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, st.out(shares_out, dy, B * n * eb));
    HIP_TRY(ctx, st.finish());
    return ShareSuccess;
}
#define TYPED_SEEDED(T, REQ, PFX)                                                                                          \
    extern "C" ShareErrorCode PFX##dev_fill_coeffs(hbmpc_ctx* ctx, const uint8_t seed[32], const T* secrets_dev, size_t B,  \
                                                   uint64_t first_index, size_t d, T* coeffs_out_dev, void* stream) {       \
        REQ(ctx);                                                                                                          \
        return fill_coeffs_dev(ctx, seed, secrets_dev, B, first_index, d, coeffs_out_dev, stream);                         \
    }                                                                                                                      \
    extern "C" ShareErrorCode PFX##dev_compute_shares_seeded(hbmpc_ctx* ctx, const uint8_t seed[32], const T* secrets_dev, \
                                                             size_t B, uint64_t first_index, size_t n, size_t d,           \
                                                             T* coeffs_ws_dev, T* shares_out_dev, void* stream) {          \
        REQ(ctx);                                                                                                          \
        return compute_shares_seeded_dev(ctx, seed, secrets_dev, B, first_index, n, d, coeffs_ws_dev, shares_out_dev, stream); \
    }                                                                                                                      \
    extern "C" ShareErrorCode PFX##compute_shares_seeded(hbmpc_ctx* ctx, const uint8_t seed[32], const T* secrets, size_t B, \
                                                         uint64_t first_index, size_t n, size_t d, T* shares_out) {        \
        REQ(ctx);                                                                                                          \
        return compute_shares_seeded_host(ctx, seed, secrets, B, first_index, n, d, shares_out);                           \
    }
TYPED_SEEDED(U256, REQ_FR, hbmpc_)
TYPED_SEEDED(uint64_t, REQ_GL, hbmpc_gl_)

extern "C" ShareErrorCode hbmpc_compute_shares(hbmpc_ctx* ctx, const U256* coeffs, size_t B, size_t n, size_t d,
                                               U256* shares_out) {
    REQ_FR(ctx);
    return eval_host(ctx, coeffs, B, n, d, shares_out);
}
extern "C" ShareErrorCode hbmpc_vandermonde_apply(hbmpc_ctx* ctx, const U256* x, size_t G, size_t n, size_t d,
                                                  U256* y_out) {
    REQ_FR(ctx);
    return eval_host(ctx, x, G, n, d, y_out);
}
extern "C" ShareErrorCode hbmpc_gl_compute_shares(hbmpc_ctx* ctx, const uint64_t* coeffs, size_t B, size_t n, size_t d,
                                                  uint64_t* shares_out) {
    REQ_GL(ctx);
    return eval_host(ctx, coeffs, B, n, d, shares_out);
}
extern "C" ShareErrorCode hbmpc_gl_vandermonde_apply(hbmpc_ctx* ctx, const uint64_t* x, size_t G, size_t n, size_t d,
                                                     uint64_t* y_out) {
    REQ_GL(ctx);
    return eval_host(ctx, x, G, n, d, y_out);
}
// common/share/mod.rs:31-45.  A constant table (rows [1, alpha_j, ..., alpha_j^d]), built where every other
// table of this library is built: on the host.
template <class H>
static ShareErrorCode make_vandermonde_t(hbmpc_ctx* ctx, size_t n, size_t d, void* v_out) {
    if (!ctx) return InvalidInput;
    if (n == 0) return ShareSuccess;
    if (!v_out) return fail(ctx, InvalidInput, "null buffer");
    if (domain_size(n) > ((size_t)1 << 32)) return fail(ctx, NoSuitableDomain, "no radix-2 domain of that size");
    const std::vector<H> el = domain_elements<H>(n, n);
    for (size_t j = 0; j < n; ++j) {
        H p = H::one();
        for (size_t k = 0; k <= d; ++k) {
            uint64_t c[4];
            p.to_canon(c);
            memcpy((uint8_t*)v_out + (j * (d + 1) + k) * H::EBYTES, c, H::EBYTES);
            p = p * el[j];
        }
    }
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_make_vandermonde(hbmpc_ctx* ctx, size_t n, size_t d, U256* v_out) {
    REQ_FR(ctx);
    return make_vandermonde_t<HFr>(ctx, n, d, v_out);
}
extern "C" ShareErrorCode hbmpc_gl_make_vandermonde(hbmpc_ctx* ctx, size_t n, size_t d, uint64_t* v_out) {
    REQ_GL(ctx);
    return make_vandermonde_t<HGl>(ctx, n, d, v_out);
}

// ---- element-wise ------------------------------------------------------------------------------
// (the launchers of tu_elem.hip size the grid: a lane per element)
// elem_grid (tu_elem.hip) takes the block count as a 32-bit grid dimension and HIP allows 2^31 - 1 of them: an N beyond that is refused
// here, never launched on a wrapped grid
static constexpr size_t ELEM_MAX_N = (size_t)0x7fffffff * 256;
#define ELEM_PROLOGUE                                                           \
    if (!ctx) return InvalidInput;                                              \
    if (N == 0) return ShareSuccess;                                            \
    if (N > ELEM_MAX_N) return fail(ctx, InvalidInput, "N out of range: more than 2^31 - 1 blocks of 256 elements"); \
    HIP_TRY(ctx, hipSetDevice(ctx->device));                                    \
    hipStream_t s = pick(ctx, stream);
// every device buffer of a call with N > 0: a null one is refused before anything is enqueued
#define ELEM_BUFS(...) do { for (const void* p_ : std::initializer_list<const void*>{__VA_ARGS__}) if (!p_) return fail(ctx, InvalidInput, "null buffer"); } while (0)

#define CHECK_PARTIES(P) do { if ((P) == 0 || (P) > 65535) return fail(ctx, InvalidInput, "parties must be in 1..65535"); } while (0)

// device buffers of either field as the kernels' 32-bit words
static const uint32_t* as_words(const void* p) { return (const uint32_t*)p; }
static uint32_t* as_words(void* p) { return (uint32_t*)p; }

static ShareErrorCode fr_op_any(hbmpc_ctx* ctx, int op, const void* a, const void* b, size_t N, void* out, void* stream) {
    ELEM_PROLOGUE
    ELEM_BUFS(a, b, out);
    if (op < 0 || op > 2) return fail(ctx, InvalidInput, "op must be 0 (add), 1 (sub) or 2 (mul)");
    const ElemConsts cs = elem_consts(ctx->impl);
    launch_binop(ctx->impl, op, as_words(a), as_words(b), N, cs, as_words(out), s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
// scalar: ONE canonical element in HOST memory
static ShareErrorCode fr_op_scalar_any(hbmpc_ctx* ctx, int op, const void* a, const void* scalar, size_t N, void* out, void* stream) {
    if (ctx && !scalar) return fail(ctx, InvalidInput, "null scalar");
    ELEM_PROLOGUE
    ELEM_BUFS(a, out);
    if (op < 0 || op > 3) return fail(ctx, InvalidInput, "op must be 0 (a + s), 1 (a - s), 2 (a * s) or 3 (s - a)");
    ScalarArg sc;
    memset(&sc, 0, sizeof sc);
    memcpy(sc.w, scalar, ebytes(ctx));
    if (ctx->impl == IMPL_GOLD) {
        uint64_t v;
        memcpy(&v, scalar, 8);
        if (v >= HGl::P) return fail(ctx, InvalidInput, "scalar is not a canonical field element");
    } else {
        uint64_t v[4];
        memcpy(v, scalar, 32);
        if (HFr::geq(v)) return fail(ctx, InvalidInput, "scalar is not a canonical field element");
    }
    const ElemConsts cs = elem_consts(ctx->impl);
    launch_scalarop(ctx->impl, op, as_words(a), sc, N, cs, as_words(out), s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
static ShareErrorCode triple_local_any(hbmpc_ctx* ctx, const void* a, const void* b, const void* r2t, size_t N, void* out,
                                       void* stream) {
    ELEM_PROLOGUE
    ELEM_BUFS(a, b, r2t, out);
    const ElemConsts cs = elem_consts(ctx->impl);
    launch_triple_local(ctx->impl, as_words(a), as_words(b), as_words(r2t), N, cs, as_words(out), s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
// TripleGenNode::init_batch for `parties` parties at once: x = a b - r2t per element, then the Vandermonde encode of the
// chunks of d + 1 -- one launch where k_eval_fft1_triple covers the shape, otherwise the two separate ones through `tmp`
static ShareErrorCode triple_encode_any(hbmpc_ctx* ctx, const void* a, const void* b, const void* r2t, size_t G, size_t n, size_t d,
                                        size_t parties, void* tmp, void* y, void* stream) {
    if (!ctx) return InvalidInput;
    if (parties == 0 || parties > 65535) return fail(ctx, InvalidInput, "parties must be in 1..65535");
    if (n <= d) return fail(ctx, InvalidInput, "number of shares must be greater than the degree");
    if (n == 0 || n > ((size_t)1 << 32)) return fail(ctx, NoSuitableDomain, "no radix-2 domain of that size");
    if (n > (1u << 20) || d > (1u << 20)) return fail(ctx, InvalidInput, "n, d beyond the supported range");
    if (G == 0) return ShareSuccess;
    if (!a || !b || !r2t || !y) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    const size_t size = domain_size(n), dp1 = d + 1;
    EncodeShape shape{EncodeKind::Triple, G, n, d, parties};
    shape.workspace = tmp != nullptr;
    const EncodePlan plan = plan_encode(encode_knobs(ctx), shape);
    for (int i = 0; i < plan.count; ++i) {
        const EncodeRoute& r = plan.route[i];
        if (r.kernel == EncodeKernel::BflyTriple) {
            mf::MfmaRowsArgs ma;
            memset(&ma, 0, sizeof ma);
            mf::mf_take_plan(r.plan, &ma);
            const size_t half = size / 2;
            const uint32_t* tab;
            std::array<size_t, 5> aux = {0, 0, 0, 0, 0};  // aux[0]: the table's words (0: the digit-sum bound could not be proved)
            // rows alpha_j^i R, R = 2^261: the kernel hands over (a b - r2t) / R (one Montgomery reduction, no conversions)
            ShareErrorCode rc = get_table(ctx, key("mfbflyR", {n, dp1}, ctx->impl), [&] {
                HFr R = HFr::one();
                const HFr two = HFr::from_u64(2);
                for (int e = 0; e < 261; ++e) R = R * two;
                std::vector<uint32_t> tbl = build_mfma_bfly_table(vandermonde<HFr>(n, dp1, R), dp1, half);
                aux[0] = tbl.size();
                return tbl;
            }, &tab, &aux);
            if (rc != ShareSuccess) return rc;
            ma.in = (const uint8_t*)a, ma.in_b = (const uint8_t*)b, ma.in_r = (const uint8_t*)r2t;
            ma.parties = (int)parties, ma.G = G, ma.in_chunk_major = 1, ma.nv = 0;
            ma.table = (const uint8_t*)tab, ma.half = (int)half, ma.nout = (int)n;
            ma.out = (uint8_t*)y, ma.out_party_major = 1, ma.out_stride = G;
            if (aux[0] != 0 && launch_mfma_bfly((int)dp1, ma, ctx->device, s)) {
                HIP_TRY(ctx, hipGetLastError());
                return ShareSuccess;
            }
        } else if (r.kernel == EncodeKernel::Fft1Triple) {
            const bool gold = is_gold(ctx);
            const uint32_t* tw;
            ShareErrorCode rc = get_table(ctx, key("tw", {size}, ctx->impl), [&] {
                return gold ? build_twiddles<HGl>(size, ctx->impl) : build_twiddles<HFr>(size, ctx->impl);
            }, &tw);
            if (rc != ShareSuccess) return rc;
            const EvalOut out{as_words(y), 0, (unsigned)parties};
            if (gold ? launch_fft1_triple_gold(ilog2(size), (int)dp1, as_words(a), as_words(b), as_words(r2t), G, (int)n, tw, out, s)
                     : launch_fft1_triple(ilog2(size), (int)dp1, as_words(a), as_words(b), as_words(r2t), G, (int)n, tw, out, elem_consts(ctx->impl).r2, s)) {
                HIP_TRY(ctx, hipGetLastError());
                return ShareSuccess;
            }
        }
    }
    // the last candidate (EncodeKernel::LocalProduct): the products into the workspace, then the chunk-major encode
    if (!tmp) return fail(ctx, InvalidInput, "no fused kernel for this shape: pass a workspace of parties * G * (d + 1) elements");
    ShareErrorCode rc = triple_local_any(ctx, a, b, r2t, parties * G * dp1, tmp, stream);
    if (rc != ShareSuccess) return rc;
    return eval_dev(ctx, tmp, G, n, d, y, stream, parties);
}
static ShareErrorCode triple_finalize_any(hbmpc_ctx* ctx, const void* rt, const void* opened, size_t N, void* c_out,
                                          void* stream, size_t parties = 1) {
    ELEM_PROLOGUE
    ELEM_BUFS(rt, opened, c_out);
    CHECK_PARTIES(parties);
    launch_triple_finalize(ctx->impl, as_words(rt), as_words(opened), N, (unsigned)parties, as_words(c_out), s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
static ShareErrorCode beaver_open_any(hbmpc_ctx* ctx, const void* a, const void* b, const void* x, const void* y, size_t N,
                                      void* d_sh, void* e_sh, void* stream) {
    ELEM_PROLOGUE
    ELEM_BUFS(a, b, x, y, d_sh, e_sh);
    launch_beaver_open(ctx->impl, as_words(a), as_words(b), as_words(x), as_words(y), N, as_words(d_sh), as_words(e_sh), s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
static ShareErrorCode beaver_open_pair_any(hbmpc_ctx* ctx, const void* a, const void* b, const void* x, const void* y, size_t N,
                                           size_t parties, void* de, void* stream) {
    ELEM_PROLOGUE
    ELEM_BUFS(a, b, x, y, de);
    CHECK_PARTIES(parties);
    launch_beaver_open_pair(ctx->impl, as_words(a), as_words(b), as_words(x), as_words(y), N, (unsigned)parties, as_words(de), s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
static ShareErrorCode beaver_finalize_any(hbmpc_ctx* ctx, const void* c, const void* x, const void* y, const void* d,
                                          const void* e, size_t N, void* z, void* stream, size_t parties = 1) {
    ELEM_PROLOGUE
    ELEM_BUFS(c, x, y, d, e, z);
    CHECK_PARTIES(parties);
    const ElemConsts cs = elem_consts(ctx->impl);
    // the kernel loops over the parties (large N: the public operands are converted once per element) or spreads them
    // over gridDim.y (small N: latency)
    const unsigned grid_parties = N >= ((size_t)1 << 16) ? 1 : (unsigned)parties;
    launch_beaver_finalize(ctx->impl, as_words(c), as_words(x), as_words(y), as_words(d), as_words(e), N, cs, as_words(z), (unsigned)parties, grid_parties, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
#define TYPED_PAIR(T, REQ, PFX)                                                                                          \
    extern "C" ShareErrorCode PFX##dev_fr_op(hbmpc_ctx* ctx, int op, const T* a, const T* b, size_t N, T* out,           \
                                             void* stream) {                                                             \
        REQ(ctx);                                                                                                        \
        return fr_op_any(ctx, op, a, b, N, out, stream);                                                                 \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##dev_fr_op_scalar(hbmpc_ctx* ctx, int op, const T* a, const T* scalar_host, size_t N,  \
                                                    T* out, void* stream) {                                              \
        REQ(ctx);                                                                                                        \
        return fr_op_scalar_any(ctx, op, a, scalar_host, N, out, stream);                                                \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##dev_triple_encode_parties(hbmpc_ctx* ctx, const T* a, const T* b, const T* r2t,       \
                                                             size_t G, size_t n, size_t d, size_t parties, T* tmp,        \
                                                             T* y_out, void* stream) {                                   \
        REQ(ctx);                                                                                                        \
        return triple_encode_any(ctx, a, b, r2t, G, n, d, parties, tmp, y_out, stream);                                  \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##dev_triple_local(hbmpc_ctx* ctx, const T* a, const T* b, const T* r2t, size_t N,      \
                                                    T* out, void* stream) {                                              \
        REQ(ctx);                                                                                                        \
        return triple_local_any(ctx, a, b, r2t, N, out, stream);                                                         \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##dev_triple_finalize(hbmpc_ctx* ctx, const T* rt, const T* opened, size_t N, T* c_out, \
                                                       void* stream) {                                                   \
        REQ(ctx);                                                                                                        \
        return triple_finalize_any(ctx, rt, opened, N, c_out, stream);                                                   \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##dev_beaver_open_shares(hbmpc_ctx* ctx, const T* a, const T* b, const T* x, const T* y, \
                                                          size_t N, T* d_sh, T* e_sh, void* stream) {                    \
        REQ(ctx);                                                                                                        \
        return beaver_open_any(ctx, a, b, x, y, N, d_sh, e_sh, stream);                                                  \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##dev_beaver_finalize(hbmpc_ctx* ctx, const T* c, const T* x, const T* y, const T* d,   \
                                                       const T* e, size_t N, T* z, void* stream) {                       \
        REQ(ctx);                                                                                                        \
        return beaver_finalize_any(ctx, c, x, y, d, e, N, z, stream);                                                    \
    }
TYPED_PAIR(U256, REQ_FR, hbmpc_)
TYPED_PAIR(uint64_t, REQ_GL, hbmpc_gl_)
#define TYPED_PARTIES(T, REQ, PFX)                                                                                       \
    extern "C" ShareErrorCode PFX##dev_beaver_open_shares_paired(hbmpc_ctx* ctx, const T* a, const T* b, const T* x,     \
                                                                 const T* y, size_t N, size_t parties, T* de_sh_out,     \
                                                                 void* stream) {                                         \
        REQ(ctx);                                                                                                        \
        return beaver_open_pair_any(ctx, a, b, x, y, N, parties, de_sh_out, stream);                                     \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##dev_triple_finalize_parties(hbmpc_ctx* ctx, const T* rt, const T* opened, size_t N,   \
                                                               size_t parties, T* c_out, void* stream) {                 \
        REQ(ctx);                                                                                                        \
        return triple_finalize_any(ctx, rt, opened, N, c_out, stream, parties);                                          \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##dev_beaver_finalize_parties(hbmpc_ctx* ctx, const T* c, const T* x, const T* y,       \
                                                               const T* d, const T* e, size_t N, size_t parties, T* z,   \
                                                               void* stream) {                                           \
        REQ(ctx);                                                                                                        \
        return beaver_finalize_any(ctx, c, x, y, d, e, N, z, stream, parties);                                           \
    }
TYPED_PARTIES(U256, REQ_FR, hbmpc_)
TYPED_PARTIES(uint64_t, REQ_GL, hbmpc_gl_)
// ---- square roots, inverses, RandBit's phase 2 (kernels_sqrt.hpp) --------------------------------------------------
// the context's constants: omega power tables, exponents, 2^-1, the subgroup look-up (tables_sqrt.hpp); one table per implementation
static ShareErrorCode sqrt_tab(hbmpc_ctx* ctx, SqrtTab* t) {
    const int impl = ctx->impl;
    std::array<size_t, 5> aux = {0, 0, 0, 0, 0};
    const uint32_t* p = nullptr;
    ShareErrorCode rc;
    try {
        rc = get_table(ctx, key("sqrt", {}, impl), [&] {
            SqrtLayout L;
            std::vector<uint32_t> w;
            if (impl == IMPL_GOLD) {
                const uint64_t mod[4] = {HGl::P, 0, 0, 0};
                w = build_sqrt_table<HGl>(mod, HGl::one(), impl, &L);
            } else {
                w = build_sqrt_table<HFr>(HFr::MOD, rdev_value(impl), impl, &L);
            }
            aux = {(size_t)L.kbits, (size_t)L.kshift, (size_t)L.bits_sqrt, (size_t)L.bits_inv, 0};
            return w;
        }, &p, &aux);
    } catch (const std::exception& e) {
        return fail(ctx, HBMPC_NO_DEVICE, e.what());
    }
    if (rc != ShareSuccess) return rc;
    const SqrtLayout L = sqrt_layout(impl, (int)aux[0], (int)aux[1], (int)aux[2], (int)aux[3]);
    t->negw = p + L.negw, t->posw = p + L.posw, t->r2 = p + L.r2, t->one_p = p + L.one_p, t->half = p + L.half, t->half_p = p + L.half_p;
    t->e_sqrt = p + L.e_sqrt, t->e_inv = p + L.e_inv, t->keyt = reinterpret_cast<const uint8_t*>(p + L.keyt);
    t->bits_sqrt = L.bits_sqrt, t->bits_inv = L.bits_inv;
    t->kshift = (uint32_t)L.kshift, t->kmask = (1u << L.kbits) - 1;
    return ShareSuccess;
}
static ShareErrorCode sqrt_inverse_any(hbmpc_ctx* ctx, bool inverse, const void* a, size_t N, void* out, uint8_t* flag, void* stream) {
    ELEM_PROLOGUE
    if (!a || !out || !flag) return fail(ctx, InvalidInput, "null buffer");
    SqrtTab t;
    const ShareErrorCode rc = sqrt_tab(ctx, &t);
    if (rc != ShareSuccess) return rc;
    if (inverse) launch_inverse(ctx->impl, as_words(a), N, t, as_words(out), flag, s);
    else launch_sqrt(ctx->impl, as_words(a), N, t, as_words(out), flag, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
static ShareErrorCode randbit_finalize_any(hbmpc_ctx* ctx, const void* a, const void* sq, size_t N, size_t parties, void* out, uint8_t* status,
                                           hbmpc_randbit_summary* summary, void* stream) {
    if (!ctx) return InvalidInput;
    if (!summary || (N && (!a || !sq || !out || !status))) return fail(ctx, InvalidInput, "null buffer");
    CHECK_PARTIES(parties);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    SqrtTab t;
    const ShareErrorCode rc = sqrt_tab(ctx, &t);
    if (rc != ShareSuccess) return rc;
    static_assert(sizeof(hbmpc_randbit_summary) == sizeof(RandBitSummaryDev), "summary layout");
    HIP_TRY(ctx, hipMemsetAsync(summary, 0xff, 8, s));  // first = all ones
    HIP_TRY(ctx, hipMemsetAsync((char*)summary + 8, 0, 8, s));
    if (N == 0) return ShareSuccess;
    launch_randbit_finalize(ctx->impl, as_words(a), as_words(sq), N, (unsigned)parties, t, as_words(out), status, reinterpret_cast<RandBitSummaryDev*>(summary), s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
// host-pointer forms: inputs staged, the two outputs copied back
static ShareErrorCode sqrt_inverse_host(hbmpc_ctx* ctx, bool inverse, const void* a, size_t N, void* out, uint8_t* flag) {
    if (!ctx) return InvalidInput;
    if (N == 0) return ShareSuccess;
    if (!a || !out || !flag) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t eb = ebytes(ctx);
    Stage st(ctx, 2 * N * eb + N, 3);
    void *pa = nullptr, *po = nullptr, *pf = nullptr;
    HIP_TRY(ctx, st.in(a, N * eb, &pa));
    HIP_TRY(ctx, st.alloc(N * eb, &po));
    HIP_TRY(ctx, st.alloc(N, &pf));
    const ShareErrorCode rc = sqrt_inverse_any(ctx, inverse, pa, N, po, (uint8_t*)pf, nullptr);
    if (rc != ShareSuccess) return rc;
    HIP_TRY(ctx, st.out(out, po, N * eb));
    HIP_TRY(ctx, st.out(flag, pf, N));
    HIP_TRY(ctx, st.finish());
    return ShareSuccess;
}
#define TYPED_SQRT(T, REQ, PFX)                                                                                                             \
    extern "C" ShareErrorCode PFX##fr_sqrt(hbmpc_ctx* ctx, const T* a, size_t N, T* root_out, uint8_t* has_root_out) {                       \
        REQ(ctx);                                                                                                                           \
        return sqrt_inverse_host(ctx, false, a, N, root_out, has_root_out);                                                                 \
    }                                                                                                                                       \
    extern "C" ShareErrorCode PFX##dev_fr_sqrt(hbmpc_ctx* ctx, const T* a, size_t N, T* root_out, uint8_t* has_root_out, void* stream) {     \
        REQ(ctx);                                                                                                                           \
        return sqrt_inverse_any(ctx, false, a, N, root_out, has_root_out, stream);                                                          \
    }                                                                                                                                       \
    extern "C" ShareErrorCode PFX##fr_inverse(hbmpc_ctx* ctx, const T* a, size_t N, T* inv_out, uint8_t* ok_out) {                            \
        REQ(ctx);                                                                                                                           \
        return sqrt_inverse_host(ctx, true, a, N, inv_out, ok_out);                                                                         \
    }                                                                                                                                       \
    extern "C" ShareErrorCode PFX##dev_fr_inverse(hbmpc_ctx* ctx, const T* a, size_t N, T* inv_out, uint8_t* ok_out, void* stream) {         \
        REQ(ctx);                                                                                                                           \
        return sqrt_inverse_any(ctx, true, a, N, inv_out, ok_out, stream);                                                                  \
    }                                                                                                                                       \
    extern "C" ShareErrorCode PFX##dev_randbit_finalize_parties(hbmpc_ctx* ctx, const T* a, const T* opened_sq, size_t N, size_t parties,    \
                                                                T* out, uint8_t* status_out, hbmpc_randbit_summary* summary_dev,            \
                                                                void* stream) {                                                             \
        REQ(ctx);                                                                                                                           \
        return randbit_finalize_any(ctx, a, opened_sq, N, parties, out, status_out, summary_dev, stream);                                   \
    }
TYPED_SQRT(U256, REQ_FR, hbmpc_)
TYPED_SQRT(uint64_t, REQ_GL, hbmpc_gl_)
#undef TYPED_SQRT
static ShareErrorCode truncpr_rdash_impl(hbmpc_ctx* ctx, const U256* r_bits, size_t m, size_t N, size_t parties, U256* r_dash,
                                         void* stream) {
    REQ_FR(ctx);
    ELEM_PROLOGUE
    ELEM_BUFS(r_dash);
    if (m && !r_bits) return fail(ctx, InvalidInput, "null buffer");  // m = 0: no bit shares are read, r' = 0
    CHECK_PARTIES(parties);
    if (!truncpr_params_ok(ctx, TP_M, 0, m)) return InvalidInput;
    const uint32_t* pow2;
    const int impl = ctx->impl;
    ShareErrorCode rc = get_table(ctx, key("pow2", {m}, impl), [&] { return build_pow2(m, impl); }, &pow2);
    if (rc != ShareSuccess) return rc;
    launch_truncpr_rdash(impl, as_words(r_bits), (int)m, N, (unsigned)parties, pow2, as_words(r_dash), s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_truncpr_rdash(hbmpc_ctx* ctx, const U256* r_bits, size_t m, size_t N,
                                                  U256* r_dash, void* stream) {
    return truncpr_rdash_impl(ctx, r_bits, m, N, 1, r_dash, stream);
}
extern "C" ShareErrorCode hbmpc_dev_truncpr_rdash_parties(hbmpc_ctx* ctx, const U256* r_bits, size_t m, size_t N,
                                                          size_t parties, U256* r_dash, void* stream) {
    return truncpr_rdash_impl(ctx, r_bits, m, N, parties, r_dash, stream);
}
extern "C" ShareErrorCode hbmpc_dev_truncpr_open_share(hbmpc_ctx* ctx, const U256* a, const U256* r_dash,
                                                       const U256* r_int, size_t k, size_t m, size_t N, U256* open_out,
                                                       void* stream) {
    REQ_FR(ctx);
    if (ctx && !truncpr_params_ok(ctx, TP_K, k, m)) return InvalidInput;
    ELEM_PROLOGUE
    ELEM_BUFS(a, r_dash, r_int, open_out);
    const HFr two = HFr::from_u64(2);
    const HFr p2m = two.pow_u64(m), p2k = two.pow_u64(k - 1);
    const ElemConsts cs = elem_consts(ctx->impl, &p2m, &p2k);
    launch_truncpr_open(ctx->impl, as_words(a), as_words(r_dash), as_words(r_int), N, cs, as_words(open_out), s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_fpmul_middle(hbmpc_ctx* ctx, const U256* c, const U256* x, const U256* y, const U256* d,
                                                 const U256* e, const U256* r_bits, const U256* r_int, size_t k, size_t m, size_t N,
                                                 size_t parties, U256* z_out, U256* r_dash_out, U256* open_out, void* stream) {
    REQ_FR(ctx);
    if (ctx && !truncpr_params_ok(ctx, TP_K, k, m)) return InvalidInput;
    ELEM_PROLOGUE
    CHECK_PARTIES(parties);
    if (!truncpr_params_ok(ctx, TP_M, k, m)) return InvalidInput;
    if (!c || !x || !y || !d || !e || !r_int || !z_out || !r_dash_out || !open_out || (m && !r_bits)) return fail(ctx, InvalidInput, "null buffer");
    TruncprConsts tc;
    const ShareErrorCode rc = truncpr_consts(ctx, k, m, false, &tc);
    if (rc != ShareSuccess) return rc;
    const unsigned grid_parties = N >= ((size_t)1 << 16) ? 1 : (unsigned)parties;  // k_beaver_finalize's rule
    launch_fpmul_middle(ctx->impl, as_words(c), as_words(x), as_words(y), as_words(d), as_words(e), as_words(r_bits), as_words(r_int), (int)m, N, tc.cs, tc.pow2,
                        as_words(z_out), as_words(r_dash_out), as_words(open_out), (unsigned)parties, grid_parties, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
static ShareErrorCode truncpr_finalize_impl(hbmpc_ctx* ctx, const U256* a, const U256* r_dash, const U256* c_open, size_t m,
                                            size_t N, size_t parties, U256* d_out, void* stream) {
    REQ_FR(ctx);
    if (ctx && !truncpr_params_ok(ctx, TP_BYTES, 0, m)) return InvalidInput;
    ELEM_PROLOGUE
    ELEM_BUFS(a, r_dash, c_open, d_out);
    CHECK_PARTIES(parties);
    const HFr inv = inv_pow2(ctx, m);
    const ElemConsts cs = elem_consts(ctx->impl, &inv);
    launch_truncpr_finalize(ctx->impl, as_words(a), as_words(r_dash), as_words(c_open), (int)(m > 256 ? 256 : m), N, (unsigned)parties, cs, as_words(d_out), s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_truncpr_finalize(hbmpc_ctx* ctx, const U256* a, const U256* r_dash,
                                                     const U256* c_open, size_t m, size_t N, U256* d_out,
                                                     void* stream) {
    return truncpr_finalize_impl(ctx, a, r_dash, c_open, m, N, 1, d_out, stream);
}
extern "C" ShareErrorCode hbmpc_dev_truncpr_finalize_parties(hbmpc_ctx* ctx, const U256* a, const U256* r_dash,
                                                             const U256* c_open, size_t m, size_t N, size_t parties,
                                                             U256* d_out, void* stream) {
    return truncpr_finalize_impl(ctx, a, r_dash, c_open, m, N, parties, d_out, stream);
}
extern "C" ShareErrorCode hbmpc_dev_modmul_ubench(hbmpc_ctx* ctx, U256* out_dev, size_t threads, uint32_t iters,
                                                  void* stream) {
    REQ_FR(ctx);
    size_t N = threads;
    ELEM_PROLOGUE
    if (threads % 256) return fail(ctx, InvalidInput, "threads must be a multiple of 256");
    const ElemConsts cs = elem_consts(ctx->impl);
    launch_modmul_ubench(ctx->impl, as_words(out_dev), threads, iters, cs, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}

extern "C" ShareErrorCode hbmpc_dev_traffic_ubench(hbmpc_ctx* ctx, const U256* x_dev, size_t G, size_t m, U256* y_dev, size_t n, void* stream) {
    REQ_FR(ctx);
    if (!x_dev || !y_dev || G == 0 || m == 0 || n == 0 || m > 64 || n > 256) return fail(ctx, InvalidInput, "null buffer or shape out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    launch_traffic_ubench((unsigned)ctx->n_cus, (const uint4*)x_dev, G, (int)m, (uint4*)y_dev, (int)n, pick(ctx, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}

// host wrappers for the element-wise calls: n_in inputs of N elements (first input may be m*N), n_out outputs
template <class Fn>
static ShareErrorCode elem_host(hbmpc_ctx* ctx, std::initializer_list<std::pair<const void*, size_t>> ins,
                                std::initializer_list<std::pair<void*, size_t>> outs, Fn fn) {
    if (!ctx) return InvalidInput;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t eb = ebytes(ctx);
    size_t total = 0;
    for (auto& in : ins) total += in.second * eb;
    for (auto& o : outs) total += o.second * eb;
    Stage st(ctx, total, ins.size() + outs.size());
    std::vector<const void*> pi;
    std::vector<void*> po;
    for (auto& in : ins) {
        if (in.second && !in.first) return fail(ctx, InvalidInput, "null buffer");
        void* p = nullptr;
        HIP_TRY(ctx, st.in(in.first, in.second * eb, &p));
        pi.push_back(p);
    }
    for (auto& o : outs) {
        if (o.second && !o.first) return fail(ctx, InvalidInput, "null buffer");
        void* p = nullptr;
        HIP_TRY(ctx, st.alloc(o.second * eb, &p));
        po.push_back(p);
    }
    ShareErrorCode rc = fn(pi, po);
    if (rc != ShareSuccess) return rc;
    size_t k = 0;
    for (auto& o : outs) HIP_TRY(ctx, st.out(o.first, po[k++], o.second * eb));
    HIP_TRY(ctx, st.finish());
    return ShareSuccess;
}
typedef std::vector<const void*> VI;
typedef std::vector<void*> VO;
#define CU(p) ((const U256*)(p))
#define MU(p) ((U256*)(p))

#define TYPED_HOST(T, REQ, PFX)                                                                                          \
    extern "C" ShareErrorCode PFX##fr_op(hbmpc_ctx* ctx, int op, const T* a, const T* b, size_t N, T* out) {             \
        REQ(ctx);                                                                                                        \
        return elem_host(ctx, {{a, N}, {b, N}}, {{out, N}},                                                              \
                         [&](VI& i, VO& o) { return fr_op_any(ctx, op, i[0], i[1], N, o[0], nullptr); });                \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##fr_op_scalar(hbmpc_ctx* ctx, int op, const T* a, const T* scalar, size_t N, T* out) {  \
        REQ(ctx);                                                                                                        \
        return elem_host(ctx, {{a, N}}, {{out, N}},                                                                      \
                         [&](VI& i, VO& o) { return fr_op_scalar_any(ctx, op, i[0], scalar, N, o[0], nullptr); });       \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##triple_local(hbmpc_ctx* ctx, const T* a, const T* b, const T* r2t, size_t N, T* out) { \
        REQ(ctx);                                                                                                        \
        return elem_host(ctx, {{a, N}, {b, N}, {r2t, N}}, {{out, N}},                                                    \
                         [&](VI& i, VO& o) { return triple_local_any(ctx, i[0], i[1], i[2], N, o[0], nullptr); });       \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##triple_finalize(hbmpc_ctx* ctx, const T* rt, const T* opened, size_t N, T* c_out) {   \
        REQ(ctx);                                                                                                        \
        return elem_host(ctx, {{rt, N}, {opened, N}}, {{c_out, N}},                                                      \
                         [&](VI& i, VO& o) { return triple_finalize_any(ctx, i[0], i[1], N, o[0], nullptr); });          \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##beaver_open_shares(hbmpc_ctx* ctx, const T* a, const T* b, const T* x, const T* y,    \
                                                      size_t N, T* d_sh, T* e_sh) {                                      \
        REQ(ctx);                                                                                                        \
        return elem_host(ctx, {{a, N}, {b, N}, {x, N}, {y, N}}, {{d_sh, N}, {e_sh, N}}, [&](VI& i, VO& o) {              \
            return beaver_open_any(ctx, i[0], i[1], i[2], i[3], N, o[0], o[1], nullptr);                                 \
        });                                                                                                              \
    }                                                                                                                    \
    extern "C" ShareErrorCode PFX##beaver_finalize(hbmpc_ctx* ctx, const T* c, const T* x, const T* y, const T* d,       \
                                                   const T* e, size_t N, T* z) {                                         \
        REQ(ctx);                                                                                                        \
        return elem_host(ctx, {{c, N}, {x, N}, {y, N}, {d, N}, {e, N}}, {{z, N}}, [&](VI& i, VO& o) {                    \
            return beaver_finalize_any(ctx, i[0], i[1], i[2], i[3], i[4], N, o[0], nullptr);                             \
        });                                                                                                              \
    }
TYPED_HOST(U256, REQ_FR, hbmpc_)
TYPED_HOST(uint64_t, REQ_GL, hbmpc_gl_)
extern "C" ShareErrorCode hbmpc_truncpr_rdash(hbmpc_ctx* ctx, const U256* r_bits, size_t m, size_t N, U256* r_dash) {
    REQ_FR(ctx);
    return elem_host(ctx, {{r_bits, m * N}}, {{r_dash, N}},
                     [&](VI& i, VO& o) { return hbmpc_dev_truncpr_rdash(ctx, CU(i[0]), m, N, MU(o[0]), nullptr); });
}
extern "C" ShareErrorCode hbmpc_truncpr_open_share(hbmpc_ctx* ctx, const U256* a, const U256* r_dash,
                                                   const U256* r_int, size_t k, size_t m, size_t N, U256* open_out) {
    REQ_FR(ctx);
    return elem_host(ctx, {{a, N}, {r_dash, N}, {r_int, N}}, {{open_out, N}}, [&](VI& i, VO& o) {
        return hbmpc_dev_truncpr_open_share(ctx, CU(i[0]), CU(i[1]), CU(i[2]), k, m, N, MU(o[0]), nullptr);
    });
}
extern "C" ShareErrorCode hbmpc_truncpr_finalize(hbmpc_ctx* ctx, const U256* a, const U256* r_dash,
                                                 const U256* c_open, size_t m, size_t N, U256* d_out) {
    REQ_FR(ctx);
    return elem_host(ctx, {{a, N}, {r_dash, N}, {c_open, N}}, {{d_out, N}}, [&](VI& i, VO& o) {
        return hbmpc_dev_truncpr_finalize(ctx, CU(i[0]), CU(i[1]), CU(i[2]), m, N, MU(o[0]), nullptr);
    });
}

// ---- wire codec ---------------------------------------------------
extern "C" ShareErrorCode hbmpc_dev_pack_fvec(hbmpc_ctx* ctx, const U256* rows_dev, size_t row_stride, size_t G,
                                              size_t n_rows, void* payloads_dev, size_t payload_stride_bytes,
                                              void* stream) {
    REQ_FR(ctx);
    if (!ctx) return InvalidInput;
    if (n_rows == 0) return ShareSuccess;
    if (!rows_dev || !payloads_dev) return fail(ctx, InvalidInput, "null buffer");
    if (payload_stride_bytes % 8 || payload_stride_bytes < 8 + 32 * G || ((uintptr_t)payloads_dev & 7) || row_stride < G)
        return fail(ctx, InvalidInput, "payload stride must be 8-byte aligned and >= 8 + 32 G; row_stride >= G");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    launch_pack_fvec((const uint64_t*)rows_dev, row_stride, G, n_rows, (uint64_t*)payloads_dev, payload_stride_bytes / 8,
                     pick(ctx, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_unpack_fvec(hbmpc_ctx* ctx, const void* payloads_dev, size_t payload_stride_bytes,
                                                size_t payload_bytes, size_t G, size_t n_rows, U256* rows_dev,
                                                size_t row_stride, uint32_t* status_dev, void* stream) {
    REQ_FR(ctx);
    if (!ctx) return InvalidInput;
    if (n_rows == 0) return ShareSuccess;
    if (!rows_dev || !payloads_dev || !status_dev) return fail(ctx, InvalidInput, "null buffer");
    if (payload_bytes < 8 || payload_bytes < 8 + 32 * G)  // common/utils.rs:7-9; a short read fails every element
        return fail(ctx, InvalidInput, "payload shorter than its length prefix requires");
    if (payload_stride_bytes % 8 || payload_stride_bytes < payload_bytes || ((uintptr_t)payloads_dev & 7) || row_stride < G)
        return fail(ctx, InvalidInput, "payload stride must be 8-byte aligned and >= payload_bytes; row_stride >= G");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, hipMemsetAsync(status_dev, 0, n_rows * 4, s));
    launch_unpack_fvec((const uint64_t*)payloads_dev, payload_stride_bytes / 8, G, n_rows, (uint64_t*)rows_dev, row_stride,
                       status_dev, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
// In-place wire path (no pack / unpack pass): see include/hbmpc_hip.h
extern "C" ShareErrorCode hbmpc_dev_vandermonde_apply_strided(hbmpc_ctx* ctx, const U256* x_dev, size_t G, size_t n, size_t d,
                                                              U256* y_out_dev, size_t y_row_stride, void* stream) {
    REQ_FR(ctx);
    return eval_dev(ctx, x_dev, G, n, d, y_out_dev, stream, 1, y_row_stride);
}
extern "C" ShareErrorCode hbmpc_gl_dev_vandermonde_apply_strided(hbmpc_ctx* ctx, const uint64_t* x_dev, size_t G, size_t n,
                                                                 size_t d, uint64_t* y_out_dev, size_t y_row_stride,
                                                                 void* stream) {
    REQ_GL(ctx);
    return eval_dev(ctx, x_dev, G, n, d, y_out_dev, stream, 1, y_row_stride);
}
// x given as d + 1 rows (see include/hbmpc_hip.h): the point-pair matrix-core kernel reads them in place; every other
// shape goes through the workspace (transpose, then the chunk-major encode)
static ShareErrorCode eval_rows_any(hbmpc_ctx* ctx, const void* x_rows, size_t x_row_stride, size_t G, size_t n, size_t d, void* tmp,
                                    void* y, void* stream, const ListSpec* lists = nullptr) {
    if (!ctx) return InvalidInput;
    if (n <= d) return fail(ctx, InvalidInput, "number of shares must be greater than the degree");
    if (n == 0 || n > ((size_t)1 << 32)) return fail(ctx, NoSuitableDomain, "no radix-2 domain of that size");
    if (n > (1u << 20) || d > (1u << 20)) return fail(ctx, InvalidInput, "n, d beyond the supported range");
    if (x_row_stride < G) return fail(ctx, InvalidInput, "input row stride must be >= G");
    if (lists) {
        if (lists->rows == 0 || lists->row0 + lists->rows > n || lists->K == 0 || G % lists->K != 0 || lists->n_slices == 0 || lists->n_slices > 2 ||
            !lists->slices)
            return fail(ctx, InvalidInput, "list rows / slices out of range");
        for (size_t k = 0; k < lists->n_slices; ++k) {
            const hbmpc_list_slice& sl = lists->slices[k];
            if (!sl.dst_dev || sl.count == 0 || sl.k0 + sl.count > lists->K || sl.party_stride < sl.count * lists->rows)
                return fail(ctx, InvalidInput, "list slice out of range");
        }
        if (lists->n_slices == 2 && lists->slices[0].k0 + lists->slices[0].count > lists->slices[1].k0)
            return fail(ctx, InvalidInput, "list slices must be in ascending, disjoint ranges of batch elements");
    }
    if (G == 0) return ShareSuccess;
    if (!x_rows || !y) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    const size_t size = domain_size(n), dp1 = d + 1;
    if (lists && lists->others && (lists->rows >= n || (G / lists->K) * (n - lists->rows) * lists->K * 32 >= ((size_t)1 << 32)))
        return fail(ctx, InvalidInput, "party-major other rows: needs a row outside the lists and less than 4 GiB of them");
    auto copy_lists = [&]() -> ShareErrorCode {  // every row is in y[row][G]: the list rows are copied out per slice
        if (!lists) return ShareSuccess;
        const size_t parties = G / lists->K;
        if (lists->others) {  // and the other rows into their party-major place
            launch_rows_party_major(is_gold(ctx) ? 1 : 4, (const uint64_t*)y, G, lists->K, (int)lists->row0, (int)lists->rows, (int)(n - lists->rows),
                                    (uint64_t*)lists->others, s);
            HIP_TRY(ctx, hipGetLastError());
        }
        for (size_t k = 0; k < lists->n_slices; ++k) {
            const hbmpc_list_slice& sl = lists->slices[k];
            const ShareErrorCode rc = hbmpc_dev_transpose(ctx, (const uint8_t*)y + (lists->row0 * G + sl.k0) * ebytes(ctx), lists->rows, sl.count, G,
                                                          sl.dst_dev, lists->rows, parties, lists->K, sl.party_stride, stream);
            if (rc != ShareSuccess) return rc;
        }
        return ShareSuccess;
    };
    EncodeShape shape{EncodeKind::Rows, G, n, d};
    shape.lists = lists != nullptr;
    const EncodePlan plan = plan_encode(encode_knobs(ctx), shape);
    for (int i = 0; i < plan.count; ++i) {
        const EncodeRoute& r = plan.route[i];
        ShareErrorCode rc = ShareSuccess;
        if (r.kernel == EncodeKernel::BflyLists || r.kernel == EncodeKernel::Bfly) {
            // the list rows straight from the kernel that computes them, or every row to y and the lists copied out
            const bool in_kernel = r.kernel == EncodeKernel::BflyLists;
            if (run_mfma(ctx, r, (const uint32_t*)x_rows, G, n, dp1, EvalOut{(uint32_t*)y, 0, 1}, s, &rc, x_row_stride, in_kernel ? lists : nullptr)) {
                if (rc != ShareSuccess) return rc;
                HIP_TRY(ctx, hipGetLastError());
                return in_kernel ? ShareSuccess : copy_lists();
            }
        } else if (r.kernel == EncodeKernel::Fft1Mix) {
            const bool gold = is_gold(ctx);
            const uint32_t* tw;
            rc = get_table(ctx, key("tw", {size}, ctx->impl), [&] {
                return gold ? build_twiddles<HGl>(size, ctx->impl) : build_twiddles<HFr>(size, ctx->impl);
            }, &tw);
            if (rc != ShareSuccess) return rc;
            MixOut o;
            memset(&o, 0, sizeof o);
            o.y = (uint32_t*)y, o.others = (uint32_t*)lists->others, o.K = lists->K, o.row0 = (int)lists->row0, o.rows = (int)lists->rows;
            for (size_t k = 0; k < lists->n_slices; ++k)
                o.list[k] = MixOut::Slice{(uint32_t*)lists->slices[k].dst_dev, lists->slices[k].party_stride, lists->slices[k].k0, lists->slices[k].count};
            if (gold ? launch_gold_fft1_mix(ilog2(size), (int)dp1, (const uint32_t*)x_rows, x_row_stride, G, (int)n, tw, o, s)
                     : launch_fft1_mix_lo(ilog2(size), (int)dp1, (const uint32_t*)x_rows, x_row_stride, G, (int)n, tw, o, s)) {
                HIP_TRY(ctx, hipGetLastError());
                return ShareSuccess;
            }
        }
    }
    // the last candidate (EncodeKernel::Transpose): the rows into the workspace chunk-major, then the chunk-major encode
    if (!tmp) return fail(ctx, InvalidInput, "no kernel reads this shape from rows: pass a workspace of G * (d + 1) elements");
    if ((dp1 + 15) / 16 > 65535) return fail(ctx, InvalidInput, "d beyond the launch grid");
    launch_transpose(is_gold(ctx) ? 1 : 4, (const uint64_t*)x_rows, dp1, G, x_row_stride, (uint64_t*)tmp, dp1, 1, 0, 0, s);
    HIP_TRY(ctx, hipGetLastError());
    const ShareErrorCode rc = eval_dev(ctx, tmp, G, n, d, y, stream);
    return rc != ShareSuccess ? rc : copy_lists();
}
extern "C" ShareErrorCode hbmpc_dev_vandermonde_apply_rows(hbmpc_ctx* ctx, const U256* x_rows_dev, size_t x_row_stride, size_t G, size_t n,
                                                           size_t d, U256* tmp_dev, U256* y_out_dev, void* stream) {
    REQ_FR(ctx);
    return eval_rows_any(ctx, x_rows_dev, x_row_stride, G, n, d, tmp_dev, y_out_dev, stream);
}
extern "C" ShareErrorCode hbmpc_gl_dev_vandermonde_apply_rows(hbmpc_ctx* ctx, const uint64_t* x_rows_dev, size_t x_row_stride, size_t G,
                                                              size_t n, size_t d, uint64_t* tmp_dev, uint64_t* y_out_dev, void* stream) {
    REQ_GL(ctx);
    return eval_rows_any(ctx, x_rows_dev, x_row_stride, G, n, d, tmp_dev, y_out_dev, stream);
}
static ShareErrorCode eval_rows_lists_any(hbmpc_ctx* ctx, const void* x_rows, size_t x_row_stride, size_t G, size_t n, size_t d, void* tmp, void* y,
                                          size_t list_row0, size_t list_rows, size_t K, const hbmpc_list_slice* slices, size_t n_slices, void* stream,
                                          void* others = nullptr, bool want_others = false) {
    if (ctx && want_others && !others) return fail(ctx, InvalidInput, "null buffer");
    const ListSpec ls{list_row0, list_rows, K, slices, n_slices, others};
    return eval_rows_any(ctx, x_rows, x_row_stride, G, n, d, tmp, y, stream, &ls);
}
// would the mixing step write its lists (and party-major other rows) from the kernel that computes them?  (otherwise: all rows to y, then copies)
extern "C" ShareErrorCode hbmpc_dev_apply_rows_lists_in_kernel(hbmpc_ctx* ctx, size_t G, size_t n, size_t d, int* yes_out) {
    if (!ctx || !yes_out) return InvalidInput;
    *yes_out = encode_lists_in_kernel(encode_knobs(ctx), G, n, d);
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_vandermonde_apply_rows_split(hbmpc_ctx* ctx, const U256* x_rows_dev, size_t x_row_stride, size_t G, size_t n, size_t d,
                                                                 U256* tmp_dev, U256* y_out_dev, size_t list_row0, size_t list_rows, size_t K,
                                                                 const hbmpc_list_slice* slices, size_t n_slices, U256* others_out_dev, void* stream) {
    REQ_FR(ctx);
    return eval_rows_lists_any(ctx, x_rows_dev, x_row_stride, G, n, d, tmp_dev, y_out_dev, list_row0, list_rows, K, slices, n_slices, stream, others_out_dev, true);
}
extern "C" ShareErrorCode hbmpc_gl_dev_vandermonde_apply_rows_split(hbmpc_ctx* ctx, const uint64_t* x_rows_dev, size_t x_row_stride, size_t G, size_t n,
                                                                    size_t d, uint64_t* tmp_dev, uint64_t* y_out_dev, size_t list_row0, size_t list_rows,
                                                                    size_t K, const hbmpc_list_slice* slices, size_t n_slices, uint64_t* others_out_dev,
                                                                    void* stream) {
    REQ_GL(ctx);
    return eval_rows_lists_any(ctx, x_rows_dev, x_row_stride, G, n, d, tmp_dev, y_out_dev, list_row0, list_rows, K, slices, n_slices, stream, others_out_dev, true);
}
extern "C" ShareErrorCode hbmpc_dev_vandermonde_apply_rows_lists(hbmpc_ctx* ctx, const U256* x_rows_dev, size_t x_row_stride, size_t G, size_t n,
                                                                 size_t d, U256* tmp_dev, U256* y_out_dev, size_t list_row0, size_t list_rows,
                                                                 size_t K, const hbmpc_list_slice* slices, size_t n_slices, void* stream) {
    REQ_FR(ctx);
    return eval_rows_lists_any(ctx, x_rows_dev, x_row_stride, G, n, d, tmp_dev, y_out_dev, list_row0, list_rows, K, slices, n_slices, stream);
}
extern "C" ShareErrorCode hbmpc_gl_dev_vandermonde_apply_rows_lists(hbmpc_ctx* ctx, const uint64_t* x_rows_dev, size_t x_row_stride, size_t G,
                                                                    size_t n, size_t d, uint64_t* tmp_dev, uint64_t* y_out_dev, size_t list_row0,
                                                                    size_t list_rows, size_t K, const hbmpc_list_slice* slices, size_t n_slices,
                                                                    void* stream) {
    REQ_GL(ctx);
    return eval_rows_lists_any(ctx, x_rows_dev, x_row_stride, G, n, d, tmp_dev, y_out_dev, list_row0, list_rows, K, slices, n_slices, stream);
}
static ShareErrorCode encode_fvec_any(hbmpc_ctx* ctx, const void* x_dev, size_t G, size_t n, size_t d, void* payloads_dev,
                                      size_t payload_stride_bytes, void* stream) {
    if (!ctx) return InvalidInput;
    if (!payloads_dev) return fail(ctx, InvalidInput, "null buffer");
    const size_t eb = ebytes(ctx);  // Fr: bodies must be 32-byte aligned; Goldilocks: 8-byte elements, any 8-byte-aligned payload
    if (((uintptr_t)payloads_dev + 8) % eb || payload_stride_bytes % eb || payload_stride_bytes < 8 + eb * G)
        return fail(ctx, InvalidInput, eb == 32 ? "payloads must start 8 bytes before a 32-byte boundary, at a stride that is a multiple of 32 and >= 8 + 32 G"
                                                : "payloads must be 8-byte aligned, at a stride that is a multiple of 8 and >= 8 + 8 G");
    ShareErrorCode rc = eval_dev(ctx, x_dev, G, n, d, (char*)payloads_dev + 8, stream, 1, payload_stride_bytes / eb);
    if (rc != ShareSuccess || G == 0) return rc;
    launch_fvec_prefix((uint64_t*)payloads_dev, payload_stride_bytes / 8, G, n, pick(ctx, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
static ShareErrorCode validate_fvec_any(hbmpc_ctx* ctx, const void* payloads_dev, size_t payload_stride_bytes,
                                        size_t payload_bytes, size_t G, size_t n_rows, uint32_t* status_dev, void* stream) {
    if (!ctx) return InvalidInput;
    if (n_rows == 0) return ShareSuccess;
    if (!payloads_dev || !status_dev) return fail(ctx, InvalidInput, "null buffer");
    const size_t eb = ebytes(ctx);
    if (payload_bytes < 8 || payload_bytes < 8 + eb * G)
        return fail(ctx, InvalidInput, "payload shorter than its length prefix requires");
    if (payload_stride_bytes % 8 || payload_stride_bytes < payload_bytes || ((uintptr_t)payloads_dev & 7))
        return fail(ctx, InvalidInput, "payload stride must be 8-byte aligned and >= payload_bytes");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, hipMemsetAsync(status_dev, 0, n_rows * 4, s));
    launch_validate_fvec((const uint64_t*)payloads_dev, payload_stride_bytes / 8, G, n_rows, status_dev, s, is_gold(ctx));
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
#define TYPED_WIRE(T, REQ, PFX)                                                                                            \
    extern "C" ShareErrorCode PFX##dev_encode_fvec(hbmpc_ctx* ctx, const T* x_dev, size_t G, size_t n, size_t d,           \
                                                   void* payloads_dev, size_t payload_stride_bytes, void* stream) {         \
        REQ(ctx);                                                                                                          \
        return encode_fvec_any(ctx, x_dev, G, n, d, payloads_dev, payload_stride_bytes, stream);                           \
    }                                                                                                                      \
    extern "C" ShareErrorCode PFX##dev_validate_fvec(hbmpc_ctx* ctx, const void* payloads_dev, size_t payload_stride_bytes, \
                                                     size_t payload_bytes, size_t G, size_t n_rows, uint32_t* status_dev,  \
                                                     void* stream) {                                                       \
        REQ(ctx);                                                                                                          \
        return validate_fvec_any(ctx, payloads_dev, payload_stride_bytes, payload_bytes, G, n_rows, status_dev, stream);   \
    }
TYPED_WIRE(U256, REQ_FR, hbmpc_)
TYPED_WIRE(uint64_t, REQ_GL, hbmpc_gl_)
extern "C" ShareErrorCode hbmpc_dev_pack_shares(hbmpc_ctx* ctx, const U256* values_dev, size_t N, size_t id,
                                                size_t degree, void* payload_dev, void* stream) {
    REQ_FR(ctx);
    if (!ctx) return InvalidInput;
    if (!payload_dev || (N && !values_dev) || ((uintptr_t)payload_dev & 7)) return fail(ctx, InvalidInput, "bad buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    launch_pack_shares((const uint64_t*)values_dev, N, id, degree, (uint64_t*)payload_dev, pick(ctx, stream));
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_unpack_shares(hbmpc_ctx* ctx, const void* payload_dev, size_t payload_bytes, size_t N,
                                                  size_t id, size_t degree, U256* values_dev, uint32_t* status_dev,
                                                  void* stream) {
    REQ_FR(ctx);
    if (!ctx) return InvalidInput;
    if (!payload_dev || !status_dev || (N && !values_dev) || ((uintptr_t)payload_dev & 7)) return fail(ctx, InvalidInput, "bad buffer");
    if (payload_bytes < 8 + 48 * N) return fail(ctx, InvalidInput, "payload shorter than its length prefix requires");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, hipMemsetAsync(status_dev, 0, 4, s));
    launch_unpack_shares((const uint64_t*)payload_dev, N, id, degree, (uint64_t*)values_dev, status_dev, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_validate_canonical(hbmpc_ctx* ctx, const U256* a_dev, size_t N, uint32_t* status_dev,
                                                       void* stream) {
    REQ_FR(ctx);
    if (!ctx) return InvalidInput;
    if (!status_dev || (N && !a_dev)) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    HIP_TRY(ctx, hipMemsetAsync(status_dev, 0, 4, s));
    if (N) launch_validate_canonical((const uint64_t*)a_dev, N, status_dev, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}

// ---- layout / verdict steps of the preprocessing producers (either field: the element size follows the context) ----
extern "C" ShareErrorCode hbmpc_dev_transpose(hbmpc_ctx* ctx, const void* src_dev, size_t rows, size_t cols, size_t src_row_stride,
                                              void* dst_dev, size_t dst_row_stride, size_t batch, size_t src_batch_stride,
                                              size_t dst_batch_stride, void* stream) {
    if (!ctx) return InvalidInput;
    if (rows == 0 || cols == 0 || batch == 0) return ShareSuccess;
    if (!src_dev || !dst_dev) return fail(ctx, InvalidInput, "null buffer");
    if (src_row_stride < cols || dst_row_stride < rows) return fail(ctx, InvalidInput, "row stride below the row length");
    if (batch > 65535 || (rows + 15) / 16 > 65535) return fail(ctx, InvalidInput, "batch / rows beyond the launch grid");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    launch_transpose(is_gold(ctx) ? 1 : 4, (const uint64_t*)src_dev, rows, cols, src_row_stride, (uint64_t*)dst_dev, dst_row_stride, batch,
                     src_batch_stride, dst_batch_stride, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
// Slices of [party][len] pools, regrouped on the way: every check before the launch, so a refused call writes nothing.  A slice whose
// group fits the take kernel's tile goes into ONE launch with the others (kernels_take.hpp); one beyond it takes launch_transpose with
// the rows as its batch (plan_take, take_plan.hpp) -- the same bytes.
extern "C" ShareErrorCode hbmpc_dev_take_rows(hbmpc_ctx* ctx, const hbmpc_take_slice* slices, size_t count, size_t rows, void* stream) {
    if (!ctx) return InvalidInput;
    if (const char* why = check_take_call(slices != nullptr, count, rows)) return fail(ctx, InvalidInput, why);
    const size_t eb = ebytes(ctx);
    TakeArgs args{};
    size_t nfused = 0, tiles = 0;
    for (size_t i = 0; i < count; ++i) {
        const hbmpc_take_slice& sl = slices[i];
        if (const char* why = check_take_slice(sl.src, sl.src_row_stride, sl.dst, sl.dst_row_stride, sl.elements, sl.group)) return fail(ctx, InvalidInput, why);
        const TakePlan pl = plan_take(eb, sl.group);
        if (pl.transpose) continue;
        const size_t C = sl.elements / sl.group, t = (C + pl.tile - 1) / pl.tile;  // elements <= 2^31: inside the grid's x on either route
        args.s[nfused] = TakeSliceArg{(const uint64_t*)sl.src, (uint64_t*)sl.dst, sl.src_row_stride, sl.dst_row_stride, C, (uint32_t)sl.group, (uint32_t)pl.tile};
        ++nfused;
        tiles = std::max(tiles, t);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    const int ew64 = (int)(eb / 8);
    if (nfused) launch_take_rows(ew64, args, (unsigned)tiles, (unsigned)rows, (unsigned)nfused, s);
    for (size_t i = 0; i < count; ++i) {
        const hbmpc_take_slice& sl = slices[i];
        if (!plan_take(eb, sl.group).transpose) continue;
        // dst[r][j][i] = src[r][i][j]: a C x group matrix per row, at most 65535 tiles of 16 i to a launch
        const size_t C = sl.elements / sl.group, step = (size_t)65535 * 16;
        for (size_t c0 = 0; c0 < C; c0 += step)
            launch_transpose(ew64, (const uint64_t*)sl.src + c0 * sl.group * ew64, std::min(step, C - c0), sl.group, sl.group, (uint64_t*)sl.dst + c0 * ew64, C, rows,
                             sl.src_row_stride, sl.dst_row_stride, s);
    }
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_check_degree(hbmpc_ctx* ctx, const void* coeffs_dev, const uint8_t* status_dev, size_t G, size_t m,
                                                 size_t want_degree, uint32_t* bad_dev, void* stream) {
    if (!ctx) return InvalidInput;
    if (!bad_dev || (G && !coeffs_dev) || m == 0 || m > 65535) return fail(ctx, InvalidInput, "null buffer or bad length");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    if (G) launch_check_degree(is_gold(ctx) ? 1 : 4, (const uint64_t*)coeffs_dev, status_dev, G, (int)m, (int)want_degree, bad_dev, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
// columns > 0: the G entries are several verifiers' columns one after the other; bad[1] is the lowest failing COLUMN (g mod columns)
static ShareErrorCode check_top_coeff_any(hbmpc_ctx* ctx, const void* top_dev, const uint8_t* status_dev, size_t G, size_t want_degree, uint32_t* bad_dev,
                                          void* stream, size_t columns) {
    if (!ctx) return InvalidInput;
    if (!bad_dev || (G && !top_dev) || want_degree > 65535) return fail(ctx, InvalidInput, "null buffer or bad degree");
    if (columns && G % columns != 0) return fail(ctx, InvalidInput, "G must be a multiple of the number of columns");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    if (G) launch_check_top_coeff(is_gold(ctx) ? 1 : 4, (const uint64_t*)top_dev, status_dev, G, (int)want_degree, bad_dev, s, columns);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_check_top_coeff(hbmpc_ctx* ctx, const void* top_dev, const uint8_t* status_dev, size_t G, size_t want_degree,
                                                    uint32_t* bad_dev, void* stream) {
    return check_top_coeff_any(ctx, top_dev, status_dev, G, want_degree, bad_dev, stream, 0);
}
extern "C" ShareErrorCode hbmpc_dev_check_top_coeff_columns(hbmpc_ctx* ctx, const void* top_dev, const uint8_t* status_dev, size_t G, size_t columns,
                                                            size_t want_degree, uint32_t* bad_dev, void* stream) {
    return check_top_coeff_any(ctx, top_dev, status_dev, G, want_degree, bad_dev, stream, columns);
}
extern "C" ShareErrorCode hbmpc_dev_check_double_share_sel(hbmpc_ctx* ctx, const void* sel_t_dev, const uint8_t* status_t_dev, const void* sel_2t_dev,
                                                           const uint8_t* status_2t_dev, size_t G, size_t columns, size_t t, uint32_t* bad_dev, void* stream) {
    if (!ctx) return InvalidInput;
    if (!bad_dev || (G && (!sel_t_dev || !sel_2t_dev || !status_t_dev || !status_2t_dev))) return fail(ctx, InvalidInput, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    if (columns && G % columns != 0) return fail(ctx, InvalidInput, "G must be a multiple of the columns");
    if (G) launch_check_double_sel(is_gold(ctx) ? 1 : 4, (const uint64_t*)sel_t_dev, status_t_dev, (const uint64_t*)sel_2t_dev, status_2t_dev, G, (int)t, bad_dev, s, columns);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_check_double_share(hbmpc_ctx* ctx, const void* coeffs_t_dev, const void* coeffs_2t_dev, size_t G, size_t m,
                                                       size_t t, uint32_t* bad_dev, void* stream) {
    if (!ctx) return InvalidInput;
    if (!bad_dev || (G && (!coeffs_t_dev || !coeffs_2t_dev)) || m == 0 || m > 65535) return fail(ctx, InvalidInput, "null buffer or bad length");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    if (G) launch_check_double(is_gold(ctx) ? 1 : 4, (const uint64_t*)coeffs_t_dev, (const uint64_t*)coeffs_2t_dev, G, (int)m, (int)t, bad_dev, s);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
// columns: 0, or the G entries are several verifiers' results for the same `columns` columns, one verifier after the other (G a multiple of it):
// bad[1] is then the lowest failing COLUMN
extern "C" ShareErrorCode hbmpc_dev_check_double_share_c0_columns(hbmpc_ctx* ctx, const void* c0_t_dev, const uint32_t* degree_t_dev, const void* c0_2t_dev,
                                                                  const uint32_t* degree_2t_dev, size_t G, size_t columns, size_t t, uint32_t* bad_dev,
                                                                  void* stream) {
    if (!ctx) return InvalidInput;
    if (!bad_dev || (G && (!c0_t_dev || !c0_2t_dev || !degree_t_dev || !degree_2t_dev))) return fail(ctx, InvalidInput, "null buffer");
    if (columns && G % columns != 0) return fail(ctx, InvalidInput, "G must be a multiple of the number of columns");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick(ctx, stream);
    if (G) launch_check_double_c0(is_gold(ctx) ? 1 : 4, (const uint64_t*)c0_t_dev, degree_t_dev, (const uint64_t*)c0_2t_dev, degree_2t_dev, G, (int)t, bad_dev, s, columns);
    HIP_TRY(ctx, hipGetLastError());
    return ShareSuccess;
}
extern "C" ShareErrorCode hbmpc_dev_check_double_share_c0(hbmpc_ctx* ctx, const void* c0_t_dev, const uint32_t* degree_t_dev, const void* c0_2t_dev,
                                                          const uint32_t* degree_2t_dev, size_t G, size_t t, uint32_t* bad_dev, void* stream) {
    return hbmpc_dev_check_double_share_c0_columns(ctx, c0_t_dev, degree_t_dev, c0_2t_dev, degree_2t_dev, G, 0, t, bad_dev, stream);
}

#include "capi_recover.inc"
#include "capi_riss.inc"

// ---- whole protocol steps for all parties on this device ------------------------------------------------------------------------
// Which form each call takes is decided in one place, plan_protocol (protocol_route.hpp); what follows is shared by their executors.
static std::vector<size_t> first_ids(size_t count) {  // senders 0 .. count - 1
    std::vector<size_t> ids(count);
    for (size_t i = 0; i < count; ++i) ids[i] = i;
    return ids;
}
// The enqueue of a one-launch protocol kernel: the decode's counters at the start of the stream's scratch go to *counters, every
// summary (kernel argument, caller's buffer) the caller did not ask for to the scratch's local summary slot, then launch() -- void,
// or a ShareErrorCode -- and its error.  The kernel's last workgroup leaves the counters at zero.
template <class Launch>
static ShareErrorCode enqueue_one_launch(hbmpc_ctx* ctx, hipStream_t s, uint32_t** counters,
                                         std::initializer_list<std::pair<uint32_t**, hbmpc_recover_summary*>> summaries, Launch launch) {
    return with_decode_counters(ctx, s, 2048, [&](uint32_t* c) -> ShareErrorCode {
        *counters = c;
        for (const auto& sm : summaries) *sm.first = sm.second ? (uint32_t*)sm.second : c + 4;
        if constexpr (std::is_void<decltype(launch())>::value) launch();
        else if (const ShareErrorCode rc = launch(); rc != ShareSuccess) return rc;
        HIP_TRY(ctx, hipGetLastError());
        return ShareSuccess;
    });
}
// The shares Multiply opens (multiplication.rs:417-426) and reconstruct_rbc's recover_secret of a - x and of b - y (:102-139): ONE
// P(0) decode over the 2 N values of a sender row, into de_out [2][N].
// pair_first (large batches): the shares are formed as the matrix-core decode loads them (kernels_mfma.hpp, k_mfma_rows<.., SUB>) --
// 4 (2t + 1) loads per element instead of a launch that writes all n parties' two shares and a decode that reads 2t + 1 of them
// back (config 5: 0.14 + 0.065 ms -> 0.11).  Otherwise, and when the decode declines that form: the shares go to de_sh_ws
// [party][2][N] and the decode reads row s as sender_ids[s]'s or, with slots, every sender's row in place at its party id.
static ShareErrorCode open_beaver_pair(hbmpc_ctx* ctx, bool pair_first, bool slots, const size_t* sender_ids, size_t S, const void* a, const void* b,
                                       const void* x, const void* y, size_t N, size_t n, size_t t, void* de_sh_ws, void* de_out, uint8_t* status_out,
                                       hbmpc_recover_summary* summary_dev, void* stream) {
    RecoverCall c{.sender_ids = sender_ids, .S = S, .G = 2 * N, .n = n, .d = t, .t = t, .out = de_out, .status = status_out, .summary = summary_dev,
                  .p0 = true, .stream = stream};
    const PairInput pi = {as_words(a), as_words(b), as_words(x), as_words(y), N};
    if (pair_first) {
        c.pair = &pi;
        const ShareErrorCode rc = batch_recover_dev(ctx, c);
        if (rc != HBMPC_NOT_FUSED) return rc;
        c.pair = nullptr;
    }
    const ShareErrorCode rc = beaver_open_pair_any(ctx, a, b, x, y, N, n, de_sh_ws, stream);
    if (rc != ShareSuccess) return rc;
    c.evals = de_sh_ws, c.slots = slots ? sender_ids : nullptr;
    return batch_recover_dev(ctx, c);
}

// ---- TripleGenNode for all parties on this device (triple_gen/triple_generation.rs:304-364) --------------------------------------
// T: U256 (H = HFr) or uint64_t (H = HGl)
template <class H, class T>
static ShareErrorCode triplegen_parties_any(hbmpc_ctx* ctx, const T* a, const T* b, const T* r2t, const T* rt, size_t N, size_t n, size_t t, T* y_ws,
                                            T* z_ws, T* opened_out, T* c_out, uint8_t* status_out, hbmpc_recover_summary* summary_first_dev,
                                            hbmpc_recover_summary* summary_dev, void* stream) {
    if (!ctx) return InvalidInput;
    if (!a || !b || !r2t || !rt || !y_ws || !z_ws || !opened_out || !c_out) return fail(ctx, InvalidInput, "null buffer");
    const size_t M = 2 * t + 1, d = 2 * t;
    if (N == 0 || n == 0 || n > 255 || N % M != 0) return fail(ctx, InvalidInput, "N must be a positive multiple of 2t + 1; n in 1 .. 255");
    if (n < 3 * t + 1) return fail(ctx, InvalidInput, "n must be >= 3t + 1 for Byzantine fault tolerance");
    const size_t G = N / M;
    const std::vector<size_t> ids = first_ids(n);
    if (plan_protocol(protocol_knobs(ctx), {ProtocolCall::TripleGen, N, n, t, 0, 0}).one_launch) {  // a workgroup per chunk (kernels_triplegen_wg.hpp)
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick(ctx, stream);
        const int impl = ctx->impl;
        TripleGenWgArgs ta;
        memset(&ta, 0, sizeof ta);
        ShareErrorCode rc = rec_table<H>(ctx, *domain_inv<H>(ctx, n), ids, n, d, t, &ta.tab);
        if (rc != ShareSuccess) return rc;
        rc = vmat_table<H>(ctx, n, d, &ta.vmat);
        if (rc != ShareSuccess) return rc;
        const ElemConsts cs = elem_consts(impl);
        memcpy(ta.r2, cs.r2, sizeof ta.r2);
        ta.a = (const uint32_t*)a, ta.b = (const uint32_t*)b, ta.r2t = (const uint32_t*)r2t, ta.rt = (const uint32_t*)rt;
        ta.Y = (uint32_t*)y_ws, ta.Z = (uint32_t*)z_ws, ta.opened = (uint32_t*)opened_out, ta.c = (uint32_t*)c_out, ta.status = status_out;
        ta.G = G, ta.N = N, ta.n = (int)n, ta.t = (int)t;
        return enqueue_one_launch(ctx, s, &ta.counters, {{&ta.summary_first, summary_first_dev}, {&ta.summary, summary_dev}}, [&] { launch_triplegen_wg(impl, ta, s); });
    }
    // [ab - r]_2t Vandermonde-encoded in chunks of 2t + 1 for every recipient (batch_recon.rs:157-165), all parties in one launch;
    // EvalBatch arm for ALL recipients in one call: the row of sender p for "chunk" j G + g is y_ws + p (n G) + (j G + g);
    // RevealBatch arm: everyone interpolates the 2t + 1 opened values per chunk from the n broadcast values;
    // [c]_t = rt_i + opened (triple_generation.rs:196-208)
    ShareErrorCode rc = triple_encode_any(ctx, a, b, r2t, G, n, d, n, c_out, y_ws, stream);
    if (rc != ShareSuccess) return rc;
    rc = batch_recover_dev(ctx, {.sender_ids = ids.data(), .S = n, .evals = y_ws, .row_stride = n * G, .G = n * G, .n = n, .d = d, .t = t, .out = z_ws,
                                 .status = status_out, .summary = summary_first_dev, .p0 = true, .stream = stream});
    if (rc != ShareSuccess) return rc;
    rc = batch_recover_dev(ctx, {.sender_ids = ids.data(), .S = n, .evals = z_ws, .G = G, .n = n, .d = d, .t = t, .out = opened_out, .status = status_out,
                                 .summary = summary_dev, .stream = stream});
    if (rc != ShareSuccess) return rc;
    return triple_finalize_any(ctx, rt, opened_out, N, c_out, stream, n);
}
extern "C" ShareErrorCode hbmpc_dev_triplegen_parties(hbmpc_ctx* ctx, const U256* a, const U256* b, const U256* r2t, const U256* rt, size_t N,
                                                      size_t n, size_t t, U256* y_ws, U256* z_ws, U256* opened_out, U256* c_out, uint8_t* status_out,
                                                      hbmpc_recover_summary* summary_first_dev, hbmpc_recover_summary* summary_dev, void* stream) {
    REQ_FR(ctx);
    return triplegen_parties_any<HFr>(ctx, a, b, r2t, rt, N, n, t, y_ws, z_ws, opened_out, c_out, status_out, summary_first_dev, summary_dev, stream);
}
extern "C" ShareErrorCode hbmpc_gl_dev_triplegen_parties(hbmpc_ctx* ctx, const uint64_t* a, const uint64_t* b, const uint64_t* r2t, const uint64_t* rt,
                                                         size_t N, size_t n, size_t t, uint64_t* y_ws, uint64_t* z_ws, uint64_t* opened_out,
                                                         uint64_t* c_out, uint8_t* status_out, hbmpc_recover_summary* summary_first_dev,
                                                         hbmpc_recover_summary* summary_dev, void* stream) {
    REQ_GL(ctx);
    return triplegen_parties_any<HGl>(ctx, a, b, r2t, rt, N, n, t, y_ws, z_ws, opened_out, c_out, status_out, summary_first_dev, summary_dev, stream);
}

// ---- FPMulNode for all parties on this device (fpmul/fpmul.rs:61-110) ----------------------------------------------------------
// The table of k_fpmul_wave: the verify rows and the P(0) row of the decode's table, and the P(0) row scaled by R (its
// dot product is the opened value in Montgomery form: what finalize_mul multiplies the shares by)
static ShareErrorCode fpmul_wave_table(hbmpc_ctx* ctx, const SortedSenders& ss, size_t n, size_t t, const uint32_t** out) {
    const int impl = ctx->impl;
    const std::shared_ptr<const DomainInv<HFr>> dom = domain_inv<HFr>(ctx, n);
    return get_table(ctx, ids_key("fpw", ss.ids, 2 * t + 1, n, t, t, impl), [&] {
        const auto rows = recover_coeff_rows<HFr>(*dom, ss.ids, t, t);  // t verify rows, then the coefficient rows
        const HFr R = rdev_value(impl);
        std::vector<uint32_t> w;
        for (size_t r = 0; r <= t; ++r)
            for (size_t i = 0; i <= t; ++i) put_const(w, rows[r][i], impl);
        for (size_t i = 0; i <= t; ++i) put_const(w, rows[t][i] * R, impl);
        return w;
    }, out);
}
// The call is ONE launch, a wave per element (kernels_fpmul_wave.hpp), or the five separate launches below -- the same bytes in
// every output buffer.
extern "C" ShareErrorCode hbmpc_dev_fpmul_parties(hbmpc_ctx* ctx, const size_t* sender_ids, size_t S, const U256* a, const U256* b, const U256* c,
                                                  const U256* x, const U256* y, const U256* r_bits, const U256* r_int, size_t k, size_t m, size_t N,
                                                  size_t n, size_t t, U256* de_sh_ws, U256* de_out, U256* z_out, U256* r_dash_out,
                                                  U256* open_sh_out, U256* c_open_out, U256* d_out, uint8_t* status_out,
                                                  hbmpc_recover_summary* summary_first_dev, hbmpc_recover_summary* summary_dev, void* stream) {
    if (!ctx) return InvalidInput;
    REQ_FR(ctx);
    if (!truncpr_params_ok(ctx, TP_ALL, k, m)) return InvalidInput;
    if (!sender_ids || !a || !b || !c || !x || !y || !r_int || (m && !r_bits) || !de_sh_ws || !de_out || !z_out || !r_dash_out || !open_sh_out ||
        !c_open_out || !d_out)
        return fail(ctx, InvalidInput, "null buffer");
    if (!batch_in_range(ctx, N, n)) return InvalidInput;
    const ProtocolPlan plan = plan_protocol(protocol_knobs(ctx), {ProtocolCall::FpMul, N, n, t, S, m});
    if (plan.one_launch) {
        SortedSenders ss;
        ShareErrorCode rc = validate_senders(ctx, sender_ids, S, N, n, t, t, &ss);
        if (rc != ShareSuccess) return rc;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick(ctx, stream);
        FpmulWaveArgs fa;
        memset(&fa, 0, sizeof fa);
        fa.N = N, fa.parties = (int)n, fa.m = (int)m, fa.needed = (int)(2 * t + 1), fa.M = (int)(t + 1), fa.mask_bits = (int)(m > 256 ? 256 : m);
        fa.lk1 = plan.lk_row, fa.lk3 = plan.lk_wave;
        if (launch_fpmul_wave(fa, ctx->device, s, true)) {
            rc = fpmul_wave_table(ctx, ss, n, t, &fa.tab);
            if (rc != ShareSuccess) return rc;
            TruncprConsts tc;
            rc = truncpr_consts(ctx, k, m, true, &tc);
            if (rc != ShareSuccess) return rc;
            memcpy(fa.c0, tc.cs.c0, sizeof fa.c0), memcpy(fa.c1, tc.cs.c1, sizeof fa.c1), memcpy(fa.cinv, tc.ci.c0, sizeof fa.cinv);
            fa.ta = (const uint32_t*)a, fa.tb = (const uint32_t*)b, fa.tc = (const uint32_t*)c, fa.x = (const uint32_t*)x, fa.y = (const uint32_t*)y;
            fa.r_bits = (const uint32_t*)r_bits, fa.r_int = (const uint32_t*)r_int, fa.pow2 = tc.pow2;
            fa.de_out = (uint32_t*)de_out, fa.z = (uint32_t*)z_out, fa.r_dash = (uint32_t*)r_dash_out, fa.open_sh = (uint32_t*)open_sh_out;
            fa.out = (uint32_t*)d_out, fa.c_open = (uint32_t*)c_open_out, fa.status = status_out;
            for (size_t i = 0; i < S; ++i) fa.rows.set(i, (unsigned)ss.ids[i]);  // the per-party arrays are indexed by party id
            return enqueue_one_launch(ctx, s, &fa.counters, {{&fa.summary_first, summary_first_dev}, {&fa.summary, summary_dev}},
                                      [&] { launch_fpmul_wave(fa, ctx->device, s, false); });
        }
    }
    // sender_ids are party ids and de_sh_ws, open_sh_out are [party][..], so both opens read every sender's row in place at its id (the slots form)
    ShareErrorCode rc = open_beaver_pair(ctx, plan.pair_first, true, sender_ids, S, a, b, x, y, N, n, t, de_sh_ws, de_out, status_out, summary_first_dev, stream);
    if (rc != ShareSuccess) return rc;
    // finalize_mul (:57-100), r' (truncpr.rs:277-283), the share TruncPr opens (:294-297), its open (truncpr.rs:215), the last step (:216-220)
    rc = hbmpc_dev_fpmul_middle(ctx, c, x, y, de_out, de_out + N, r_bits, r_int, k, m, N, n, z_out, r_dash_out, open_sh_out, stream);
    if (rc != ShareSuccess) return rc;
    rc = batch_recover_dev(ctx, {.sender_ids = sender_ids, .S = S, .evals = open_sh_out, .G = N, .n = n, .d = t, .t = t, .out = c_open_out,
                                 .status = status_out, .summary = summary_dev, .p0 = true, .stream = stream, .slots = sender_ids});
    if (rc != ShareSuccess) return rc;
    return hbmpc_dev_truncpr_finalize_parties(ctx, z_out, r_dash_out, c_open_out, m, N, n, d_out, stream);
}

#include "capi_truncpr.inc"
#include "capi_mul.inc"
#include "capi_input.inc"
#include "capi_batchrecon.inc"
#include "capi_randbit.inc"
#include "capi_prandbit.inc"
#include "capi_riss_seeded.inc"
#include "capi_producers.inc"
#include "capi_shamir.inc"
