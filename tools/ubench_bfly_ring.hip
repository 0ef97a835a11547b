// ubench_bfly_ring.hip -- the ring form of the headline encode (tools/kernels_mfma_bfly_ring_lab.hpp: a loader wave per workgroup
// fills an LDS ring with whole lines, the other waves compute) against the production k_mfma_bfly<6,12,8> on config 2's shape
// (n = 16, t = 5): byte comparison of the whole output at several G, then ms per launch of every (CW, S, D, loader form), with
// and without the arithmetic, all in one process and in alternating passes.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench_bfly_ring.hip -o tools/ubench_bfly_ring
//   tools/ubench_bfly_ring [log2_chunks=20] [reps=20] [passes=3]
//   tools/ubench_bfly_ring edges [reps=20] [passes=3]
// "edges": the fixed cost of a launch (profiles/encode_launch_edges.txt).  The 12-wave, 4-deep ring with the start it had (table,
// barrier, first request) and with the library's start (first requests before the barrier), the library's own k_mfma_bfly_ring, and
// the 2 x 4 cache policies of the loader's reads and the row stores: outputs against the gathering kernel at the sizes around D and
// S items per workgroup, ms per launch at 2^15 .. 2^21 chunks (policies: 2^20 and 2^21), the fixed cost T(2^20) - [T(2^21) - T(2^20)],
// and one stamped launch per start: where a workgroup's time goes before its first store and how far apart the workgroups end.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "kernels_mfma_bfly_lab.hpp"
#include "kernels_mfma_bfly_ring_lab.hpp"
#include "../mpc-protocols_amd/csrc/tables.hpp"
#include "../mpc-protocols_amd/csrc/tables_mfma.hpp"

using namespace hbmpc;
#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e = (x);                                                        \
        if (e != hipSuccess) {                                                     \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e)); \
            exit(2);                                                               \
        }                                                                          \
    } while (0)

static std::mt19937_64 rng(0xB0F2);
static void rand_canon(uint64_t c[4]) {
    for (;;) {
        for (int i = 0; i < 4; ++i) c[i] = rng();
        c[3] &= 0x7fffffffffffffffULL;
        if (!HFr::geq(c)) return;
    }
}
template <class F>
static float time_ms(F f, int reps) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) f();
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < reps; ++i) f();
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    return ms / reps;
}

constexpr int M = 6, NP = 8, N = 16;
constexpr int ROWB = M * 1024 + 256;

template <int ABL>
static void launch_prod(mf::MfmaRowsArgs a, int nwg) {
    if (!mf::mf_plan_pairs(NP, (160 * 1024) / ROWB, nwg, &a)) exit(3);
    static bool attr = false;
    if (!attr) { CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&mf::k_mfma_bfly_lab<M, 12, NP, ABL>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr = true; }
    hipLaunchKernelGGL((mf::k_mfma_bfly_lab<M, 12, NP, ABL>), dim3((unsigned)mf::mf_grid(a)), dim3(64 * 12), (size_t)NP * ROWB, 0, a);
}
template <int CW, int S, int D, bool DMA, int ABL>
static void launch_ring(mf::MfmaRowsArgs a, int nwg) {
    if (!mf::mf_plan_pairs(NP, (160 * 1024) / ROWB, nwg, &a)) exit(3);
    if (a.nroles != 1 || a.role[0].nrows != NP) exit(4);
    static bool attr = false;
    if (!attr) { CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&mf::k_mfma_bfly_ring_lab<M, CW, NP, S, D, DMA, ABL>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr = true; }
    hipLaunchKernelGGL((mf::k_mfma_bfly_ring_lab<M, CW, NP, S, D, DMA, ABL>), dim3((unsigned)mf::mf_grid(a)), dim3(64 * (CW + 1)), mf::bfly_ring_lds_bytes(M, NP, S), 0, a);
}

struct Variant {
    const char* name;
    void (*full)(mf::MfmaRowsArgs, int);
    void (*traffic)(mf::MfmaRowsArgs, int);  // neither MFMAs nor epilogue arithmetic nor table reads: loads, the LDS trip and stores
};
#define RING(CW, S, D, DMA) {"ring CW=" #CW " S=" #S " D=" #D " " #DMA, &launch_ring<CW, S, D, DMA, 0>, &launch_ring<CW, S, D, DMA, 7>}
#define dma true
#define reg false
static const Variant variants[] = {
    {"production k_mfma_bfly<6,12,8> (gathers)", &launch_prod<0>, &launch_prod<7>},
    RING(8, 16, 2, dma),  RING(8, 16, 4, dma),  RING(8, 16, 2, reg),  RING(8, 16, 4, reg),
    RING(9, 18, 4, dma),  RING(9, 18, 4, reg),
    RING(11, 11, 2, dma), RING(11, 11, 4, dma), RING(11, 11, 2, reg), RING(11, 11, 4, reg),
    RING(12, 12, 2, dma), RING(12, 12, 4, dma), RING(12, 12, 8, dma), RING(12, 12, 11, dma), RING(12, 12, 2, reg), RING(12, 12, 4, reg),
    RING(15, 15, 2, dma), RING(15, 15, 4, dma), RING(15, 15, 2, reg), RING(15, 15, 4, reg),
};
#undef dma
#undef reg
constexpr int NV = sizeof(variants) / sizeof(variants[0]);

// ---- edges
constexpr int ECW = 12, ES = 12, ED = 4;  // BFLY_RING_LIB
template <int START, int LP, int SP, int ABL, bool STAMP = false>
static void launch_edge(mf::MfmaRowsArgs a, int nwg) {
    if (!mf::mf_plan_pairs(NP, (160 * 1024) / ROWB, nwg, &a)) exit(3);
    if (a.nroles != 1 || a.role[0].nrows != NP) exit(4);
    auto k = &mf::k_mfma_bfly_ring_lab<M, ECW, NP, ES, ED, true, ABL, START, LP, SP, STAMP>;
    static bool attr = false;
    if (!attr) { CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr = true; }
    hipLaunchKernelGGL(k, dim3((unsigned)mf::mf_grid(a)), dim3(64 * (ECW + 1)), mf::bfly_ring_lds_bytes(M, NP, ES), 0, a);
}
static void launch_library(mf::MfmaRowsArgs a, int nwg) {
    if (!mf::mf_plan_pairs(NP, (160 * 1024) / ROWB, nwg, &a)) exit(3);
    if (a.nroles != 1 || a.role[0].nrows != NP) exit(4);
    auto k = &mf::k_mfma_bfly_ring<M, ECW, NP, ES, ED>;
    static bool attr = false;
    if (!attr) { CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr = true; }
    hipLaunchKernelGGL(k, dim3((unsigned)mf::mf_grid(a)), dim3(64 * (ECW + 1)), mf::bfly_ring_lds_bytes(M, NP, ES), 0, a);
}
#define EDGE(START, LP, SP) {"ring 12/12/4 start=" #START " loads=" #LP " stores=" #SP, &launch_edge<START, mf::RP_##LP, mf::RP_##SP, 0>, &launch_edge<START, mf::RP_##LP, mf::RP_##SP, 7>}
static const Variant edge_variants[] = {
    {"k_mfma_bfly<6,12,8> (gathers)", &launch_prod<0>, &launch_prod<7>},
    {"library k_mfma_bfly_ring<6,12,8,12,4>", &launch_library, nullptr},
    EDGE(0, DEFAULT, DEFAULT),
    EDGE(1, DEFAULT, DEFAULT), EDGE(1, DEFAULT, NT), EDGE(1, DEFAULT, SC1), EDGE(1, DEFAULT, SC0_SC1),
    EDGE(1, NT, DEFAULT),      EDGE(1, NT, NT),      EDGE(1, NT, SC1),      EDGE(1, NT, SC0_SC1),
};
constexpr int NE = sizeof(edge_variants) / sizeof(edge_variants[0]), NE_STARTS = 4;  // the first NE_STARTS: timed at every size

__global__ void k_count_diff(const uint4* x, const uint4* y, size_t n, unsigned* count) {
    unsigned mine = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 p = x[i], q = y[i];
        mine += p.x != q.x || p.y != q.y || p.z != q.z || p.w != q.w;
    }
    if (mine) atomicAdd(count, mine);
}

static void print_stamps(const char* name, const std::vector<unsigned long long>& st, int wgs) {
    struct Iv { const char* what; int from, to; };
    const Iv ivs[] = {{"entry -> table in LDS", mf::RING_STAMP_ENTRY, mf::RING_STAMP_TABLE},
                      {"entry -> first DMA issued", mf::RING_STAMP_ENTRY, mf::RING_STAMP_FIRST_DMA},
                      {"first DMA issued -> first slot published", mf::RING_STAMP_FIRST_DMA, mf::RING_STAMP_FIRST_PUBLISHED},
                      {"entry -> first slot published", mf::RING_STAMP_ENTRY, mf::RING_STAMP_FIRST_PUBLISHED},
                      {"first slot published -> first row store issued", mf::RING_STAMP_FIRST_PUBLISHED, mf::RING_STAMP_FIRST_STORE},
                      {"entry -> first row store issued", mf::RING_STAMP_ENTRY, mf::RING_STAMP_FIRST_STORE},
                      {"first -> last row store issued", mf::RING_STAMP_FIRST_STORE, mf::RING_STAMP_LAST_STORE}};
    auto at = [&](int w, int k) { return st[(size_t)w * mf::RING_STAMPS + k]; };
    unsigned long long e0 = ~0ull, e1 = 0, l0 = ~0ull, l1 = 0;
    int have = 0;
    for (int w = 0; w < wgs; ++w) {
        if (!at(w, mf::RING_STAMP_LAST_STORE)) continue;  // a workgroup without items
        ++have;
        e0 = std::min(e0, at(w, mf::RING_STAMP_ENTRY)), e1 = std::max(e1, at(w, mf::RING_STAMP_ENTRY));
        l0 = std::min(l0, at(w, mf::RING_STAMP_LAST_STORE)), l1 = std::max(l1, at(w, mf::RING_STAMP_LAST_STORE));
    }
    printf("%s: %d workgroups with items; microseconds (100 MHz clock), min / median / max over the workgroups\n", name, have);
    if (!have) return;
    for (const Iv& iv : ivs) {
        std::vector<double> d;
        for (int w = 0; w < wgs; ++w)
            if (at(w, mf::RING_STAMP_LAST_STORE)) d.push_back(((double)at(w, iv.to) - (double)at(w, iv.from)) * 0.01);
        std::sort(d.begin(), d.end());
        printf("  %-48s %8.2f %8.2f %8.2f\n", iv.what, d.front(), d[d.size() / 2], d.back());
    }
    printf("  %-48s %8.2f\n", "first entry -> last entry (the launch's skew)", (double)(e1 - e0) * 0.01);
    printf("  %-48s %8.2f\n", "first -> last of the last stores (the tail)", (double)(l1 - l0) * 0.01);
    printf("  %-48s %8.2f\n", "first entry -> last of the last stores", (double)(l1 - e0) * 0.01);
}

static int edges_main(int reps, int passes) {
    const int LG0 = 15, LG1 = 21;
    const size_t G = (size_t)1 << LG1;
    const size_t half = domain_size(N) / 2;
    std::vector<HFr> el = domain_elements<HFr>(N, N);
    std::vector<std::vector<HFr>> V(N, std::vector<HFr>(M));
    for (int j = 0; j < N; ++j) {
        HFr p = HFr::one();
        for (int k = 0; k < M; ++k) V[j][k] = p, p = p * el[j];
    }
    const auto tb = build_mfma_bfly_table(V, M, half);
    uint8_t *d_tb, *d_x, *d_y0, *d_y1;
    unsigned* d_count;
    const size_t out_bytes = (size_t)N * G * 32;
    CK(hipMalloc(&d_tb, tb.size() * 4));
    CK(hipMemcpy(d_tb, tb.data(), tb.size() * 4, hipMemcpyHostToDevice));
    {
        std::vector<uint64_t> x(G * M * 4);
        for (size_t i = 0; i < G * M; ++i) rand_canon(&x[4 * i]);
        CK(hipMalloc(&d_x, G * M * 32));
        CK(hipMemcpy(d_x, x.data(), G * M * 32, hipMemcpyHostToDevice));
    }
    CK(hipMalloc(&d_y0, out_bytes));
    CK(hipMalloc(&d_y1, out_bytes));
    CK(hipMalloc(&d_count, 4));
    auto args = [&](size_t g, uint8_t* out) {
        mf::MfmaRowsArgs a = {};
        a.in = d_x, a.G = g, a.in_chunk_major = 1, a.nv = 0, a.out_party_major = 1, a.out_stride = g, a.out = out;
        a.table = d_tb, a.half = (int)half, a.nout = N;
        return a;
    };
    // outputs and the 4 KiB behind them, against the gathering kernel: G around one tile, around D and S items in the first of 8
    // workgroups (tiles up to 12 are all its own, tile 96 is its 13th), several rounds, and the timed sizes
    struct Case { size_t g; int nwg; };
    const Case cases[] = {{1, 8},   {31, 8},  {32, 8},        {33, 8},    {95, 8},      {97, 8},                {129, 8}, {383, 8},
                          {385, 8}, {543, 8}, {32 * 96 + 1, 8}, {40017, 8}, {16613, 256}, {(size_t)1 << 20, 256}, {G, 256}};
    int bad = 0;
    for (const Case& cs : cases) {
        const size_t bytes = (size_t)N * cs.g * 32, span = std::min(bytes + 4096, out_bytes);
        CK(hipMemset(d_y0, 0xee, span));
        edge_variants[0].full(args(cs.g, d_y0), cs.nwg);
        CK(hipDeviceSynchronize());
        for (int v = 1; v < NE; ++v) {
            CK(hipMemset(d_y1, 0xee, span));
            CK(hipMemset(d_count, 0, 4));
            edge_variants[v].full(args(cs.g, d_y1), cs.nwg);
            CK(hipDeviceSynchronize());  // a fault ends the program here (CK exits)
            k_count_diff<<<1024, 256>>>((const uint4*)d_y0, (const uint4*)d_y1, span / 16, d_count);
            unsigned diff = 0;
            CK(hipMemcpy(&diff, d_count, 4, hipMemcpyDeviceToHost));
            if (diff) printf("G=%zu wgs=%d %s: DIFFERS in %u pieces\n", cs.g, cs.nwg, edge_variants[v].name, diff), ++bad;
        }
        std::vector<uint8_t> guard(span - bytes);
        if (!guard.empty()) CK(hipMemcpy(guard.data(), d_y0 + bytes, guard.size(), hipMemcpyDeviceToHost));
        for (uint8_t b : guard) bad += b != 0xee;
        printf("G=%zu, %d workgroups: %d ring variants compared with the gathering kernel\n", cs.g, cs.nwg, NE - 1);
        fflush(stdout);
    }
    if (bad) {
        printf("FAILED: %d differences; no timing\n", bad);
        return 1;
    }
    // ms per launch: every size for the starts, the two largest for the policies; alternating passes, each figure `reps` launches
    const int NL = LG1 - LG0 + 1;
    std::vector<float> tf((size_t)NE * NL * passes, 0.f), tt((size_t)NE * NL * passes, 0.f);
    auto at = [&](std::vector<float>& t, int v, int lg, int p) -> float& { return t[((size_t)v * NL + (lg - LG0)) * passes + p]; };
    for (int p = 0; p < passes; ++p)
        for (int lg = LG0; lg <= LG1; ++lg)
            for (int v = 0; v < NE; ++v) {
                if (v >= NE_STARTS && lg < 20) continue;
                const mf::MfmaRowsArgs a = args((size_t)1 << lg, d_y1);
                at(tf, v, lg, p) = time_ms([&] { edge_variants[v].full(a, 256); }, reps);
                if (edge_variants[v].traffic) at(tt, v, lg, p) = time_ms([&] { edge_variants[v].traffic(a, 256); }, reps);
            }
    printf("timing: 256 workgroups, %d launches per figure, %d alternating passes; microseconds per launch, full / traffic only\n", reps, passes);
    for (int lg = LG0; lg <= LG1; ++lg) {
        printf("G=2^%d (%.1f MB)\n", lg, (double)((size_t)1 << lg) * (M + N) * 32 / 1e6);
        for (int v = 0; v < NE; ++v) {
            if (v >= NE_STARTS && lg < 20) continue;
            printf("  %-52s", edge_variants[v].name);
            for (int p = 0; p < passes; ++p) printf("  %7.2f /%7.2f", at(tf, v, lg, p) * 1e3, at(tt, v, lg, p) * 1e3);
            printf("\n");
        }
    }
    printf("fixed cost of a launch, T(2^20) - [T(2^21) - T(2^20)], microseconds, full / traffic only, per pass\n");
    for (int v = 0; v < NE; ++v) {
        printf("  %-52s", edge_variants[v].name);
        for (int p = 0; p < passes; ++p)
            printf("  %7.2f /%7.2f", (2 * at(tf, v, 20, p) - at(tf, v, 21, p)) * 1e3, (2 * at(tt, v, 20, p) - at(tt, v, 21, p)) * 1e3);
        printf("\n");
    }
    // one stamped launch per start behind three plain ones, twice, at 2^20
    {
        const mf::MfmaRowsArgs a = args((size_t)1 << 20, d_y1);
        std::vector<unsigned long long> st((size_t)mf::RING_STAMP_MAX_WGS * mf::RING_STAMPS);
        for (int rep = 0; rep < 2; ++rep)
            for (int start = 0; start < 2; ++start) {
                std::fill(st.begin(), st.end(), 0ull);
                CK(hipMemcpyToSymbol(HIP_SYMBOL(mf::ring_lab_stamps), st.data(), st.size() * 8));
                for (int i = 0; i < 3; ++i) edge_variants[2 + start].full(a, 256);
                if (start) launch_edge<1, mf::RP_DEFAULT, mf::RP_DEFAULT, 0, true>(a, 256);
                else launch_edge<0, mf::RP_DEFAULT, mf::RP_DEFAULT, 0, true>(a, 256);
                CK(hipDeviceSynchronize());
                CK(hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(mf::ring_lab_stamps), st.size() * 8));
                print_stamps(start ? "stamped, G=2^20, start=1 (requests before the barrier)" : "stamped, G=2^20, start=0 (table, barrier, first request)", st, 256);
            }
    }
    CK(hipFree(d_tb)); CK(hipFree(d_x)); CK(hipFree(d_y0)); CK(hipFree(d_y1)); CK(hipFree(d_count));
    printf("all outputs identical\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "edges")) return edges_main(argc > 2 ? atoi(argv[2]) : 20, argc > 3 ? atoi(argv[3]) : 3);
    const int lg = argc > 1 ? atoi(argv[1]) : 20, reps = argc > 2 ? atoi(argv[2]) : 20, passes = argc > 3 ? atoi(argv[3]) : 3;
    const size_t G = (size_t)1 << lg;
    const size_t half = domain_size(N) / 2;
    std::vector<HFr> el = domain_elements<HFr>(N, N);
    std::vector<std::vector<HFr>> V(N, std::vector<HFr>(M));
    for (int j = 0; j < N; ++j) {
        HFr p = HFr::one();
        for (int k = 0; k < M; ++k) V[j][k] = p, p = p * el[j];
    }
    const auto tb = build_mfma_bfly_table(V, M, half);
    uint8_t *d_tb, *d_x, *d_y0, *d_y1;
    CK(hipMalloc(&d_tb, tb.size() * 4));
    CK(hipMemcpy(d_tb, tb.data(), tb.size() * 4, hipMemcpyHostToDevice));
    std::vector<uint64_t> x(G * M * 4);
    for (size_t i = 0; i < G * M; ++i) rand_canon(&x[4 * i]);
    CK(hipMalloc(&d_x, G * M * 32));
    CK(hipMalloc(&d_y0, (size_t)N * G * 32));
    CK(hipMalloc(&d_y1, (size_t)N * G * 32));
    CK(hipMemcpy(d_x, x.data(), G * M * 32, hipMemcpyHostToDevice));
    std::vector<uint8_t> y0((size_t)N * G * 32), y1((size_t)N * G * 32);

    // every variant against the production kernel, byte for byte, rows guarded by a fill the kernels must leave alone
    struct Case { size_t g; int nwg; };
    const Case cases[] = {{1, 8}, {33, 8}, {32 * 17 - 1, 8}, {40017, 8}, {16613, 256}, {G, 256}};
    int bad = 0;
    for (const Case& cs : cases) {
        if (cs.g > G) continue;
        mf::MfmaRowsArgs a = {};
        a.in = d_x, a.G = cs.g, a.in_chunk_major = 1, a.nv = 0, a.out_party_major = 1, a.out_stride = cs.g;
        a.table = d_tb, a.half = (int)half, a.nout = N;
        const size_t bytes = (size_t)N * cs.g * 32;
        a.out = d_y0;
        CK(hipMemset(d_y0, 0xee, bytes + (cs.g < G ? 64 : 0)));
        variants[0].full(a, cs.nwg);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(y0.data(), d_y0, bytes, hipMemcpyDeviceToHost));
        for (int v = 1; v < NV; ++v) {
            a.out = d_y1;
            const size_t span = bytes + 4096 < (size_t)N * G * 32 ? bytes + 4096 : (size_t)N * G * 32;
            CK(hipMemset(d_y1, 0xee, span));
            variants[v].full(a, cs.nwg);
            CK(hipDeviceSynchronize());  // a fault ends the program here (CK exits)
            CK(hipMemcpy(y1.data(), d_y1, span, hipMemcpyDeviceToHost));
            size_t diff = memcmp(y0.data(), y1.data(), bytes) != 0;
            for (size_t i = bytes; i < span && !diff; ++i) diff = y1[i] != 0xee;
            if (diff) printf("G=%zu wgs=%d %s: DIFFERS\n", cs.g, cs.nwg, variants[v].name), ++bad;
        }
        printf("G=%zu, %d workgroups: %d ring variants compared with the production kernel\n", cs.g, cs.nwg, NV - 1);
        fflush(stdout);
    }
    if (bad) {
        printf("FAILED: %d differences; no timing\n", bad);
        return 1;
    }
    mf::MfmaRowsArgs a = {};
    a.in = d_x, a.G = G, a.in_chunk_major = 1, a.nv = 0, a.out_party_major = 1, a.out_stride = G, a.out = d_y1;
    a.table = d_tb, a.half = (int)half, a.nout = N;
    const double bytes = (double)G * (M + N) * 32;
    printf("timing: G=%zu, %d launches per figure, %d alternating passes; algorithmic bytes %.1f MB (at 8 TB/s %.4f ms)\n", G, reps, passes, bytes / 1e6, bytes / 8e12 * 1e3);
    printf("%-44s", "variant");
    for (int p = 0; p < passes; ++p) printf("  full_ms traffic_ms");
    printf("\n");
    std::vector<float> tf((size_t)NV * passes), tt((size_t)NV * passes);
    for (int p = 0; p < passes; ++p)
        for (int v = 0; v < NV; ++v) {
            tf[(size_t)v * passes + p] = time_ms([&] { variants[v].full(a, 256); }, reps);
            tt[(size_t)v * passes + p] = time_ms([&] { variants[v].traffic(a, 256); }, reps);
        }
    for (int v = 0; v < NV; ++v) {
        printf("%-44s", variants[v].name);
        for (int p = 0; p < passes; ++p) printf("  %7.4f %10.4f", tf[(size_t)v * passes + p], tt[(size_t)v * passes + p]);
        printf("\n");
    }
    CK(hipFree(d_tb)); CK(hipFree(d_x)); CK(hipFree(d_y0)); CK(hipFree(d_y1));
    printf("all outputs identical\n");
    return 0;
}
