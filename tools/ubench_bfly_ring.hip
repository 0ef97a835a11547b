// ubench_bfly_ring.hip -- the ring form of the headline encode (tools/kernels_mfma_bfly_ring_lab.hpp: a loader wave per workgroup
// fills an LDS ring with whole lines, the other waves compute) against the production k_mfma_bfly<6,12,8> on config 2's shape
// (n = 16, t = 5): byte comparison of the whole output at several G, then ms per launch of every (CW, S, D, loader form), with
// and without the arithmetic, all in one process and in alternating passes.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench_bfly_ring.hip -o tools/ubench_bfly_ring
//   tools/ubench_bfly_ring [log2_chunks=20] [reps=20] [passes=3]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

int main(int argc, char** argv) {
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
