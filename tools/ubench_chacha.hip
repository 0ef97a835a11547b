// The ceiling tools/bench_riss_seeded.py reports k_riss_sample_fold against: ChaCha20 blocks per second with nothing else to do.
// Every lane runs `iters` blocks of csrc/kernels_rng.hpp's chacha20_block back to back -- the key in SGPRs, the position from the lane
// index, no memory traffic inside the loop -- and one word per lane is stored at the end so that the blocks are not dead code.  The grid
// fills every CU with 8 waves per SIMD, the occupancy of the sampling kernels.
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 -I mpc-protocols_amd/csrc tools/ubench_chacha.hip -o tools/ubench_chacha
//     tools/ubench_chacha [iters per lane = 64] [samples = 15]      -> one JSON line
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "kernels_rng.hpp"

using namespace hbmpc;

__global__ __launch_bounds__(256) void k_chacha_loop(SeedArg key, uint32_t iters, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t acc = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < iters; ++k) {
        uint32_t blk[16];
        chacha20_block(key, k, i, blk);
#pragma unroll
        for (int w = 0; w < 16; ++w) acc ^= blk[w];  // every word of the block is used, as the sampler reads all eight candidates
    }
    out[i] = acc;
}

#define CK(call)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                    \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

int main(int argc, char** argv) {
    const uint32_t iters = argc > 1 ? (uint32_t)atoi(argv[1]) : 64;
    const int samples = argc > 2 ? atoi(argv[2]) : 15;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const unsigned blocks = (unsigned)prop.multiProcessorCount * 8 * 16;  // 8 blocks of 4 waves per CU resident, 16 rounds of them
    uint32_t* out = nullptr;
    CK(hipMalloc(&out, (size_t)blocks * 256 * 4));
    SeedArg key;
    for (int w = 0; w < 8; ++w) key.k[w] = 0x03020100u + 0x04040404u * w;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int w = 0; w < 3; ++w) hipLaunchKernelGGL(k_chacha_loop, dim3(blocks), dim3(256), 0, 0, key, iters, out);
    CK(hipDeviceSynchronize());
    std::vector<float> ms(samples);
    for (int s = 0; s < samples; ++s) {
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k_chacha_loop, dim3(blocks), dim3(256), 0, 0, key, iters, out);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms[s], e0, e1));
    }
    CK(hipGetLastError());
    std::sort(ms.begin(), ms.end());
    const double n_blocks = (double)blocks * 256 * iters;
    printf("{\"chacha_blocks\": %.0f, \"ms_median\": %.4f, \"ms_p10\": %.4f, \"ms_p90\": %.4f, \"blocks_per_s\": %.4e, \"cus\": %d}\n", n_blocks,
           ms[samples / 2], ms[samples / 10], ms[samples - 1 - samples / 10], n_blocks / (ms[samples / 2] * 1e-3), prop.multiProcessorCount);
    CK(hipFree(out));
    return 0;
}
