// kernels_shamir.hpp -- the small-weight encode of the integer-point Shamir scheme (common/share/shamir.rs:44-88 for B secrets at once).
//
// shares[i][b] = sum_k coeffs[b][k] points[i]^k.  At integer points the weights points[i]^k are plain integers below 2^64 (the route
// planner, shamir_route.hpp, sends every other call to the Horner kernels), so an output is d + 1 products of a canonical element by
// one or two 32-bit words, summed in a wide accumulator and reduced once (shamir_arith.hpp) -- canonical words in and out, no
// Montgomery form.
//
// A lane owns a secret.  The 64 coefficient rows of a wave are contiguous in memory: the wave copies them to LDS with 16-byte
// loads (a lane's own row is (d + 1) elements apart from its neighbour's: read directly, a wave's load would touch 64 lines), then
// every lane walks its row once per point from LDS, a row padded so that the 64 lanes' reads fall on different banks.  The weights
// are the same for every lane: w[i][k] is read through a uniform address (scalar loads, held in SGPRs).  A point's 64 outputs of a
// wave are contiguous: 2 KiB over Fr, written as two 16-byte stores per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "shamir_arith.hpp"

namespace hbmpc {

// coeffs [B][d + 1] elements of NL / 2 units of 8 bytes; w [m][d + 1] weights; out [m][B] (it may not overlap coeffs); row_units: a
// row in LDS in 8-byte units (shamir_row_units); aligned16: coeffs is 16-byte aligned (Goldilocks rows at an odd 8-byte offset
// take 8-byte loads)
template <int NL, bool W32>
__global__ __launch_bounds__(256) void k_shamir_encode(const uint64_t* __restrict__ coeffs, size_t B, int m, int dp1,
                                                       const uint64_t* __restrict__ w, uint64_t* __restrict__ out, int row_units,
                                                       int aligned16) {
    constexpr int EU = NL / 2;  // 8-byte units of an element
    extern __shared__ __attribute__((aligned(16))) uint64_t shamir_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const size_t base = ((size_t)blockIdx.x * waves + wave) * 64;  // the wave's first secret
    uint64_t* rows = shamir_lds + (size_t)wave * 64 * row_units;
    const size_t ru = (size_t)dp1 * EU;                                    // units of a row in memory
    const size_t nrows = base < B ? (B - base < 64 ? B - base : 64) : 0;
    const size_t units = nrows * ru;                                          // units of the wave's rows
    const uint64_t* src = coeffs + base * ru;
    // stage: unit u of the wave's block belongs to row u / ru, offset u % ru
    const uint32_t ru32 = (uint32_t)ru, units32 = (uint32_t)units, su32 = (uint32_t)row_units;  // at most 64 rows of at most 128 units
    if (aligned16) {  // two units (16 bytes) per lane and step; a last odd unit (Goldilocks, odd d + 1, a short last wave) by itself
        const uint32_t pairs = units32 >> 1;
        for (uint32_t q = (uint32_t)lane; q < pairs; q += 64) {
            const uint32_t u = q * 2;
            const uint4 v = *reinterpret_cast<const uint4*>(src + u);
            uint32_t r = u / ru32, c = u - r * ru32;
            if constexpr (NL == 8) {  // both units in one row, at a 16-byte boundary of it
                *reinterpret_cast<uint4*>(rows + r * su32 + c) = v;
            } else {
                rows[r * su32 + c] = (uint64_t)v.x | ((uint64_t)v.y << 32);
                if (++c == ru32) c = 0, ++r;
                rows[r * su32 + c] = (uint64_t)v.z | ((uint64_t)v.w << 32);
            }
        }
        if ((units32 & 1) && lane == 0) {
            const uint32_t u = units32 - 1, r = u / ru32;
            rows[r * su32 + (u - r * ru32)] = src[u];
        }
    } else {
        for (uint32_t u = (uint32_t)lane; u < units32; u += 64) {
            const uint32_t r = u / ru32;
            rows[r * su32 + (u - r * ru32)] = src[u];
        }
    }
    __syncthreads();
    if ((size_t)lane >= nrows) return;
    const uint64_t* row = rows + (size_t)lane * row_units;
    const size_t b = base + lane;
    for (int i = 0; i < m; ++i) {
        const uint64_t* wi = w + (size_t)i * dp1;  // uniform: scalar loads
        shamir::Acc<NL> acc;
        shamir::acc_zero<NL>(acc);
        for (int k = 0; k < dp1; ++k) {
            uint32_t c[NL];
            if constexpr (NL == 8) {
                const uint4 lo = *reinterpret_cast<const uint4*>(row + (size_t)k * 4);
                const uint4 hi = *reinterpret_cast<const uint4*>(row + (size_t)k * 4 + 2);
                c[0] = lo.x, c[1] = lo.y, c[2] = lo.z, c[3] = lo.w, c[4] = hi.x, c[5] = hi.y, c[6] = hi.z, c[7] = hi.w;
            } else {
                const uint64_t v = row[k];
                c[0] = (uint32_t)v, c[1] = (uint32_t)(v >> 32);
            }
            shamir::acc_mac<NL, W32>(acc, c, wi[k]);
        }
        uint32_t y[NL];
        shamir::acc_reduce<NL>(acc, y);
        uint64_t* dst = out + ((size_t)i * B + b) * EU;
        if constexpr (NL == 8) {
            // out rows are 32 B elements: 16-byte aligned whenever the caller's buffer is (8-byte stores otherwise)
            if ((reinterpret_cast<uintptr_t>(out) & 15) == 0) {
                reinterpret_cast<uint4*>(dst)[0] = make_uint4(y[0], y[1], y[2], y[3]);
                reinterpret_cast<uint4*>(dst)[1] = make_uint4(y[4], y[5], y[6], y[7]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) dst[j] = (uint64_t)y[2 * j] | ((uint64_t)y[2 * j + 1] << 32);
            }
        } else {
            dst[0] = (uint64_t)y[0] | ((uint64_t)y[1] << 32);
        }
    }
}

}  // namespace hbmpc
