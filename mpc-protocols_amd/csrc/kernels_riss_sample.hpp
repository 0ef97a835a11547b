// kernels_riss_sample.hpp -- seeded dealing of the RISS contributions of PRandBit / PRandInt on the device.
// The reference draws every r_T from the node's rng (generate_riss, fpmul/prandbitd.rs:534-539; gen_big_uint_range :766-784); a
// device-resident dealer needs values that are a function of (seed, position) only, and the protocol only ever uses their sums over
// the n senders -- 1/n of the data.  Contract "hbmpc-riss-chacha20-v1" (the library's own, restated in tests/riss_seeded_model.py):
// the value of (seed, domain, set index T, element index i, lk_bits) is
//   for attempt = 0, 1, ...:
//       blk = chacha20_block(key = seed as eight LE words, state words 12..15 = (attempt, T | domain << 16, i mod 2^32, i div 2^32))
//       for c = 0 .. 7:  v = (blk[2c] | blk[2c+1] << 32) & (2^(lk_bits+1) - 1);  if v <= 2^lk_bits: return v
// -- the reference's range [0, 2^(l+k)], bound included (:518, :766-771), uniform by rejection; one block chain per value (a candidate
// is accepted with probability just over 1/2, so a second block is needed about once in 256 values).  T is the index in
// hbmpc_riss_tsets order (< 8192: 16 bits); domain 0 = PRandBit, 1 = PRandInt, so both may share a sender's seed.
//
// Both kernels are pure VALU (about 1 000 integer operations per block), a lane per (set, element) on the grid of k_riss_fold: T is
// the block's, so state word 13 and the key are wave-uniform.  The working state of a block is 16 VGPRs and nothing else is live
// across it but the index and the running sum, so the kernels stay far below the 64 VGPRs that admit 8 waves per SIMD; those waves,
// not an unrolled sender loop, cover the rotate / add chains (each quarter-round column is already four independent chains).
#pragma once
#include "kernels_rng.hpp"

namespace hbmpc {

// one value of the contract; tdom = T | domain << 16, mask = 2^(lk_bits+1) - 1, bound = 2^lk_bits
__device__ __forceinline__ uint64_t riss_draw(const SeedArg& key, uint32_t tdom, uint64_t i, uint64_t mask, uint64_t bound) {
    for (uint32_t attempt = 0;; ++attempt) {
        uint32_t blk[16];
        chacha20_block(key, ((uint64_t)tdom << 32) | attempt, i, blk);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint64_t v = (((uint64_t)blk[2 * c + 1] << 32) | blk[2 * c]) & mask;
            if (v <= bound) return v;
        }
    }
}

// ONE sender: out [Tn][B], row T what the sender sends to the parties outside T.  Grid: Tn * ceil(B / 256) blocks of 256.
__global__ __launch_bounds__(256) void k_riss_sample(SeedArg seed, uint32_t domain, size_t B, uint64_t first_index, uint64_t bound,
                                                     uint64_t* __restrict__ out) {
    const size_t nb = (B + 255) / 256;
    const size_t T = blockIdx.x / nb, b = (blockIdx.x % nb) * 256 + threadIdx.x;
    if (b >= B) return;
    out[T * B + b] = riss_draw(seed, (uint32_t)T | (domain << 16), first_index + b, 2 * bound - 1, bound);
}

// ALL n senders, folded in registers: seeds [n] (device memory) -> sums [Tn][B]; the contributions never exist.  The sender index is
// the loop counter, so a sender's eight key words are read through the scalar cache into SGPRs.  No LDS; one 8-byte store per lane,
// consecutive lanes to consecutive words.  Every drawn value is within the bound by construction: there is no verdict to write.
__global__ __launch_bounds__(256) void k_riss_sample_fold(const SeedArg* __restrict__ seeds, unsigned n, uint32_t domain, size_t B,
                                                          uint64_t first_index, uint64_t bound, uint64_t* __restrict__ sums) {
    const size_t nb = (B + 255) / 256;
    const size_t T = blockIdx.x / nb, b = (blockIdx.x % nb) * 256 + threadIdx.x;
    if (b >= B) return;
    const uint32_t tdom = (uint32_t)T | (domain << 16);
    const uint64_t i = first_index + b, mask = 2 * bound - 1;
    uint64_t sum = 0;
#pragma unroll 1
    for (unsigned s = 0; s < n; ++s) {
        const SeedArg key = seeds[s];
        sum += riss_draw(key, tdom, i, mask, bound);
    }
    sums[T * B + b] = sum;
}

}  // namespace hbmpc
