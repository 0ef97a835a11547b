// sqrt_args.hpp -- what the kernels of kernels_sqrt.hpp take by value or write for the host
#pragma once
#include <stdint.h>

namespace hbmpc {

// one context's constants (tables_sqrt.hpp lays them out; every pointer is inside one table)
struct SqrtTab {
    const uint32_t* negw;   // [3][256][NL]: omega^(-j 2^(8m)), device-constant form
    const uint32_t* posw;   // [4][256][NL]: omega^(j 2^(8m))
    const uint32_t* r2;     // [NL] R^2 (canonical data -> Montgomery form)
    const uint32_t* one_p;  // [NL] 1 in plain limb form (Montgomery form -> canonical data)
    const uint32_t* half;   // [NL] 2^-1, device-constant form
    const uint32_t* half_p; // [NL] 2^-1 in plain limb form
    const uint32_t* e_sqrt; // (T-1)/2, 8 words, least significant first
    const uint32_t* e_inv;  // p - 2
    const uint8_t* keyt;    // [1 << kbits]: key of omega^(j 2^24) -> j
    int bits_sqrt, bits_inv;
    uint32_t kshift, kmask;
};

// RandBit's verdict (include/hbmpc_hip.h hbmpc_randbit_summary): the 64-bit minimum of (status << 32) | index -- a zero square
// (status 1) ranks before a missing root (status 2), as ZeroSquare is checked over the whole batch first -- and the count
struct RandBitSummaryDev {
    unsigned long long first;
    uint32_t n_failed;
    uint32_t reserved;
};
constexpr uint64_t SQRT_KEY_MUL = 0x9E3779B97F4A7C15ull;  // the look-up key's multiplicative hash (sqrt_key; the host proves its slice collision-free)

}  // namespace hbmpc
