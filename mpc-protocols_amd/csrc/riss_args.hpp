// riss_args.hpp -- the table that the kernels of kernels_riss.hpp take by value, and the bound the host checks shapes against
#pragma once
#include <stdint.h>

namespace hbmpc {

constexpr unsigned RISS_MAX_TSETS = 8192;  // C(n, t) of a supported shape (the accumulator bound above rests on it)

// one (context, n, t[, own party]) coefficient table (tables_riss.hpp lays it out; every pointer is inside one cached table)
struct RissTab {
    const uint32_t* coef;   // [Tn][ncols][NC]: f_T(alpha_col) as a canonical integer, NC = 8 words (Fr) or 2 (Goldilocks); zero when col is in T
    const uint32_t* coef2;  // [Tn][ncols]: f2_T(3^col) in GF(2^8), a word each (scalar loads); NULL when n > 255
    const uint32_t* red;    // Fr: 1 and 2^224 in device-constant form, [2][NL]
    unsigned ncols;
};

}  // namespace hbmpc
