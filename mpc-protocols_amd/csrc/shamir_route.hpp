// shamir_route.hpp -- which kernel an integer-point Shamir encode (hbmpc_[gl_]dev_shamir_compute_shares) takes: ONE place for
// the rule (plain C++, no HIP).  The route is a pure function of (field, m, d, B, points) and of the forced route
// (hbmpc_set_shamir_route, a test and sweep aid).
//
//   SmallWeight   k_shamir_encode (kernels_shamir.hpp): the weights points[i]^k as plain integers below 2^64, canonical words,
//                 one reduction per output (shamir_arith.hpp).  Taken when every points[i]^d < 2^64 as an INTEGER (the ids are not
//                 reduced first: over Goldilocks an id >= p has d <= 1 here), the accumulator's bound holds and the wave's rows fit
//                 its share of 64 KB of LDS.
//   Wide          k_eval_wide: a wave per secret, a lane per point, Horner with the points in device-constant form as alpha.
//   Generic       k_eval_generic: a lane per secret, the same Horner walk.
// All three are bit-exact.  Small batches go to the wave-per-secret kernel under the rule of the domain encode
// (encode_route.hpp: up to wide_max_chunks / 4 secrets): there a lane per secret leaves the chip empty, and a lane of the
// small-weight kernel walks all m outputs of its secret one after the other.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hbmpc {

enum class ShamirKernel { SmallWeight = 1, Wide = 2, Generic = 3 };
enum { SHAMIR_ROUTE_AUTO = 0, SHAMIR_ROUTE_SMALL_WEIGHT = 1, SHAMIR_ROUTE_GENERIC = 2 };

// shamir_arith.hpp's bound asks for d + 1 <= 2^32; the weights of a call are a table of m (d + 1) words that every wave reads
constexpr size_t SHAMIR_MAX_TERMS = (size_t)1 << 20;
constexpr size_t SHAMIR_MAX_WEIGHTS = (size_t)1 << 16;
constexpr size_t SHAMIR_LDS_BYTES = 64 * 1024;

struct ShamirKnobs {
    int nl;        // 32-bit limbs of an element: 8 (bls12-381 Fr) or 2 (Goldilocks)
    int forced;    // SHAMIR_ROUTE_*
    size_t wide_max_chunks;
};
struct ShamirPlan {
    ShamirKernel kernel = ShamirKernel::Generic;
    bool w32 = false;         // SmallWeight: every weight is below 2^32
    int waves = 0;            // SmallWeight: waves of a workgroup
    size_t lds_bytes = 0;     // SmallWeight: LDS of a workgroup
    size_t row_units = 0;     // SmallWeight: a secret's row in LDS, in 8-byte units (padded: see kernels_shamir.hpp)
};

// x^e < 2^64 as integers?  *out = x^e when it is
inline bool shamir_pow_fits(uint64_t x, size_t e, uint64_t* out) {
    uint64_t acc = 1;
    for (size_t i = 0; i < e; ++i) {
        if (x != 0 && acc > UINT64_MAX / x) return false;
        acc *= x;
        if (x <= 1) break;  // 0 and 1 stay put
    }
    *out = e == 0 ? 1 : acc;
    return true;
}

// LDS row of one secret in 8-byte units: its (d + 1) NL / 2 units of coefficients, padded so that the lanes of a wave reading their
// own rows at the same offset fall on different banks (16-byte reads over Fr: an odd number of 16-byte slots; 8-byte reads over
// Goldilocks: an odd number of units)
inline size_t shamir_row_units(int nl, size_t d) {
    const size_t ru = (d + 1) * (size_t)(nl / 2);
    return nl == 8 ? ru + 2 : (ru | 1);
}

// does the small-weight kernel cover the call?  Fills the plan's launch shape when it does.
inline bool shamir_small_weight_covers(int nl, size_t m, size_t d, const uint64_t* points, ShamirPlan* out) {
    if (d + 1 > SHAMIR_MAX_TERMS || m == 0 || m * (d + 1) > SHAMIR_MAX_WEIGHTS) return false;
    uint64_t top = 0;
    for (size_t i = 0; i < m; ++i) {
        uint64_t w;
        if (!shamir_pow_fits(points[i], d, &w)) return false;
        if (w > top) top = w;
    }
    const size_t su = shamir_row_units(nl, d), per_wave = 64 * su * 8;
    if (per_wave > SHAMIR_LDS_BYTES) return false;
    size_t waves = SHAMIR_LDS_BYTES / per_wave;
    if (waves > 4) waves = 4;
    out->w32 = top < ((uint64_t)1 << 32);
    out->waves = (int)waves;
    out->lds_bytes = waves * per_wave;
    out->row_units = su;
    return true;
}

inline ShamirPlan plan_shamir_encode(const ShamirKnobs& k, size_t m, size_t d, size_t B, const uint64_t* points) {
    ShamirPlan p;
    const bool small = shamir_small_weight_covers(k.nl, m, d, points, &p);
    const bool wide_size = B <= k.wide_max_chunks / 4;
    if (small && k.forced != SHAMIR_ROUTE_GENERIC && (k.forced == SHAMIR_ROUTE_SMALL_WEIGHT || !wide_size)) {
        p.kernel = ShamirKernel::SmallWeight;
        return p;
    }
    p = ShamirPlan{};
    p.kernel = wide_size ? ShamirKernel::Wide : ShamirKernel::Generic;
    return p;
}

}  // namespace hbmpc
