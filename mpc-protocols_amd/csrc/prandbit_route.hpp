// prandbit_route.hpp -- which form hbmpc_dev_prandbit_parties / hbmpc_dev_prandint_parties take, and the LDS layout of their one-launch
// kernel (kernels_prandbit_wg.hpp): ONE place for the rule (plain C++, no HIP), as protocol_route.hpp is for the other protocol calls.
//
// Either form writes the same bytes to every output buffer.  One decline stays with the executor: the launcher's dry run (the LDS
// attribute above 64 KB, launchers.hpp); the call then runs its separate launches.
#pragma once
#include <stddef.h>

#include "field_dispatch.hpp"

#if defined(__HIPCC__)
#define HB_ROUTE_HD __host__ __device__
#else
#define HB_ROUTE_HD
#endif

namespace hbmpc {

constexpr int PRANDBIT_WG_LANES = 256;
constexpr int PRANDBIT_WG_MERGE_WORDS = 27 + 9 + 1;  // a slice's partial sums on their way to slice 0: RissAcc<U29>, RissAcc<Gold>, the GF(2^8) byte
constexpr size_t PRANDBIT_WG_LDS_BYTES = 160 * 1024;

// LDS words of k_prandbit_wg for n parties, t faults, Tn = C(n, t) sets; a workgroup takes one chunk of M = t + 1 elements.
//   the constants: cF [Tn][n][8] f_T(alpha_j) over Fr | cG [Tn][n][2] over Goldilocks | c2 [Tn][n] in GF(2^8), a word each
//                  | vmat [n][M][2] | tab [t verify rows | M coefficient rows][M][2] (Goldilocks, ids 0 .. 2t, degree t)
//   the chunk:     S [Tn][M][2] the folded sums | X [n][M][2] r + b | Y [n][n][2] the messages | Z [n][2] | O [M][2] the opened values
//                  | flags [n + 1] | merge [ks - 1][n M][PRANDBIT_WG_MERGE_WORDS]
// ks: the slices of the sets that the conversion's lanes take when there are fewer outputs (n M) than lanes.
struct PRandBitWgLds {
    int cF, cG, c2, vmat, tab, S, X, Y, Z, O, flags, merge, ks;
    size_t total;
    HB_ROUTE_HD PRandBitWgLds(size_t n, size_t t, size_t Tn) {
        const size_t M = t + 1, outs = n * M;
        size_t k = outs ? PRANDBIT_WG_LANES / outs : 1;
        if (k > Tn) k = Tn;
        if (k > 8) k = 8;
        if (k < 1) k = 1;
        ks = (int)k;
        size_t o = 0;
        cF = (int)o, o += Tn * n * 8;
        cG = (int)o, o += Tn * n * 2;
        c2 = (int)o, o += Tn * n;
        vmat = (int)o, o += n * M * 2;
        tab = (int)o, o += (t + M) * M * 2;
        S = (int)o, o += Tn * M * 2;
        X = (int)o, o += n * M * 2;
        Y = (int)o, o += n * n * 2;
        Z = (int)o, o += n * 2;
        O = (int)o, o += M * 2;
        flags = (int)o, o += n + 1;
        o = (o + 3) & ~(size_t)3;
        merge = (int)o, o += (k - 1) * outs * PRANDBIT_WG_MERGE_WORDS;
        total = o;
    }
};

// the context fields the rule reads: the Fr context's, and `direct_fail` of the Goldilocks context (whose decodes the open replaces)
struct PRandBitKnobs {
    int impl_fr;
    bool force_generic, direct_fail;
    size_t fused_prandbit_max;  // chunks (0: never)
};
// the call: bit = PRandBit (else PRandInt, which has no open: open_senders and direct_fail are not read), B elements per party,
// Tn = C(n, t), open_senders as the caller gave it (0 = 2t + 1)
struct PRandBitShape {
    bool bit;
    size_t B, n, t, Tn, open_senders;
};
struct PRandBitPlan {
    bool one_launch;
    size_t chunks;     // workgroups of the one launch: ceil(B / (t + 1))
    size_t senders;    // of the open
    size_t lds_bytes;  // of the layout (0 when the shape is outside the kernel's range)
};

inline PRandBitPlan plan_prandbit(const PRandBitKnobs& k, const PRandBitShape& s) {
    PRandBitPlan p{false, 0, s.open_senders ? s.open_senders : 2 * s.t + 1, 0};
    p.chunks = (s.B + s.t) / (s.t + 1);
    // the kernel: a lane per (party, element) of the chunk, a lane per (party, recipient) of the encode; Fr in 29-bit limbs
    const bool shape = s.t >= 1 && s.n >= 3 * s.t + 1 && s.n <= 16;
    if (shape) p.lds_bytes = PRandBitWgLds(s.n, s.t, s.Tn).total * 4;
    // one launch has no OEC round and writes a failed chunk itself, as the one-launch decodes do (recover_route.hpp)
    const bool open_ok = !s.bit || (k.direct_fail && p.senders == 2 * s.t + 1);
    p.one_launch = shape && k.impl_fr == IMPL_U29 && !k.force_generic && open_ok && p.lds_bytes <= PRANDBIT_WG_LDS_BYTES && p.chunks >= 1 &&
                   p.chunks <= k.fused_prandbit_max;
    return p;
}

}  // namespace hbmpc
