// fft_bounds.hpp -- compile-time structure of the pruned FFT of kernels_eval.hpp: which inputs are zero and how far the lazy
// radix-2^29 arithmetic (fr_u29.hpp) may run before it has to reduce.  Plain constexpr C++, no HIP: the kernels take their
// decisions from it, and tests/cpp/fft_bounds_dump.cpp prints the same decisions on the CPU for the model of tests/fft_model.py.
#pragma once

namespace hbmpc {

constexpr int bitrev_c(int log, int p) {
    int r = 0;
    for (int b = 0; b < log; ++b)
        if (p & (1 << b)) r |= 1 << (log - 1 - b);
    return r;
}
struct Bd {
    int lbu;  // limb bound in units of 2^29 (0: element is identically zero)
    int vb;   // value bound in units of r
};
constexpr int sub_k(int vb) {
    return vb <= 1 ? 2 : vb <= 2 ? 4 : vb <= 4 ? 8 : vb <= 8 ? 16 : vb <= 16 ? 32 : vb <= 32 ? 64 : (1 << 20);
}

// bound of X[idx] after `stage` butterfly stages (stage 0 = bit-reversed inputs).  The code
// generator in kernels_eval.hpp takes EXACTLY the same decisions (normalise u when lbu would pass 7, canonicalise
// a lazy v before it is subtracted un-multiplied, normalise it before it is multiplied).
constexpr Bd fft_bd(int LOG, int CNT, int LBU0, int VB0, int stage, int idx) {
    if (stage == 0) return bitrev_c(LOG, idx) < CNT ? Bd{LBU0, VB0} : Bd{0, 0};
    const int B = 1 << (stage - 1);
    const int pos = idx & (2 * B - 1), k = pos & (B - 1);
    const int iu = (idx & ~(2 * B - 1)) + k, iv = iu + B;
    const bool upper = pos >= B;
    const Bd u = fft_bd(LOG, CNT, LBU0, VB0, stage - 1, iu), v = fft_bd(LOG, CNT, LBU0, VB0, stage - 1, iv);
    if (v.lbu == 0) return u;
    // k != 0: t is a mulc output; k == 0: t is v itself when it is tight, else v canonicalised
    const Bd t0 = k != 0 ? Bd{1, 2} : ((v.lbu == 1 && v.vb <= 2) ? v : Bd{1, 1});
    const int K = sub_k(t0.vb);
    if (u.lbu == 0) return upper ? Bd{2, K} : t0;
    const Bd un = (u.lbu + 2 > 7) ? Bd{1, u.vb} : u;
    return upper ? Bd{un.lbu + 2, un.vb + K} : Bd{un.lbu + t0.lbu, un.vb + t0.vb};
}

// the largest value bound over the outputs (1 << 20: a limb bound beyond 7)
template <int LOG, int CNT, int LBU0, int VB0>
constexpr int fft_max_vb() {
    int m = 0;
    for (int i = 0; i < (1 << LOG); ++i) {
        const Bd b = fft_bd(LOG, CNT, LBU0, VB0, LOG, i);
        if (b.vb > m) m = b.vb;
        if (b.lbu > 7) return 1 << 20;
    }
    return m;
}

}  // namespace hbmpc
