// tables_riss.hpp -- host-side constants of kernels_riss.hpp: the maximal unqualified sets of (n, t), GF(2^8), and the coefficient
// table f_T(alpha_j) of one context and (n, t) for the context's prime field and for GF(2^8).
//   f_T is the degree-t polynomial with f_T(0) = 1 and f_T(alpha_m) = 0 for m in T (fpmul/mod.rs:258-279, f256.rs:236-256), so
//   f_T(x) = prod_{m in T} (1 - x / alpha_m) and only f_T(alpha_j) is ever used (prandbitd.rs:328-334): no polynomial is built.
#pragma once
#include <stdexcept>
#include <vector>

#include "riss_args.hpp"
#include "tables.hpp"

namespace hbmpc {

constexpr size_t RISS_MAX_ENTRIES = (size_t)1 << 20;  // C(n, t) n of a table (32 MiB of Fr coefficients)

// C(n, t), or SIZE_MAX when it exceeds `cap`
inline size_t riss_binomial(size_t n, size_t t, size_t cap) {
    if (t > n) return 0;
    if (t > n - t) t = n - t;
    unsigned __int128 c = 1;
    for (size_t k = 1; k <= t; ++k) {
        c = c * (n - t + k) / k;  // exact: C(n - t + k, k)
        if (c > cap) return SIZE_MAX;
    }
    return (size_t)c;
}
// combinations(0..n, t) in the order itertools (Rust and Python) yields them: lexicographic (prandbitd.rs:479)
inline std::vector<std::vector<uint32_t>> riss_tsets(size_t n, size_t t) {
    std::vector<std::vector<uint32_t>> out;
    if (t > n) return out;
    std::vector<uint32_t> c(t);
    for (size_t k = 0; k < t; ++k) c[k] = (uint32_t)k;
    for (;;) {
        out.push_back(c);
        size_t k = t;
        while (k > 0 && c[k - 1] == n - t + (k - 1)) --k;
        if (k == 0) return out;
        ++c[k - 1];
        for (size_t m = k; m < t; ++m) c[m] = c[m - 1] + 1;
    }
}

// GF(2^8), AES polynomial 0x11B, generator 3 (f256.rs:58-110); Gf256Domain's element(i) = 3^i (f256.rs:266-292)
inline uint8_t gf256_mul(uint8_t x, uint8_t y) {
    unsigned r = 0, a = x, b = y;
    for (; b; b >>= 1) {
        if (b & 1) r ^= a;
        a <<= 1;
        if (a & 0x100) a ^= 0x11B;
    }
    return (uint8_t)r;
}
inline uint8_t gf256_inv(uint8_t x) {  // x^254
    uint8_t r = 1;
    for (int i = 0; i < 254; ++i) r = gf256_mul(r, x);
    return r;
}

struct RissLayout {  // word offsets inside the table
    size_t coef = 0, red = 0, coef2 = 0, words = 0;
    size_t Tn = 0, ncols = 0;
    bool has2 = false;
};
// own < 0: every set, a column per party (zero where the party is in the set).  own >= 0: that party's sets only (combinations order with its own
// sets skipped, as the reference enumerates them: prandbitd.rs:483-487), one column.
inline RissLayout riss_layout(int impl, size_t n, size_t Tn_all, size_t Tn_own, long own) {
    RissLayout L;
    const size_t nc = impl == IMPL_GOLD ? 2 : 8;
    L.Tn = own < 0 ? Tn_all : Tn_own, L.ncols = own < 0 ? n : 1;
    L.has2 = n <= 255;
    L.coef = 0;
    L.red = L.coef + L.Tn * L.ncols * nc;
    L.coef2 = L.red + (impl == IMPL_GOLD ? 0 : 2 * (size_t)impl_nl(impl));
    L.words = L.coef2 + (L.has2 ? L.Tn * L.ncols : 0);
    return L;
}
inline void riss_put_canon(std::vector<uint32_t>& out, const HFr& v) {
    uint64_t c[4];
    v.to_canon(c);
    for (int i = 0; i < 4; ++i) out.push_back((uint32_t)c[i]), out.push_back((uint32_t)(c[i] >> 32));
}
inline void riss_put_canon(std::vector<uint32_t>& out, const HGl& v) { out.push_back((uint32_t)v.v), out.push_back((uint32_t)(v.v >> 32)); }
inline void riss_put_red(std::vector<uint32_t>& out, const HFr&, int impl) {
    put_const(out, HFr::one(), impl);  // mont(x, 1 Rdev) = x mod r
    HFr p = HFr::one(), two = HFr::from_u64(2);
    for (int i = 0; i < 224; ++i) p = p * two;
    put_const(out, p, impl);           // mont(x, 2^224 Rdev) = 2^224 x mod r
}
inline void riss_put_red(std::vector<uint32_t>&, const HGl&, int) {}

template <class H>
inline std::vector<uint32_t> build_riss_table(size_t n, size_t t, long own, int impl, RissLayout* lay) {
    const auto tsets = riss_tsets(n, t);
    size_t Tn_own = 0;
    if (own >= 0)
        for (const auto& T : tsets) {
            bool in = false;
            for (uint32_t m : T) in |= (long)m == own;
            Tn_own += !in;
        }
    const RissLayout L = riss_layout(impl, n, tsets.size(), Tn_own, own);
    const size_t size = domain_size(n);
    const std::vector<H> el = domain_elements<H>(n, size);  // el[size - m] = 1 / alpha_m
    std::vector<uint8_t> g(n <= 255 ? n : 0), ginv(g.size());
    for (size_t j = 0; j < g.size(); ++j) g[j] = j ? gf256_mul(g[j - 1], 3) : 1, ginv[j] = gf256_inv(g[j]);
    std::vector<uint32_t> out, c2(L.has2 ? L.Tn * L.ncols : 0, 0);
    out.reserve(L.words);
    size_t row = 0;
    for (const auto& T : tsets) {
        bool skip = false;
        for (uint32_t m : T) skip |= (long)m == own;
        if (skip) continue;
        for (size_t col = 0; col < L.ncols; ++col) {
            const size_t j = own < 0 ? col : (size_t)own;
            H f = H::one();
            uint8_t f2 = 1;
            for (uint32_t m : T) {
                f = f * (el[m] - el[j]) * el[(size - m) % size];  // 1 - alpha_j / alpha_m; zero when j is in T
                if (L.has2) f2 = gf256_mul(f2, 1 ^ gf256_mul(g[j], ginv[m]));
            }
            riss_put_canon(out, f);
            if (L.has2) c2[row * L.ncols + col] = f2;
        }
        ++row;
    }
    if (row != L.Tn || out.size() != L.red) throw std::runtime_error("riss table layout");
    riss_put_red(out, H::one(), impl);
    if (out.size() != L.coef2) throw std::runtime_error("riss table layout");
    out.insert(out.end(), c2.begin(), c2.end());
    if (out.size() != L.words) throw std::runtime_error("riss table layout");
    *lay = L;
    return out;
}

}  // namespace hbmpc
