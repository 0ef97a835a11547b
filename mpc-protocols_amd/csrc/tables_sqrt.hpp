// tables_sqrt.hpp -- host-side constants of kernels_sqrt.hpp for one context (field and implementation): omega powers for the
// discrete log and for omega^v, the two fixed exponents, 2^-1, and the reverse look-up of the 256-element subgroup.
#pragma once
#include <cstring>
#include <stdexcept>
#include <vector>

#include "sqrt_args.hpp"
#include "tables.hpp"

namespace hbmpc {

struct SqrtLayout {  // word offsets inside the table; kbits / kshift / exponent bit counts
    size_t negw, posw, r2, one_p, half, half_p, e_sqrt, e_inv, keyt;
    int kbits, kshift, bits_sqrt, bits_inv;
};
inline SqrtLayout sqrt_layout(int impl, int kbits, int kshift, int bits_sqrt, int bits_inv) {
    const size_t nl = (size_t)impl_nl(impl);
    SqrtLayout L;
    L.negw = 0;
    L.posw = L.negw + 3 * 256 * nl;
    L.r2 = L.posw + 4 * 256 * nl;
    L.one_p = L.r2 + nl, L.half = L.one_p + nl, L.half_p = L.half + nl;
    L.e_sqrt = L.half_p + nl, L.e_inv = L.e_sqrt + 8, L.keyt = L.e_inv + 8;
    L.kbits = kbits, L.kshift = kshift, L.bits_sqrt = bits_sqrt, L.bits_inv = bits_inv;
    return L;
}
inline int bit_length(const uint64_t e[4]) {
    for (int i = 255; i >= 0; --i)
        if ((e[i >> 6] >> (i & 63)) & 1) return i + 1;
    return 0;
}
// mod: the field's modulus p (four 64-bit limbs); rdev: the device Montgomery radix as a field value (1 for Goldilocks).
// Returns the table words and fills *lay.  The look-up key of a value is bits [kshift, kshift + kbits) of SQRT_KEY_MUL times the
// two low limbs of its device-constant (Montgomery) form; the smallest kbits, then the lowest kshift, for which the 256 subgroup
// elements have distinct keys is taken (std::runtime_error when none has; 12 to 14 bits in the three implementations).
template <class H>
inline std::vector<uint32_t> build_sqrt_table(const uint64_t mod[4], const H& rdev, int impl, SqrtLayout* lay) {
    // e_sqrt = (T - 1) / 2 = (p - 1) >> 33 (T = (p - 1) / 2^32 is odd); e_inv = p - 2
    uint64_t pm1[4] = {mod[0] - 1, mod[1], mod[2], mod[3]}, es[4], ei[4] = {mod[0] - 2, mod[1], mod[2], mod[3]};
    for (int i = 0; i < 4; ++i) es[i] = (pm1[i] >> 33) | (i < 3 ? pm1[i + 1] << 31 : 0);
    const H w = H::two_adic_root(), wi = w.inv();
    // the 256-element subgroup zeta^j (zeta = omega^(2^24)) and the low words of their device forms
    H zeta = w;
    for (int i = 0; i < 24; ++i) zeta = zeta * zeta;
    std::vector<uint64_t> low(256);  // the hashed low limbs (kernels_sqrt.hpp sqrt_key)
    {
        H z = H::one();
        for (int j = 0; j < 256; ++j) {
            std::vector<uint32_t> v;
            put_const(v, z, impl);
            low[j] = (((uint64_t)v[1] << 32) | v[0]) * SQRT_KEY_MUL;
            z = z * zeta;
        }
    }
    int kbits = -1, kshift = 0;
    for (int kb = 8; kb <= 20 && kbits < 0; ++kb)
        for (int sh = 0; sh + kb <= 64 && kbits < 0; ++sh) {
            std::vector<uint8_t> seen((size_t)1 << kb, 0);
            bool ok = true;
            for (int j = 0; j < 256 && ok; ++j) {
                const uint32_t k = (uint32_t)(low[j] >> sh) & ((1u << kb) - 1);
                ok = !seen[k];
                seen[k] = 1;
            }
            if (ok) kbits = kb, kshift = sh;
        }
    if (kbits < 0) throw std::runtime_error("no collision-free key slice for the 256-element subgroup");
    *lay = sqrt_layout(impl, kbits, kshift, bit_length(es), bit_length(ei));
    std::vector<uint32_t> out;
    out.reserve(lay->keyt + ((size_t)1 << kbits) / 4 + 1);
    for (int m = 0; m < 3; ++m) {  // negw[m][j] = omega^(-j 2^(8m))
        H step = wi;
        for (int i = 0; i < 8 * m; ++i) step = step * step;
        H p = H::one();
        for (int j = 0; j < 256; ++j, p = p * step) put_const(out, p, impl);
    }
    for (int m = 0; m < 4; ++m) {  // posw[m][j] = omega^(j 2^(8m))
        H step = w;
        for (int i = 0; i < 8 * m; ++i) step = step * step;
        H p = H::one();
        for (int j = 0; j < 256; ++j, p = p * step) put_const(out, p, impl);
    }
    const H half = H::from_u64(2).inv();
    put_const(out, rdev, impl);  // put_const writes v Rdev: Rdev^2, the r2 of mont(x, r2) = x Rdev
    put_plain(out, H::one(), impl);
    put_const(out, half, impl);
    put_plain(out, half, impl);
    for (int i = 0; i < 4; ++i) out.push_back((uint32_t)es[i]), out.push_back((uint32_t)(es[i] >> 32));
    for (int i = 0; i < 4; ++i) out.push_back((uint32_t)ei[i]), out.push_back((uint32_t)(ei[i] >> 32));
    if (out.size() != lay->keyt) throw std::runtime_error("sqrt table layout");
    std::vector<uint8_t> keyt(((size_t)1 << kbits) + 4, 0);
    for (int j = 0; j < 256; ++j) keyt[(uint32_t)(low[j] >> kshift) & ((1u << kbits) - 1)] = (uint8_t)j;
    const size_t words = keyt.size() / 4;
    out.resize(lay->keyt + words);
    memcpy(out.data() + lay->keyt, keyt.data(), words * 4);
    return out;
}

}  // namespace hbmpc
