// field_dispatch.hpp -- the one place where a context's run-time field implementation becomes a compile-time type.
// Host-only (the host-side test programs include it through tables.hpp): the field types are only named here, a caller that
// launches a kernel includes their headers itself.
//   by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_x<field_t<decltype(f)>>), ...); });
#pragma once
#include <stddef.h>

namespace hbmpc {

struct U29;    // fr_u29.hpp: bls12-381 Fr, nine 29-bit limbs
struct Sat32;  // fr_sat.hpp: bls12-381 Fr, eight 32-bit limbs
struct Gold;   // fr_gold.hpp: Goldilocks64

enum FieldImpl { IMPL_U29 = 0, IMPL_SAT32 = 1, IMPL_GOLD = 2 };
inline int impl_nl(int impl) { return impl == IMPL_U29 ? 9 : impl == IMPL_SAT32 ? 8 : 2; }
inline size_t impl_ebytes(int impl) { return impl == IMPL_GOLD ? 8 : 32; }  // bytes per stored element

template <class F>
struct FieldTag {
    using type = F;
};
template <class Tag>
using field_t = typename Tag::type;  // of a lambda's `auto f`: field_t<decltype(f)>

template <class Fn>
inline void by_field(int impl, Fn&& fn) {
    if (impl == IMPL_U29) fn(FieldTag<U29>{});
    else if (impl == IMPL_SAT32) fn(FieldTag<Sat32>{});
    else fn(FieldTag<Gold>{});
}
// kernels that exist over Fr only (their callers refuse a Goldilocks context first): no Gold instantiation is made
template <class Fn>
inline void by_fr_impl(int impl, Fn&& fn) {
    if (impl == IMPL_U29) fn(FieldTag<U29>{});
    else fn(FieldTag<Sat32>{});
}

}  // namespace hbmpc
