#include <cstring>
#include "field_dispatch.hpp"
#include "fr_gold.hpp"
#include "kernels_eval.hpp"
#include "launchers.hpp"
#include "wide_plan.hpp"
namespace hbmpc {
// a run-time flag as a compile-time one: fn(std::true_type{}) or fn(std::false_type{})
template <class Fn>
static void by_bool(bool b, Fn&& fn) {
    if (b) fn(std::true_type{});
    else fn(std::false_type{});
}
void launch_eval_generic(int impl, const uint32_t* x, size_t G, int n, int dp1, const uint32_t* alpha, EvalOut y,
                         hipStream_t s) {
    const unsigned grid = (unsigned)((G + 255) / 256);
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_eval_generic<field_t<decltype(f)>>), dim3(grid, y.parties), dim3(256), 0, s, x, G, n, dp1, alpha, y.y, y.ys ? y.ys : G); });
}
void launch_eval_wide_dot(const uint32_t* x, size_t G, int n, int dp1, const uint32_t* vmat, EvalOut y, hipStream_t s) {
    const unsigned grid = (unsigned)((G + 3) / 4);
    int lk = 0;
    while (lk < 2 && (n << (lk + 1)) <= 64 && (2 << lk) <= dp1) ++lk;
    hipLaunchKernelGGL((k_eval_wide_dot<U29>), dim3(grid, y.parties), dim3(256), (size_t)n * dp1 * U29::NL * 4, s, x, G, n, dp1, vmat, y.y, y.ys ? y.ys : G, lk);
}
void launch_eval_wide(int impl, const uint32_t* x, size_t G, int n, int dp1, const uint32_t* alpha, EvalOut y, hipStream_t s) {
    const unsigned grid = (unsigned)((G + 3) / 4);
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_eval_wide<field_t<decltype(f)>>), dim3(grid, y.parties), dim3(256), 0, s, x, G, n, dp1, alpha, y.y, y.ys ? y.ys : G); });
}
void launch_recover_generic(int impl, bool p0, const RecoverArgs& ra, unsigned grid, hipStream_t s) {
    by_field(impl, [&](auto f) {
        using F = typename decltype(f)::type;
        by_bool(p0, [&](auto P0) { hipLaunchKernelGGL((k_batch_recover_generic<F, decltype(P0)::value>), dim3(grid), dim3(256), 0, s, ra); });
    });
}
void launch_recover_wide(int impl, bool p0, const RecoverArgs& ra, const SecondArgs* sc, hipStream_t s, int ow_sel) {
    const unsigned grid = (unsigned)((ra.G + 3) / 4);
    WideArgs wa;
    wa.r = ra;
    wa.fused = sc != nullptr;
    if (sc) wa.sc = *sc;
    else memset(&wa.sc, 0, sizeof wa.sc);
    wa.ow = p0 ? 0 : ow_sel;
    const size_t nv = (size_t)(ra.needed - ra.m);
    const WidePlan wp = wide_plan(impl, ra.needed, ra.m, p0, ow_sel, ra.bc == ra.vm + nv * (size_t)ra.m * (size_t)impl_nl(impl), ((uintptr_t)ra.vm & 15) == 0);
    const size_t lds = wp.lds;
    wa.tab_words = wp.tab_words, wa.split = wp.split, wa.lk = wp.lk;
    const bool tab = wa.tab_words != 0;
    by_field(impl, [&](auto f) {
        using F = typename decltype(f)::type;
        by_bool(p0, [&](auto P0) {
            if (tab) hipLaunchKernelGGL((k_batch_recover_wide<F, decltype(P0)::value, true>), dim3(grid), dim3(256), lds, s, wa);
            else hipLaunchKernelGGL((k_batch_recover_wide<F, decltype(P0)::value, false>), dim3(grid), dim3(256), lds, s, wa);
        });
    });
}
void launch_second_chance(int impl, const SecondArgs& a, unsigned grid, hipStream_t s) {
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_second_chance<field_t<decltype(f)>>), dim3(grid), dim3(256), 0, s, a); });
}
void launch_matvec(int impl, const uint32_t* lb, const uint32_t* y, int S, uint32_t* out, hipStream_t s) {
    const unsigned grid = (unsigned)((S + 255) / 256);
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_matvec<field_t<decltype(f)>>), dim3(grid), dim3(256), 0, s, lb, y, S, out); });
}
}
