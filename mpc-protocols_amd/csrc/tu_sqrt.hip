#include "field_dispatch.hpp"
#include "kernels_sqrt.hpp"
#include "launchers.hpp"
namespace hbmpc {
// elements per lane of the batched inversion: one Fermat inversion per lane amortised over B elements (sat32 spills at 8)
template <class F>
constexpr int INV_B = std::is_same<F, Sat32>::value ? 2 : 8;
void launch_sqrt(int impl, const uint32_t* a, size_t N, const SqrtTab& t, uint32_t* root, uint8_t* has_root, hipStream_t s) {
    const unsigned grid = (unsigned)((N + 255) / 256);
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_sqrt<field_t<decltype(f)>>), dim3(grid), dim3(256), 0, s, a, N, t, root, has_root); });
}
void launch_inverse(int impl, const uint32_t* a, size_t N, const SqrtTab& t, uint32_t* inv, uint8_t* ok, hipStream_t s) {
    by_field(impl, [&](auto f) {
        using F = typename decltype(f)::type;
        constexpr int B = INV_B<F>;
        const unsigned grid = (unsigned)((N + 256 * B - 1) / (256 * B));
        hipLaunchKernelGGL((k_inverse<F, B>), dim3(grid), dim3(256), 0, s, a, N, t, inv, ok);
    });
}
void launch_randbit_finalize(int impl, const uint32_t* a, const uint32_t* sq, size_t N, unsigned parties, const SqrtTab& t, uint32_t* out,
                             uint8_t* status, RandBitSummaryDev* summary, hipStream_t s) {
    const unsigned grid = (unsigned)((N + 255) / 256);
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_randbit_finalize<field_t<decltype(f)>>), dim3(grid), dim3(256), 0, s, a, sq, N, parties, t, out, status, summary); });
}
}  // namespace hbmpc
