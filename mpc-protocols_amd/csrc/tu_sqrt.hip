#include "kernels_sqrt.hpp"
namespace hbmpc {
// elements per lane of the batched inversion: one Fermat inversion per lane amortised over B elements (sat32 spills at 8)
constexpr int INV_B = 8, INV_B_SAT = 2;
void launch_sqrt(int impl, const uint32_t* a, size_t N, const SqrtTab& t, uint32_t* root, uint8_t* has_root, hipStream_t s) {
    const unsigned grid = (unsigned)((N + 255) / 256);
    if (impl == 0) hipLaunchKernelGGL((k_sqrt<U29>), dim3(grid), dim3(256), 0, s, a, N, t, root, has_root);
    else if (impl == 1) hipLaunchKernelGGL((k_sqrt<Sat32>), dim3(grid), dim3(256), 0, s, a, N, t, root, has_root);
    else hipLaunchKernelGGL((k_sqrt<Gold>), dim3(grid), dim3(256), 0, s, a, N, t, root, has_root);
}
void launch_inverse(int impl, const uint32_t* a, size_t N, const SqrtTab& t, uint32_t* inv, uint8_t* ok, hipStream_t s) {
    const int B = impl == 1 ? INV_B_SAT : INV_B;
    const unsigned grid = (unsigned)((N + 256 * B - 1) / (256 * B));
    if (impl == 0) hipLaunchKernelGGL((k_inverse<U29, INV_B>), dim3(grid), dim3(256), 0, s, a, N, t, inv, ok);
    else if (impl == 1) hipLaunchKernelGGL((k_inverse<Sat32, INV_B_SAT>), dim3(grid), dim3(256), 0, s, a, N, t, inv, ok);
    else hipLaunchKernelGGL((k_inverse<Gold, INV_B>), dim3(grid), dim3(256), 0, s, a, N, t, inv, ok);
}
void launch_randbit_finalize(int impl, const uint32_t* a, const uint32_t* sq, size_t N, unsigned parties, const SqrtTab& t, uint32_t* out,
                             uint8_t* status, RandBitSummaryDev* summary, hipStream_t s) {
    const unsigned grid = (unsigned)((N + 255) / 256);
    if (impl == 0) hipLaunchKernelGGL((k_randbit_finalize<U29>), dim3(grid), dim3(256), 0, s, a, sq, N, parties, t, out, status, summary);
    else if (impl == 1) hipLaunchKernelGGL((k_randbit_finalize<Sat32>), dim3(grid), dim3(256), 0, s, a, sq, N, parties, t, out, status, summary);
    else hipLaunchKernelGGL((k_randbit_finalize<Gold>), dim3(grid), dim3(256), 0, s, a, sq, N, parties, t, out, status, summary);
}
}  // namespace hbmpc
