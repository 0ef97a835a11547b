// seeded RISS dealing (kernels_riss_sample.hpp): one sender's contributions, or all n senders' folded in registers
#include "kernels_riss_sample.hpp"
#include "launchers.hpp"
namespace hbmpc {
void launch_riss_sample(const uint32_t seed[8], uint32_t domain, size_t Tn, size_t B, uint64_t first_index, uint64_t bound, uint64_t* out,
                        hipStream_t s) {
    SeedArg k;
    for (int i = 0; i < 8; ++i) k.k[i] = seed[i];
    const size_t blocks = Tn * ((B + 255) / 256);
    hipLaunchKernelGGL(k_riss_sample, dim3((unsigned)blocks), dim3(256), 0, s, k, domain, B, first_index, bound, out);
}
void launch_riss_sample_fold(const uint32_t* seeds, unsigned n, uint32_t domain, size_t Tn, size_t B, uint64_t first_index, uint64_t bound,
                             uint64_t* sums, hipStream_t s) {
    const size_t blocks = Tn * ((B + 255) / 256);
    hipLaunchKernelGGL(k_riss_sample_fold, dim3((unsigned)blocks), dim3(256), 0, s, (const SeedArg*)seeds, n, domain, B, first_index, bound, sums);
}
}  // namespace hbmpc
