#include "field_dispatch.hpp"
#include "kernels_riss.hpp"
#include "launchers.hpp"
namespace hbmpc {
void launch_riss_fold(const uint64_t* contrib, unsigned n, size_t Tn, size_t B, uint64_t bound, uint64_t* sums, uint8_t* bad, hipStream_t s) {
    const size_t blocks = Tn * ((B + 255) / 256);
    hipLaunchKernelGGL((k_riss_fold<8>), dim3((unsigned)blocks), dim3(256), 0, s, contrib, n, Tn, B, bound, sums, bad);
}
void launch_riss_convert(int impl, bool wide, const uint64_t* r, size_t B, unsigned Tn, const RissTab& tab, const uint32_t* cols, unsigned parties,
                         uint32_t* out, uint8_t* out2, hipStream_t s) {
    const unsigned gx = (unsigned)((B + 63) / 64);
    by_field(impl, [&](auto f) {
        using F = typename decltype(f)::type;
        if (wide) {
            const dim3 grid(gx, (parties + 15) / 16);
            if (out2) hipLaunchKernelGGL((k_riss_convert<F, 4, 1, true>), grid, dim3(256), 0, s, r, B, Tn, tab, cols, parties, out, out2);
            else hipLaunchKernelGGL((k_riss_convert<F, 4, 1, false>), grid, dim3(256), 0, s, r, B, Tn, tab, cols, parties, out, out2);
        } else {
            const dim3 grid(gx, parties);
            if (out2) hipLaunchKernelGGL((k_riss_convert<F, 1, 4, true>), grid, dim3(256), 0, s, r, B, Tn, tab, cols, parties, out, out2);
            else hipLaunchKernelGGL((k_riss_convert<F, 1, 4, false>), grid, dim3(256), 0, s, r, B, Tn, tab, cols, parties, out, out2);
        }
    });
}
void launch_prandbit_finalize(int impl, const uint64_t* v, const uint32_t* r_p, const uint8_t* r_2, size_t N, unsigned parties, uint32_t* bp,
                              uint8_t* b2, hipStream_t s) {
    const dim3 grid((unsigned)((N + 255) / 256), parties);
    by_fr_impl(impl, [&](auto f) { hipLaunchKernelGGL((k_prandbit_finalize<field_t<decltype(f)>>), grid, dim3(256), 0, s, v, r_p, r_2, N, bp, b2); });
}
}  // namespace hbmpc
