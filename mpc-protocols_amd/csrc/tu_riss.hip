#include "kernels_riss.hpp"
namespace hbmpc {
void launch_riss_fold(const uint64_t* contrib, unsigned n, size_t Tn, size_t B, uint64_t bound, uint64_t* sums, uint8_t* bad, hipStream_t s) {
    const size_t blocks = Tn * ((B + 255) / 256);
    hipLaunchKernelGGL((k_riss_fold<8>), dim3((unsigned)blocks), dim3(256), 0, s, contrib, n, Tn, B, bound, sums, bad);
}
template <class F>
static void convert_f(bool wide, const uint64_t* r, size_t B, unsigned Tn, const RissTab& tab, const uint32_t* cols, unsigned parties, uint32_t* out,
                      uint8_t* out2, hipStream_t s) {
    const unsigned gx = (unsigned)((B + 63) / 64);
    if (wide) {
        const dim3 grid(gx, (parties + 15) / 16);
        if (out2) hipLaunchKernelGGL((k_riss_convert<F, 4, 1, true>), grid, dim3(256), 0, s, r, B, Tn, tab, cols, parties, out, out2);
        else hipLaunchKernelGGL((k_riss_convert<F, 4, 1, false>), grid, dim3(256), 0, s, r, B, Tn, tab, cols, parties, out, out2);
    } else {
        const dim3 grid(gx, parties);
        if (out2) hipLaunchKernelGGL((k_riss_convert<F, 1, 4, true>), grid, dim3(256), 0, s, r, B, Tn, tab, cols, parties, out, out2);
        else hipLaunchKernelGGL((k_riss_convert<F, 1, 4, false>), grid, dim3(256), 0, s, r, B, Tn, tab, cols, parties, out, out2);
    }
}
void launch_riss_convert(int impl, bool wide, const uint64_t* r, size_t B, unsigned Tn, const RissTab& tab, const uint32_t* cols, unsigned parties,
                         uint32_t* out, uint8_t* out2, hipStream_t s) {
    if (impl == 0) convert_f<U29>(wide, r, B, Tn, tab, cols, parties, out, out2, s);
    else if (impl == 1) convert_f<Sat32>(wide, r, B, Tn, tab, cols, parties, out, out2, s);
    else convert_f<Gold>(wide, r, B, Tn, tab, cols, parties, out, out2, s);
}
void launch_prandbit_finalize(int impl, const uint64_t* v, const uint32_t* r_p, const uint8_t* r_2, size_t N, unsigned parties, uint32_t* bp,
                              uint8_t* b2, hipStream_t s) {
    const dim3 grid((unsigned)((N + 255) / 256), parties);
    if (impl == 0) hipLaunchKernelGGL((k_prandbit_finalize<U29>), grid, dim3(256), 0, s, v, r_p, r_2, N, bp, b2);
    else hipLaunchKernelGGL((k_prandbit_finalize<Sat32>), grid, dim3(256), 0, s, v, r_p, r_2, N, bp, b2);
}
}  // namespace hbmpc
