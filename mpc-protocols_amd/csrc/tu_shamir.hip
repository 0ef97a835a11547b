#include "kernels_shamir.hpp"
#include "launchers.hpp"
namespace hbmpc {
template <int NL, bool W32>
static void launch_shamir_t(const void* coeffs, size_t B, int m, int dp1, const uint64_t* w, void* out, int waves, size_t lds_bytes,
                            int row_units, hipStream_t s) {
    const size_t per_block = (size_t)waves * 64;
    const unsigned grid = (unsigned)((B + per_block - 1) / per_block);
    const int aligned16 = ((uintptr_t)coeffs & 15) == 0;
    hipLaunchKernelGGL((k_shamir_encode<NL, W32>), dim3(grid), dim3((unsigned)per_block), lds_bytes, s, (const uint64_t*)coeffs, B, m, dp1, w,
                       (uint64_t*)out, row_units, aligned16);
}
void launch_shamir_encode(int nl, bool w32, const void* coeffs, size_t B, int m, int dp1, const uint64_t* w, void* out, int waves,
                          size_t lds_bytes, int row_units, hipStream_t s) {
    if (nl == 8) {
        if (w32) launch_shamir_t<8, true>(coeffs, B, m, dp1, w, out, waves, lds_bytes, row_units, s);
        else launch_shamir_t<8, false>(coeffs, B, m, dp1, w, out, waves, lds_bytes, row_units, s);
    } else {
        if (w32) launch_shamir_t<2, true>(coeffs, B, m, dp1, w, out, waves, lds_bytes, row_units, s);
        else launch_shamir_t<2, false>(coeffs, B, m, dp1, w, out, waves, lds_bytes, row_units, s);
    }
}
}  // namespace hbmpc
