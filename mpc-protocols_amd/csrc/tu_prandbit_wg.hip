// PRandBit / PRandInt for all parties of a small batch in one launch (kernels_prandbit_wg.hpp)
#include <hip/hip_runtime.h>

#include "fr_gold.hpp"
#include "fr_u29.hpp"
#include "kernels_prandbit_wg.hpp"
#include "launchers.hpp"

namespace hbmpc {
// The kernel exists over U29 (plan_prandbit sends a Sat32 context down the separate launches).  dry_run: only say whether the layout
// fits and the LDS attribute above 64 KB could be set.
bool launch_prandbit_wg(bool bit, const PRandBitWgArgs& a, int device, hipStream_t s, bool dry_run) {
    static std::atomic<bool> attr_bit[HBMPC_MAX_DEVICES], attr_int[HBMPC_MAX_DEVICES];
    const PRandBitWgLds L(a.n, a.t, a.Tn);
    const size_t bytes = L.total * 4;
    if (bytes > PRANDBIT_WG_LDS_BYTES) return false;
    const void* kernel = bit ? (const void*)k_prandbit_wg<U29, true> : (const void*)k_prandbit_wg<U29, false>;
    if (!ensure_dynamic_lds(kernel, bit ? attr_bit : attr_int, device, bytes)) return false;
    if (dry_run) return true;
    const dim3 grid((unsigned)((a.B + (size_t)a.t) / (size_t)(a.t + 1)));
    if (bit) hipLaunchKernelGGL((k_prandbit_wg<U29, true>), grid, dim3(256), bytes, s, a);
    else hipLaunchKernelGGL((k_prandbit_wg<U29, false>), grid, dim3(256), bytes, s, a);
    return true;
}
}  // namespace hbmpc
