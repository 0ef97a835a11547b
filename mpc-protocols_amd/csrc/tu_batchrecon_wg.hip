// BatchReconNode for all parties of a small batch in one launch (kernels_batchrecon_wg.hpp)
#include <hip/hip_runtime.h>

#include "field_dispatch.hpp"
#include "fr_gold.hpp"
#include "fr_u29.hpp"
#include "kernels_batchrecon_wg.hpp"
#include "launchers.hpp"

namespace hbmpc {
// The kernel exists over U29 and Goldilocks (plan_batchrecon sends a Sat32 context down the three launches).  dry_run: only say whether
// the layout fits a workgroup's LDS and the LDS attribute above 64 KB could be set.
bool launch_batchrecon_wg(int impl, const BatchReconWgArgs& a, int device, hipStream_t s, bool dry_run) {
    static std::atomic<bool> attr_u29[HBMPC_MAX_DEVICES], attr_gold[HBMPC_MAX_DEVICES];
    bool ran = false;
    by_field(impl, [&](auto f) {
        using F = typename decltype(f)::type;
        if constexpr (!std::is_same<F, Sat32>::value) {
            const BatchReconWgLds L(a.n, a.t, a.d, F::NL == 9 ? 12 : F::NL, F::NL, a.same != 0);  // the kernel's own LS, NL
            const size_t bytes = (size_t)L.total * 4;
            if (bytes > 160 * 1024) return;
            if (!ensure_dynamic_lds((const void*)k_batchrecon_wg<F>, F::NL == 9 ? attr_u29 : attr_gold, device, bytes)) return;
            ran = true;
            if (!dry_run) hipLaunchKernelGGL((k_batchrecon_wg<F>), dim3((unsigned)a.G), dim3(256), bytes, s, a);
        }
    });
    return ran;
}
}  // namespace hbmpc
