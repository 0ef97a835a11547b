// RanSha and RanDouSha for all parties of a small batch in one launch each (kernels_producers_wg.hpp)
#include <hip/hip_runtime.h>

#include "field_dispatch.hpp"
#include "fr_gold.hpp"
#include "fr_u29.hpp"
#include "kernels_producers_wg.hpp"
#include "launchers.hpp"

namespace hbmpc {
// The kernels exist over U29 and Goldilocks (plan_producers sends a Sat32 context down the separate launches).  dry_run: only say whether
// the layout fits a workgroup's LDS, the verifiers' rows fit the workgroup and the LDS attribute above 64 KB could be set.
bool launch_producers_wg(int impl, bool randousha, const ProducersWgArgs& a, int device, hipStream_t s, bool dry_run) {
    static std::atomic<bool> attr[4][HBMPC_MAX_DEVICES];
    bool ran = false;
    by_field(impl, [&](auto f) {
        using F = typename decltype(f)::type;
        if constexpr (!std::is_same<F, Sat32>::value) {
            constexpr bool gold = F::NL != 9;
            const int ns = randousha ? 2 : 1;
            const ProducersWgLds L(a.n, ns, a.nver, (a.sh[0].nv + a.sh[0].M) * a.sh[0].M, (a.sh[1].nv + a.sh[1].M) * a.sh[1].M, gold ? F::NL : 12, F::NL);  // the kernel's own LS, NL
            const size_t bytes = (size_t)L.total * 4;
            if (bytes > 160 * 1024 || a.n > 16 || a.nver > 15) return;
            for (int i = 0; i < ns; ++i)  // a lane per (verifier, row) at least
                if (a.nver * (randousha && gold ? a.sh[i].M : a.sh[i].nv + ns) > 256) return;
            const void* fn = randousha ? (const void*)k_randousha_wg<F> : (const void*)k_ransha_wg<F>;
            if (!ensure_dynamic_lds(fn, attr[(randousha ? 2 : 0) + (gold ? 1 : 0)], device, bytes)) return;
            ran = true;
            if (dry_run) return;
            if (randousha) hipLaunchKernelGGL((k_randousha_wg<F>), dim3((unsigned)a.K), dim3(256), bytes, s, a);
            else hipLaunchKernelGGL((k_ransha_wg<F>), dim3((unsigned)a.K), dim3(256), bytes, s, a);
        }
    });
    return ran;
}
}  // namespace hbmpc
