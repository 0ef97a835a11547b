// TripleGenNode for all parties of a small batch in one launch (kernels_triplegen_wg.hpp)
#include <hip/hip_runtime.h>

#include "field_dispatch.hpp"
#include "fr_gold.hpp"
#include "fr_u29.hpp"
#include "kernels_triplegen_wg.hpp"
#include "launchers.hpp"

namespace hbmpc {
void launch_triplegen_wg(int impl, const TripleGenWgArgs& a, hipStream_t s) {
    by_field(impl, [&](auto f) {
        using F = typename decltype(f)::type;
        // the kernel exists over U29 and Goldilocks; the caller sends a Sat32 context down the four-launch path
        if constexpr (!std::is_same<F, Sat32>::value) {
            const TripleGenWgLds L(a.n, a.t, F::NL == 9 ? 12 : F::NL, F::NL);  // the kernel's own LS, NL
            hipLaunchKernelGGL((k_triplegen_wg<F>), dim3((unsigned)a.G), dim3(256), (size_t)L.total * 4, s, a);
        }
    });
}
}  // namespace hbmpc
