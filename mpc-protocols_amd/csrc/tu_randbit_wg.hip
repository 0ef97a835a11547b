// RandBit for all parties of a small batch in one launch (kernels_randbit_wg.hpp)
#include <hip/hip_runtime.h>

#include "field_dispatch.hpp"
#include "fr_gold.hpp"
#include "fr_u29.hpp"
#include "kernels_randbit_wg.hpp"
#include "launchers.hpp"

namespace hbmpc {
void launch_randbit_wg(int impl, const RandBitWgArgs& a, hipStream_t s) {
    by_field(impl, [&](auto f) {
        using F = typename decltype(f)::type;
        // the kernel exists over U29 and Goldilocks; the caller sends a Sat32 context down the nine launches
        if constexpr (!std::is_same<F, Sat32>::value) {
            const RandBitWgLds L(a.n, a.t, F::NL == 9 ? 12 : F::NL, F::NL);  // the kernel's own LS, NL
            hipLaunchKernelGGL((k_randbit_wg<F>), dim3((unsigned)(a.N / (size_t)(a.t + 1))), dim3(256), (size_t)L.total * 4, s, a);
        }
    });
}
}  // namespace hbmpc
