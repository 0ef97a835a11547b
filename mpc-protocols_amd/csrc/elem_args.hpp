// elem_args.hpp -- the structs that the element-wise kernels (kernels_elem.hpp) take by value; the host fills them
#pragma once
#include <stdint.h>

namespace hbmpc {

// device-constant-form scalars every element-wise kernel may need
struct ElemConsts {
    uint32_t r2[9];     // R^2 mod r  (mont(x, r2) = x*R: canonical -> Montgomery)
    uint32_t c0[9];     // kernel-specific constant 0 (e.g. 2^m, (2^m)^-1) in device-constant form
    uint32_t c1[9];     // kernel-specific constant 1 (e.g. 2^(k-1) as a canonical element in limb form)
};
// the one field element of k_scalarop: it travels in the kernel arguments
struct ScalarArg {
    alignas(16) uint32_t w[8];  // canonical element (Goldilocks: the first two words)
};

}  // namespace hbmpc
