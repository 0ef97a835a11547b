// TruncPrNode / FPDivConstNode for all parties of a small batch in one launch (kernels_truncpr_wave.hpp)
#include <hip/hip_runtime.h>

#include "fr_u29.hpp"
#include "kernels_truncpr_wave.hpp"
#include "launchers.hpp"

namespace hbmpc {
template <bool HAS_W>
static bool launch_one(const TruncprWaveArgs& a, int device, hipStream_t s, size_t lds, bool dry_run) {
    static std::atomic<bool> attr_set[HBMPC_MAX_DEVICES];
    if (!ensure_dynamic_lds(reinterpret_cast<const void*>(&k_truncpr_wave<U29, HAS_W>), attr_set, device, lds)) return false;
    if (!dry_run) hipLaunchKernelGGL((k_truncpr_wave<U29, HAS_W>), dim3((unsigned)((a.N + 3) / 4)), dim3(256), lds, s, a);
    return true;
}
bool launch_truncpr_wave(const TruncprWaveArgs& a, int device, hipStream_t s, bool dry_run) {
    const int nv = a.needed - a.M;
    const TruncprWaveLds L(a.parties, a.m, (nv + 1) * a.M * 9);
    const size_t lds = L.total * 4;
    if (lds > 160 * 1024) return false;
    return a.w ? launch_one<true>(a, device, s, lds, dry_run) : launch_one<false>(a, device, s, lds, dry_run);
}
}  // namespace hbmpc
