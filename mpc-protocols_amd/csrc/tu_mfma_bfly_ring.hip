// tu_mfma_bfly_ring.hip -- instantiations of k_mfma_bfly_ring (kernels_mfma_bfly_ring.hpp): the plain chunk-major encode with one role
// of 4 or 8 pairs whose table and ring fit the LDS (bfly_ring_plan.hpp)
#include <utility>

#include "kernels_mfma_bfly_ring.hpp"
#include "launchers.hpp"
namespace hbmpc {
namespace {
template <int M, int NP>
bool launch(const mf::MfmaRowsArgs& a, int device, hipStream_t s) {
    if constexpr (mf::bfly_ring_fits(M, NP)) {
        constexpr mf::BflyRingShape R = mf::BFLY_RING_LIB;
        const size_t lds = mf::bfly_ring_lds_bytes(M, NP, R.slots);
        static std::atomic<bool> attr_set[HBMPC_MAX_DEVICES];
        if (!ensure_dynamic_lds(reinterpret_cast<const void*>(&mf::k_mfma_bfly_ring<M, R.cw, NP, R.slots, R.depth>), attr_set, device, lds)) return false;
        hipLaunchKernelGGL((mf::k_mfma_bfly_ring<M, R.cw, NP, R.slots, R.depth>), dim3((unsigned)mf::mf_grid(a)), dim3(64 * (R.cw + 1)), lds, s, a);
        return true;
    }
    return false;
}
template <int M>
bool one(const mf::MfmaRowsArgs& a, int device, hipStream_t s) {
    if (a.role[0].nrows == 8) return launch<M, 8>(a, device, s);
    if (a.role[0].nrows == 4) return launch<M, 4>(a, device, s);
    return false;
}
template <int LO, int... I>
bool range(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s, std::integer_sequence<int, I...>) {
    bool hit = false;
    ((m == LO + I ? (hit = one<LO + I>(a, device, s)) : false), ...);
    return hit;
}
}  // namespace
bool launch_mfma_bfly_ring(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s) {
    // chunk-major inputs, plain outputs, one role: not the rows, TRIPLE, DEG or LISTS instances
    if (!a.in_chunk_major || a.in_b || a.ncoeffs || a.list_rows || a.other_stride || a.nroles != 1 || a.G == 0) return false;
    return range<2>(m, a, device, s, std::make_integer_sequence<int, mf::BFLY_RING_MAX_M - 1>{});
}
}  // namespace hbmpc
