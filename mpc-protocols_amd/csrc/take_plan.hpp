// take_plan.hpp -- which route a slice of hbmpc_dev_take_rows takes and the tile it moves: plain C++ (no HIP), so that the rule is read by
// the launcher (tu_take.hip), by the C ABI (hbmpc_capi.hip) and by a CPU test (tests/cpp/take_routes_dump.cpp) from one place.
//
// A slice regroups dst[r][j * C + i] = src[r][i * group + j] (C = elements / group).  The take kernel (kernels_take.hpp) gives a workgroup
// `tile` consecutive i: a contiguous source run of tile * group elements goes through LDS and leaves as `group` runs of `tile` elements.
// The LDS holds kTakeRunBytes * kTakeGroupMax bytes of elements, so
//   tile = (kTakeRunBytes / element bytes) * min(kTakeSmallGroupRuns, kTakeGroupMax / group)     (16 or 64 elements: runs of 512 bytes;
//                                                                                                a small group: up to 8 such runs)
// and a group beyond kTakeGroupMax takes the transpose kernel (k_transpose, a 16 x 64 tile), slice by slice.  Both routes write the
// same bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hbmpc {

constexpr size_t kTakeSlicesMax = 8;       // slices of one call: they travel in the kernel arguments
constexpr size_t kTakeGroupMax = 64;       // the largest group the take kernel's tile holds
constexpr size_t kTakeRunBytes = 512;      // the shortest run a full tile writes
constexpr size_t kTakeSmallGroupRuns = 8;  // a tile of a small group is up to this many runs long
constexpr size_t kTakeRowsMax = 65535;     // rows ride in the launch grid's y

struct TakePlan {
    bool transpose;  // true: launch_transpose for this slice
    size_t tile;     // the take kernel's i per workgroup (0 on the transpose route)
};

inline TakePlan plan_take(size_t element_bytes, size_t group) {
    if (group > kTakeGroupMax) return TakePlan{true, 0};
    size_t runs = kTakeGroupMax / group;
    if (runs > kTakeSmallGroupRuns) runs = kTakeSmallGroupRuns;
    return TakePlan{false, kTakeRunBytes / element_bytes * runs};
}

// The call's argument checks, in the order the header gives: null when the arguments pass, else what is wrong.  Pure functions of the
// arguments -- no device is touched -- so that the refusals are tested on the CPU too.
inline const char* check_take_call(bool has_slices, size_t count, size_t rows) {
    if (!has_slices || count == 0 || count > kTakeSlicesMax) return "1 to 8 slices";
    if (rows == 0 || rows > kTakeRowsMax) return "1 to 65535 rows";
    return nullptr;
}
inline const char* check_take_slice(const void* src, size_t src_row_stride, const void* dst, size_t dst_row_stride, size_t elements, size_t group) {
    constexpr size_t kMax = (size_t)1 << 40;
    if (!src || !dst || (((uintptr_t)src | (uintptr_t)dst) & 7)) return "null or misaligned buffer";
    if (elements == 0 || group == 0 || elements % group != 0) return "elements must be a positive multiple of group";
    if (src_row_stride < elements || dst_row_stride < elements) return "row stride below the row length";
    if (elements > ((size_t)1 << 31) || src_row_stride > kMax || dst_row_stride > kMax) return "slice beyond 2^31 elements or stride beyond 2^40";
    return nullptr;
}

// what the kernel gets, by value in its arguments (the decode kernels pass their RowsArg the same way)
struct TakeSliceArg {
    const uint64_t* src;
    uint64_t* dst;
    size_t src_row_stride, dst_row_stride;  // elements
    size_t C;                               // elements / group
    uint32_t group, tile;                   // tile: plan_take's
};
struct TakeArgs {
    TakeSliceArg s[kTakeSlicesMax];
};

}  // namespace hbmpc
