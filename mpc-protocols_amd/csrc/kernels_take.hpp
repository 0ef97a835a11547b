// kernels_take.hpp -- hbmpc_dev_take_rows: slices of [party][len] pools, regrouped on the way (take_plan.hpp has the tile rule).
//
//   dst[r][j * C + i] = src[r][i * group + j]     i < C = elements / group, j < group, for every row r and slice s
//
// The workgroup (tile, row, slice) owns `tile` consecutive i.  Its source is ONE contiguous run of tile * group elements: it streams
// into LDS with 16-byte loads, and leaves as `group` runs of `tile` elements with 16-byte stores.  Everything is counted in 64-bit
// words (W per element), so a run that starts on an odd word -- an 8-byte element at an odd offset -- moves one word alone at its head
// and tail and whole aligned 16-byte pairs between them; nothing assumes more than the 8-byte alignment the C ABI checks.
// The LDS row of one i is group * W words plus one word of padding: the stores read along i, and an odd pitch keeps those reads on
// different banks.  No atomics, no hand-off between workgroups; a workgroup past its slice's last tile leaves before the barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "take_plan.hpp"

namespace hbmpc {

// LDS words: kTakeRunBytes * kTakeGroupMax bytes of elements and a padding word per i of the longest tile (8-byte elements, a small group)
constexpr unsigned kTakeLdsWords = (unsigned)(kTakeRunBytes * kTakeGroupMax / 8 + kTakeRunBytes / 8 * kTakeSmallGroupRuns);

// A run of `len` words at the 8-byte aligned p is cut into slots: slot 0 = the head word (where p is not 16-byte aligned), slots
// 1 .. pairs = aligned 16-byte pairs, slot pairs + 1 = the tail word.  Returns the first word of the slot and how many it holds (0, 1 or 2).
__device__ __forceinline__ unsigned take_slot(unsigned head, unsigned len, unsigned slot, unsigned* first) {
    const unsigned pairs = (len - head) >> 1;
    if (slot == 0) {
        *first = 0;
        return head;
    }
    if (slot <= pairs) {
        *first = head + 2 * (slot - 1);
        return 2;
    }
    *first = head + 2 * pairs;
    return len - *first;  // slot == pairs + 1: 0 or 1
}

template <int W>
__global__ __launch_bounds__(256) void k_take_rows(const TakeArgs a) {
    __shared__ uint64_t lds[kTakeLdsWords];
    const TakeSliceArg sl = a.s[blockIdx.z];
    const size_t i0 = (size_t)blockIdx.x * sl.tile;
    if (i0 >= sl.C) return;  // the grid's x is the longest slice's
    const size_t r = blockIdx.y;
    const unsigned ni = sl.C - i0 < sl.tile ? (unsigned)(sl.C - i0) : sl.tile;
    const unsigned rowlen = sl.group * W, pitch = rowlen + 1;

    {  // in: word q of the run is word q % rowlen of i = q / rowlen
        const uint64_t* p = sl.src + (r * sl.src_row_stride + i0 * sl.group) * W;
        const unsigned len = ni * rowlen, head = (unsigned)(((uintptr_t)p >> 3) & 1);
        const unsigned slots = ((len - head) >> 1) + 2;
        for (unsigned k = threadIdx.x; k < slots; k += 256) {
            unsigned q;
            const unsigned cnt = take_slot(head, len, k, &q);
            if (cnt == 2) {
                const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p + q);
                lds[q + q / rowlen] = v.x;
                lds[q + 1 + (q + 1) / rowlen] = v.y;
            } else if (cnt == 1) {
                lds[q + q / rowlen] = p[q];
            }
        }
    }
    __syncthreads();
    {  // out: run j holds word k % W of element (i = k / W, j) at its word k
        const unsigned len = ni * W, per_run = (len >> 1) + 2;  // slots of a run, whichever its head
        uint64_t* const d0 = sl.dst + (r * sl.dst_row_stride + i0) * W;
        for (unsigned k = threadIdx.x; k < per_run * sl.group; k += 256) {
            const unsigned j = k / per_run, slot = k - j * per_run;
            uint64_t* p = d0 + (size_t)j * sl.C * W;
            const unsigned head = (unsigned)(((uintptr_t)p >> 3) & 1);
            if (slot > ((len - head) >> 1) + 1) continue;
            unsigned q;
            const unsigned cnt = take_slot(head, len, slot, &q);
            const unsigned at0 = q / W * pitch + j * W + q % W;
            if (cnt == 2) {
                ulonglong2 v;
                v.x = lds[at0];
                v.y = lds[(q + 1) / W * pitch + j * W + (q + 1) % W];
                *reinterpret_cast<ulonglong2*>(p + q) = v;
            } else if (cnt == 1) {
                p[q] = lds[at0];
            }
        }
    }
}

}  // namespace hbmpc
