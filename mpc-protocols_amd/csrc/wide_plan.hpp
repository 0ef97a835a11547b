// wide_plan.hpp -- the launch parameters of k_batch_recover_wide (kernels_recover.hpp) as plain host arithmetic, without a HIP
// include: tu_generic.hip launches with them, tests/cpp/wide_plan_dump.cpp prints them for the CPU tests.
#pragma once
#include <cstddef>

#include "field_dispatch.hpp"  // FieldImpl, impl_nl, impl_ebytes

namespace hbmpc {

struct WidePlan {
    size_t lds;     // LDS bytes of one workgroup (4 chunks): [4][needed] sender values, then the staged table
    int tab_words;  // 0 when the call's table cannot be staged (not contiguous, or beyond what a launch may ask for without raising
                    // the function's limit): the TAB = false instance
    int split;      // the table is staged word by word from two ranges (a single output row that does not follow the verify rows)
    int lk;         // log2 of the lanes that share a row's products (dot_shared): U29, staged table, every row still fits the wave
};
// p0: one output row; ow_sel: output rows per chunk when not all m (0 = m); contiguous: the output rows follow the verify rows in
// memory; aligned: the table starts on 16 bytes
inline WidePlan wide_plan(int impl, int needed, int m, bool p0, int ow_sel, bool contiguous, bool aligned) {
    const size_t ew = impl_ebytes(impl) / 4, nl = (size_t)impl_nl(impl);
    const size_t nv = (size_t)(needed - m), ow = p0 ? 1 : ow_sel ? (size_t)ow_sel : (size_t)m;
    const size_t front = 4 * (size_t)needed * ew * 4;
    const size_t tw = (nv + ow) * (size_t)m * nl;
    const bool fits = front + tw * 4 <= 64 * 1024;
    const bool whole = contiguous && aligned;
    const bool staged = fits && (whole || p0);  // a single output row elsewhere in the table (one coefficient): staged from both ranges
    WidePlan w;
    w.split = staged && !whole ? 1 : 0;
    w.tab_words = staged ? (int)tw : 0;
    w.lds = front + (staged ? tw * 4 : 0);
    w.lk = 0;
    if (staged && impl == IMPL_U29) {  // a row's products shared by up to four lanes while every row still fits the wave
        const int rows = (needed - m) + (p0 ? 1 : ow_sel ? ow_sel : m);
        while (w.lk < 2 && (rows << (w.lk + 1)) <= 64 && (2 << w.lk) <= m) ++w.lk;
    }
    return w;
}

}  // namespace hbmpc
