// The launch parameters of k_batch_recover_wide (mpc-protocols_amd/csrc/wide_plan.hpp) on the CPU: one query per stdin line
//   <field> <needed> <m> <p0> <ow_sel> <contiguous> <aligned>
// field: fr (u29), sat32, gl; the others are integers (p0, contiguous, aligned: 0 or 1).  One line out per query:
//   <lds bytes> <tab_words> <split> <lk>
// tests/decode_inputs.py derives the rows per sweep, the terms per lane and which staging loops run from these numbers and restates
// nothing of the rule.
#include <stdio.h>
#include <string.h>

#include "../../mpc-protocols_amd/csrc/wide_plan.hpp"

using namespace hbmpc;

int main() {
    char field[16];
    int needed, m, p0, ow_sel, contiguous, aligned;
    while (scanf("%15s %d %d %d %d %d %d", field, &needed, &m, &p0, &ow_sel, &contiguous, &aligned) == 7) {
        const int impl = !strcmp(field, "gl") ? IMPL_GOLD : !strcmp(field, "sat32") ? IMPL_SAT32 : !strcmp(field, "fr") ? IMPL_U29 : -1;
        if (impl < 0 || m < 1 || needed < m || needed > 255 || ow_sel < 0 || ow_sel > m) {
            fprintf(stderr, "bad query %s %d %d %d %d %d %d\n", field, needed, m, p0, ow_sel, contiguous, aligned);
            return 2;
        }
        const WidePlan w = wide_plan(impl, needed, m, p0 != 0, ow_sel, contiguous != 0, aligned != 0);
        printf("%zu %d %d %d\n", w.lds, w.tab_words, w.split, w.lk);
    }
    return 0;
}
