// The pruned FFT's compile-time bookkeeping (mpc-protocols_amd/csrc/fft_bounds.hpp) on the CPU: one query per stdin line
//   <LOG> <CNT> <LBU0> <VB0>
// First the constants the lazy arithmetic rests on, whatever the queries:
//   const <name> <9 limbs, hex>      U_MOD and U_SUBC2 .. U_SUBC64 of fr_consts.h
//   subk <vb> <K>                    sub_k(vb), vb = 0 .. 65
// then per query
//   query <LOG> <CNT> <LBU0> <VB0>
//   bd <stage> <idx> <lbu> <vb>      fft_bd for every stage 0 .. LOG and idx < 2^LOG
//   bitrev <p> <bitrev_c(LOG, p)>    for every p < 2^LOG
// tests/fft_model.py takes every decision from these lines and restates none of them.
#include <stdio.h>

#include "../../mpc-protocols_amd/csrc/fft_bounds.hpp"
#include "../../mpc-protocols_amd/csrc/fr_consts.h"

using namespace hbmpc;

static void limbs(const char* name, const uint32_t (&v)[9]) {
    printf("const %s", name);
    for (int i = 0; i < 9; ++i) printf(" %08x", v[i]);
    printf("\n");
}

int main() {
    limbs("U_MOD", consts::U_MOD);
    limbs("U_SUBC2", consts::U_SUBC2);
    limbs("U_SUBC4", consts::U_SUBC4);
    limbs("U_SUBC8", consts::U_SUBC8);
    limbs("U_SUBC16", consts::U_SUBC16);
    limbs("U_SUBC32", consts::U_SUBC32);
    limbs("U_SUBC64", consts::U_SUBC64);
    for (int vb = 0; vb <= 65; ++vb) printf("subk %d %d\n", vb, sub_k(vb));
    int LOG, CNT, LBU0, VB0;
    while (scanf("%d %d %d %d", &LOG, &CNT, &LBU0, &VB0) == 4) {
        if (LOG < 0 || LOG > 4 || CNT < 1 || CNT > (1 << LOG) || LBU0 < 1 || VB0 < 1) {
            fprintf(stderr, "bad query %d %d %d %d\n", LOG, CNT, LBU0, VB0);
            return 2;
        }
        printf("query %d %d %d %d\n", LOG, CNT, LBU0, VB0);
        for (int stage = 0; stage <= LOG; ++stage)
            for (int idx = 0; idx < (1 << LOG); ++idx) {
                const Bd b = fft_bd(LOG, CNT, LBU0, VB0, stage, idx);
                printf("bd %d %d %d %d\n", stage, idx, b.lbu, b.vb);
            }
        for (int p = 0; p < (1 << LOG); ++p) printf("bitrev %d %d\n", p, bitrev_c(LOG, p));
    }
    return 0;
}
