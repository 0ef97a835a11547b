// The PRandBit / PRandInt calls' planner (mpc-protocols_amd/csrc/prandbit_route.hpp) on the CPU: one query per stdin line
//   <call> <knobs> <field> <chunks> <n> <t> <open_senders>
// call: prandbit, prandint.  knobs: a comma-separated list of default, generic, single0 (the Goldilocks context's
// hbmpc_set_single_launch_decode(0)) and max<N> (hbmpc_set_fused_prandbit).  field: fr, sat32 (the Fr context's implementation).
// chunks: B = chunks (t + 1) elements per party.  One line out per query:
//   "<one|launches> chunks=<workgroups> senders=<of the open> lds=<bytes of the layout, 0 outside the kernel's range> ks=<slices>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../mpc-protocols_amd/csrc/prandbit_route.hpp"

using namespace hbmpc;

static size_t binomial(size_t n, size_t t) {
    unsigned __int128 c = 1;
    for (size_t k = 1; k <= t; ++k) c = c * (n - t + k) / k;
    return (size_t)c;
}

int main() {
    char call[32], knobs[128], field[16];
    size_t chunks, n, t, S;
    while (scanf("%31s %127s %15s %zu %zu %zu %zu", call, knobs, field, &chunks, &n, &t, &S) == 7) {
        PRandBitKnobs k{!strcmp(field, "sat32") ? IMPL_SAT32 : IMPL_U29, false, true, 256};
        for (char* tok = strtok(knobs, ","); tok; tok = strtok(nullptr, ",")) {
            bool known = !strcmp(tok, "default");
            if (!strcmp(tok, "generic")) k.force_generic = known = true;
            if (!strcmp(tok, "single0")) k.direct_fail = false, known = true;
            if (!strncmp(tok, "max", 3)) k.fused_prandbit_max = strtoull(tok + 3, nullptr, 10), known = true;
            if (!known) {
                fprintf(stderr, "unknown knob %s\n", tok);
                return 2;
            }
        }
        const bool bit = !strcmp(call, "prandbit");
        if (!bit && strcmp(call, "prandint")) {
            fprintf(stderr, "unknown call %s\n", call);
            return 2;
        }
        if (t > n) {
            fprintf(stderr, "t > n\n");
            return 2;
        }
        const size_t Tn = binomial(n, t);
        const PRandBitPlan p = plan_prandbit(k, PRandBitShape{bit, chunks * (t + 1), n, t, Tn, S});
        printf("%s chunks=%zu senders=%zu lds=%zu ks=%d\n", p.one_launch ? "one" : "launches", p.chunks, p.senders, p.lds_bytes,
               p.lds_bytes ? PRandBitWgLds(n, t, Tn).ks : 0);
    }
    return 0;
}
