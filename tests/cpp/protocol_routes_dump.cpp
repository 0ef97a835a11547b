// The protocol calls' planner (mpc-protocols_amd/csrc/protocol_route.hpp) on the CPU: one query per stdin line
//   <call> <knobs> <field> <N> <n> <t> <S> <m>
// call: triplegen, fpmul, truncpr, mul, randbit.  knobs: a comma-separated list of default, generic, single0 and <call>max<N> (the
// hbmpc_set_fused_<call> setters).  field: fr, sat32, gl.  N: elements per party; S and m are read by the calls that have them.
// One line out per query: "one" (TripleGen, RandBit), "one lk=<lk>" (TruncPr, Mul), "one lk=<lk1> lk3=<lk3>" (FPMul), or
// "launches pair=<0|1>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../mpc-protocols_amd/csrc/protocol_route.hpp"

using namespace hbmpc;

int main() {
    static const char* const names[5] = {"triplegen", "fpmul", "truncpr", "mul", "randbit"};
    char call[32], knobs[128], field[16];
    size_t N, n, t, S, m;
    while (scanf("%31s %127s %15s %zu %zu %zu %zu %zu", call, knobs, field, &N, &n, &t, &S, &m) == 8) {
        // the defaults of a context (hbmpc_ctx; hbmpc_create sets the RandBit threshold per field)
        const bool gl = !strcmp(field, "gl");
        ProtocolKnobs k{gl ? IMPL_GOLD : !strcmp(field, "sat32") ? IMPL_SAT32 : IMPL_U29, false, true, 1024, 2048, 768, 1024, gl ? 1024u : 256u, 8192};
        size_t* const maxes[5] = {&k.fused_triplegen_max, &k.fused_fpmul_max, &k.fused_truncpr_max, &k.fused_mul_max, &k.fused_randbit_max};
        for (char* tok = strtok(knobs, ","); tok; tok = strtok(nullptr, ",")) {
            bool known = !strcmp(tok, "default");
            if (!strcmp(tok, "generic")) k.force_generic = known = true;
            if (!strcmp(tok, "single0")) k.direct_fail = false, known = true;
            for (int i = 0; i < 5; ++i) {
                const size_t len = strlen(names[i]);
                if (!strncmp(tok, names[i], len) && !strncmp(tok + len, "max", 3)) *maxes[i] = strtoull(tok + len + 3, nullptr, 10), known = true;
            }
            if (!known) {
                fprintf(stderr, "unknown knob %s\n", tok);
                return 2;
            }
        }
        int c = 0;
        while (c < 5 && strcmp(call, names[c])) ++c;
        if (c == 5) {
            fprintf(stderr, "unknown call %s\n", call);
            return 2;
        }
        const ProtocolCall pc = (ProtocolCall)c;
        const ProtocolPlan p = plan_protocol(k, ProtocolShape{pc, N, n, t, S, m});
        if (!p.one_launch) printf("launches pair=%d\n", p.pair_first ? 1 : 0);
        else if (pc == ProtocolCall::FpMul) printf("one lk=%d lk3=%d\n", p.lk_row, p.lk_wave);
        else if (pc == ProtocolCall::TruncPr) printf("one lk=%d\n", p.lk_wave);
        else if (pc == ProtocolCall::Mul) printf("one lk=%d\n", p.lk_row);
        else printf("one\n");
    }
    return 0;
}
