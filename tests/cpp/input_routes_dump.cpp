// The planner's rule for hbmpc_[gl_]dev_input_parties (mpc-protocols_amd/csrc/protocol_route.hpp, ProtocolCall::Input) on the CPU: one
// query per stdin line
//   <knobs> <field> <N> <n> <t> <S>
// knobs: a comma-separated list of default, generic, single0 and inputmax<N> (hbmpc_set_fused_input).  field: fr, sat32, gl.
// N: elements; S: senders.  One line out per query: "one lk=<lk>" or "launches".  The one argument is a context's default threshold
// (fused_input_max in csrc/hbmpc_capi.hip, which the test reads from there): the planner header holds the rule, not the defaults.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../mpc-protocols_amd/csrc/protocol_route.hpp"

using namespace hbmpc;

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: input_routes_dump <a context's default fused_input_max>\n");
        return 2;
    }
    const size_t input_default = strtoull(argv[1], nullptr, 10);
    char knobs[128], field[16];
    size_t N, n, t, S;
    while (scanf("%127s %15s %zu %zu %zu %zu", knobs, field, &N, &n, &t, &S) == 6) {
        const bool gl = !strcmp(field, "gl");
        ProtocolKnobs k{gl ? IMPL_GOLD : !strcmp(field, "sat32") ? IMPL_SAT32 : IMPL_U29, false, true, 1024, 2048, 768, 1024, gl ? 1024u : 256u, 8192, input_default};
        for (char* tok = strtok(knobs, ","); tok; tok = strtok(nullptr, ",")) {
            bool known = !strcmp(tok, "default");
            if (!strcmp(tok, "generic")) k.force_generic = known = true;
            if (!strcmp(tok, "single0")) k.direct_fail = false, known = true;
            if (!strncmp(tok, "inputmax", 8)) k.fused_input_max = strtoull(tok + 8, nullptr, 10), known = true;
            if (!known) {
                fprintf(stderr, "unknown knob %s\n", tok);
                return 2;
            }
        }
        const ProtocolPlan p = plan_protocol(k, ProtocolShape{ProtocolCall::Input, N, n, t, S, 0});
        if (p.one_launch) printf("one lk=%d\n", p.lk_wave);
        else printf("launches\n");
    }
    return 0;
}
