// The planner's rule for the producers' device calls on the CPU (mpc-protocols_amd/csrc/protocol_route.hpp, plan_producers): one query per
// stdin line,
//   <ransha|randousha> <knobs> <field> <K> <n> <t> <S>
// knobs: a comma-separated list of default, generic, single0, producersmax<K> (hbmpc_set_fused_producers).  field: fr, sat32, gl.
// One line out per query: "one" or "launches".  The one argument is a context's default threshold (FUSED_PRODUCERS_FR / _GL in
// csrc/hbmpc_capi.hip, which the test reads from there), as "<fr>,<gl>": the planner header holds the rule, not the defaults.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../mpc-protocols_amd/csrc/protocol_route.hpp"

using namespace hbmpc;

int main(int argc, char** argv) {
    size_t def_fr = 0, def_gl = 0;
    if (argc != 2 || sscanf(argv[1], "%zu,%zu", &def_fr, &def_gl) != 2) {
        fprintf(stderr, "usage: producers_routes_dump <default fused_producers_max over Fr>,<over Goldilocks>\n");
        return 2;
    }
    char call[32], knobs[128], field[16];
    size_t K, n, t, S;
    while (scanf("%31s %127s %15s %zu %zu %zu %zu", call, knobs, field, &K, &n, &t, &S) == 7) {
        const bool gl = !strcmp(field, "gl");
        ProtocolKnobs k{gl ? IMPL_GOLD : !strcmp(field, "sat32") ? IMPL_SAT32 : IMPL_U29, false, true, 1024, 2048, 768, 1024, gl ? 1024u : 256u, 8192};
        size_t mx = gl ? def_gl : def_fr;
        for (char* tok = strtok(knobs, ","); tok; tok = strtok(nullptr, ",")) {
            bool known = !strcmp(tok, "default");
            if (!strcmp(tok, "generic")) k.force_generic = known = true;
            if (!strcmp(tok, "single0")) k.direct_fail = false, known = true;
            if (!strncmp(tok, "producersmax", 12)) mx = strtoull(tok + 12, nullptr, 10), known = true;
            if (!known) {
                fprintf(stderr, "unknown knob %s\n", tok);
                return 2;
            }
        }
        const bool dou = !strcmp(call, "randousha");
        if (!dou && strcmp(call, "ransha")) {
            fprintf(stderr, "bad query %s\n", call);
            return 2;
        }
        const ProducersPlan p = plan_producers(k, mx, ProducersShape{dou ? ProducerCall::RanDouSha : ProducerCall::RanSha, K, n, t, S});
        printf("%s\n", p.one_launch ? "one" : "launches");
    }
    return 0;
}
