// The planner's rules on the CPU (mpc-protocols_amd/csrc/protocol_route.hpp): one query per stdin line, either
//   batchrecon <knobs> <field> <N> <n> <t> <d> <S1> <S2>   plan_batchrecon, the rule of hbmpc_[gl_]dev_batchrecon_parties
//   <call> <knobs> <field> <N> <n> <t> <S> <m>             plan_protocol: a query of tests/cpp/protocol_routes_dump.cpp, answered as there
// knobs: a comma-separated list of default, generic, single0, batchreconmax<G> (hbmpc_set_fused_batchrecon) and that tool's
// <call>max<N>.  field: fr, sat32, gl.  One line out per query; batchrecon: "one lk=<lk>" or "launches lk=<lk>", lk the EvalBatch arm's
// lane share.  The one argument is a context's default threshold (FUSED_BATCHRECON_FR / _GL in csrc/hbmpc_capi.hip, which the test
// reads from there), as "<fr>,<gl>": the planner header holds the rule, not the defaults.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../mpc-protocols_amd/csrc/protocol_route.hpp"

using namespace hbmpc;

int main(int argc, char** argv) {
    size_t def_fr = 0, def_gl = 0;
    if (argc != 2 || sscanf(argv[1], "%zu,%zu", &def_fr, &def_gl) != 2) {
        fprintf(stderr, "usage: batchrecon_routes_dump <default fused_batchrecon_max over Fr>,<over Goldilocks>\n");
        return 2;
    }
    static const char* const names[5] = {"triplegen", "fpmul", "truncpr", "mul", "randbit"};
    char call[32], knobs[128], field[16];
    while (scanf("%31s %127s %15s", call, knobs, field) == 3) {
        const bool gl = !strcmp(field, "gl");
        ProtocolKnobs k{gl ? IMPL_GOLD : !strcmp(field, "sat32") ? IMPL_SAT32 : IMPL_U29, false, true, 1024, 2048, 768, 1024, gl ? 1024u : 256u, 8192};
        size_t brmax = gl ? def_gl : def_fr;
        size_t* const maxes[5] = {&k.fused_triplegen_max, &k.fused_fpmul_max, &k.fused_truncpr_max, &k.fused_mul_max, &k.fused_randbit_max};
        for (char* tok = strtok(knobs, ","); tok; tok = strtok(nullptr, ",")) {
            bool known = !strcmp(tok, "default");
            if (!strcmp(tok, "generic")) k.force_generic = known = true;
            if (!strcmp(tok, "single0")) k.direct_fail = false, known = true;
            if (!strncmp(tok, "batchreconmax", 13)) brmax = strtoull(tok + 13, nullptr, 10), known = true;
            for (int i = 0; i < 5; ++i) {
                const size_t len = strlen(names[i]);
                if (!strncmp(tok, names[i], len) && !strncmp(tok + len, "max", 3)) *maxes[i] = strtoull(tok + len + 3, nullptr, 10), known = true;
            }
            if (!known) {
                fprintf(stderr, "unknown knob %s\n", tok);
                return 2;
            }
        }
        if (!strcmp(call, "batchrecon")) {
            size_t N, n, t, d, S1, S2;
            if (scanf("%zu %zu %zu %zu %zu %zu", &N, &n, &t, &d, &S1, &S2) != 6) return 2;
            const BatchReconPlan p = plan_batchrecon(k, brmax, BatchReconShape{N, n, t, d, S1, S2});
            printf("%s lk=%d\n", p.one_launch ? "one" : "launches", p.lk_eval);
            continue;
        }
        int c = 0;
        while (c < 5 && strcmp(call, names[c])) ++c;
        size_t N, n, t, S, m;
        if (c == 5 || scanf("%zu %zu %zu %zu %zu", &N, &n, &t, &S, &m) != 5) {
            fprintf(stderr, "bad query %s\n", call);
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
