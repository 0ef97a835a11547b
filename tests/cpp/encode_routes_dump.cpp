// The encode route planner (mpc-protocols_amd/csrc/encode_route.hpp) on the CPU: one query per stdin line
//   <call> <knobs> <field> <G> <n> <d> <parties>
// call: shares (chunk-major; parties > 1: vandermonde_apply_parties), strided (chunk-major, an output row stride), rows, lists
// (rows writing the producers' lists), triple, triple_ws (triple with a workspace).  knobs: a comma-separated list of the knob
// settings the tests use (default, mc0 .. mc3, min<N>, generic, fusion0, small0, wgs8).  field: fr, sat32, gl.
// One line out per query: the first route, "kernel M=<d + 1> rows=<rows per role> roles=<roles> <one|per-party>" (a route through
// the workspace names the chunk-major route it continues with after '>'), then " lists_in_kernel=<0|1>" for lists calls and
// " all=" with every candidate in order.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../mpc-protocols_amd/csrc/encode_route.hpp"

using namespace hbmpc;

static const char* kernel_name(EncodeKernel k) {
    switch (k) {
    case EncodeKernel::WideDot: return "WideDot";
    case EncodeKernel::Wide: return "Wide";
    case EncodeKernel::MfmaRowsTeam: return "MfmaRowsTeam";
    case EncodeKernel::MfmaRows: return "MfmaRows";
    case EncodeKernel::Bfly: return "Bfly";
    case EncodeKernel::BflyParties: return "BflyParties";
    case EncodeKernel::BflyLists: return "BflyLists";
    case EncodeKernel::BflyTriple: return "BflyTriple";
    case EncodeKernel::MfmaRowsGl: return "MfmaRowsGl";
    case EncodeKernel::Fft1: return "Fft1";
    case EncodeKernel::Fft1Mix: return "Fft1Mix";
    case EncodeKernel::Fft1Triple: return "Fft1Triple";
    case EncodeKernel::FftP: return "FftP";
    case EncodeKernel::Transpose: return "Transpose";
    case EncodeKernel::LocalProduct: return "LocalProduct";
    case EncodeKernel::Generic: return "Generic";
    }
    return "?";
}
static bool is_mfma(EncodeKernel k) {
    return k == EncodeKernel::MfmaRowsTeam || k == EncodeKernel::MfmaRows || k == EncodeKernel::Bfly || k == EncodeKernel::BflyParties ||
           k == EncodeKernel::BflyLists || k == EncodeKernel::BflyTriple;
}
static std::string describe(const EncodeKnobs& k, const EncodeShape& s, const EncodeRoute& r) {
    char buf[160];
    const bool mf = is_mfma(r.kernel);
    const bool one = r.kernel == EncodeKernel::BflyParties || r.kernel == EncodeKernel::BflyTriple || r.kernel == EncodeKernel::BflyLists ||
                     !(mf || r.kernel == EncodeKernel::MfmaRowsGl) || s.parties == 1;
    snprintf(buf, sizeof buf, "%s M=%zu rows=%d roles=%d %s", kernel_name(r.kernel), s.d + 1, mf ? r.plan.role[0].nrows : 0, mf ? r.plan.nroles : 0,
             one ? "one" : "per-party");
    std::string out = buf;
    if (r.kernel == EncodeKernel::Transpose || r.kernel == EncodeKernel::LocalProduct) {
        EncodeShape cm{EncodeKind::ChunkMajor, s.G, s.n, s.d, s.parties};
        out += ">" + describe(k, cm, plan_encode(k, cm).route[0]);
    }
    return out;
}

int main() {
    char call[32], knobs[128], field[16];
    size_t G, n, d, parties;
    while (scanf("%31s %127s %15s %zu %zu %zu %zu", call, knobs, field, &G, &n, &d, &parties) == 7) {
        // the defaults of a context on a device with 256 CUs (hbmpc_ctx)
        EncodeKnobs k{IMPL_U29, false, true, true, true, true, 8192, 2049, 4096, 0, 256};
        k.impl = !strcmp(field, "gl") ? IMPL_GOLD : !strcmp(field, "sat32") ? IMPL_SAT32 : IMPL_U29;
        for (char* tok = strtok(knobs, ","); tok; tok = strtok(nullptr, ",")) {
            if (!strncmp(tok, "mc", 2)) {  // hbmpc_set_matrix_cores(on, 0)
                const int on = atoi(tok + 2);
                k.matrix_cores = on != 0, k.mfma_team = on != 2, k.mfma_bfly = on != 3;
            } else if (!strncmp(tok, "min", 3) && atoi(tok + 3) > 0) {  // hbmpc_set_matrix_cores(.., min_chunks = N)
                const size_t mn = (size_t)atoi(tok + 3);
                k.mfma_min_encode = mn < 2049 ? mn : 2049, k.mfma_min_gold = mn < 4096 ? mn : 4096;
            } else if (!strcmp(tok, "generic")) {
                k.force_generic = true;
            } else if (!strcmp(tok, "fusion0")) {
                k.list_rows_in_kernel = false;
            } else if (!strcmp(tok, "small0")) {
                k.wide_max_chunks = 0;
            } else if (!strcmp(tok, "wgs8")) {
                k.mfma_wgs = 8;
            } else if (strcmp(tok, "default")) {
                fprintf(stderr, "unknown knob %s\n", tok);
                return 2;
            }
        }
        EncodeShape s{EncodeKind::ChunkMajor, G, n, d, parties};
        const std::string c = call;
        if (c == "strided") s.ys = G + 1;
        if (c == "rows" || c == "lists") s.kind = EncodeKind::Rows, s.lists = c == "lists";
        if (c == "triple" || c == "triple_ws") s.kind = EncodeKind::Triple, s.workspace = c == "triple_ws";
        const EncodePlan p = plan_encode(k, s);
        std::string line = describe(k, s, p.route[0]);
        if (s.lists) line += std::string(" lists_in_kernel=") + (encode_lists_in_kernel(k, G, n, d) ? "1" : "0");
        line += " all=";
        for (int i = 0; i < p.count; ++i) line += std::string(i ? "," : "") + kernel_name(p.route[i].kernel);
        printf("%s\n", line.c_str());
    }
    return 0;
}
