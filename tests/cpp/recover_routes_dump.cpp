// The decode route planner (mpc-protocols_amd/csrc/recover_route.hpp) on the CPU: one query per stdin line
//   <call> <knobs> <field> <G> <n> <d> <t> <S> <facts>
// call: dev (a device-pointer call), host (a host-pointer call), p0, p0_host, coeff<k> (P(0)-shaped, coefficient k), top<k>_group<g>
// (coefficient k, groups of g chunks), sel<a>_<b> (select-two: coefficients a and b), sel<a>_<b>_group<g>, slots, pair<N> (the fpmul
// pair form over N elements per half), interp, interp_deg, interp_c0 (batch_interpolate_dev without / with degrees / with c0 and
// degrees; S points of n, G chunks).  knobs: a comma-separated list of the knob settings the tests use (default, mc0 .. mc2, min<N>,
// generic, small0, wgs8, single0, second0, lazy0 .. lazy2, fusion0).  field: fr, sat32, gl.  facts: a comma-separated list of
// capturing, cached, or "-".
// One line out per query: "notfused-early", "notfused", "single-invalid", or the plan:
//   "<first> M=<d + 1> rows=<rows per role, comma-separated> roles=<n> <one|tail> rmax=<r> second=<none|kernel|m|generic>
//    tables=<eager|lazy> gao=<inline|unscale|none> all=<every candidate in order>"
// (the tail fields name what follows a first route that is not one launch; "all=" is empty when no route is planned).
// Interpolation: "<first> all=<every candidate> c0_only=<0|1>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../mpc-protocols_amd/csrc/recover_route.hpp"

using namespace hbmpc;

static const char* kernel_name(RecoverKernel k) {
    switch (k) {
    case RecoverKernel::MfmaRowsSub: return "MfmaRowsSub";
    case RecoverKernel::MfmaRowsGl: return "MfmaRowsGl";
    case RecoverKernel::MfmaRowsTeam: return "MfmaRowsTeam";
    case RecoverKernel::MfmaRows: return "MfmaRows";
    case RecoverKernel::Wide: return "Wide";
    case RecoverKernel::RecoverM: return "RecoverM";
    case RecoverKernel::GoldRecoverM: return "GoldRecoverM";
    case RecoverKernel::Generic: return "Generic";
    }
    return "?";
}
static const char* interp_name(InterpKernel k) {
    switch (k) {
    case InterpKernel::IdftDegrees: return "IdftDegrees";
    case InterpKernel::Idft: return "Idft";
    case InterpKernel::Decode: return "Decode";
    }
    return "?";
}

static std::string describe(const RecoverShape& s, const RecoverPlan& p) {
    std::string all;
    for (int i = 0; i < p.count; ++i) all += std::string(i ? "," : "") + kernel_name(p.route[i].kernel);
    char buf[256];
    if (p.count == 0) {
        snprintf(buf, sizeof buf, "none rmax=%zu all=", p.rmax);
        return buf;
    }
    const RecoverRoute& r = p.route[0];
    const bool roles = r.kernel == RecoverKernel::MfmaRowsSub || r.kernel == RecoverKernel::MfmaRowsTeam || r.kernel == RecoverKernel::MfmaRows;
    std::string rows;
    for (int i = 0; roles && i < r.plan.nroles; ++i) rows += (i ? "," : "") + std::to_string(r.plan.role[i].nrows);
    const char* second = !p.second ? "none" : r.second_in_kernel ? "kernel" : p.second_kernel == SecondKernel::M ? "m" : "generic";
    const char* gao = r.one_launch ? "none" : p.gao_inline ? "inline" : "unscale";
    snprintf(buf, sizeof buf, "%s M=%zu rows=%s roles=%d %s rmax=%zu second=%s tables=%s gao=%s all=%s", kernel_name(r.kernel), s.d + 1,
             rows.empty() ? "0" : rows.c_str(), roles ? r.plan.nroles : 0, r.one_launch ? "one" : "tail", p.rmax, second,
             p.lazy ? "lazy" : "eager", gao, all.c_str());
    return buf;
}

int main() {
    char call[64], knobs[128], field[16], factstr[64];
    size_t G, n, d, t, S;
    while (scanf("%63s %127s %15s %zu %zu %zu %zu %zu %63s", call, knobs, field, &G, &n, &d, &t, &S, factstr) == 9) {
        // the defaults of a context on a device with 256 CUs (hbmpc_ctx)
        RecoverKnobs k{IMPL_U29, false, true, true, true, true, true, true, 1, 8192, 4096, 2048, 2048, 8193, 0, 256};
        k.impl = !strcmp(field, "gl") ? IMPL_GOLD : !strcmp(field, "sat32") ? IMPL_SAT32 : IMPL_U29;
        for (char* tok = strtok(knobs, ","); tok; tok = strtok(nullptr, ",")) {
            if (!strncmp(tok, "mc", 2)) {  // hbmpc_set_matrix_cores(on, 0)
                const int on = atoi(tok + 2);
                k.matrix_cores = on != 0, k.mfma_team = on != 2, k.mfma_bfly = on != 3;
            } else if (!strncmp(tok, "min", 3) && atoi(tok + 3) > 0) {  // hbmpc_set_matrix_cores(.., min_chunks = N)
                const size_t mn = (size_t)atoi(tok + 3);
                k.mfma_min_cached = mn < 4096 ? mn : 4096, k.mfma_min_direct = k.mfma_min_gold_direct = mn < 2048 ? mn : 2048;
                k.mfma_min_gold_oec = mn < 8193 ? mn : 8193;
            } else if (!strcmp(tok, "generic")) {
                k.force_generic = true;
            } else if (!strcmp(tok, "small0")) {
                k.wide_max_chunks = 0;
            } else if (!strcmp(tok, "wgs8")) {
                k.mfma_wgs = 8;
            } else if (!strcmp(tok, "single0")) {
                k.direct_fail = false;
            } else if (!strcmp(tok, "second0")) {
                k.second_chance = false;
            } else if (!strncmp(tok, "lazy", 4)) {
                k.lazy_fallback_tables = atoi(tok + 4);
            } else if (!strcmp(tok, "fusion0")) {
                k.list_rows_in_kernel = false;
            } else if (strcmp(tok, "default")) {
                fprintf(stderr, "unknown knob %s\n", tok);
                return 2;
            }
        }
        RecoverFacts f;
        f.capturing = strstr(factstr, "capturing") != nullptr;
        f.fallback_cached = strstr(factstr, "cached") != nullptr;
        const std::string c = call;
        if (c.rfind("interp", 0) == 0) {
            const InterpPlan p = plan_interpolate(k, G, n, S, 0, c != "interp", c == "interp_c0");
            std::string all;
            for (int i = 0; i < p.count; ++i) all += std::string(i ? "," : "") + interp_name(p.route[i]);
            printf("%s all=%s c0_only=%d\n", interp_name(p.route[0]), all.c_str(), p.c0_only ? 1 : 0);
            continue;
        }
        RecoverShape s{G, n, d, t, S};
        s.host_call = c == "host" || c == "p0_host";
        s.p0 = c == "p0" || c == "p0_host" || c.rfind("coeff", 0) == 0 || c.rfind("top", 0) == 0 || c.rfind("pair", 0) == 0;
        s.slots = c == "slots";
        int a = 0, b = 0, g = 0;
        if (sscanf(call, "coeff%d", &a) == 1) s.only_coeff = a;
        if (sscanf(call, "top%d_group%d", &a, &g) == 2) s.only_coeff = a, s.group = (size_t)g;
        if (sscanf(call, "sel%d_%d", &a, &b) == 2) s.only_coeff = a, s.second_coeff = b;
        if (sscanf(call, "sel%d_%d_group%d", &a, &b, &g) == 3) s.group = (size_t)g;
        if (sscanf(call, "pair%d", &a) == 1) s.pair = true, s.pair_N = (size_t)a;
        if (recover_cover(k, s, true) != RecoverCover::Run) {
            printf("notfused-early\n");
            continue;
        }
        const RecoverCover cv = recover_cover(k, s, false);
        if (cv != RecoverCover::Run) {
            printf("%s\n", cv == RecoverCover::NotFused ? "notfused" : "single-invalid");
            continue;
        }
        printf("%s\n", describe(s, plan_recover(k, s, f)).c_str());
    }
    return 0;
}
