// The take planner's rule on the CPU (mpc-protocols_amd/csrc/take_plan.hpp): one query "<element bytes> <group>" per stdin line, one
// line out per query: "take tile=<i per workgroup>" or "transpose".  With the argument "limits" it prints the header's constants instead:
// "<slices max> <group max> <rows max> <LDS bytes a tile needs at most>", and with "check" it answers argument checks: one query
// "<has slices> <count> <rows> <src> <src stride> <dst> <dst stride> <elements> <group>" per line (pointers as integers) -> "ok" or
// "refused: <why>" -- the call's checks first, then the slice's, as hbmpc_dev_take_rows applies them.
#include <stdio.h>
#include <string.h>

#include "../../mpc-protocols_amd/csrc/take_plan.hpp"

using namespace hbmpc;

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "limits")) {
        size_t worst = 0;
        for (size_t eb = 8; eb <= 32; eb += 24)
            for (size_t g = 1; g <= kTakeGroupMax; ++g) {
                const size_t bytes = plan_take(eb, g).tile * (g * eb + 8);  // an LDS row is one i: group elements and a padding word
                if (bytes > worst) worst = bytes;
            }
        printf("%zu %zu %zu %zu\n", kTakeSlicesMax, kTakeGroupMax, kTakeRowsMax, worst);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "check")) {
        int has;
        size_t count, rows, src, srs, dst, drs, elements, group;
        while (scanf("%d %zu %zu %zu %zu %zu %zu %zu %zu", &has, &count, &rows, &src, &srs, &dst, &drs, &elements, &group) == 9) {
            const char* why = check_take_call(has != 0, count, rows);
            if (!why) why = check_take_slice((const void*)src, srs, (const void*)dst, drs, elements, group);
            if (why) printf("refused: %s\n", why);
            else printf("ok\n");
        }
        return 0;
    }
    size_t eb, group;
    while (scanf("%zu %zu", &eb, &group) == 2) {
        if ((eb != 8 && eb != 32) || group == 0) {
            fprintf(stderr, "bad query %zu %zu\n", eb, group);
            return 2;
        }
        const TakePlan p = plan_take(eb, group);
        if (p.transpose) printf("transpose\n");
        else printf("take tile=%zu\n", p.tile);
    }
    return 0;
}
