// mfma_plan.hpp -- host-side row planning of the matrix-core kernels (kernels_mfma.hpp, kernels_mfma_bfly.hpp): which table rows
// every workgroup keeps resident in LDS.  Plain C++ (no HIP): the encode route planner (encode_route.hpp) and its CPU test use it too.
// A is mf::MfmaRowsArgs or mf::MfPlan -- anything with the role fields below.
#pragma once
#include <stdint.h>

namespace hbmpc {
namespace mf {

struct MfmaRole {
    int row0, nrows;  // rows [row0, row0 + nrows) of the table
};
constexpr int MF_MAX_ROLES = 4;
// the role fields of MfmaRowsArgs on their own (what the planner hands the executors)
struct MfPlan {
    int nroles;
    int nblocks;
    int role_nwg[MF_MAX_ROLES];
    uint8_t blk_role[64], blk_idx[64];
    MfmaRole role[MF_MAX_ROLES];
};
template <class A>
inline void mf_take_plan(const MfPlan& p, A* a) {
    a->nroles = p.nroles, a->nblocks = p.nblocks;
    for (int k = 0; k < MF_MAX_ROLES; ++k) a->role_nwg[k] = p.role_nwg[k], a->role[k] = p.role[k];
    for (int j = 0; j < 64; ++j) a->blk_role[j] = p.blk_role[j], a->blk_idx[j] = p.blk_idx[j];
}

// nwg workgroups (rounded down to blocks of 8, at most 64 blocks) shared among the roles already in a->role[0 .. a->nroles)
// in proportion to their rows
template <class A>
inline bool mf_deal_blocks(int rows, int nwg, A* a) {
    const int nroles = a->nroles;
    int nblocks = nwg / 8;
    nblocks = nblocks > 64 ? 64 : nblocks < nroles ? nroles : nblocks;
    a->nblocks = nblocks;
    // blocks per role in proportion to its rows (at least one), dealt out by largest remaining deficit
    int have[MF_MAX_ROLES] = {0, 0, 0, 0};
    for (int j = 0; j < nblocks; ++j) {
        int best = 0;
        double bestd = -1e30;
        for (int k = 0; k < nroles; ++k) {
            const double want = (double)(j + 1) * a->role[k].nrows / rows;
            const double dfc = have[k] == 0 && nblocks - j <= nroles ? 1e9 : want - have[k];  // nobody is left without a block
            if (dfc > bestd) bestd = dfc, best = k;
        }
        a->blk_role[j] = (uint8_t)best;
        a->blk_idx[j] = (uint8_t)have[best]++;
    }
    for (int k = 0; k < nroles; ++k) {
        if (have[k] == 0) return false;
        a->role_nwg[k] = have[k] * 8;
    }
    return true;
}
// Host side: cut `rows` table rows (the first nv of them verify rows) into roles of at most `cap` rows.  Everything in one
// role when it fits; otherwise the verify rows form role 0 and the output rows are cut evenly into as few roles as
// possible.  nwg workgroups (rounded down to blocks of 8, at most 64 blocks) are shared in proportion to the rows.
// Returns false when the verify rows do not fit one role (the caller then uses the lane-per-chunk kernels).
template <class A>
inline bool mf_plan_roles(int rows, int nv, int cap, int nwg, A* a) {
    if (cap < 1 || nv > cap || rows < 1) return false;
    int nroles = 0;
    if (rows <= cap) {
        a->role[nroles++] = MfmaRole{0, rows};
    } else {
        if (nv > 0) a->role[nroles++] = MfmaRole{0, nv};
        const int ow = rows - nv, parts = (ow + cap - 1) / cap, per = (ow + parts - 1) / parts;
        for (int r = nv; r < rows; r += per) {
            if (nroles == MF_MAX_ROLES) return false;
            a->role[nroles++] = MfmaRole{r, rows - r < per ? rows - r : per};
        }
    }
    a->nroles = nroles;
    return mf_deal_blocks(rows, nwg, a);
}
// the point pairs of kernels_mfma_bfly.hpp: `pairs` (a power of two) table rows in roles of EQUAL size, the largest power
// of two that fits `cap` rows -- the kernel's unrolled pair loop has one trip count for every workgroup of a launch
template <class A>
inline bool mf_plan_pairs(int pairs, int cap, int nwg, A* a) {
    if (cap < 1 || pairs < 1 || (pairs & (pairs - 1)) != 0) return false;
    int per = pairs;
    while (per > cap) per >>= 1;
    if (per < 1 || pairs / per > MF_MAX_ROLES) return false;
    a->nroles = pairs / per;
    for (int k = 0; k < a->nroles; ++k) a->role[k] = MfmaRole{k * per, per};
    return mf_deal_blocks(pairs, nwg, a);
}

}  // namespace mf
}  // namespace hbmpc
