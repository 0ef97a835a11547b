// bfly_ring_sim.cpp -- the schedule of the ring encode (csrc/bfly_ring_plan.hpp) run on the CPU: one loader and CW consumers per
// workgroup, stepped one action at a time under four interleavings, following the protocol of k_mfma_bfly_ring
// (csrc/kernels_mfma_bfly_ring.hpp) word for word:
//   loader    for q = 0 ..: wait freed[slot(q)] == seq(q - S) (q >= S) | request item q into its slot | once D items are in flight,
//             wait for the oldest to land and write filled[slot] = seq | after the last request, publish the rest in order
//   consumer  for its q = w, w + CW, ..: wait filled[slot(q)] == seq(q) | read the slot out | write freed[slot] = seq(q)
// Checked: some agent can always move until all are done (every wait is satisfied); every tile of the input is consumed exactly once,
// by the wave the plan names; no slot is refilled before its occupant was read out; no slot is read before it was published, and it
// holds the item its reader expects; every 16-byte piece the loader asks for lies inside the input, and inside its tile where the
// tile is whole.  Stand-alone (tests/test_bfly_ring_plan.py builds it with the sanitizers and runs it); exit status 0 = all held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../mpc-protocols_amd/csrc/bfly_ring_plan.hpp"

using namespace hbmpc::mf;

enum Order { ROUND_ROBIN, LOADER_FIRST, LOADER_LAST, RANDOM, NORDERS };
static const char* order_name[NORDERS] = {"round-robin", "loader first", "loader last", "seeded random"};

static int failures = 0;
#define REQUIRE(cond, ...)                   \
    do {                                     \
        if (!(cond)) {                       \
            if (failures < 20) {             \
                fprintf(stderr, "FAILED: "); \
                fprintf(stderr, __VA_ARGS__); \
                fprintf(stderr, "\n");       \
            }                                \
            ++failures;                      \
            return false;                    \
        }                                    \
    } while (0)

struct Slot {
    uint32_t filled = 0, freed = 0;  // the two flag words
    long item = -1;                  // what the loader last requested into it
    bool landed = false;             // ... and has waited for
    bool read_out = true;            // its occupant was read (an empty slot counts as read)
};

// one workgroup; consumed[t] counts the reads of tile t over the whole launch
static bool run_workgroup(size_t G, int m, size_t role_wgs, size_t wg, BflyRingShape sh, Order order, uint64_t seed, bool check_pieces,
                          std::vector<uint8_t>& consumed) {
    const int CW = sh.cw, S = sh.slots, D = sh.depth;
    const size_t ntiles = bfly_ring_ntiles(G), nitems = bfly_ring_items(ntiles, role_wgs, wg, CW), total = G * (size_t)m * 32;
    std::vector<Slot> slot(S);
    size_t requested = 0, published = 0;  // the loader: items requested, items published
    std::vector<size_t> next(CW);         // consumer w: its next item
    std::vector<int> phase(CW, 0);        // 0: waiting for filled, 1: has read, owes the freed write
    for (int w = 0; w < CW; ++w) next[w] = (size_t)w;
    // the plan's item list against its definition: tile(q) exists exactly for q < nitems
    REQUIRE(nitems == 0 || bfly_ring_tile(role_wgs, wg, CW, nitems - 1) < ntiles, "G=%zu wg=%zu: last item is no tile", G, wg);
    REQUIRE(bfly_ring_tile(role_wgs, wg, CW, nitems) >= ntiles, "G=%zu wg=%zu: item %zu would be a tile too", G, wg, nitems);

    auto loader_done = [&] { return published == nitems; };
    // one loader action; false when it has to wait
    auto loader_step = [&]() -> bool {
        if (requested < nitems && requested - published < (size_t)D) {
            const size_t q = requested;
            Slot& sl = slot[bfly_ring_slot(S, q)];
            if (q >= (size_t)S && sl.freed != bfly_ring_seq(S, q - S)) return false;  // wait_freed
            REQUIRE(sl.read_out, "G=%zu wg=%zu: slot %d refilled with item %zu before item %ld was read out", G, wg, bfly_ring_slot(S, q), q, sl.item);
            const size_t t = bfly_ring_tile(role_wgs, wg, CW, q);
            if (check_pieces)
                for (int p = 0; p < 64 * m; ++p) {
                    const size_t off = bfly_ring_piece_offset(G, m, t, p), want = t * 32 * (size_t)m * 32 + (size_t)p * 16;
                    REQUIRE(off + 16 <= total, "G=%zu tile %zu piece %d: bytes [%zu, %zu) outside the input of %zu", G, t, p, off, off + 16, total);
                    REQUIRE(want + 16 > total || off == want, "G=%zu tile %zu piece %d: offset %zu, not %zu", G, t, p, off, want);
                }
            sl.item = (long)q, sl.landed = false, sl.read_out = false;
            ++requested;
            return true;
        }
        if (published < requested) {  // D in flight, or nothing left to request: the oldest lands and is published
            Slot& sl = slot[bfly_ring_slot(S, published)];
            REQUIRE(sl.item == (long)published, "G=%zu wg=%zu: slot of item %zu holds item %ld at its publication", G, wg, published, sl.item);
            sl.landed = true;
            sl.filled = bfly_ring_seq(S, published);
            ++published;
            return true;
        }
        return false;
    };
    auto consumer_done = [&](int w) { return next[w] >= nitems; };
    auto consumer_step = [&](int w) -> bool {
        const size_t q = next[w];
        Slot& sl = slot[bfly_ring_slot(S, q)];
        if (phase[w] == 0) {
            if (sl.filled != bfly_ring_seq(S, q)) return false;  // the poll
            REQUIRE(sl.landed && sl.item == (long)q, "G=%zu wg=%zu wave %d: reads slot %d for item %zu, it holds item %ld (landed %d)", G, wg, w,
                    bfly_ring_slot(S, q), q, sl.item, (int)sl.landed);
            REQUIRE(bfly_ring_wave(CW, q) == w, "G=%zu wg=%zu: item %zu read by wave %d", G, wg, q, w);
            const size_t t = bfly_ring_tile(role_wgs, wg, CW, q);
            REQUIRE(t < ntiles, "G=%zu wg=%zu: item %zu is tile %zu of %zu", G, wg, q, t, ntiles);
            REQUIRE(consumed[t] == 0, "G=%zu: tile %zu consumed twice", G, t);
            consumed[t] = 1;
            sl.read_out = true;
            phase[w] = 1;
            return true;
        }
        sl.freed = bfly_ring_seq(S, q);
        phase[w] = 0;
        next[w] += (size_t)CW;
        return true;
    };
    uint64_t rs = seed * 0x9E3779B97F4A7C15ull + wg + 1;
    auto rnd = [&] {
        rs ^= rs << 13, rs ^= rs >> 7, rs ^= rs << 17;
        return rs;
    };
    const size_t limit = 4 * (nitems + 1) * (size_t)(CW + 1) + 64;  // every action moves some agent: far more than enough
    int rr = 0;
    for (size_t step = 0;; ++step) {
        bool all = loader_done();
        for (int w = 0; w < CW && all; ++w) all = consumer_done(w);
        if (all) break;
        REQUIRE(step < limit, "G=%zu wg=%zu %s: no end after %zu steps", G, wg, order_name[order], step);
        // agents in the order this interleaving tries them: index CW is the loader
        bool moved = false;
        const int na = CW + 1;
        const int first = order == ROUND_ROBIN ? rr : order == RANDOM ? (int)(rnd() % (uint64_t)na) : 0;
        for (int k = 0; k < na && !moved; ++k) {
            int agent;
            if (order == LOADER_FIRST) agent = k == 0 ? CW : k - 1;
            else if (order == LOADER_LAST) agent = k;
            else agent = (first + k) % na;
            if (agent == CW) moved = !loader_done() && loader_step();
            else moved = !consumer_done(agent) && consumer_step(agent);
            if (failures) return false;
            if (moved && order == ROUND_ROBIN) rr = (agent + 1) % na;
        }
        REQUIRE(moved, "G=%zu wg=%zu %s: nobody can move (requested %zu, published %zu of %zu)", G, wg, order_name[order], requested, published, nitems);
    }
    for (int s = 0; s < S; ++s) REQUIRE(slot[s].read_out, "G=%zu wg=%zu: item %ld left in slot %d", G, wg, slot[s].item, s);
    return true;
}

static bool run_launch(size_t G, int m, size_t role_wgs, BflyRingShape sh, Order order, bool check_pieces) {
    const size_t ntiles = bfly_ring_ntiles(G);
    std::vector<uint8_t> consumed(ntiles, 0);
    for (size_t wg = 0; wg < role_wgs; ++wg)
        if (!run_workgroup(G, m, role_wgs, wg, sh, order, G * 31 + role_wgs, check_pieces, consumed)) return false;
    for (size_t t = 0; t < ntiles; ++t) REQUIRE(consumed[t] == 1, "G=%zu wgs=%zu: tile %zu never consumed", G, role_wgs, t);
    return true;
}

int main() {
    const BflyRingShape shapes[] = {BFLY_RING_LIB, BflyRingShape{8, 16, 2}, BflyRingShape{3, 6, 6}, BflyRingShape{1, 1, 1}};
    const int ms[] = {2, 6, 9};
    const size_t wgs[] = {8, 256};
    size_t launches = 0;
    for (const BflyRingShape sh : shapes) {
        if (!bfly_ring_shape_ok(2, 8, sh)) {
            fprintf(stderr, "FAILED: shape CW=%d S=%d D=%d is not a ring shape\n", sh.cw, sh.slots, sh.depth);
            return 1;
        }
        for (const size_t role_wgs : wgs) {
            std::vector<size_t> Gs = {1, 31, 32, 33, (size_t)1 << 20};
            // tile counts around CW, S and 2 S per workgroup, the last tile whole, one chunk short and one chunk long
            for (const int per : {sh.cw, sh.slots, 2 * sh.slots})
                for (int dt = -1; dt <= 1; ++dt)
                    for (const size_t r : {(size_t)0, (size_t)1, (size_t)31}) Gs.push_back(32 * (role_wgs * (size_t)per + (size_t)dt) - r);
            for (const size_t G : Gs)
                for (int o = 0; o < NORDERS; ++o) {
                    const int m = ms[(launches / NORDERS) % 3];
                    // the piece ranges do not depend on the interleaving: checked under the first one, for every m at the small sizes
                    if (!run_launch(G, m, role_wgs, sh, (Order)o, o == 0)) return 1;
                    if (o == 0 && G < ((size_t)1 << 20))
                        for (const int m2 : ms)
                            if (m2 != m && !run_launch(G, m2, role_wgs, sh, ROUND_ROBIN, true)) return 1;
                    ++launches;
                }
        }
    }
    // the LDS budget: the library's shape holds the headline's table and ring, and declines what does not fit
    if (!bfly_ring_fits(6, 8) || bfly_ring_lds_bytes(6, 8, BFLY_RING_LIB.slots) > BFLY_RING_LDS_BYTES || bfly_ring_fits(8, 8) || bfly_ring_fits(11, 8) ||
        !bfly_ring_fits(9, 4) || bfly_ring_fits(10, 4) || bfly_ring_fits(6, 16) || bfly_ring_fits(1, 8)) {
        fprintf(stderr, "FAILED: the ring's LDS predicate\n");
        return 1;
    }
    printf("bfly_ring_sim: %zu launches under %d interleavings each: every wait satisfied, every tile consumed once by its wave, no slot refilled early or read early, every piece inside the input\n",
           launches / NORDERS, (int)NORDERS);
    return failures != 0;
}
