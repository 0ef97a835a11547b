// bfly_ring_plan.hpp -- the static schedule of the ring form of the paired-point encode: one LOADER wave per workgroup streams the
// workgroup's 32-chunk tiles, as whole lines in memory order, into a ring of LDS slots; CW compute waves take them from there.
// Plain C++ (no HIP): the kernel, the host and the CPU simulation (tests/cpp/bfly_ring_sim.cpp) all include this file, so there is
// one place that says which tile an item is, whose it is and where it lies.
//
// A workgroup's item list is a pure function of (G, role_wgs, wg_in_role): item q is tile
//     (q / CW) role_wgs CW + wg_in_role CW + q % CW
// -- the tiles the CW waves of today's kernel walk, in the order they reach them -- as long as that tile exists.  Item q belongs to
// compute wave q % CW and lies in slot q % S; S is a multiple of CW, so a slot only ever serves one wave.  Two flag words per slot,
// one writer and one reader each, both zero at the start:
//     filled[slot] = q / S + 1   by the loader when item q has landed         (the owner waits for exactly this value)
//     freed[slot]  = q / S + 1   by the owner when it has read item q out     (the loader waits for it before item q + S)
// The loader keeps at most D <= S tiles in flight and publishes in order, so every wait is for an event the schedule guarantees:
// item q + S needs item q freed, which needs item q published, which needs only items < q + D <= q + S requested.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hbmpc {
namespace mf {

constexpr size_t BFLY_RING_LDS_BYTES = 160 * 1024;
constexpr int BFLY_RING_TABLE_BIAS = 256;  // MF_BFLY_BIAS of kernels_mfma_bfly.hpp: the two accumulator biases behind a pair's M slabs

struct BflyRingShape {
    int cw;      // compute waves
    int slots;   // S
    int depth;   // D: tiles the loader keeps in flight
};

constexpr size_t bfly_ring_slot_bytes(int m) { return (size_t)m * 1024; }
constexpr size_t bfly_ring_table_bytes(int m, int np) { return (size_t)np * ((size_t)m * 1024 + BFLY_RING_TABLE_BIAS); }
// table, S slots, then filled[S] and freed[S]
constexpr size_t bfly_ring_flags_offset(int m, int np, int slots) { return bfly_ring_table_bytes(m, np) + (size_t)slots * bfly_ring_slot_bytes(m); }
constexpr size_t bfly_ring_lds_bytes(int m, int np, int slots) { return bfly_ring_flags_offset(m, np, slots) + (size_t)slots * 8; }
constexpr bool bfly_ring_shape_ok(int m, int np, BflyRingShape s) {
    return s.cw >= 1 && s.cw <= 15 && s.slots >= s.cw && s.slots % s.cw == 0 && s.depth >= 1 && s.depth <= s.slots && (np == 4 || np == 8) &&
           bfly_ring_lds_bytes(m, np, s.slots) <= BFLY_RING_LDS_BYTES;
}

// What the library runs: 12 compute waves (the three waves per SIMD of k_mfma_bfly; with the loader 13 of the 16 a CU takes at 126
// VGPRs or fewer), one slot per compute wave and four tiles in flight.  Two slots per wave do not fit beside a table of 8 pairs
// from M = 5 on, and the sweep on the headline shape (profiles/ring_encode_sweep.txt) found nothing in them at 8 or 9 waves: a wave
// frees its slot as soon as it has read it out, so its next tile lands while it computes.  The ring form is taken when the table
// of a role of 4 or 8 pairs and these slots fit the LDS (8 pairs: M <= 7, 4 pairs: M <= 9); everything else keeps k_mfma_bfly.
constexpr BflyRingShape BFLY_RING_LIB = {12, 12, 4};
constexpr int BFLY_RING_MAX_M = 9;
constexpr bool bfly_ring_fits(int m, int np) { return m >= 2 && m <= BFLY_RING_MAX_M && bfly_ring_shape_ok(m, np, BFLY_RING_LIB); }

// ... and when the batch is large enough: a tile's way to its first MFMA is longer through the loader and the LDS than through a
// wave's own gather, a fixed cost of 2 - 3 microseconds per launch that the whole-line reads only win back over several tiles per
// wave.  Headline shape, 256 workgroups (profiles/ring_encode_sizes.txt): 2^15 .. 2^17 chunks 4 - 20 % slower than k_mfma_bfly, 2^18
// (2.7 tiles per compute wave) even, 2^19 (5.3) 9 - 11 % faster, 2^20 8 - 9 %.  So: at least four tiles for every compute wave.
constexpr size_t bfly_ring_min_tiles(size_t role_wgs) { return 4 * role_wgs * (size_t)BFLY_RING_LIB.cw; }

constexpr size_t bfly_ring_ntiles(size_t G) { return (G + 31) / 32; }
// how many items workgroup wg of role_wgs has
constexpr size_t bfly_ring_items(size_t ntiles, size_t role_wgs, size_t wg, int cw) {
    const size_t base = wg * (size_t)cw, step = role_wgs * (size_t)cw;
    if (base >= ntiles) return 0;
    const size_t left = ntiles - base, rem = left % step;
    return left / step * (size_t)cw + (rem < (size_t)cw ? rem : (size_t)cw);
}
constexpr size_t bfly_ring_tile(size_t role_wgs, size_t wg, int cw, size_t q) {
    return q / (size_t)cw * role_wgs * (size_t)cw + wg * (size_t)cw + q % (size_t)cw;
}
constexpr int bfly_ring_wave(int cw, size_t q) { return (int)(q % (size_t)cw); }
constexpr int bfly_ring_slot(int slots, size_t q) { return (int)(q % (size_t)slots); }
constexpr uint32_t bfly_ring_seq(int slots, size_t q) { return (uint32_t)(q / (size_t)slots) + 1; }
// the 16-byte piece p (0 .. 64 m - 1) of tile t: its byte offset in the input of G chunks of m elements.  Pieces past the end of the
// input (the last tile of a G that is no multiple of 32) read the input's last 16 bytes instead: their chunks are dead, their
// columns are computed and never stored.
constexpr size_t bfly_ring_piece_offset(size_t G, int m, size_t t, int p) {
    const size_t total = G * (size_t)m * 32, off = t * 32 * (size_t)m * 32 + (size_t)p * 16;
    return off + 16 <= total ? off : total - 16;
}

}  // namespace mf
}  // namespace hbmpc
