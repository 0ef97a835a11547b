// kernels_mfma_bfly_ring.hpp -- the ring form of the plain chunk-major paired-point encode (kernels_mfma_bfly.hpp: same table, same
// pairs, same bytes out), the headline compute_shares kernel.
//
// Workgroup = CW compute waves + 1 LOADER wave.  The loader streams the workgroup's 32-chunk tiles as whole lines -- lane l takes the
// 16-byte piece 64 i + l of a tile's M KB, so a load instruction touches 8 lines instead of the 32 of a lane-pair-per-chunk gather --
// by LDS-DMA (global_load_lds_dwordx4: no data registers) into a ring of S LDS slots behind the table, D tiles in flight, and
// publishes a slot when a counted vmcnt wait says its tile has landed.  The compute waves issue no vector-memory loads at all: poll
// the slot's flag, M ds_read_b128 (chunk c, coefficient i, half h at 32 M c + 32 i + 16 h), free the slot, then flip, pairs and plain
// conditional stores -- nothing in their loop waits on vmcnt, so the stores are fire-and-forget and the STATIC / dropped-store
// machinery of k_mfma_bfly is not needed; one input register set instead of two.  The HBM latency and the LDS trip sit in the
// loader's time.  The schedule (which tile, whose, which slot, which flag value) is bfly_ring_plan.hpp, simulated on the CPU by
// tests/cpp/bfly_ring_sim.cpp; there is one barrier, after the table load and the zeroing of the flags, and none after it.
// The start: the loader needs nothing from the table, so it requests its first D tiles BEFORE the barrier and takes no part in the
// table copy (vmcnt is a wave's own counter: the barrier does not wait for them); the compute waves copy the table with all of a
// thread's loads issued before its first LDS write, one memory round trip instead of one per piece.  A tile's first MFMA is then
// one latency from the kernel's entry, not several.  LP / SP: the cache policy of the loader's reads and of the row stores, every
// byte being touched once (RingPolicy; the library's choice and the A/B behind it: profiles/encode_launch_edges.txt).
// Measured forms and shapes: profiles/ring_encode_sweep.txt (tools/ubench_bfly_ring.hip).
#pragma once
#include <stddef.h>

#include "bfly_ring_plan.hpp"
#include "kernels_mfma_bfly.hpp"

namespace hbmpc {
namespace mf {

// one LDS-DMA piece: lane l's 16 bytes at sbase + voff land at lds_dst + 16 l (sbase, lds_dst wave-uniform).  M0 is compiler-reserved:
// saved and restored inside the statement; the nop covers a base or destination fresh from a v_readfirstlane.
// POL: RP_DEFAULT or RP_NT.
enum RingPolicy { RP_DEFAULT = 0, RP_NT = 1, RP_SC1 = 2, RP_SC0_SC1 = 3 };
#define HBMPC_RING_DMA16(MOD)                                                                                                       \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %1, %2" MOD "\n\ts_mov_b32 m0, %0" \
                 : "=&s"(keep)                                                                                                      \
                 : "v"(voff), "s"(sbase), "s"(lds_dst)                                                                              \
                 : "memory")
template <int POL = RP_DEFAULT>
HB_DEV void ring_dma16(const uint8_t* sbase, uint32_t voff, uint32_t lds_dst) {
    static_assert(POL == RP_DEFAULT || POL == RP_NT, "loader policy");
    uint32_t keep;
    if constexpr (POL == RP_NT) HBMPC_RING_DMA16(" nt");
    else HBMPC_RING_DMA16("");
}
#undef HBMPC_RING_DMA16
// one lane's 16 bytes of an output row with a cache policy other than the default (that one is a plain C++ store)
template <int POL>
HB_DEV void ring_store16(uint8_t* p, const uint32_t (&w)[4]) {
    static_assert(POL == RP_NT || POL == RP_SC1 || POL == RP_SC0_SC1, "store policy");
    const v4i v = {(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
    if constexpr (POL == RP_NT) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(p), "v"(v) : "memory");
    else if constexpr (POL == RP_SC1) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory");
}
// the library's policies (profiles/encode_launch_edges.txt)
constexpr int BFLY_RING_LOAD_POLICY = RP_DEFAULT, BFLY_RING_STORE_POLICY = RP_NT;
// the flag words are read and written as LDS words (a volatile access through a generic pointer would be a flat one and wait for vmcnt)
using ring_flag_t = __attribute__((address_space(3))) volatile uint32_t;
HB_DEV uint32_t ring_flag(const ring_flag_t* p) { return __builtin_amdgcn_readfirstlane(*p); }

template <int M, int CW, int NP, int S, int D, int LP = BFLY_RING_LOAD_POLICY, int SP = BFLY_RING_STORE_POLICY>
__global__ __launch_bounds__(64 * (CW + 1)) void k_mfma_bfly_ring(MfmaRowsArgs a) {
    static_assert(bfly_ring_shape_ok(M, NP, BflyRingShape{CW, S, D}), "ring shape");
    static_assert(M * (D - 1) <= 63, "vmcnt counts to 63");
    constexpr int ROWB = M * 1024 + MF_BFLY_BIAS;
    constexpr int TILEB = M * 1024;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];  // NP * ROWB, S slots, filled[S], freed[S]
    const int blk8 = (int)blockIdx.x >> 3;
    // blk_idx[blk8] out of its word: a scalar load like every other kernel argument (a byte load is a vector one, a memory round trip
    // in front of the loader's first request)
    static_assert(offsetof(MfmaRowsArgs, blk_idx) % 4 == 0, "blk_idx is read by words");
    const uint32_t blk_word = reinterpret_cast<const uint32_t*>(a.blk_idx)[blk8 >> 2];
    const uint32_t wg_in_role = ((blk_word >> (8 * (blk8 & 3))) & 0xffu) * 8 + (blockIdx.x & 7);
    const MfmaRole role = a.role[0];  // one role
    const uint32_t role_wgs = (uint32_t)a.role_nwg[0];
    uint8_t* const ring = lds + bfly_ring_table_bytes(M, NP);
    ring_flag_t* const filled = (ring_flag_t*)(lds + bfly_ring_flags_offset(M, NP, S));
    ring_flag_t* const freed = filled + S;
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto items = [&] { return (uint32_t)bfly_ring_items(bfly_ring_ntiles(a.G), role_wgs, wg_in_role, CW); };
    auto tile_of = [&](uint32_t q) { return bfly_ring_tile(role_wgs, wg_in_role, CW, q); };
    // The two kinds of wave part here and each reaches the barrier in its own text: the compiler's waits for the table's loads
    // must not get into the loader, where they would wait for its tiles as well.
    if (wave == CW) {
        // ---- the loader
        const uint32_t nitems = items();
        const size_t total = a.G * (size_t)(M * 32);
        // this lane's piece offsets inside a tile; in the input's last tile, pieces past the end read its last 16 bytes
        auto piece = [&](size_t tb, int i) {
            const uint32_t off = (uint32_t)(i * 64 + lane) * 16u;
            const size_t left = total - tb;  // >= 16: the tile exists
            return left >= (size_t)TILEB || off + 16 <= left ? off : (uint32_t)(left - 16);
        };
        const uint32_t ring_lds = (uint32_t)(uintptr_t)ring;  // the LDS byte address: the low word of the flat address
        auto request = [&](uint32_t q) {
            const size_t tb = tile_of(q) * (size_t)(32 * M * 32);
            const uint32_t dst = __builtin_amdgcn_readfirstlane(ring_lds + (q % S) * TILEB);
#pragma unroll
            for (int i = 0; i < M; ++i) ring_dma16<LP>(a.in + tb, piece(tb, i), dst + i * 1024);
        };
        auto wait_freed = [&](uint32_t q) {
            if (q >= S) {
                const uint32_t need = q / S;  // the sequence number of item q - S
                while (ring_flag(freed + q % S) != need) __builtin_amdgcn_s_sleep(1);
            }
        };
        auto publish = [&](uint32_t q) { filled[q % S] = q / S + 1; };
        // the first D tiles, before the barrier: their slots are free, and nothing is published before it (it is the compute
        // waves that zero the flags).  vmcnt is this wave's own: the barrier does not wait for the tiles.
        for (uint32_t q = 0; q < nitems && q < (uint32_t)D; ++q) request(q);
        __syncthreads();
        if (nitems == 0) return;
        if (nitems >= (uint32_t)D) {  // item D - 1 is requested: item 0 has landed when D - 1 tiles are left in flight
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(M * (D - 1)) : "memory");
            publish(0);
        }
        for (uint32_t q = D; q < nitems; ++q) {
            wait_freed(q);
            request(q);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(M * (D - 1)) : "memory");
            publish(q + 1 - D);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        for (uint32_t q = nitems >= D - 1 ? nitems - (D - 1) : 0; q < nitems; ++q) publish(q);
        return;
    }
    // ---- a compute wave
    const int c = lane & 31, h = lane >> 5;
    const Half H = make_half(h);  // its constants' loads fly with the table's
    uint32_t nitems;
    {
        // the table, by the compute waves: every load of a thread first (a last, partial round clamped), then its LDS writes
        constexpr int PIECES = NP * (ROWB / 16), NTC = 64 * CW, ROUNDS = (PIECES + NTC - 1) / NTC;
        const uint8_t* src = a.table + (size_t)role.row0 * ROWB;
        v4i t[ROUNDS];
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) {
            const int p = (int)threadIdx.x + k * NTC;
            t[k] = *reinterpret_cast<const v4i*>(src + (size_t)((k + 1) * NTC <= PIECES || p < PIECES ? p : PIECES - 1) * 16);
        }
        nitems = items();  // under the loads
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) asm volatile("" : "+v"(t[k]));  // all loaded here: none is moved down into its write's branch
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) {
            const int p = (int)threadIdx.x + k * NTC;
            if ((k + 1) * NTC <= PIECES || p < PIECES) *reinterpret_cast<v4i*>(lds + (size_t)p * 16) = t[k];
        }
        if (threadIdx.x < 2 * S) filled[threadIdx.x] = 0;
    }
    __syncthreads();
    for (uint32_t q = wave; q < nitems; q += CW) {
        const uint32_t slot = q % S, seq = q / S + 1;
        while (ring_flag(filled + slot) != seq) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");  // the data reads stay below the poll
        v4i data[M];
        {
            const uint8_t* sp = ring + slot * TILEB + c * (M * 32) + 16 * h;
#pragma unroll
            for (int i = 0; i < M; ++i) data[i] = *reinterpret_cast<const v4i*>(sp + i * 32);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        freed[slot] = seq;
#pragma unroll
        for (int i = 0; i < M; ++i) data[i] = flip(data[i]);
        const BflyOut o = bfly_out(a, tile_of(q), c, h);
        auto store_row = [&](uint32_t k, bool exists, const uint32_t (&Rw)[4]) {
            uint8_t* qb = a.out_party_major ? a.out + (size_t)k * a.out_stride * 32 : a.out + (size_t)k * 32;  // wave-uniform
            if (exists && o.live) {
                if constexpr (SP == RP_DEFAULT) *reinterpret_cast<uint4*>(qb + o.qo) = make_uint4(Rw[0], Rw[1], Rw[2], Rw[3]);
                else ring_store16<SP>(qb + o.qo, Rw);
            }
        };
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            uint32_t pe[8], pt[8];
            bfly_pair<M>(lds + (size_t)p * ROWB, lane, h, data, pe, pt);
            uint32_t k32 = (uint32_t)(role.row0 + p);
            asm volatile("" : "+s"(k32));  // the output row bases are recomputed, not kept per unrolled pair (scalar registers)
            {
                uint64_t T[4];
                uint32_t Rw[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) T[j] = (uint64_t)(pe[2 * j + 1] + pt[2 * j + 1]) * H.k16 + (pe[2 * j] + pt[2 * j]);
                reduce_words(T, Rw, H);
                store_row(k32, true, Rw);
            }
            const bool partner = (int)k32 + a.half < a.nout;
            if (partner) {
                uint64_t T[4];
                uint32_t Rw[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) T[j] = (uint64_t)(pe[2 * j + 1] - pt[2 * j + 1]) * H.k16 + (pe[2 * j] - pt[2 * j]);
                reduce_words(T, Rw, H);
                store_row(k32 + (uint32_t)a.half, true, Rw);
            }
        }
    }
}

}  // namespace mf
}  // namespace hbmpc
