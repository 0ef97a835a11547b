// kernels_mfma_bfly_ring_lab.hpp -- laboratory forms of k_mfma_bfly_ring (csrc/kernels_mfma_bfly_ring.hpp), for tools/ubench_bfly_ring.hip
// only; nothing here is compiled into the library.  The table copy, the pair core (bfly_pair, with its ABL hooks) and the output
// offsets are the library's own functions (csrc/kernels_mfma_bfly.hpp); the ring set-up, the LDS-DMA loader and a compute wave's take
// of a slot are written in place in k_mfma_bfly_ring -- as functions they change its instructions (profiles/bfly_shared_body.txt) --
// and are COPIES of that text here, kept equal by hand, next to the second loader form.
//
// Workgroup = CW compute waves + 1 loader wave.  The loader streams the workgroup's tiles as whole lines (lane l takes the 16-byte
// piece 64 i + l of a tile's M KB) into a ring of S LDS slots behind the table, D tiles in flight; the compute waves issue no
// vector-memory loads at all: poll the slot's flag, M ds_read_b128 (chunk c, coefficient i, half h at 32 M c + 32 i + 16 h), free
// the slot, then flip, pairs and plain conditional stores.  The schedule (which tile, whose, which slot, which flag value) is
// csrc/bfly_ring_plan.hpp; one barrier, after the table load and the zeroing of the flags.
//   DMA   loader form: true = global_load_lds_dwordx4 straight into the slot ("landed" = a counted vmcnt wait, no data registers),
//         false = global_load_dwordx4 into D register sets, ds_write_b128 into the slot
//   ABL   timing-only ablations as in kernels_mfma_bfly_lab.hpp: 1 no epilogue arithmetic, 2 no MFMAs, 4 no table reads
//   START 0 = the table by all 13 waves through bfly_table_to_lds, the barrier, then the loader's first request (the library's start
//         until profiles/encode_launch_edges.txt); 1 = the library's start: the loader's first D requests before the barrier, the
//         table by the compute waves with every load of a thread ahead of its first LDS write (DMA form only)
//   LP SP the cache policy of the loader's reads and of the row stores (RingPolicy)
//   STAMP every workgroup records the 100 MHz wall clock at six points into ring_lab_stamps (RING_STAMP_*)
#pragma once
#include "../mpc-protocols_amd/csrc/kernels_mfma_bfly_ring.hpp"
#include "kernels_mfma_bfly_lab.hpp"

namespace hbmpc {
namespace mf {

enum { RING_STAMP_ENTRY, RING_STAMP_TABLE, RING_STAMP_FIRST_DMA, RING_STAMP_FIRST_PUBLISHED, RING_STAMP_FIRST_STORE, RING_STAMP_LAST_STORE, RING_STAMPS };
constexpr int RING_STAMP_MAX_WGS = 512;
__device__ unsigned long long ring_lab_stamps[RING_STAMP_MAX_WGS * RING_STAMPS];

template <int M, int CW, int NP, int S, int D, bool DMA, int ABL = 0, int START = 0, int LP = RP_DEFAULT, int SP = RP_DEFAULT, bool STAMP = false>
__global__ __launch_bounds__(64 * (CW + 1)) void k_mfma_bfly_ring_lab(MfmaRowsArgs a) {
    static_assert(bfly_ring_shape_ok(M, NP, BflyRingShape{CW, S, D}), "ring shape");
    static_assert(M * (D - 1) <= 63, "vmcnt counts to 63");
    static_assert(DMA || (START == 0 && LP == RP_DEFAULT), "the new start and the loader's policy exist in the DMA form");
    constexpr int ROWB = M * 1024 + MF_BFLY_BIAS;
    constexpr int NT = 64 * (CW + 1);
    constexpr int TILEB = M * 1024;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];  // NP * ROWB, S slots, filled[S], freed[S]
    const int blk8 = (int)blockIdx.x >> 3;
    uint32_t blk_idx;
    if constexpr (START == 0) blk_idx = a.blk_idx[blk8];
    else blk_idx = (reinterpret_cast<const uint32_t*>(a.blk_idx)[blk8 >> 2] >> (8 * (blk8 & 3))) & 0xffu;  // a scalar load
    const uint32_t wg_in_role = blk_idx * 8 + (blockIdx.x & 7);
    const MfmaRole role = a.role[0];  // one role
    const uint32_t role_wgs = (uint32_t)a.role_nwg[0];
    // one lane of the wave that passes a point keeps its time; a workgroup beyond the buffer keeps none
    auto stamp = [&](int which) {
        if constexpr (STAMP)
            if ((threadIdx.x & 63) == 0 && blockIdx.x < (unsigned)RING_STAMP_MAX_WGS) ring_lab_stamps[blockIdx.x * RING_STAMPS + which] = wall_clock64();
    };
    if (threadIdx.x < 64) stamp(RING_STAMP_ENTRY);
    uint8_t* const ring = lds + bfly_ring_table_bytes(M, NP);
    ring_flag_t* const filled = (ring_flag_t*)(lds + bfly_ring_flags_offset(M, NP, S));
    ring_flag_t* const freed = filled + S;
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto items = [&] { return (uint32_t)bfly_ring_items(bfly_ring_ntiles(a.G), role_wgs, wg_in_role, CW); };
    auto tile_of = [&](uint32_t q) { return bfly_ring_tile(role_wgs, wg_in_role, CW, q); };
    if constexpr (START == 0) {
        bfly_table_to_lds<NT>(lds, a.table + (size_t)role.row0 * ROWB, NP * (ROWB / 16));
        if (threadIdx.x < 2 * S) filled[threadIdx.x] = 0;
        __syncthreads();
        if (threadIdx.x < 64) stamp(RING_STAMP_TABLE);
    }
    // START = 1: the two kinds of wave part here and each reaches the barrier in its own text (the library kernel says why)
    if (wave == CW) {
        // ---- the loader
        const uint32_t nitems = items();
        const size_t total = a.G * (size_t)(M * 32);
        auto wait_freed = [&](uint32_t q) {
            if (q >= S) {
                const uint32_t need = q / S;  // the sequence number of item q - S
                while (ring_flag(freed + q % S) != need) __builtin_amdgcn_s_sleep(1);
            }
        };
        auto publish = [&](uint32_t q) {
            filled[q % S] = q / S + 1;
            if (q == 0) stamp(RING_STAMP_FIRST_PUBLISHED);
        };
        // this lane's piece offsets inside a tile; in the input's last tile, pieces past the end read its last 16 bytes
        auto piece = [&](size_t tb, int i) {
            const uint32_t off = (uint32_t)(i * 64 + lane) * 16u;
            const size_t left = total - tb;  // >= 16: the tile exists
            return left >= (size_t)TILEB || off + 16 <= left ? off : (uint32_t)(left - 16);
        };
        if constexpr (DMA) {
            const uint32_t ring_lds = (uint32_t)(uintptr_t)ring;  // the LDS byte address: the low word of the flat address
            auto request = [&](uint32_t q) {
                const size_t tb = tile_of(q) * (size_t)(32 * M * 32);
                const uint32_t dst = __builtin_amdgcn_readfirstlane(ring_lds + (q % S) * TILEB);
#pragma unroll
                for (int i = 0; i < M; ++i) ring_dma16<LP>(a.in + tb, piece(tb, i), dst + i * 1024);
                if (q == 0) stamp(RING_STAMP_FIRST_DMA);
            };
            if constexpr (START != 0) {
                // the first D tiles, before the barrier: their slots are free, and nothing is published before it
                for (uint32_t q = 0; q < nitems && q < (uint32_t)D; ++q) request(q);
                __syncthreads();
                if (nitems == 0) return;
                if (nitems >= (uint32_t)D) {  // item D - 1 is requested: item 0 has landed when D - 1 tiles are left in flight
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(M * (D - 1)) : "memory");
                    publish(0);
                }
            }
            if (nitems == 0) return;
            for (uint32_t q = START != 0 ? D : 0; q < nitems; ++q) {
                wait_freed(q);
                request(q);
                if (q + 1 >= D) {
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(M * (D - 1)) : "memory");
                    publish(q + 1 - D);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            for (uint32_t q = nitems >= D - 1 ? nitems - (D - 1) : 0; q < nitems; ++q) publish(q);
        } else {
            if (nitems == 0) return;
            // D register sets; every load is issued, past the end too (the workgroup's last item again), so that hipcc can count
            // the loads behind the one it waits for
            v4i r[D][M];
            auto request = [&](uint32_t q, v4i (&dst)[M]) {
                const size_t tb = tile_of(q < nitems ? q : nitems - 1) * (size_t)(32 * M * 32);
#pragma unroll
                for (int i = 0; i < M; ++i) dst[i] = *reinterpret_cast<const v4i*>(a.in + tb + piece(tb, i));
            };
#pragma unroll
            for (int j = 0; j < D; ++j) request(j, r[j]);
            for (uint32_t q0 = 0; q0 < nitems; q0 += D) {
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const uint32_t q = q0 + j;
                    if (q < nitems) {
                        wait_freed(q);
                        uint8_t* sp = ring + (q % S) * TILEB + lane * 16;
#pragma unroll
                        for (int i = 0; i < M; ++i) *reinterpret_cast<v4i*>(sp + i * 1024) = r[j][i];
                        asm volatile("" ::: "memory");
                        publish(q);  // LDS operations of one wave execute in order: the flag lands behind the data
                    }
                    request(q + D, r[j]);
                }
            }
        }
        return;
    }
    // ---- a compute wave (START = 1: its constants' loads and the item count in front of the table's loads and the barrier)
    const int c = lane & 31, h = lane >> 5;
    const Half H = make_half(h);
    const uint32_t nitems = items();
    if constexpr (START != 0) {
        // the table, by the compute waves: every load of a thread first (a last, partial round clamped), then its LDS writes
        constexpr int PIECES = NP * (ROWB / 16), NTC = 64 * CW, ROUNDS = (PIECES + NTC - 1) / NTC;
        const uint8_t* src = a.table + (size_t)role.row0 * ROWB;
        v4i t[ROUNDS];
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) {
            const int p = (int)threadIdx.x + k * NTC;
            t[k] = *reinterpret_cast<const v4i*>(src + (size_t)((k + 1) * NTC <= PIECES || p < PIECES ? p : PIECES - 1) * 16);
        }
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) asm volatile("" : "+v"(t[k]));  // all loaded here: none is moved down into its write's branch
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) {
            const int p = (int)threadIdx.x + k * NTC;
            if ((k + 1) * NTC <= PIECES || p < PIECES) *reinterpret_cast<v4i*>(lds + (size_t)p * 16) = t[k];
        }
        if (threadIdx.x < 2 * S) filled[threadIdx.x] = 0;
        __syncthreads();
        if (threadIdx.x < 64) stamp(RING_STAMP_TABLE);
    }
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
            bfly_pair<M, ABL>(lds + (size_t)p * ROWB, lane, h, data, pe, pt);
            uint32_t k32 = (uint32_t)(role.row0 + p);
            asm volatile("" : "+s"(k32));  // the output row bases are recomputed, not kept per unrolled pair (scalar registers)
            uint32_t Rw[4];
            bfly_words_lab<false, ABL>(pe, pt, H, Rw);
            store_row(k32, true, Rw);
            if (p == 0 && q == 0) stamp(RING_STAMP_FIRST_STORE);
            if ((int)k32 + a.half < a.nout) {  // the partner exists
                bfly_words_lab<true, ABL>(pe, pt, H, Rw);
                store_row(k32 + (uint32_t)a.half, true, Rw);
            }
        }
        if (q + 1 == nitems) stamp(RING_STAMP_LAST_STORE);  // the workgroup's last item: its wave's last store is issued
    }
}

}  // namespace mf
}  // namespace hbmpc
