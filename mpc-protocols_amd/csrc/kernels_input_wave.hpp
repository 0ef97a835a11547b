// Input (honeybadger/input/input.rs) for all parties of a SMALL batch in one launch: a wave per batch element.
//
// The client opens the mask of element g from the senders' shares (input.rs:489-506: recover_secret per element, the first error
// aborts), broadcasts masked = x + mask, and server p keeps masked - r_p (:85-100, :300-301).  The separate steps -- the decode
// of the masks and one element-wise kernel -- are two launches of a few us each whatever the batch; here an element is one
// round trip of loads, the decode with a lane per table row (the t verify rows and the P(0) row; the products of a row shared
// by a DPP quad where the rows fit, dot_shared) and the last step with a lane per party.
//
// An element whose mask does not open (no OEC round at exactly 2t + 1 senders) is REFUSED: its mask, its masked value and all of
// its shares are zero, never x + 0 -- that would broadcast the client's input in the clear.  It is counted in the summary.
// The bytes of every buffer a caller can see are those of the two launches (tests/test_gpu_input.py).
//
// Not here: sessions, RBC and the InputMessage / OutputMessage envelopes; the 48-byte Vec<RobustShare> and Vec<F> payloads
// (hbmpc_dev_unpack_shares / hbmpc_dev_pack_fvec convert them); sampling the masks (they are RanSha's outputs).
#pragma once
#include "wave_core.hpp"

namespace hbmpc {

struct InputWaveArgs {
    const uint32_t* x;     // [N] the client's values
    const uint32_t* r_sh;  // [party][N] the parties' shares of the masks
    const uint32_t* tab;   // [t verify rows | P(0) row][t + 1] constants (the head of fpmul_wave_table)
    uint32_t *mask, *masked;  // [N]
    uint32_t* in_sh;       // [party][N]
    uint8_t* status;       // [N] as the decode leaves it
    uint32_t* summary;     // the open's summary
    uint32_t* counters;    // the stream's decode counters, zero at the start and at the end
    size_t N;
    int parties, needed, M;  // needed = 2 t + 1 senders, M = t + 1
    int lk;                  // log2 of the lanes that share a table row's products (0 .. 2)
    RowsArg rows;            // rows[i] = party id of the i-th lowest sender
};

// LDS words of one workgroup (4 elements): per wave the parties' shares as limbs at the 12-word stride of wave_core.hpp, the
// opened mask (8 words), x (8) and 4 words that keep the next wave's rows 16-byte aligned at any P; then the table.
struct InputWaveLds {
    size_t per_wave, val, bc, tab, total;
    __host__ __device__ InputWaveLds(int parties, int tab_words) {
        val = 0;
        bc = val + (size_t)parties * 12;  // the opened mask | x
        per_wave = bc + 20;
        tab = 4 * per_wave;
        total = tab + (((size_t)tab_words + 3) & ~(size_t)3);
    }
};

template <class F>
__global__ __launch_bounds__(256) void k_input_wave(InputWaveArgs a) {
    using E = typename F::E;
    static_assert(F::EW == 8 && F::NL == 9, "U29 only");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t g_raw = (size_t)blockIdx.x * 4 + wave;
    const bool live = g_raw < a.N;  // the last workgroup's idle waves redo element N - 1 and store nothing
    const size_t g = live ? g_raw : a.N - 1;
    const int M = a.M, nv = a.needed - M, P = a.parties;
    const int tab_words = (nv + 1) * M * 9;
    const InputWaveLds L(P, tab_words);
    uint32_t* W = lds + (size_t)wave * L.per_wave;
    uint32_t *val = W + L.val, *bc = W + L.bc, *tab = lds + L.tab;

    // ---- every global load of the element, then the LDS writes (wave_core.hpp) ---------------------------------------------------
    TableStage tabs;
    tabs.load(a.tab, tab_words);
    uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0, x0 = r0, x1 = r0;
    if (lane < P) {
        const uint32_t* s = a.r_sh + ((size_t)lane * a.N + g) * 8;
        r0 = *reinterpret_cast<const uint4*>(s), r1 = *reinterpret_cast<const uint4*>(s + 4);
    }
    if (lane == 0) {
        const uint32_t* s = a.x + g * 8;
        x0 = *reinterpret_cast<const uint4*>(s), x1 = *reinterpret_cast<const uint4*>(s + 4);
    }
    tabs.store(tab, a.tab, tab_words);
    const uint32_t rw[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    const E rp = F::from_words(rw);  // party `lane`'s share of the mask, kept for the last step
    if (lane < P) put_limbs<F>(val + lane * 12, rp);
    if (lane == 0) {
        *reinterpret_cast<uint4*>(bc + 8) = x0;
        *reinterpret_cast<uint4*>(bc + 12) = x1;
    }
    __syncthreads();

    // ---- the client's open of the mask (input.rs:489-502) ------------------------------------------------------------------------
    const bool ok = open_single<F>(val, tab, bc, a.lk, nv, M, a.rows, live, g, a.counters, a.mask, a.status);
    __syncthreads();

    // ---- masked = x + mask (input.rs:503-506); party `lane` keeps masked - r (:85-100).  A refused element: zeros ----------------
    if (lane < P) {
        const E masked = F::canon_loose(F::add(F::load(bc + 8), F::load(bc)));
        const E sh = F::canon_loose(F::template sub<2>(masked, rp));
        if (live) {
            put_words<F>(a.in_sh + ((size_t)lane * a.N + g) * 8, ok ? sh : F::zero());
            if (lane == 0) put_words<F>(a.masked + g * 8, ok ? masked : F::zero());
        }
    }

    // ---- the summary: the last workgroup turns the counters into it and leaves the counters at zero ----------------------------
    finish_direct(a.counters, a.summary);
}

}  // namespace hbmpc
