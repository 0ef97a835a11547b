// launchers.hpp -- every kernel instantiation and every launch lives in a translation unit of its own kind (tu_*.hip), so
// that they compile in parallel and the C ABI files (hbmpc_capi.hip, capi_*.inc, capi_pipelines.hip) hold host code only; these
// are their entry points.  A bool one returns false when the requested shape is not one it instantiates.  Where a launcher
// takes `impl` (FieldImpl), the field type is picked by by_field / by_fr_impl of field_dispatch.hpp and nowhere else.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "eval_out.hpp"
#include "kernels_gao.hpp"
#include "kernels_recover.hpp"

#include <atomic>

namespace hbmpc {

// More than 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize once per (kernel, device).  Returns
// false when the launch must not be attempted (the caller falls back to the lane kernels): a device ordinal beyond the
// table, or the attribute call failed.  Threads that drive different contexts on one device may race here: the flag is
// atomic and setting the attribute twice is harmless.
constexpr int HBMPC_MAX_DEVICES = 64;
inline bool ensure_dynamic_lds(const void* kernel, std::atomic<bool>* flags, int device, size_t lds_bytes) {
    if (lds_bytes <= 64 * 1024) return true;
    if (device < 0 || device >= HBMPC_MAX_DEVICES) return false;
    if (flags[device].load(std::memory_order_acquire)) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    flags[device].store(true, std::memory_order_release);
    return true;
}

// single-pass pruned FFT, U29, size = 2^log <= 16, cnt = d+1 coefficients
bool launch_fft1_lo(int log, int cnt, const uint32_t* x, size_t G, int n, const uint32_t* tw, EvalOut y, hipStream_t s);
bool launch_fft1_16a(int cnt, const uint32_t* x, size_t G, int n, const uint32_t* tw, EvalOut y, hipStream_t s);
bool launch_fft1_16b(int cnt, const uint32_t* x, size_t G, int n, const uint32_t* tw, EvalOut y, hipStream_t s);
bool launch_fft1_16c(int cnt, const uint32_t* x, size_t G, int n, const uint32_t* tw, EvalOut y, hipStream_t s);
bool launch_fft1_16d(int cnt, const uint32_t* x, size_t G, int n, const uint32_t* tw, EvalOut y, hipStream_t s);
inline bool launch_fft1_16(int cnt, const uint32_t* x, size_t G, int n, const uint32_t* tw, EvalOut y, hipStream_t s) {
    return launch_fft1_16a(cnt, x, G, n, tw, y, s) || launch_fft1_16b(cnt, x, G, n, tw, y, s) || launch_fft1_16c(cnt, x, G, n, tw, y, s) ||
           launch_fft1_16d(cnt, x, G, n, tw, y, s);
}
// triple_gen's local product fused into the encode (k_eval_fft1_triple); false when the shape is not instantiated
bool launch_fft1_triple(int lg, int cnt, const uint32_t* a, const uint32_t* b, const uint32_t* r2t, size_t G, int n,
                        const uint32_t* tw, EvalOut y, const uint32_t r2[9], hipStream_t s);
bool launch_fft1_triple_gold(int lg, int cnt, const uint32_t* a, const uint32_t* b, const uint32_t* r2t, size_t G, int n,
                             const uint32_t* tw, EvalOut y, hipStream_t s);
// multi-pass (size = 16 P), U29, dp1 <= 32
bool launch_fftP_a(int dp1, const uint32_t* x, size_t G, int n, int P, const uint32_t* tw16, const uint32_t* twist,
                   EvalOut y, hipStream_t s);
bool launch_fftP_b(int dp1, const uint32_t* x, size_t G, int n, int P, const uint32_t* tw16, const uint32_t* twist,
                   EvalOut y, hipStream_t s);
bool launch_fftP_c(int dp1, const uint32_t* x, size_t G, int n, int P, const uint32_t* tw16, const uint32_t* twist,
                   EvalOut y, hipStream_t s);
bool launch_fftP_d(int dp1, const uint32_t* x, size_t G, int n, int P, const uint32_t* tw16, const uint32_t* twist,
                   EvalOut y, hipStream_t s);
bool launch_fftP_fold(int dp1, const uint32_t* x, size_t G, int n, int P, const uint32_t* tw16, const uint32_t* twist,
                      EvalOut y, hipStream_t s);
inline bool launch_fftP(int dp1, const uint32_t* x, size_t G, int n, int P, const uint32_t* tw16, const uint32_t* twist, EvalOut y,
                        hipStream_t s) {
    return launch_fftP_a(dp1, x, G, n, P, tw16, twist, y, s) || launch_fftP_b(dp1, x, G, n, P, tw16, twist, y, s) ||
           launch_fftP_c(dp1, x, G, n, P, tw16, twist, y, s) || launch_fftP_d(dp1, x, G, n, P, tw16, twist, y, s) ||
           launch_fftP_fold(dp1, x, G, n, P, tw16, twist, y, s);
}
// Goldilocks instantiations of the same templates
bool launch_gold_fft1(int log, int cnt, const uint32_t* x, size_t G, int n, const uint32_t* tw, EvalOut y, hipStream_t s);
bool launch_gold_fftP(int dp1, const uint32_t* x, size_t G, int n, int P, const uint32_t* tw16, const uint32_t* twist,
                      EvalOut y, hipStream_t s);
bool launch_gold_recover(int m, bool p0, const RecoverArgs& ra, unsigned grid, hipStream_t s);
// the small-weight encode of the integer-point Shamir scheme (kernels_shamir.hpp); nl = 8 (Fr) or 2 (Goldilocks), the launch shape from
// plan_shamir_encode (shamir_route.hpp)
void launch_shamir_encode(int nl, bool w32, const void* coeffs, size_t B, int m, int dp1, const uint64_t* w, void* out, int waves,
                          size_t lds_bytes, int row_units, hipStream_t s);
// generic Horner evaluation
void launch_eval_generic(int impl, const uint32_t* x, size_t G, int n, int dp1, const uint32_t* alpha, EvalOut y,
                         hipStream_t s);
// batch recover, U29, register-resident m <= 16 (launch_recover tries the four translation units)
bool launch_recover_a(int m, bool p0, const RecoverArgs& ra, unsigned grid, hipStream_t s);
bool launch_recover_b(int m, bool p0, const RecoverArgs& ra, unsigned grid, hipStream_t s);
bool launch_recover_c(int m, bool p0, const RecoverArgs& ra, unsigned grid, hipStream_t s);
bool launch_recover_d(int m, bool p0, const RecoverArgs& ra, unsigned grid, hipStream_t s);
inline bool launch_recover(int m, bool p0, const RecoverArgs& ra, unsigned grid, hipStream_t s) {
    return launch_recover_a(m, p0, ra, grid, s) || launch_recover_b(m, p0, ra, grid, s) || launch_recover_c(m, p0, ra, grid, s) ||
           launch_recover_d(m, p0, ra, grid, s);
}

void launch_recover_generic(int impl, bool p0, const RecoverArgs& ra, unsigned grid, hipStream_t s);
// matrix-core form of the constant-matrix maps (kernels_mfma.hpp), m = 2 .. 15; false when m is not instantiated there.
// team: the workgroup-per-tile form for batches with fewer tiles than waves (kernels_mfma_team.hpp)
namespace mf { struct MfmaRowsArgs; struct MfmaGlArgs; }
bool launch_mfma_rows_gl(const mf::MfmaGlArgs& a, unsigned grid, int device, hipStream_t s);  // Goldilocks (kernels_mfma_gl.hpp)
// the decode whose sender values are differences formed after loading (k_mfma_rows<.., SUB>), m = 2 .. MF_SUB_MAX_M (tables_mfma.hpp)
bool launch_mfma_rows_sub(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s);
bool launch_mfma_rows_a(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s, bool team = false);
bool launch_mfma_rows_b(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s, bool team = false);
bool launch_mfma_rows_c(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s, bool team = false);
bool launch_mfma_rows_d(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s, bool team = false);
inline bool launch_mfma_rows(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s, bool team = false) {
    return launch_mfma_rows_a(m, a, device, s, team) || launch_mfma_rows_b(m, a, device, s, team) || launch_mfma_rows_c(m, a, device, s, team) ||
           launch_mfma_rows_d(m, a, device, s, team);
}
// the encode on a domain of roots of unity with the points taken in pairs (k, k + size / 2): half the MFMAs (kernels_mfma_bfly.hpp);
// with a.in_b set: the fused local product + encode of triple generation (one role of 8 or 16 pairs; false otherwise)
bool launch_mfma_bfly_a(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s);
bool launch_mfma_bfly_b(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s);
bool launch_mfma_bfly_c(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s);
bool launch_mfma_bfly_d(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s);
inline bool launch_mfma_bfly(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s) {
    return launch_mfma_bfly_a(m, a, device, s) || launch_mfma_bfly_b(m, a, device, s) || launch_mfma_bfly_c(m, a, device, s) ||
           launch_mfma_bfly_d(m, a, device, s);
}
// the ring form of the plain chunk-major paired-point encode (kernels_mfma_bfly_ring.hpp: a loader wave fills an LDS ring with whole
// lines); false, with nothing enqueued, for every shape bfly_ring_plan.hpp does not take -- the caller then uses launch_mfma_bfly
bool launch_mfma_bfly_ring(int m, const mf::MfmaRowsArgs& a, int device, hipStream_t s);
// small batches: one wave per chunk, one evaluation point / one table row per lane (k_eval_wide, k_batch_recover_wide)
void launch_eval_wide(int impl, const uint32_t* x, size_t G, int n, int dp1, const uint32_t* alpha, EvalOut y, hipStream_t s);
void launch_eval_wide_dot(const uint32_t* x, size_t G, int n, int dp1, const uint32_t* vmat, EvalOut y, hipStream_t s);  // U29, vmat [n][dp1] <= 48 KB
void launch_recover_wide(int impl, bool p0, const RecoverArgs& ra, const SecondArgs* fused_second, hipStream_t s, int ow_sel = 0);  // ow_sel: output rows when the table holds selected ones
// FPMulNode for all parties of a small batch in one launch (kernels_fpmul_wave.hpp); false: the shape does not fit a workgroup's LDS
struct FpmulWaveArgs;
struct TripleGenWgArgs;
void launch_triplegen_wg(int impl, const TripleGenWgArgs& a, hipStream_t s);  // TripleGenNode, a workgroup per chunk (kernels_triplegen_wg.hpp): U29 or Goldilocks
struct RandBitWgArgs;
void launch_randbit_wg(int impl, const RandBitWgArgs& a, hipStream_t s);  // RandBit, a workgroup per chunk of t + 1 elements (kernels_randbit_wg.hpp): U29 or Goldilocks
// BatchReconNode, a workgroup per chunk of d + 1 elements (kernels_batchrecon_wg.hpp): U29 or Goldilocks.  false: no kernel over this
// field, the layout does not fit a workgroup's LDS or the LDS attribute could not be set; dry_run: only say which
struct BatchReconWgArgs;
bool launch_batchrecon_wg(int impl, const BatchReconWgArgs& a, int device, hipStream_t s, bool dry_run);
// RanSha / RanDouSha (randousha), a workgroup per batch element (kernels_producers_wg.hpp): U29 or Goldilocks.  false as above
struct ProducersWgArgs;
bool launch_producers_wg(int impl, bool randousha, const ProducersWgArgs& a, int device, hipStream_t s, bool dry_run);
bool launch_fpmul_wave(const FpmulWaveArgs& a, int device, hipStream_t s, bool dry_run);
// TruncPrNode / FPDivConstNode (a.w set) the same way (kernels_truncpr_wave.hpp); dry_run: only say whether the LDS layout fits
struct TruncprWaveArgs;
bool launch_truncpr_wave(const TruncprWaveArgs& a, int device, hipStream_t s, bool dry_run);
// Multiply (Beaver) the same way (kernels_mul_wave.hpp)
struct MulWaveArgs;
bool launch_mul_wave(const MulWaveArgs& a, int device, hipStream_t s, bool dry_run);
// Input the same way (kernels_input_wave.hpp)
struct InputWaveArgs;
bool launch_input_wave(const InputWaveArgs& a, int device, hipStream_t s, bool dry_run);
// flagged chunks: two cheap interpolation candidates before the OEC/Gao kernel (k_second_chance)
void launch_second_chance(int impl, const SecondArgs& a, unsigned grid, hipStream_t s);
bool launch_second_chance_m(int m, const SecondArgs& a, unsigned grid, hipStream_t s);  // U29, m = 2 .. 16 at compile time; false otherwise
// OEC / Gao, matvec
void launch_gao_u29(const GaoArgs& ga, size_t n, unsigned grid, hipStream_t s, bool inline_unscale);
void launch_gao_sat(const GaoArgs& ga, size_t n, unsigned grid, hipStream_t s, bool inline_unscale);
void launch_gao_gold(const GaoArgs& ga, size_t n, unsigned grid, hipStream_t s, bool inline_unscale);
void launch_matvec(int impl, const uint32_t* lb, const uint32_t* y, int S, uint32_t* out, hipStream_t s);

// seeded coefficient generation (kernels_rng.hpp); ew = u32 words per element
void launch_fill_coeffs(int ew, const uint32_t seed[8], const uint32_t* secrets, size_t B, uint64_t first_index, int dp1,
                        uint32_t* coeffs, hipStream_t s);
// wire codec (kernels_codec.hpp)
void launch_pack_fvec(const uint64_t* rows, size_t row_stride, size_t G, size_t n_rows, uint64_t* payloads,
                      size_t payload_stride_words, hipStream_t s);
void launch_fvec_prefix(uint64_t* payloads, size_t payload_stride_words, size_t G, size_t n_rows, hipStream_t s);
void launch_validate_fvec(const uint64_t* payloads, size_t payload_stride_words, size_t G, size_t n_rows, uint32_t* status,
                          hipStream_t s, bool gold = false);
void launch_unpack_fvec(const uint64_t* payloads, size_t payload_stride_words, size_t G, size_t n_rows, uint64_t* rows,
                        size_t row_stride, uint32_t* status, hipStream_t s);
void launch_pack_shares(const uint64_t* values, size_t N, uint64_t id, uint64_t degree, uint64_t* payload, hipStream_t s);
void launch_unpack_shares(const uint64_t* payload, size_t N, uint64_t id, uint64_t degree, uint64_t* values,
                          uint32_t* status, hipStream_t s);
void launch_validate_canonical(const uint64_t* a, size_t N, uint32_t* status, hipStream_t s);
void launch_poly_degree(const uint64_t* coeffs, size_t G, int m, int ew64, uint32_t* degree_out, hipStream_t s, uint64_t* c0_out = nullptr);  // c0_out: the constant terms too
void launch_mfma_table(const uint64_t* coeff, int m, int rows, const uint64_t e[4], uint32_t bmag, uint8_t* table, uint64_t* partial,
                       hipStream_t s);  // kernels_tables.hpp
// layout + verdict kernels of the preprocessing producers (kernels_codec.hpp); ew64 = 64-bit words per element
void launch_transpose(int ew64, const uint64_t* src, size_t rows, size_t cols, size_t src_row_stride, uint64_t* dst, size_t dst_row_stride,
                      size_t batch, size_t src_batch_stride, size_t dst_batch_stride, hipStream_t s);
void launch_check_degree(int ew64, const uint64_t* coeffs, const uint8_t* status, size_t G, int m, int want, uint32_t* bad, hipStream_t s);
void launch_check_double_sel(int ew64, const uint64_t* sel_t, const uint8_t* st_t, const uint64_t* sel_2t, const uint8_t* st_2t, size_t G, int t, uint32_t* bad,
                             hipStream_t s, size_t columns = 0);
void launch_pick_two(int ew64, const uint64_t* coeffs, size_t G, int m, int d, uint64_t* sel, uint8_t* status, hipStream_t s);
void launch_check_top_coeff(int ew64, const uint64_t* top, const uint8_t* status, size_t G, int want, uint32_t* bad, hipStream_t s, size_t columns = 0);
void launch_check_double(int ew64, const uint64_t* ct, const uint64_t* c2t, size_t G, int m, int t, uint32_t* bad, hipStream_t s);
void launch_check_double_c0(int ew64, const uint64_t* c0t, const uint32_t* degt, const uint64_t* c02t, const uint32_t* deg2t, size_t G, int t,
                            uint32_t* bad, hipStream_t s, size_t columns = 0);
bool launch_fft1_mix_lo(int log, int cnt, const uint32_t* x, size_t xs, size_t G, int n, const uint32_t* tw, const MixOut& o, hipStream_t s);
bool launch_gold_fft1_mix(int log, int cnt, const uint32_t* x, size_t xs, size_t G, int n, const uint32_t* tw, const MixOut& o, hipStream_t s);
void launch_rows_party_major(int ew64, const uint64_t* src, size_t G, size_t K, int row0, int rows, int nother, uint64_t* dst, hipStream_t s);
void launch_take_c0(int ew64, const uint64_t* coeffs, size_t G, int m, uint64_t* c0, hipStream_t s);
// slices of [party][len] pools, regrouped (tu_take.hip, kernels_take.hpp; the arguments and the tile rule: take_plan.hpp)
struct TakeArgs;
void launch_take_rows(int ew64, const TakeArgs& a, unsigned tiles, unsigned rows, unsigned count, hipStream_t s);

// element-wise share arithmetic (tu_elem.hip, kernels_elem.hpp): a lane per element; `parties` > 1: [party][N] operands, the
// party in blockIdx.y.  grid_parties of the two kernels that loop over the parties themselves: 1 or `parties` (the caller picks by N)
struct ElemConsts;
struct ScalarArg;
void launch_binop(int impl, int op, const uint32_t* a, const uint32_t* b, size_t N, const ElemConsts& cs, uint32_t* out, hipStream_t s);
void launch_scalarop(int impl, int op, const uint32_t* a, const ScalarArg& sc, size_t N, const ElemConsts& cs, uint32_t* out, hipStream_t s);
void launch_triple_local(int impl, const uint32_t* a, const uint32_t* b, const uint32_t* r2t, size_t N, const ElemConsts& cs, uint32_t* out, hipStream_t s);
void launch_triple_finalize(int impl, const uint32_t* rt, const uint32_t* opened, size_t N, unsigned parties, uint32_t* c_out, hipStream_t s);
void launch_beaver_open(int impl, const uint32_t* a, const uint32_t* b, const uint32_t* x, const uint32_t* y, size_t N, uint32_t* d_sh, uint32_t* e_sh,
                        hipStream_t s);
void launch_beaver_open_pair(int impl, const uint32_t* a, const uint32_t* b, const uint32_t* x, const uint32_t* y, size_t N, unsigned parties, uint32_t* de,
                             hipStream_t s);
void launch_beaver_finalize(int impl, const uint32_t* c, const uint32_t* x, const uint32_t* y, const uint32_t* d, const uint32_t* e, size_t N,
                            const ElemConsts& cs, uint32_t* z, unsigned parties, unsigned grid_parties, hipStream_t s);
// Fr only (by_fr_impl)
void launch_truncpr_rdash(int impl, const uint32_t* r_bits, int m, size_t N, unsigned parties, const uint32_t* pow2, uint32_t* r_dash, hipStream_t s);
void launch_truncpr_open(int impl, const uint32_t* a, const uint32_t* r_dash, const uint32_t* r_int, size_t N, const ElemConsts& cs, uint32_t* open_out,
                         hipStream_t s);
void launch_fpmul_middle(int impl, const uint32_t* c, const uint32_t* x, const uint32_t* y, const uint32_t* d, const uint32_t* e, const uint32_t* r_bits,
                         const uint32_t* r_int, int m, size_t N, const ElemConsts& cs, const uint32_t* pow2, uint32_t* z, uint32_t* r_dash,
                         uint32_t* open_out, unsigned parties, unsigned grid_parties, hipStream_t s);
void launch_truncpr_front(int impl, const uint32_t* a, const uint32_t* w, const uint32_t* r_bits, const uint32_t* r_int, int m, size_t N,
                          const ElemConsts& cs, const uint32_t* pow2, uint32_t* c, uint32_t* r_dash, uint32_t* open_out, unsigned parties,
                          unsigned grid_parties, hipStream_t s);  // w null: no multiplier (c is not written)
void launch_truncpr_finalize(int impl, const uint32_t* a, const uint32_t* r_dash, const uint32_t* c_open, int m, size_t N, unsigned parties,
                             const ElemConsts& cs, uint32_t* d_out, hipStream_t s);
// Input after the open, either field: masked = x + mask, in_sh[p] = masked - r[p]; a mask that did not open (status >= 2) leaves zeros
void launch_input_finish(int impl, const uint8_t* status, uint32_t* mask, const uint32_t* x, const uint32_t* r, size_t N, unsigned parties, uint32_t* masked,
                         uint32_t* in_sh, hipStream_t s);
void launch_modmul_ubench(int impl, uint32_t* out, size_t threads, uint32_t iters, const ElemConsts& cs, hipStream_t s);
void launch_traffic_ubench(unsigned wgs, const uint4* x, size_t G, int m, uint4* y, int n, hipStream_t s);
// square roots, inverses, RandBit's last step (tu_sqrt.hip, kernels_sqrt.hpp)
struct SqrtTab;
struct RandBitSummaryDev;
void launch_sqrt(int impl, const uint32_t* a, size_t N, const SqrtTab& t, uint32_t* root, uint8_t* has_root, hipStream_t s);
void launch_inverse(int impl, const uint32_t* a, size_t N, const SqrtTab& t, uint32_t* inv, uint8_t* ok, hipStream_t s);
void launch_randbit_finalize(int impl, const uint32_t* a, const uint32_t* sq, size_t N, unsigned parties, const SqrtTab& t, uint32_t* out,
                             uint8_t* status, RandBitSummaryDev* summary, hipStream_t s);
// PRandBit / PRandInt (tu_riss.hip, kernels_riss.hpp)
struct RissTab;
void launch_riss_fold(const uint64_t* contrib, unsigned n, size_t Tn, size_t B, uint64_t bound, uint64_t* sums, uint8_t* bad, hipStream_t s);
// wide: one workgroup per 64 elements and 16 parties; otherwise one per 64 elements and party, the sets in four slices (the caller
// picks by measurement: capi_riss.inc)
void launch_riss_convert(int impl, bool wide, const uint64_t* r, size_t B, unsigned Tn, const RissTab& tab, const uint32_t* cols, unsigned parties,
                         uint32_t* out, uint8_t* out2, hipStream_t s);
void launch_prandbit_finalize(int impl, const uint64_t* v, const uint32_t* r_p, const uint8_t* r_2, size_t N, unsigned parties, uint32_t* bp,
                              uint8_t* b2, hipStream_t s);  // Fr only
// seeded RISS dealing (tu_riss_sample.hip, kernels_riss_sample.hpp; contract "hbmpc-riss-chacha20-v1"): one sender's out [Tn][B], or
// seeds [n][8] words in device memory -> sums [Tn][B] of all n senders.  The grid of launch_riss_fold; bound = 2^lk_bits
void launch_riss_sample(const uint32_t seed[8], uint32_t domain, size_t Tn, size_t B, uint64_t first_index, uint64_t bound, uint64_t* out,
                        hipStream_t s);
void launch_riss_sample_fold(const uint32_t* seeds, unsigned n, uint32_t domain, size_t Tn, size_t B, uint64_t first_index, uint64_t bound,
                             uint64_t* sums, hipStream_t s);
// PRandBit (bit) / PRandInt for all parties, a workgroup per chunk of t + 1 elements (kernels_prandbit_wg.hpp): the Fr side over U29
// only (Goldilocks is the second field inside the same kernel).
// false: the layout does not fit a workgroup's LDS or the LDS attribute could not be set; dry_run: only say which
struct PRandBitWgArgs;
bool launch_prandbit_wg(bool bit, const PRandBitWgArgs& a, int device, hipStream_t s, bool dry_run);

}  // namespace hbmpc
