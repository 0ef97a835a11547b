// the element-wise kernels of one party or of all parties of a device (kernels_elem.hpp): a lane per element, 256 lanes per
// workgroup; the party-batched ones take the party from blockIdx.y
#include "field_dispatch.hpp"
#include "fr_gold.hpp"
#include "kernels_elem.hpp"
#include "launchers.hpp"
namespace hbmpc {
static dim3 elem_grid(size_t N, unsigned parties = 1) { return dim3((unsigned)((N + 255) / 256), parties); }
// the run-time op (validated by the caller) becomes the kernels' compile-time OP here, once for every field
void launch_binop(int impl, int op, const uint32_t* a, const uint32_t* b, size_t N, const ElemConsts& cs, uint32_t* out, hipStream_t s) {
    by_field(impl, [&](auto f) {
        using F = typename decltype(f)::type;
        if (op == OP_ADD) hipLaunchKernelGGL((k_binop<F, OP_ADD>), elem_grid(N), dim3(256), 0, s, a, b, N, cs, out);
        else if (op == OP_SUB) hipLaunchKernelGGL((k_binop<F, OP_SUB>), elem_grid(N), dim3(256), 0, s, a, b, N, cs, out);
        else if (op == OP_MUL) hipLaunchKernelGGL((k_binop<F, OP_MUL>), elem_grid(N), dim3(256), 0, s, a, b, N, cs, out);
    });
}
void launch_scalarop(int impl, int op, const uint32_t* a, const ScalarArg& sc, size_t N, const ElemConsts& cs, uint32_t* out, hipStream_t s) {
    by_field(impl, [&](auto f) {
        using F = typename decltype(f)::type;
        if (op == OP_ADD) hipLaunchKernelGGL((k_scalarop<F, OP_ADD>), elem_grid(N), dim3(256), 0, s, a, sc, N, cs, out);
        else if (op == OP_SUB) hipLaunchKernelGGL((k_scalarop<F, OP_SUB>), elem_grid(N), dim3(256), 0, s, a, sc, N, cs, out);
        else if (op == OP_MUL) hipLaunchKernelGGL((k_scalarop<F, OP_MUL>), elem_grid(N), dim3(256), 0, s, a, sc, N, cs, out);
        else if (op == OP_RSUB) hipLaunchKernelGGL((k_scalarop<F, OP_RSUB>), elem_grid(N), dim3(256), 0, s, a, sc, N, cs, out);
    });
}
void launch_triple_local(int impl, const uint32_t* a, const uint32_t* b, const uint32_t* r2t, size_t N, const ElemConsts& cs, uint32_t* out, hipStream_t s) {
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_triple_local<field_t<decltype(f)>>), elem_grid(N), dim3(256), 0, s, a, b, r2t, N, cs, out); });
}
void launch_triple_finalize(int impl, const uint32_t* rt, const uint32_t* opened, size_t N, unsigned parties, uint32_t* c_out, hipStream_t s) {
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_triple_finalize<field_t<decltype(f)>>), elem_grid(N, parties), dim3(256), 0, s, rt, opened, N, c_out); });
}
void launch_beaver_open(int impl, const uint32_t* a, const uint32_t* b, const uint32_t* x, const uint32_t* y, size_t N, uint32_t* d_sh, uint32_t* e_sh,
                        hipStream_t s) {
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_beaver_open<field_t<decltype(f)>>), elem_grid(N), dim3(256), 0, s, a, b, x, y, N, d_sh, e_sh); });
}
void launch_beaver_open_pair(int impl, const uint32_t* a, const uint32_t* b, const uint32_t* x, const uint32_t* y, size_t N, unsigned parties, uint32_t* de,
                             hipStream_t s) {
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_beaver_open_pair<field_t<decltype(f)>>), elem_grid(N, parties), dim3(256), 0, s, a, b, x, y, N, de); });
}
void launch_beaver_finalize(int impl, const uint32_t* c, const uint32_t* x, const uint32_t* y, const uint32_t* d, const uint32_t* e, size_t N,
                            const ElemConsts& cs, uint32_t* z, unsigned parties, unsigned grid_parties, hipStream_t s) {
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_beaver_finalize<field_t<decltype(f)>>), elem_grid(N, grid_parties), dim3(256), 0, s, c, x, y, d, e, N, cs, z, parties); });
}
void launch_truncpr_rdash(int impl, const uint32_t* r_bits, int m, size_t N, unsigned parties, const uint32_t* pow2, uint32_t* r_dash, hipStream_t s) {
    by_fr_impl(impl, [&](auto f) { hipLaunchKernelGGL((k_truncpr_rdash<field_t<decltype(f)>>), elem_grid(N, parties), dim3(256), 0, s, r_bits, m, N, pow2, r_dash); });
}
void launch_truncpr_open(int impl, const uint32_t* a, const uint32_t* r_dash, const uint32_t* r_int, size_t N, const ElemConsts& cs, uint32_t* open_out,
                         hipStream_t s) {
    by_fr_impl(impl, [&](auto f) { hipLaunchKernelGGL((k_truncpr_open<field_t<decltype(f)>>), elem_grid(N), dim3(256), 0, s, a, r_dash, r_int, N, cs, open_out); });
}
void launch_fpmul_middle(int impl, const uint32_t* c, const uint32_t* x, const uint32_t* y, const uint32_t* d, const uint32_t* e, const uint32_t* r_bits,
                         const uint32_t* r_int, int m, size_t N, const ElemConsts& cs, const uint32_t* pow2, uint32_t* z, uint32_t* r_dash,
                         uint32_t* open_out, unsigned parties, unsigned grid_parties, hipStream_t s) {
    by_fr_impl(impl, [&](auto f) { hipLaunchKernelGGL((k_fpmul_middle<field_t<decltype(f)>>), elem_grid(N, grid_parties), dim3(256), 0, s,
                       c, x, y, d, e, r_bits, r_int, m, N, cs, pow2, z, r_dash, open_out, parties); });
}
void launch_truncpr_front(int impl, const uint32_t* a, const uint32_t* w, const uint32_t* r_bits, const uint32_t* r_int, int m, size_t N,
                          const ElemConsts& cs, const uint32_t* pow2, uint32_t* c, uint32_t* r_dash, uint32_t* open_out, unsigned parties,
                          unsigned grid_parties, hipStream_t s) {
    by_fr_impl(impl, [&](auto f) {
        using F = field_t<decltype(f)>;
        if (w) hipLaunchKernelGGL((k_truncpr_front<F, true>), elem_grid(N, grid_parties), dim3(256), 0, s, a, w, r_bits, r_int, m, N, cs, pow2, c, r_dash, open_out, parties);
        else hipLaunchKernelGGL((k_truncpr_front<F, false>), elem_grid(N, grid_parties), dim3(256), 0, s, a, w, r_bits, r_int, m, N, cs, pow2, c, r_dash, open_out, parties);
    });
}
void launch_truncpr_finalize(int impl, const uint32_t* a, const uint32_t* r_dash, const uint32_t* c_open, int m, size_t N, unsigned parties,
                             const ElemConsts& cs, uint32_t* d_out, hipStream_t s) {
    by_fr_impl(impl, [&](auto f) { hipLaunchKernelGGL((k_truncpr_finalize<field_t<decltype(f)>>), elem_grid(N, parties), dim3(256), 0, s, a, r_dash, c_open, m, N, cs, d_out); });
}
void launch_input_finish(int impl, const uint8_t* status, uint32_t* mask, const uint32_t* x, const uint32_t* r, size_t N, unsigned parties, uint32_t* masked,
                         uint32_t* in_sh, hipStream_t s) {
    by_field(impl, [&](auto f) { hipLaunchKernelGGL((k_input_finish<field_t<decltype(f)>>), elem_grid(N, parties + 1), dim3(256), 0, s, status, mask, x, r, N, masked, in_sh); });
}
void launch_modmul_ubench(int impl, uint32_t* out, size_t threads, uint32_t iters, const ElemConsts& cs, hipStream_t s) {
    by_fr_impl(impl, [&](auto f) { hipLaunchKernelGGL((k_modmul_ubench<field_t<decltype(f)>>), elem_grid(threads), dim3(256), 0, s, out, iters, cs); });
}
void launch_traffic_ubench(unsigned wgs, const uint4* x, size_t G, int m, uint4* y, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_traffic_ubench, dim3(wgs), dim3(768), 0, s, x, G, m, y, n);
}
}  // namespace hbmpc
