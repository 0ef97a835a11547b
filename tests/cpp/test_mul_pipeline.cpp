// include/hbmpc_pipelines.hpp's Mul (Beaver multiplication for all n simulated parties, hbmpc_pipe_mul_create) against the
// protocol algebra at n = 4, t = 1, N = 5: upload, run and download; with c = a b the output opens to x y.  Both settings of the
// one-launch threshold, then the same sequence replayed as a HIP graph.
#include <cstdio>
#include <cstring>
#include <vector>

#include "hbmpc_pipelines.hpp"
#include "hbmpc_shares.hpp"

using namespace hbmpc;
static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            ++g_failed;                                                          \
        }                                                                        \
    } while (0)

static uint64_t g_state = 0x0123456789ABCDEFull;
static uint64_t next64() {
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static U256 rand_fr() { return U256{{next64(), next64(), next64(), next64() % 0x73eda753299d7d48ULL}}; }

// [n][N] degree-d sharings of N secrets (random higher coefficients), by the library's own compute_shares
static std::vector<U256> share_all(const std::vector<U256>& secrets, size_t n, size_t d) {
    const size_t N = secrets.size();
    std::vector<U256> coeffs(N * (d + 1)), out(n * N);
    for (size_t i = 0; i < N; ++i) {
        coeffs[i * (d + 1)] = secrets[i];
        for (size_t k = 1; k <= d; ++k) coeffs[i * (d + 1) + k] = rand_fr();
    }
    pl_check(hbmpc_compute_shares(context(), coeffs.data(), N, n, d, out.data()), context(), "compute_shares");
    return out;
}
static std::vector<U256> open_all(const std::vector<U256>& shares, size_t n, size_t N, size_t d, size_t t) {
    std::vector<size_t> ids;
    for (size_t i = 0; i < n; ++i) ids.push_back(i);
    std::vector<U256> p0(N);
    pl_check(hbmpc_batch_recover_p0(context(), ids.data(), n, shares.data(), N, n, d, t, p0.data(), nullptr), context(), "open");
    return p0;
}
static std::vector<U256> mul_all(const std::vector<U256>& a, const std::vector<U256>& b) {
    std::vector<U256> c(a.size());
    pl_check(hbmpc_fr_op(context(), 2, a.data(), b.data(), a.size(), c.data()), context(), "mul");
    return c;
}
static bool same(const std::vector<U256>& a, const std::vector<U256>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(U256)) == 0;
}

static std::vector<U256> mul(void* stream) {
    const size_t n = 4, t = 1, N = 5;
    std::vector<U256> x(N), y(N), ta(N), tb(N);
    for (size_t i = 0; i < N; ++i) x[i] = rand_fr(), y[i] = rand_fr(), ta[i] = rand_fr(), tb[i] = rand_fr();
    Mul mp(context(), n, t, N, stream);
    mp.upload(mp.x, share_all(x, n, t).data(), n * N);
    mp.upload(mp.y, share_all(y, n, t).data(), n * N);
    mp.upload(mp.ta, share_all(ta, n, t).data(), n * N);
    mp.upload(mp.tb, share_all(tb, n, t).data(), n * N);
    mp.upload(mp.tc, share_all(mul_all(ta, tb), n, t).data(), n * N);
    mp.run();
    std::vector<U256> out(n * N), dop(N), eop(N);
    mp.download(out.data(), mp.out, n * N);
    mp.download(dop.data(), mp.dop, N);
    mp.download(eop.data(), mp.eop, N);
    CHECK(mp.last_summary().n_failed == 0);
    CHECK(same(open_all(out, n, N, t, t), mul_all(x, y)));  // [z]_t opens to x * y
    std::vector<U256> d(N), e(N);
    pl_check(hbmpc_fr_op(context(), 1, ta.data(), x.data(), N, d.data()), context(), "sub");
    pl_check(hbmpc_fr_op(context(), 1, tb.data(), y.data(), N, e.data()), context(), "sub");
    CHECK(same(dop, d) && same(eop, e));  // the opened a - x and b - y
    mp.capture();
    std::vector<U256> zero(n * N, U256{{0, 0, 0, 0}}), out2(n * N);
    mp.upload(mp.out, zero.data(), n * N);
    mp.replay();
    mp.download(out2.data(), mp.out, n * N);
    CHECK(same(out, out2));
    return out;
}

int main() {
    void* stream = nullptr;
    pl_check(hbmpc_stream_create(context(), &stream), context(), "stream_create");
    std::printf("mul (one launch where the call qualifies)\n");
    pl_check(hbmpc_set_fused_mul(context(), (size_t)1 << 20), context(), "set_fused_mul");
    g_state = 7;
    const std::vector<U256> one = mul(stream);
    std::printf("mul (the separate launches)\n");
    pl_check(hbmpc_set_fused_mul(context(), 0), context(), "set_fused_mul");
    g_state = 7;
    CHECK(same(one, mul(stream)));  // the same inputs: the same bytes in both forms
    pl_check(hbmpc_stream_destroy(context(), stream), context(), "stream_destroy");
    std::printf(g_failed ? "%d CHECKS FAILED\n" : "mul pipeline passed (%d failures)\n", g_failed);
    return g_failed ? 1 : 0;
}
