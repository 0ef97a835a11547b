// include/hbmpc_pipelines.hpp's Input and Output (hbmpc_pipe_input_create, hbmpc_pipe_output_create) against the protocol algebra at
// n = 4, t = 1, N = 5: the client's values go in through Input, the shares it leaves go to Output, and what Output opens is what
// the client put in.  Both settings of the one-launch threshold, then the same sequence replayed as a HIP graph.
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
static bool same(const std::vector<U256>& a, const std::vector<U256>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(U256)) == 0;
}

static std::vector<U256> round_trip(void* stream) {
    const size_t n = 4, t = 1, N = 5;
    std::vector<U256> x(N), mask(N);
    for (size_t i = 0; i < N; ++i) x[i] = rand_fr(), mask[i] = rand_fr();
    Input in(context(), n, t, N, stream);
    in.upload(in.x, x.data(), N);
    in.upload(in.r, share_all(mask, n, t).data(), n * N);
    in.run();
    std::vector<U256> sh(n * N), opened(N), masked(N), sum(N);
    in.download(sh.data(), in.out, n * N);
    in.download(opened.data(), in.mask, N);
    in.download(masked.data(), in.masked, N);
    CHECK(in.last_summary().n_failed == 0);
    pl_check(hbmpc_fr_op(context(), 0, x.data(), mask.data(), N, sum.data()), context(), "add");
    CHECK(same(opened, mask) && same(masked, sum));  // the opened masks, and x + mask
    Output out(context(), n, t, N, stream);
    out.upload(out.sh, sh.data(), n * N);
    out.run();
    std::vector<U256> back(N);
    out.download(back.data(), out.out, N);
    CHECK(out.last_summary().n_failed == 0);
    CHECK(same(back, x));  // the shares Input leaves open to the client's values
    in.capture();
    std::vector<U256> zero(n * N, U256{{0, 0, 0, 0}}), sh2(n * N);
    in.upload(in.out, zero.data(), n * N);
    in.replay();
    in.download(sh2.data(), in.out, n * N);
    CHECK(same(sh, sh2));
    out.capture();
    out.upload(out.out, zero.data(), N);
    out.replay();
    out.download(back.data(), out.out, N);
    CHECK(same(back, x));
    return sh;
}

int main() {
    void* stream = nullptr;
    pl_check(hbmpc_stream_create(context(), &stream), context(), "stream_create");
    std::printf("input -> output (one launch where the call qualifies)\n");
    pl_check(hbmpc_set_fused_input(context(), (size_t)1 << 20), context(), "set_fused_input");
    g_state = 7;
    const std::vector<U256> one = round_trip(stream);
    std::printf("input -> output (the separate launches)\n");
    pl_check(hbmpc_set_fused_input(context(), 0), context(), "set_fused_input");
    g_state = 7;
    CHECK(same(one, round_trip(stream)));  // the same inputs: the same bytes in both forms
    pl_check(hbmpc_stream_destroy(context(), stream), context(), "stream_destroy");
    std::printf(g_failed ? "%d CHECKS FAILED\n" : "input pipeline passed (%d failures)\n", g_failed);
    return g_failed ? 1 : 0;
}
