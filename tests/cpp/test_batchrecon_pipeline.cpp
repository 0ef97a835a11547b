// include/hbmpc_pipelines.hpp's BatchRecon (hbmpc_pipe_batchrecon_create) against the protocol algebra at n = 4, t = 1, d = 1, three
// chunks: degree-1 sharings of six secrets go in, the six secrets come out, through run() and through deal() + finish().  Both settings
// of the one-launch threshold give the same bytes in every buffer, then the same sequence replayed as a HIP graph.
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

struct Outputs {
    std::vector<U256> Y, Z, opened;
    std::vector<uint8_t> rstatus, status;
    bool operator==(const Outputs& o) const { return same(Y, o.Y) && same(Z, o.Z) && same(opened, o.opened) && rstatus == o.rstatus && status == o.status; }
};

static Outputs collect(BatchRecon& br, size_t n, size_t G, size_t N) {
    Outputs o{std::vector<U256>(n * n * G), std::vector<U256>(n * G), std::vector<U256>(N), std::vector<uint8_t>(n * G), std::vector<uint8_t>(G)};
    br.download(o.Y.data(), br.Y, n * n * G);
    br.download(o.Z.data(), br.Z, n * G);
    br.download(o.opened.data(), br.opened, N);
    pl_check(hbmpc_memcpy_d2h(context(), o.rstatus.data(), br.rstatus, n * G, nullptr), context(), "d2h");
    pl_check(hbmpc_memcpy_d2h(context(), o.status.data(), br.status, G, nullptr), context(), "d2h");
    br.sync();
    pl_check(hbmpc_stream_sync(context(), nullptr), context(), "sync");
    return o;
}

static Outputs round_trip(void* stream) {
    const size_t n = 4, t = 1, d = 1, G = 3, N = G * (d + 1);
    std::vector<U256> secrets(N);
    for (size_t i = 0; i < N; ++i) secrets[i] = rand_fr();
    BatchRecon br(context(), n, t, d, N, stream);
    br.upload(br.x, share_all(secrets, n, d).data(), n * N);
    br.run(true);
    const Outputs eager = collect(br, n, G, N);
    CHECK(br.last_summary().n_failed == 0);
    CHECK(same(eager.opened, secrets));  // the sharings open to their secrets
    for (uint8_t s : eager.rstatus) CHECK(s == 0);
    for (uint8_t s : eager.status) CHECK(s == 0);
    // the two arms as separate launches leave the same bytes
    std::vector<U256> zero(n * n * G, U256{{0, 0, 0, 0}});
    br.upload(br.Y, zero.data(), n * n * G), br.upload(br.Z, zero.data(), n * G), br.upload(br.opened, zero.data(), N);
    br.deal(true);
    br.finish(true);
    CHECK(collect(br, n, G, N) == eager);
    // ... and so does the replayed graph
    br.capture();
    br.upload(br.Y, zero.data(), n * n * G), br.upload(br.Z, zero.data(), n * G), br.upload(br.opened, zero.data(), N);
    br.replay();
    CHECK(collect(br, n, G, N) == eager);
    return eager;
}

int main() {
    void* stream = nullptr;
    pl_check(hbmpc_stream_create(context(), &stream), context(), "stream_create");
    std::printf("batchrecon (one launch)\n");
    pl_check(hbmpc_set_fused_batchrecon(context(), (size_t)1 << 20), context(), "set_fused_batchrecon");
    g_state = 7;
    const Outputs one = round_trip(stream);
    std::printf("batchrecon (the three launches)\n");
    pl_check(hbmpc_set_fused_batchrecon(context(), 0), context(), "set_fused_batchrecon");
    g_state = 7;
    CHECK(one == round_trip(stream));  // the same inputs: the same bytes in both forms
    pl_check(hbmpc_stream_destroy(context(), stream), context(), "stream_destroy");
    std::printf(g_failed ? "%d CHECKS FAILED\n" : "batchrecon pipeline passed (%d failures)\n", g_failed);
    return g_failed ? 1 : 0;
}
