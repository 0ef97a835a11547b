// The C++ wrappers of the PRandBit / PRandInt handles (include/hbmpc_pipelines.hpp: RissPipeline, PRandBitPipe, PRandIntPipe) for
// n = 5, t = 1, with the checks of test_prandbit_handle.c: the bits are shared as constant polynomials, so the opened values must be
// sum r_T + b as plain integers; a replayed graph gives the bytes of the eager run; PRandInt gives PRandBit's r_p.  Needs an MI355X.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hbmpc_pipelines.hpp"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

static int run(hbmpc_ctx* fr, hbmpc_ctx* gl) {
    const size_t n = 5, t = 1, sets = 5, B = 4, lk = 55;
    void* stream = nullptr;
    CHECK(hbmpc_stream_create(fr, &stream) == ShareSuccess);
    std::vector<uint64_t> contrib(n * sets * B), b_q(n * B), total(B, 0), opened(B), again(B);
    uint64_t state = 0x9E3779B97F4A7C15ull;
    for (auto& v : contrib) v = (state = state * 6364136223846793005ull + 1442695040888963407ull) >> (64 - lk);
    for (size_t i = 0; i < B; ++i) {
        for (size_t j = 0; j < n; ++j) b_q[j * B + i] = i & 1;
        for (size_t sk = 0; sk < n * sets; ++sk) total[i] += contrib[sk * B + i];
    }
    std::vector<U256> rp(n * B), rp_int(n * B), bp(n * B), bp_again(n * B);
    {
        hbmpc::PRandBitPipe pb(gl, fr, n, t, B, lk, stream);
        size_t count = 0;
        CHECK(pb.typed<uint64_t>("contrib", &count) == pb.contrib && count == n * sets * B);
        pb.upload_typed("contrib", contrib.data(), contrib.size());
        pb.upload_typed("b_q", b_q.data(), b_q.size());
        pb.run(true);
        pb.download_typed("opened", opened.data(), B);
        pb.download_typed("r_p", rp.data(), n * B);
        pb.download_typed("b_p", bp.data(), n * B);
        for (size_t i = 0; i < B; ++i) CHECK(opened[i] == total[i] + (i & 1));
        CHECK(pb.last_summary().n_failed == 0);
        pb.capture();
        std::vector<U256> zero(n * B);
        memset(zero.data(), 0, zero.size() * sizeof(U256));
        pb.upload_typed("b_p", zero.data(), n * B);
        pb.replay();
        pb.sync();
        pb.download_typed("b_p", bp_again.data(), n * B);
        pb.download_typed("opened", again.data(), B);
        CHECK(memcmp(bp.data(), bp_again.data(), n * B * sizeof(U256)) == 0 && again == opened);
        bool threw = false;
        try {
            hbmpc::PRandBitPipe bad(gl, fr, n, t, B - 1, lk, stream);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw);
    }
    {
        hbmpc::PRandIntPipe pi(fr, n, t, B, lk, stream);
        pi.upload_typed("contrib", contrib.data(), contrib.size());
        pi.run();
        pi.download_typed("r_p", rp_int.data(), n * B);
        CHECK(memcmp(rp.data(), rp_int.data(), n * B * sizeof(U256)) == 0);
    }
    CHECK(hbmpc_stream_destroy(fr, stream) == ShareSuccess);
    return 0;
}

int main() {
    hbmpc_ctx *fr = nullptr, *gl = nullptr;
    if (hbmpc_create(0, Bls12_381Fr, &fr) != ShareSuccess || hbmpc_create(0, Goldilocks64, &gl) != ShareSuccess) {
        printf("FAILED: no device (%s)\n", hbmpc_last_error(nullptr));
        return 1;
    }
    int rc = 1;
    try {
        rc = run(fr, gl);
    } catch (const std::exception& e) {
        printf("FAILED: %s\n", e.what());
    }
    hbmpc_destroy(gl);
    hbmpc_destroy(fr);
    if (rc == 0) printf("PRandBit pipeline wrappers passed\n");
    return rc;
}
