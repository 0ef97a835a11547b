// The C++ compositions PRandInt / PRandBit of include/hbmpc_pipelines.hpp for n = 5, t = 1 (the reference's own test shape,
// tests/prandbitd_test.rs): the opened value is sum r_T + b, the Fr output shares open to the bit, one lying sender in the open
// changes nothing, and PRandInt gives the same Fr shares of the random integers.  Needs an MI355X.
#include <cstdio>
#include <cstring>
#include <vector>

#include "hbmpc_pipelines.hpp"

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            return 1;                                                  \
        }                                                              \
    } while (0)

static uint64_t lcg_state = 0x853C49E6748FEA9Bull;
static uint64_t lcg() {
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return lcg_state;
}

int main() try {
    const size_t n = 5, t = 1, B = 6, lk = 55, sets = 5;
    hbmpc_ctx *fr = nullptr, *gl = nullptr;
    void* stream = nullptr;
    CHECK(hbmpc_create(0, Bls12_381Fr, &fr) == ShareSuccess && hbmpc_create(0, Goldilocks64, &gl) == ShareSuccess);
    CHECK(hbmpc_stream_create(fr, &stream) == ShareSuccess);
    {
        hbmpc::PRandBit pb(gl, fr, n, t, B, stream);
        CHECK(pb.tsets == sets && pb.G == B / (t + 1));
        std::vector<uint64_t> contrib(n * sets * B), total(B, 0), coeffs(B * (t + 1)), b_q(n * B), bits(B);
        for (auto& v : contrib) v = lcg() >> (64 - lk);
        for (size_t s = 0; s < n; ++s)
            for (size_t k = 0; k < sets; ++k)
                for (size_t i = 0; i < B; ++i) total[i] += contrib[(s * sets + k) * B + i];
        for (size_t i = 0; i < B; ++i) bits[i] = lcg() >> 63, coeffs[i * (t + 1)] = bits[i], coeffs[i * (t + 1) + 1] = lcg() >> 1;
        CHECK(hbmpc_gl_compute_shares(gl, coeffs.data(), B, n, t, b_q.data()) == ShareSuccess);
        CHECK(hbmpc_memcpy_h2d(fr, pb.contrib, contrib.data(), contrib.size() * 8, stream) == ShareSuccess);
        CHECK(hbmpc_memcpy_h2d(fr, pb.b_q, b_q.data(), b_q.size() * 8, stream) == ShareSuccess);
        pb.run(lk);
        std::vector<uint64_t> opened(B), Y(n * n * pb.G);
        std::vector<U256> b_p(n * B), r_p(n * B);
        std::vector<uint8_t> b_2(n * B), bad(n * sets);
        using hbmpc::pl_check;
        auto fetch = [&]() {
            pl_check(hbmpc_memcpy_d2h(fr, opened.data(), pb.opened, B * 8, stream), fr, "d2h");
            pl_check(hbmpc_memcpy_d2h(fr, b_p.data(), pb.b_p, n * B * 32, stream), fr, "d2h");
            pl_check(hbmpc_memcpy_d2h(fr, b_2.data(), pb.b_2, n * B, stream), fr, "d2h");
            pl_check(hbmpc_memcpy_d2h(fr, bad.data(), pb.bad, n * sets, stream), fr, "d2h");
            pl_check(hbmpc_memcpy_d2h(fr, r_p.data(), pb.r_p, n * B * 32, stream), fr, "d2h");
            pb.sync();
        };
        fetch();
        for (uint8_t v : bad) CHECK(v == 0);
        const size_t ids[5] = {0, 1, 2, 3, 4}, deg[5] = {1, 1, 1, 1, 1};
        for (size_t i = 0; i < B; ++i) {
            CHECK(opened[i] == total[i] + bits[i]);  // 25 2^55 + 1 < p
            U256 col[5], co[5], rec;
            size_t nco = 0;
            for (size_t j = 0; j < n; ++j) col[j] = b_p[j * B + i];
            CHECK(hbmpc_recover_secret(fr, ids, deg, col, n, n, t, co, &nco, &rec) == ShareSuccess);
            CHECK(rec.data[0] == bits[i] && rec.data[1] == 0 && rec.data[2] == 0 && rec.data[3] == 0);
        }
        // sender 2 lies in the open
        const std::vector<uint64_t> opened0 = opened;
        const std::vector<U256> b_p0 = b_p;
        const std::vector<uint8_t> b_20 = b_2;
        pb.prepare(lk);
        CHECK(hbmpc_memcpy_d2h(fr, Y.data(), pb.Y, Y.size() * 8, stream) == ShareSuccess);
        pb.sync();
        for (size_t k = 0; k < n * pb.G; ++k) Y[2 * n * pb.G + k] ^= 3;
        CHECK(hbmpc_memcpy_h2d(fr, pb.Y, Y.data(), Y.size() * 8, stream) == ShareSuccess);
        pb.finish();
        fetch();
        CHECK(opened == opened0 && memcmp(b_p.data(), b_p0.data(), n * B * 32) == 0 && b_2 == b_20);
        // PRandInt: the same Fr shares, for a B that is no multiple of t + 1
        hbmpc::PRandInt pi(fr, n, t, B - 1, stream);
        std::vector<uint64_t> c2(n * sets * (B - 1));
        for (size_t r = 0; r < n * sets; ++r) memcpy(&c2[r * (B - 1)], &contrib[r * B], (B - 1) * 8);
        CHECK(hbmpc_memcpy_h2d(fr, pi.contrib, c2.data(), c2.size() * 8, stream) == ShareSuccess);
        pi.run(lk);
        std::vector<U256> r_pi(n * (B - 1));
        CHECK(hbmpc_memcpy_d2h(fr, r_pi.data(), pi.r_p, r_pi.size() * 32, stream) == ShareSuccess);
        pi.sync();
        for (size_t j = 0; j < n; ++j) CHECK(memcmp(&r_pi[j * (B - 1)], &r_p[j * B], (B - 1) * 32) == 0);
        bool threw = false;
        try {
            hbmpc::PRandBit odd(gl, fr, n, t, B + 1, stream);
        } catch (const std::exception&) {
            threw = true;
        }
        CHECK(threw);
    }
    hbmpc_stream_destroy(fr, stream);
    hbmpc_destroy(fr);
    hbmpc_destroy(gl);
    printf("PRandBit pipelines passed\n");
    return 0;
} catch (const std::exception& e) {
    printf("FAILED: %s\n", e.what());
    return 1;
}
