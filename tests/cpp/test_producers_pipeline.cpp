// include/hbmpc_pipelines.hpp's free functions ransha_parties / randousha_parties (and DevBlock) at n = 4, t = 1, three columns, against the
// RanSha / RanDouSha handles from the same polynomials: the same dealt shares and output lists, a clean verdict; the same from the dealt
// shares; a changed dealt share and unequal secrets are counted.  Both settings of the one-launch threshold.
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
static bool same(const std::vector<U256>& a, const std::vector<U256>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(U256)) == 0;
}
static std::vector<U256> fetch(const U256* dev, size_t elements, void* stream) {
    std::vector<U256> v(elements);
    pl_check(hbmpc_memcpy_d2h(context(), v.data(), dev, elements * sizeof(U256), stream), context(), "d2h");
    pl_check(hbmpc_stream_sync(context(), stream), context(), "sync");
    return v;
}
static void put(U256* dev, const std::vector<U256>& v, void* stream) {
    pl_check(hbmpc_memcpy_h2d(context(), dev, v.data(), v.size() * sizeof(U256), stream), context(), "h2d");
    pl_check(hbmpc_stream_sync(context(), stream), context(), "sync");
}

static void round_trip(void* stream) {
    const size_t n = 4, t = 1, K = 3, eb = sizeof(U256);
    const uint32_t none = 0xffffffffu;
    // ---- RanSha ----
    std::vector<U256> co(n * K * (t + 1));
    for (U256& c : co) c = rand_fr();
    RanSha h(context(), n, t, K, stream);
    h.upload(h.coeffs, co.data(), co.size());
    h.run();
    uint32_t hv[2];
    h.verdict(hv);
    const std::vector<U256> want_S = fetch(h.S, n * n * K, stream), want_out = fetch(h.out, n * h.nout, stream);
    DevBlock blk(context(), (co.size() + n * n * K + n * h.nout) * eb);
    U256 *d_co = blk.at<U256>(0), *d_S = blk.at<U256>(co.size() * eb), *d_out = blk.at<U256>((co.size() + n * n * K) * eb);
    put(d_co, co, stream);
    uint32_t v[2] = {7, 7};
    ransha_parties(context(), d_co, d_S, K, n, t, d_out, v, stream);
    CHECK(hv[0] == 0 && v[0] == 0 && v[1] == none);
    CHECK(same(fetch(d_S, n * n * K, stream), want_S));
    CHECK(same(fetch(d_out, n * h.nout, stream), want_out));
    put(d_out, std::vector<U256>(n * h.nout, U256{{0, 0, 0, 0}}), stream);
    ransha_parties(context(), nullptr, d_S, K, n, t, d_out, v, stream);  // from the dealt shares
    CHECK(v[0] == 0 && v[1] == none);
    CHECK(same(fetch(d_out, n * h.nout, stream), want_out));
    std::vector<U256> lied = want_S;  // dealer 2's share for recipient 1 in column 2: a verify sender, so both verifiers see it
    lied[(2 * n + 1) * K + 2].data[0] ^= 1;
    put(d_S, lied, stream);
    ransha_parties(context(), nullptr, d_S, K, n, t, d_out, v, stream);
    CHECK(v[0] == 2 * t && v[1] == 2);

    // ---- RanDouSha ----
    std::vector<U256> ct(n * K * (t + 1)), c2(n * K * (2 * t + 1));
    for (U256& c : ct) c = rand_fr();
    for (U256& c : c2) c = rand_fr();
    for (size_t i = 0; i < n * K; ++i) c2[i * (2 * t + 1)] = ct[i * (t + 1)];  // equal secrets
    RanDouSha hd(context(), n, t, K, stream);
    hd.upload(hd.coeffs_t, ct.data(), ct.size());
    hd.upload(hd.coeffs_2t, c2.data(), c2.size());
    hd.run();
    hd.verdict(hv);
    const std::vector<U256> want_t = fetch(hd.out_t, n * hd.nout, stream), want_2t = fetch(hd.out_2t, n * hd.nout, stream);
    const size_t dealt = n * n * K, outs = n * hd.nout;
    DevBlock bd(context(), (ct.size() + c2.size() + 2 * dealt + 2 * outs) * eb);
    U256 *d_ct = bd.at<U256>(0), *d_c2 = bd.at<U256>(ct.size() * eb), *d_St = bd.at<U256>((ct.size() + c2.size()) * eb);
    U256 *d_S2 = d_St + dealt, *d_ot = d_S2 + dealt, *d_o2 = d_ot + outs;
    put(d_ct, ct, stream), put(d_c2, c2, stream);
    randousha_parties(context(), d_ct, d_c2, d_St, d_S2, K, n, t, d_ot, d_o2, v, stream);
    CHECK(hv[0] == 0 && v[0] == 0 && v[1] == none);
    CHECK(same(fetch(d_St, dealt, stream), fetch(hd.S_t, dealt, stream)) && same(fetch(d_S2, dealt, stream), fetch(hd.S_2t, dealt, stream)));
    CHECK(same(fetch(d_ot, outs, stream), want_t) && same(fetch(d_o2, outs, stream), want_2t));
    randousha_parties(context(), nullptr, nullptr, d_St, d_S2, K, n, t, d_ot, d_o2, v, stream);
    CHECK(v[0] == 0 && v[1] == none);
    CHECK(same(fetch(d_ot, outs, stream), want_t) && same(fetch(d_o2, outs, stream), want_2t));
    c2[(1 * K + 1) * (2 * t + 1)].data[0] ^= 1;  // dealer 1, column 1: unequal secrets, every verifier
    put(d_c2, c2, stream);
    randousha_parties(context(), d_ct, d_c2, d_St, d_S2, K, n, t, d_ot, d_o2, v, stream);
    CHECK(v[0] == n - t - 1 && v[1] == 1);
}

int main() {
    void* stream = nullptr;
    pl_check(hbmpc_stream_create(context(), &stream), context(), "stream_create");
    std::printf("producers (one launch)\n");
    pl_check(hbmpc_set_fused_producers(context(), (size_t)1 << 20), context(), "set_fused_producers");
    round_trip(stream);
    std::printf("producers (the separate launches)\n");
    pl_check(hbmpc_set_fused_producers(context(), 0), context(), "set_fused_producers");
    round_trip(stream);
    pl_check(hbmpc_stream_destroy(context(), stream), context(), "stream_destroy");
    std::printf(g_failed ? "%d CHECKS FAILED\n" : "producers wrappers passed (%d failures)\n", g_failed);
    return g_failed ? 1 : 0;
}
