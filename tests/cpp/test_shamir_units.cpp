// The reference's share tests (common/share/shamir.rs:250-326: recover, add, scalar multiply, degree mismatch, insufficient shares)
// restated over Shamirshare of include/hbmpc_shares.hpp at the reference's own points ([1..6], [1..7, 20]), over both fields, plus the
// scheme's own refusals; then the plain C99 caller of the host calls (test_shamir_abi.c).  Needs an MI355X.
#include <cstdio>
#include <vector>

#include "hbmpc_shares.hpp"

extern "C" int shamir_c99_calls(void);

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);         \
            return 1;                                                     \
        }                                                                 \
    } while (0)

template <class S>
static int run(const char* name) {
    using F = typename S::F;
    using Share = typename S::Shamirshare;
    using Vec = std::vector<typename S::template ShamirShare<hbmpc::Shamir>>;
    uint64_t state = 0x243F6A8885A308D3ull;
    typename S::Rng rng = [&state]() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return F::from(state >> 11);
    };
    const std::vector<size_t> ids6 = {1, 2, 3, 4, 5, 6}, ids8 = {1, 2, 3, 4, 5, 6, 7, 20}, ids3 = {1, 2, 3};
    {  // should_recover_secret
        const F secret = F::from(918520);
        const Vec shares = Share::compute_shares(secret, 6, 5, &ids6, rng).unwrap();
        CHECK(shares.size() == 6 && shares[3].id == 4 && shares[3].degree == 5);
        const auto rec = Share::recover_secret(shares, 6, 0).unwrap();
        CHECK(rec.second == secret && rec.first.size() == 6 && rec.first[0] == secret);
    }
    {  // should_add_shares
        const F s1 = F::from(10), s2 = F::from(20);
        const Vec a = Share::compute_shares(s1, 6, 5, &ids6, rng).unwrap(), b = Share::compute_shares(s2, 6, 5, &ids6, rng).unwrap();
        Vec sum;
        for (size_t i = 0; i < a.size(); ++i) sum.push_back((a[i] + b[i]).unwrap());
        CHECK(Share::recover_secret(sum, 6, 0).unwrap().second == s1 + s2);
    }
    {  // should_multiply_scalar, at the points [1..7, 20]
        const F secret = F::from(55);
        const Vec shares = Share::compute_shares(secret, 8, 5, &ids8, rng).unwrap();
        CHECK(shares.size() == 8 && shares[7].id == 20);
        Vec tripled;
        for (const auto& s : shares) tripled.push_back((s * F::from(3)).unwrap());
        CHECK(Share::recover_secret(tripled, 8, 0).unwrap().second == secret * F::from(3));
    }
    {  // test_degree_mismatch
        Vec shares = Share::compute_shares(F::from(918520), 6, 5, &ids6, rng).unwrap();
        shares[2].degree = 4;
        CHECK(Share::recover_secret(shares, 6, 0).unwrap_err() == DegreeMismatch);
    }
    {  // test_insufficient_shares
        const Vec shares = Share::compute_shares(F::from(918520), 3, 2, &ids3, rng).unwrap();
        const Vec tail(shares.begin() + 1, shares.end());
        CHECK(Share::recover_secret(tail, 3, 0).unwrap_err() == InsufficientShares);
    }
    {  // the scheme's refusals (shamir.rs:51-70, 95-114), and a share sum across ids (common/mod.rs:167-188)
        const std::vector<size_t> few = {1, 2}, zero = {1, 0, 3}, dup = {1, 2, 2};
        CHECK(Share::compute_shares(F::from(1), 3, 2, nullptr, rng).unwrap_err() == InvalidInput);
        CHECK(Share::compute_shares(F::from(1), 3, 2, &few, rng).unwrap_err() == InsufficientShares);
        CHECK(Share::compute_shares(F::from(1), 3, 2, &zero, rng).unwrap_err() == InvalidInput);
        CHECK(Share::compute_shares(F::from(1), 3, 2, &dup, rng).unwrap_err() == InvalidInput);
        CHECK(Share::recover_secret(Vec{}, 3, 0).unwrap_err() == InvalidInput);
        Vec shares = Share::compute_shares(F::from(7), 3, 2, &ids3, rng).unwrap();
        CHECK((shares[0] + shares[1]).unwrap_err() == IdMismatch);
        shares[1].id = 1;
        CHECK(Share::recover_secret(shares, 3, 0).unwrap_err() == InvalidInput);
    }
    printf("%s: Shamirshare unit tests passed\n", name);
    return 0;
}

int main() {
    if (run<hbmpc::FrScheme>("bls12-381 Fr")) return 1;
    if (run<hbmpc::GlScheme>("Goldilocks")) return 1;
    if (shamir_c99_calls()) return 1;
    printf("all Shamirshare unit tests passed\n");
    return 0;
}
