/* A plain C99 caller of the PRandBit / PRandInt entry points of include/hbmpc_hip.h (fpmul/prandbitd.rs) for n = 5, t = 1 -- the
 * reference's own test shape (tests/prandbitd_test.rs): fold through device buffers, the conversion in both fields and both forms,
 * the finalize.  The checks need no arithmetic of their own: the converted shares must lie on one degree-t polynomial whose constant
 * term is the sum of the r_T, which the library's own robust recover tells.  Needs an MI355X. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "hbmpc_hip.h"

#define N_ 5
#define T_ 1
#define SETS 5 /* C(5, 1) */
#define OWN 4  /* C(4, 1) */
#define B_ 4
#define LK 55

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, hbmpc_last_error(NULL)); \
            return 1;                                                             \
        }                                                                         \
    } while (0)

static uint64_t lcg_state = 0x2545F4914F6CDD1Dull;
static uint64_t lcg(void) {
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return lcg_state;
}

static int run(hbmpc_ctx* fr, hbmpc_ctx* gl) {
    static uint64_t contrib[N_][SETS][B_], sums[SETS][B_], own[OWN][B_], total[B_], gshares[N_][B_], gone[B_], opened[B_];
    static uint8_t bad[N_][SETS], s2[N_][B_], s2one[B_], b2[N_][B_];
    static U256 shares[N_][B_], one[B_], bp[N_][B_], back[B_];
    size_t ids_all[N_] = {0, 1, 2, 3, 4}, deg[N_] = {T_, T_, T_, T_, T_}, tset_ids[SETS * T_], count = 0, nco = 0, party[1];
    void *d_contrib = NULL, *d_sums = NULL, *d_bad = NULL;
    int s, k, i, j;
    /* the enumeration: {0}, {1}, .. {4} */
    CHECK(hbmpc_riss_tsets(N_, T_, NULL, &count) == ShareSuccess && count == SETS);
    CHECK(hbmpc_riss_tsets(N_, T_, tset_ids, &count) == ShareSuccess);
    for (k = 0; k < SETS; ++k) CHECK(tset_ids[k] == (size_t)k);
    CHECK(hbmpc_riss_tsets(19, 6, NULL, &count) == InvalidInput);
    /* fold: every value <= 2^55, one offender */
    for (s = 0; s < N_; ++s)
        for (k = 0; k < SETS; ++k)
            for (i = 0; i < B_; ++i) contrib[s][k][i] = lcg() >> (64 - LK);
    contrib[1][2][3] = (uint64_t)1 << LK; /* the bound itself is allowed */
    CHECK(hbmpc_dev_alloc(fr, sizeof contrib, &d_contrib) == ShareSuccess && hbmpc_dev_alloc(fr, sizeof sums, &d_sums) == ShareSuccess &&
          hbmpc_dev_alloc(fr, sizeof bad, &d_bad) == ShareSuccess);
    CHECK(hbmpc_memcpy_h2d(fr, d_contrib, contrib, sizeof contrib, NULL) == ShareSuccess && hbmpc_stream_sync(fr, NULL) == ShareSuccess);
    CHECK(hbmpc_dev_riss_fold(fr, (const uint64_t*)d_contrib, N_, SETS, B_, 60, (uint64_t*)d_sums, (uint8_t*)d_bad, NULL) == HBMPC_FIELD_CAPACITY);
    CHECK(hbmpc_dev_riss_fold(gl, (const uint64_t*)d_contrib, N_, SETS, B_, LK, (uint64_t*)d_sums, (uint8_t*)d_bad, NULL) == ShareSuccess);
    CHECK(hbmpc_stream_sync(gl, NULL) == ShareSuccess);
    CHECK(hbmpc_dev_riss_fold(fr, (const uint64_t*)d_contrib, N_, SETS, B_, LK, (uint64_t*)d_sums, (uint8_t*)d_bad, NULL) == ShareSuccess);
    CHECK(hbmpc_memcpy_d2h(fr, sums, d_sums, sizeof sums, NULL) == ShareSuccess && hbmpc_memcpy_d2h(fr, bad, d_bad, sizeof bad, NULL) == ShareSuccess);
    CHECK(hbmpc_stream_sync(fr, NULL) == ShareSuccess);
    memset(total, 0, sizeof total);
    for (k = 0; k < SETS; ++k)
        for (i = 0; i < B_; ++i) {
            uint64_t want = 0;
            for (s = 0; s < N_; ++s) want += contrib[s][k][i];
            CHECK(sums[k][i] == want);
            total[i] += want;
        }
    for (s = 0; s < N_; ++s)
        for (k = 0; k < SETS; ++k) CHECK(bad[s][k] == 0);
    contrib[3][4][0] += (uint64_t)1 << LK;
    CHECK(hbmpc_memcpy_h2d(fr, d_contrib, contrib, sizeof contrib, NULL) == ShareSuccess);
    CHECK(hbmpc_dev_riss_fold(fr, (const uint64_t*)d_contrib, N_, SETS, B_, LK, (uint64_t*)d_sums, (uint8_t*)d_bad, NULL) == ShareSuccess);
    CHECK(hbmpc_memcpy_d2h(fr, bad, d_bad, sizeof bad, NULL) == ShareSuccess && hbmpc_stream_sync(fr, NULL) == ShareSuccess);
    for (s = 0; s < N_; ++s)
        for (k = 0; k < SETS; ++k) CHECK(bad[s][k] == (s == 3 && k == 4));
    /* conversion over Fr: all parties; the shares open to sum r_T */
    CHECK(hbmpc_riss_convert_parties(fr, &sums[0][0], N_, T_, B_, NULL, N_, 0, &shares[0][0], &s2[0][0]) == ShareSuccess);
    for (i = 0; i < B_; ++i) {
        U256 col[N_], co[N_], rec;
        for (j = 0; j < N_; ++j) col[j] = shares[j][i];
        CHECK(hbmpc_recover_secret(fr, ids_all, deg, col, N_, N_, T_, co, &nco, &rec) == ShareSuccess);
        CHECK(nco == T_ + 1 && rec.data[0] == total[i] && rec.data[1] == 0 && rec.data[2] == 0 && rec.data[3] == 0);
    }
    /* ... and over Goldilocks */
    CHECK(hbmpc_gl_riss_convert_parties(gl, &sums[0][0], N_, T_, B_, NULL, N_, 0, &gshares[0][0], NULL) == ShareSuccess);
    for (i = 0; i < B_; ++i) {
        uint64_t col[N_], co[N_], rec;
        for (j = 0; j < N_; ++j) col[j] = gshares[j][i];
        CHECK(hbmpc_gl_recover_secret(gl, ids_all, deg, col, N_, N_, T_, co, &nco, &rec) == ShareSuccess);
        CHECK(nco == T_ + 1 && rec == total[i]); /* 25 2^55 < p: no wrap */
    }
    /* the one-party form gives the same bytes for every party */
    for (j = 0; j < N_; ++j) {
        int row = 0;
        for (k = 0; k < SETS; ++k)
            if (k != j) memcpy(own[row++], sums[k], sizeof own[0]);
        party[0] = (size_t)j;
        CHECK(hbmpc_riss_convert_parties(fr, &own[0][0], N_, T_, B_, party, 1, 1, one, s2one) == ShareSuccess);
        CHECK(memcmp(one, shares[j], sizeof one) == 0 && memcmp(s2one, s2[j], sizeof s2one) == 0);
        CHECK(hbmpc_gl_riss_convert_parties(gl, &own[0][0], N_, T_, B_, party, 1, 1, gone, NULL) == ShareSuccess);
        CHECK(memcmp(gone, gshares[j], sizeof gone) == 0);
    }
    /* finalize: bp + r_p = G(v), b2 = r_2 ^ lsb(v) */
    for (i = 0; i < B_; ++i) opened[i] = total[i] + (uint64_t)(i & 1);
    CHECK(hbmpc_prandbit_finalize_parties(fr, opened, &shares[0][0], &s2[0][0], B_, N_, &bp[0][0], &b2[0][0]) == ShareSuccess);
    for (j = 0; j < N_; ++j) {
        CHECK(hbmpc_fr_op(fr, 0, bp[j], shares[j], B_, back) == ShareSuccess);
        for (i = 0; i < B_; ++i) {
            CHECK(back[i].data[0] == opened[i] && back[i].data[1] == 0 && back[i].data[2] == 0 && back[i].data[3] == 0);
            CHECK(b2[j][i] == (uint8_t)(s2[j][i] ^ (opened[i] & 1)));
        }
    }
    /* the stated codes */
    CHECK(hbmpc_gl_riss_convert_parties(fr, &sums[0][0], N_, T_, B_, NULL, N_, 0, &gshares[0][0], NULL) == TypeMismatch);
    CHECK(hbmpc_riss_convert_parties(gl, &sums[0][0], N_, T_, B_, NULL, N_, 0, &shares[0][0], NULL) == TypeMismatch);
    CHECK(hbmpc_prandbit_finalize_parties(gl, opened, &shares[0][0], &s2[0][0], B_, N_, &bp[0][0], &b2[0][0]) == TypeMismatch);
    CHECK(hbmpc_riss_convert_parties(fr, &sums[0][0], 19, 6, B_, NULL, 19, 0, &shares[0][0], NULL) == InvalidInput);
    CHECK(hbmpc_riss_convert_parties(fr, &sums[0][0], N_, 2, B_, NULL, N_, 0, &shares[0][0], NULL) == InvalidInput); /* n < 3t + 1 */
    hbmpc_dev_free(fr, d_contrib);
    hbmpc_dev_free(fr, d_sums);
    hbmpc_dev_free(fr, d_bad);
    return 0;
}

int main(void) {
    hbmpc_ctx *fr = NULL, *gl = NULL;
    int bad;
    if (hbmpc_create(0, Bls12_381Fr, &fr) != ShareSuccess || hbmpc_create(0, Goldilocks64, &gl) != ShareSuccess) {
        printf("hbmpc_create failed: %s\n", hbmpc_last_error(NULL));
        return 2;
    }
    bad = run(fr, gl);
    hbmpc_destroy(fr);
    hbmpc_destroy(gl);
    if (bad == 0) printf("PRandBit C ABI calls passed\n");
    return bad;
}
