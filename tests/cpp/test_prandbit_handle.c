/* A plain C99 caller of the PRandBit / PRandInt handles of include/hbmpc_hip.h (hbmpc_pipe_prandbit_create, hbmpc_pipe_prandint_create;
 * fpmul/prandbitd.rs) for n = 5, t = 1 -- the reference's own test shape (tests/prandbitd_test.rs): buffers by name, run, capture and
 * replay.  The checks need no field arithmetic of their own: the bits are shared as constant polynomials (a valid sharing of degree
 * <= t), the opened values must be sum r_T + b as plain integers, and the output shares must open to the bits, which the library's own
 * robust recover tells.  Needs an MI355X. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "hbmpc_hip.h"

#define N_ 5
#define T_ 1
#define SETS 5 /* C(5, 1) */
#define B_ 4
#define G_ 2   /* B / (t + 1) */
#define LK 55

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, hbmpc_last_error(NULL)); \
            return 1;                                                             \
        }                                                                         \
    } while (0)

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static uint64_t lcg(void) {
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return lcg_state;
}

static uint64_t contrib[N_][SETS][B_], b_q[N_][B_], sums[SETS][B_], opened[B_], total[B_], bits[B_];
static uint8_t bad[N_][SETS], b2[N_][B_], rstatus[N_ * G_];
static U256 bp[N_][B_], bp_again[N_][B_], rp[N_][B_];

/* every output share column opens to the bit */
static int opens_to_bits(hbmpc_ctx* fr, U256 (*shares)[B_]) {
    size_t ids_all[N_] = {0, 1, 2, 3, 4}, deg[N_] = {T_, T_, T_, T_, T_}, nco = 0;
    int i, j;
    for (i = 0; i < B_; ++i) {
        U256 col[N_], co[N_], rec;
        for (j = 0; j < N_; ++j) col[j] = shares[j][i];
        CHECK(hbmpc_recover_secret(fr, ids_all, deg, col, N_, N_, T_, co, &nco, &rec) == ShareSuccess);
        CHECK(rec.data[0] == bits[i] && rec.data[1] == 0 && rec.data[2] == 0 && rec.data[3] == 0);
    }
    return 0;
}

static int run(hbmpc_ctx* fr, hbmpc_ctx* gl) {
    hbmpc_pipe *pb = NULL, *pi = NULL;
    hbmpc_recover_summary sm;
    void* stream = NULL;
    void* dev = NULL;
    size_t count = 0;
    int s, k, i, j;
    for (s = 0; s < N_; ++s)
        for (k = 0; k < SETS; ++k)
            for (i = 0; i < B_; ++i) contrib[s][k][i] = lcg() >> (64 - LK);
    contrib[1][2][3] = (uint64_t)1 << LK; /* the bound itself is allowed */
    memset(total, 0, sizeof total);
    for (i = 0; i < B_; ++i) {
        bits[i] = (uint64_t)(i & 1);
        for (j = 0; j < N_; ++j) b_q[j][i] = bits[i];
        for (s = 0; s < N_; ++s)
            for (k = 0; k < SETS; ++k) total[i] += contrib[s][k][i];
    }
    CHECK(hbmpc_stream_create(fr, &stream) == ShareSuccess);
    /* refused shapes and contexts */
    CHECK(hbmpc_pipe_prandbit_create(fr, gl, N_, T_, B_ - 1, LK, 0, stream, &pb) == InvalidInput && pb == NULL);
    CHECK(hbmpc_pipe_prandbit_create(fr, gl, 3, T_, B_, LK, 0, stream, &pb) == InvalidInput);
    CHECK(hbmpc_pipe_prandbit_create(gl, fr, N_, T_, B_, LK, 0, stream, &pb) == TypeMismatch);
    CHECK(hbmpc_pipe_prandbit_create(NULL, gl, N_, T_, B_, LK, 0, stream, &pb) == InvalidInput);
    CHECK(hbmpc_pipe_prandint_create(gl, N_, T_, B_, LK, stream, &pi) == TypeMismatch);
    /* PRandBit: buffers by name, each counted in its own element type */
    CHECK(hbmpc_pipe_prandbit_create(fr, gl, N_, T_, B_, LK, 0, stream, &pb) == ShareSuccess && pb != NULL);
    CHECK(hbmpc_pipe_buffer(pb, "contrib", &dev, &count) == ShareSuccess && dev != NULL && count == N_ * SETS * B_);
    CHECK(hbmpc_pipe_buffer(pb, "b_p", NULL, &count) == ShareSuccess && count == N_ * B_);
    CHECK(hbmpc_pipe_buffer(pb, "bad", NULL, &count) == ShareSuccess && count == N_ * SETS);
    CHECK(hbmpc_pipe_buffer(pb, "rstatus", NULL, &count) == ShareSuccess && count == N_ * G_);
    CHECK(hbmpc_pipe_buffer(pb, "no_such_buffer", NULL, &count) == InvalidInput);
    CHECK(hbmpc_pipe_upload(pb, "no_such_buffer", contrib, 1) == InvalidInput);
    CHECK(hbmpc_pipe_upload(pb, "contrib", contrib, N_ * SETS * B_ + 1) == InvalidInput);
    CHECK(hbmpc_pipe_upload(pb, "contrib", contrib, N_ * SETS * B_) == ShareSuccess && hbmpc_pipe_upload(pb, "b_q", b_q, N_ * B_) == ShareSuccess);
    CHECK(hbmpc_pipe_set_checked(pb, 1) == ShareSuccess && hbmpc_pipe_run(pb) == ShareSuccess);
    CHECK(hbmpc_pipe_download(pb, "sums", sums, SETS * B_) == ShareSuccess && hbmpc_pipe_download(pb, "bad", bad, N_ * SETS) == ShareSuccess);
    CHECK(hbmpc_pipe_download(pb, "opened", opened, B_) == ShareSuccess && hbmpc_pipe_download(pb, "b_p", bp, N_ * B_) == ShareSuccess);
    CHECK(hbmpc_pipe_download(pb, "b_2", b2, N_ * B_) == ShareSuccess && hbmpc_pipe_download(pb, "rstatus", rstatus, N_ * G_) == ShareSuccess);
    CHECK(hbmpc_pipe_download(pb, "r_p", rp, N_ * B_) == ShareSuccess);
    CHECK(hbmpc_pipe_summary(pb, &sm) == ShareSuccess && sm.n_failed == 0);
    for (k = 0; k < SETS; ++k)
        for (i = 0; i < B_; ++i) {
            uint64_t want = 0;
            for (s = 0; s < N_; ++s) want += contrib[s][k][i];
            CHECK(sums[k][i] == want);
        }
    for (s = 0; s < N_; ++s)
        for (k = 0; k < SETS; ++k) CHECK(bad[s][k] == 0);
    for (i = 0; i < N_ * G_; ++i) CHECK(rstatus[i] == 0);
    for (i = 0; i < B_; ++i) CHECK(opened[i] == total[i] + bits[i]); /* 25 values of at most 2^55 and a bit: no wrap in Goldilocks */
    if (opens_to_bits(fr, bp)) return 1;
    /* captured and replayed with the outputs cleared in between: the bytes of the eager run */
    CHECK(hbmpc_pipe_capture(pb) == ShareSuccess);
    memset(bp_again, 0, sizeof bp_again);
    CHECK(hbmpc_pipe_upload(pb, "b_p", bp_again, N_ * B_) == ShareSuccess && hbmpc_pipe_upload(pb, "opened", bp_again, B_) == ShareSuccess);
    CHECK(hbmpc_pipe_replay(pb) == ShareSuccess && hbmpc_pipe_sync(pb) == ShareSuccess);
    CHECK(hbmpc_pipe_download(pb, "b_p", bp_again, N_ * B_) == ShareSuccess && memcmp(bp, bp_again, sizeof bp) == 0);
    CHECK(hbmpc_pipe_download(pb, "opened", sums, B_) == ShareSuccess && memcmp(sums, opened, sizeof opened) == 0);
    /* a tampered share of sender 0: checked mode returns the decode's error, and the summary counts the chunk's recipients */
    b_q[0][1] += 5;
    CHECK(hbmpc_pipe_upload(pb, "b_q", b_q, N_ * B_) == ShareSuccess);
    CHECK(hbmpc_pipe_run(pb) == DecodingError);
    CHECK(hbmpc_pipe_set_checked(pb, 0) == ShareSuccess && hbmpc_pipe_run(pb) == ShareSuccess);
    CHECK(hbmpc_pipe_download(pb, "opened", opened, B_) == ShareSuccess);
    CHECK(opened[0] == 0 && opened[1] == 0 && opened[2] == total[2] + bits[2] && opened[3] == total[3] + bits[3]);
    hbmpc_pipe_destroy(pb);
    /* PRandInt: any B; the same Fr shares as PRandBit's r_p */
    CHECK(hbmpc_pipe_prandint_create(fr, N_, T_, B_, LK, stream, &pi) == ShareSuccess && pi != NULL);
    CHECK(hbmpc_pipe_buffer(pi, "b_q", NULL, &count) == InvalidInput);
    CHECK(hbmpc_pipe_upload(pi, "contrib", contrib, N_ * SETS * B_) == ShareSuccess && hbmpc_pipe_run(pi) == ShareSuccess);
    CHECK(hbmpc_pipe_download(pi, "r_p", bp_again, N_ * B_) == ShareSuccess && memcmp(bp_again, rp, sizeof rp) == 0);
    hbmpc_pipe_destroy(pi);
    CHECK(hbmpc_stream_destroy(fr, stream) == ShareSuccess);
    return 0;
}

int main(void) {
    hbmpc_ctx *fr = NULL, *gl = NULL;
    int rc;
    if (hbmpc_create(0, Bls12_381Fr, &fr) != ShareSuccess || hbmpc_create(0, Goldilocks64, &gl) != ShareSuccess) {
        printf("FAILED: no device (%s)\n", hbmpc_last_error(NULL));
        return 1;
    }
    rc = run(fr, gl);
    hbmpc_destroy(gl);
    hbmpc_destroy(fr);
    if (rc == 0) printf("PRandBit handle calls passed\n");
    return rc;
}
