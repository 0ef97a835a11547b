/* A plain C99 caller of the integer-point Shamir host calls of include/hbmpc_hip.h, beside test_c_abi.c: the shape of the reference's
 * own C test of its exported ABI (mpc/src/ffi/tests/secret_share.c), for shamir_share_compute_shares / shamir_share_recover_secret
 * (ffi/c_bindings/share/mod.rs:288-385), both fields.  Linked into test_shamir_units.  Needs an MI355X. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "hbmpc_hip.h"

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);                 \
            return 1;                                                             \
        }                                                                         \
    } while (0)

static int fr_calls(hbmpc_ctx* ctx) {
    const U256 secret = {{16, 33, 44, 81}};
    const uint64_t ids[8] = {1, 2, 3, 4, 5, 6, 7, 20}, zero_id[3] = {1, 0, 2}, dup[3] = {1, 2, 2};
    size_t deg[8] = {5, 5, 5, 5, 5, 5, 5, 5}, nco = 0;
    U256 coeffs[6], shares[8], co[8], rec, grid[8 * 2], gco[2 * 8];
    uint32_t gdeg[2];
    int i;
    coeffs[0] = secret;
    for (i = 1; i < 6; ++i) {
        const U256 c = {{(uint64_t)i * 0x9E3779B97F4A7C15ull, (uint64_t)i + 7, 3, (uint64_t)i}};
        coeffs[i] = c;
    }
    CHECK(hbmpc_shamir_compute_shares(ctx, coeffs, 1, ids, 8, 5, shares) == ShareSuccess);
    CHECK(hbmpc_shamir_recover_secret(ctx, ids, deg, shares, 8, co, &nco, &rec) == ShareSuccess);
    CHECK(nco == 6 && memcmp(&rec, &secret, sizeof rec) == 0 && memcmp(co, coeffs, sizeof coeffs) == 0);
    CHECK(hbmpc_shamir_recover_secret(ctx, ids, deg, shares, 5, co, &nco, &rec) == InsufficientShares);
    deg[2] = 4;
    CHECK(hbmpc_shamir_recover_secret(ctx, ids, deg, shares, 8, co, &nco, &rec) == DegreeMismatch);
    deg[2] = 5;
    shares[7].data[0] ^= 1; /* eight points off a quintic */
    CHECK(hbmpc_shamir_recover_secret(ctx, ids, deg, shares, 8, co, &nco, &rec) == DegreeMismatch);
    shares[7].data[0] ^= 1;
    CHECK(hbmpc_shamir_compute_shares(ctx, coeffs, 1, NULL, 8, 5, shares) == InvalidInput);
    CHECK(hbmpc_shamir_compute_shares(ctx, coeffs, 1, ids, 5, 5, shares) == InsufficientShares);
    CHECK(hbmpc_shamir_compute_shares(ctx, coeffs, 1, zero_id, 3, 2, shares) == InvalidInput);
    CHECK(hbmpc_shamir_compute_shares(ctx, coeffs, 1, dup, 3, 2, shares) == InvalidInput);
    /* the batched open: two columns, the second with a zero top coefficient */
    CHECK(hbmpc_shamir_compute_shares(ctx, coeffs, 1, ids, 8, 5, shares) == ShareSuccess);
    for (i = 0; i < 8; ++i) grid[i * 2] = shares[i];
    memset(&coeffs[5], 0, sizeof coeffs[5]);
    CHECK(hbmpc_shamir_compute_shares(ctx, coeffs, 1, ids, 8, 5, shares) == ShareSuccess);
    for (i = 0; i < 8; ++i) grid[i * 2 + 1] = shares[i];
    CHECK(hbmpc_shamir_batch_interpolate(ctx, ids, 8, grid, 2, gco, gdeg) == ShareSuccess);
    CHECK(gdeg[0] == 5 && gdeg[1] == 4 && memcmp(&gco[8], coeffs, 5 * sizeof(U256)) == 0 && memcmp(&gco[0], &secret, sizeof secret) == 0);
    CHECK(hbmpc_shamir_batch_interpolate(ctx, dup, 3, grid, 2, gco, gdeg) == InvalidInput);
    CHECK(hbmpc_gl_shamir_compute_shares(ctx, (const uint64_t*)coeffs, 1, ids, 8, 5, (uint64_t*)shares) == TypeMismatch);
    return 0;
}

static int gl_calls(hbmpc_ctx* ctx) {
    const uint64_t p = 0xFFFFFFFF00000001ull;
    const uint64_t ids[3] = {1, 2, 3}, twice[2] = {1, p + 1}, at_p[2] = {1, p}, top[2] = {0xFFFFFFFFFFFFFFFFull, 2};
    const uint64_t coeffs[2] = {918520, 77};
    size_t deg[3] = {1, 1, 1}, nco = 0;
    uint64_t shares[3], co[3], rec = 0;
    CHECK(hbmpc_gl_shamir_compute_shares(ctx, coeffs, 1, ids, 3, 1, shares) == ShareSuccess);
    CHECK(shares[0] == 918520 + 77 && shares[2] == 918520 + 3 * 77);
    CHECK(hbmpc_gl_shamir_recover_secret(ctx, ids, deg, shares, 3, co, &nco, &rec) == ShareSuccess);
    CHECK(nco == 2 && rec == 918520 && co[1] == 77);
    CHECK(hbmpc_gl_shamir_compute_shares(ctx, coeffs, 1, twice, 2, 1, shares) == ShareSuccess && shares[0] == shares[1]);
    CHECK(hbmpc_gl_shamir_recover_secret(ctx, twice, deg, shares, 2, co, &nco, &rec) == InvalidInput);
    CHECK(hbmpc_gl_shamir_compute_shares(ctx, coeffs, 1, at_p, 2, 1, shares) == InvalidInput);
    CHECK(hbmpc_gl_shamir_compute_shares(ctx, coeffs, 1, top, 2, 1, shares) == ShareSuccess);
    CHECK(shares[0] == 918520 + 77 * (0xFFFFFFFFFFFFFFFFull - p) && shares[1] == 918520 + 2 * 77);
    return 0;
}

int shamir_c99_calls(void) {
    hbmpc_ctx *fr = NULL, *gl = NULL;
    int rc;
    CHECK(hbmpc_create(0, Bls12_381Fr, &fr) == ShareSuccess);
    CHECK(hbmpc_create(0, Goldilocks64, &gl) == ShareSuccess);
    rc = fr_calls(fr) || gl_calls(gl);
    hbmpc_destroy(fr);
    hbmpc_destroy(gl);
    if (!rc) printf("C99 Shamir calls passed\n");
    return rc;
}
