// CPU-only dump of the host-side table builders for tests/test_host_tables.py, which compares every value with the big-int
// oracle: the share tables (mpc-protocols_amd/csrc/tables.hpp, host_fr.hpp), the matrix-core tables (tables_mfma.hpp,
// tables_mfma_gl.hpp), the square root's constants (tables_sqrt.hpp) and the RISS coefficients (tables_riss.hpp).  Built with
// -fsanitize=address,undefined: together these are the host arithmetic of the product.
//   usage: host_tables_dump <fr|gl> <n> <d> <t> <id0,id1,...> [full]
//          host_tables_dump sqrt <fr-u29|fr-sat32|gl>          build_sqrt_table: a line "sqrt <layout numbers>", then the words
//          host_tables_dump riss <fr|fr-sat32|gl> <n> <t> <own|-1>   build_riss_table: a line "riss <layout numbers>", then the words
// The share tables' lines end with "recover_vm" / "recover_bc" (build_recover_tables: the optimistic decode's verify and coefficient rows in
// the device-constant form) and, with OEC rounds, "second" (build_second_tables).
// (the words of these two modes follow their line as raw little-endian 32-bit values: the tables reach tens of megabytes)
// full: the matrix-core tables are printed whatever their size, and so are the tables of the other instances -- enc (one row per point),
// bflyR (point pairs, rows alpha^i 2^261: triple generation), bflyinv (point pairs of the inverse transform on a full domain)
// (tests/test_mfma_inputs.py compares each byte for byte with the integer model of tests/mfma_model.py)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../mpc-protocols_amd/csrc/tables.hpp"
#include "../../mpc-protocols_amd/csrc/tables_mfma.hpp"
#include "../../mpc-protocols_amd/csrc/tables_mfma_gl.hpp"
#include "../../mpc-protocols_amd/csrc/tables_riss.hpp"
#include "../../mpc-protocols_amd/csrc/tables_sqrt.hpp"

using namespace hbmpc;

template <class H>
static void put(const char* tag, const H& v) {
    uint64_t c[4];
    v.to_canon(c);
    std::printf("%s %016llx%016llx%016llx%016llx\n", tag, (unsigned long long)c[3], (unsigned long long)c[2], (unsigned long long)c[1],
                (unsigned long long)c[0]);
}
static void put_words(const char* tag, const std::vector<uint32_t>& tab) {
    std::printf("%s", tag);
    for (uint32_t x : tab) std::printf(" %08x", x);
    std::printf("\n");
}
template <class H>
static int run(size_t n, size_t d, size_t t, const std::vector<size_t>& ids, bool full) {
    const size_t m = d + 1, needed = d + t + 1;
    H w;
    if (!domain_omega(domain_size(n), &w)) return 2;
    put("omega", w);
    const std::vector<H> el = domain_elements<H>(n, n);
    for (const H& e : el) put("alpha", e);
    std::vector<H> xs(m);
    for (size_t i = 0; i < m; ++i) xs[i] = el[ids[i]];
    const auto basis = lagrange_basis(xs);  // basis[i][k]
    for (size_t i = 0; i < m; ++i)
        for (size_t k = 0; k < m; ++k) put("basis", basis[i][k]);
    for (size_t s = m; s < needed; ++s)
        for (size_t i = 0; i < m; ++i) put("verify", horner(basis[i], el[ids[s]]));
    put("inv7", H::from_u64(7).inv());
    put("pow", H::from_u64(3).pow_u64(1000003));
    // the device-constant encodings of one value in every representation it is shipped in
    std::vector<uint32_t> words;
    put_const(words, el[n > 1 ? 1 : 0], std::is_same<H, HGl>::value ? IMPL_GOLD : IMPL_U29);
    std::printf("const");
    for (uint32_t x : words) std::printf(" %08x", x);
    std::printf("\n");
    // the optimistic decode's tables as the kernels read them (build_recover_tables): verify rows, then coefficient rows
    {
        const RecoverTables T = build_recover_tables<H>(ids, n, d, t, std::is_same<H, HGl>::value ? IMPL_GOLD : IMPL_U29);
        put_words("recover_vm", T.vm);
        put_words("recover_bc", T.bc);
    }
    // the second-chance tables (k_second_chance): window offsets, then every table word in the device-constant form
    const size_t S = ids.size(), rmax = S > needed ? (t < S - needed ? t : S - needed) : 0;
    if (rmax >= 1) {
        const int impl = std::is_same<H, HGl>::value ? IMPL_GOLD : IMPL_U29;
        const SecondTables T = build_second_tables<H>(ids, n, d, needed + rmax, impl);
        SecondTables L;
        L.layout(m, needed + rmax, (size_t)impl_nl(impl));
        std::printf("second %zu %d", needed + rmax, T.n_windows);
        for (int w = 0; w < T.n_windows; ++w) {
            std::printf(" %d", T.win_start[w]);
            if (L.n_windows != T.n_windows || L.win_start[w] != T.win_start[w] || L.ev_off[w] != T.ev_off[w] || L.bc_off[w] != T.bc_off[w]) return 3;
        }
        for (uint32_t x : T.words) std::printf(" %08x", x);
        std::printf("\n");
    }
    // the byte-digit tables of the matrix-core kernels (tables_mfma.hpp / tables_mfma_gl.hpp) over the decode rows of this
    // sender set: built under the sanitizers for every shape they cover, printed for the small ones
    if (m >= 2 && m <= (std::is_same<H, HGl>::value ? MFGL_MAX_M : MF_MAX_M)) {
        const auto rows = recover_coeff_rows<H>(ids, n, d, t);
        std::vector<uint32_t> tab;
        if constexpr (std::is_same<H, HGl>::value) tab = build_mfma_table_gl(rows, m);
        else tab = build_mfma_table(rows, m);
        std::printf("mfma_bytes %zu\n", tab.size() * 4);
        if (full || tab.size() * 4 <= 65536) put_words("mfma", tab);
    }
    // full: the encode's table with one row per point
    if (full && m >= 2 && m <= (std::is_same<H, HGl>::value ? MFGL_MAX_M : MF_MAX_M)) {
        std::vector<std::vector<H>> V(n, std::vector<H>(m));
        for (size_t j = 0; j < n; ++j) {
            H p = H::one();
            for (size_t k = 0; k < m; ++k) V[j][k] = p, p = p * el[j];
        }
        if constexpr (std::is_same<H, HGl>::value) put_words("enc", build_mfma_table_gl(V, m));
        else put_words("enc", build_mfma_table(V, m));
    }
    // the point-pair table of the matrix-core encode (tables_mfma.hpp::build_mfma_bfly_table) for y = X * V on this domain
    if constexpr (std::is_same<H, HFr>::value) {
        if (m >= 2 && m <= MF_BFLY_MAX_M && domain_size(n) >= 4) {
            std::vector<std::vector<HFr>> V(n, std::vector<HFr>(m));
            for (size_t j = 0; j < n; ++j) {
                HFr p = HFr::one();
                for (size_t k = 0; k < m; ++k) V[j][k] = p, p = p * el[j];
            }
            const size_t half = domain_size(n) / 2;
            const auto tab = build_mfma_bfly_table(V, m, half);
            std::printf("bfly_bytes %zu\n", tab.size() * 4);
            if (full || tab.size() * 4 <= 140000) put_words("bfly", tab);
            if (full && m <= MF_MAX_M) {  // triple generation: the same rows times the Montgomery radix 2^261
                HFr R = HFr::one();
                const HFr two = HFr::from_u64(2);
                for (int e = 0; e < 261; ++e) R = R * two;
                for (auto& row : V)
                    for (auto& v : row) v = v * R;
                put_words("bflyR", build_mfma_bfly_table(V, m, half));
            }
        }
        if (full && n == domain_size(n) && n >= 8 && n <= MF_BFLY_MAX_M) {  // the inverse transform: omega^(-i k) / n
            const HFr ninv = HFr::from_u64(n).inv();
            std::vector<std::vector<HFr>> C(n, std::vector<HFr>(n));
            for (size_t i = 0; i < n; ++i)
                for (size_t k = 0; k < n; ++k) C[i][k] = el[(n - (i * k) % n) % n] * ninv;
            put_words("bflyinv", build_mfma_bfly_table(C, n, n / 2));
        }
    }
    return 0;
}
static int impl_of(const char* name) {
    if (std::strcmp(name, "gl") == 0) return IMPL_GOLD;
    if (std::strcmp(name, "fr-sat32") == 0) return IMPL_SAT32;
    if (std::strcmp(name, "fr-u29") == 0 || std::strcmp(name, "fr") == 0) return IMPL_U29;
    return -1;
}
static HFr rdev_of(int impl) {  // the device Montgomery radix as a field value: 2^261 (u29) or 2^256 (sat32)
    HFr two = HFr::from_u64(2), p = HFr::one();
    for (int i = 0; i < (impl == IMPL_U29 ? 261 : 256); ++i) p = p * two;
    return p;
}
static int put_raw(const std::vector<uint32_t>& w) {
    std::fflush(stdout);
    return std::fwrite(w.data(), 4, w.size(), stdout) == w.size() ? 0 : 4;
}
static int run_sqrt(int impl) {
    SqrtLayout L;
    std::vector<uint32_t> w;
    if (impl == IMPL_GOLD) {
        const uint64_t mod[4] = {HGl::P, 0, 0, 0};
        w = build_sqrt_table<HGl>(mod, HGl::one(), impl, &L);
    } else {
        w = build_sqrt_table<HFr>(HFr::MOD, rdev_of(impl), impl, &L);
    }
    std::printf("sqrt %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %zu\n", L.negw, L.posw, L.r2, L.one_p, L.half, L.half_p, L.e_sqrt, L.e_inv,
                L.keyt, L.kbits, L.kshift, L.bits_sqrt, L.bits_inv, impl_nl(impl), w.size());
    return put_raw(w);
}
static int run_riss(int impl, size_t n, size_t t, long own) {
    RissLayout L;
    const std::vector<uint32_t> w = impl == IMPL_GOLD ? build_riss_table<HGl>(n, t, own, impl, &L) : build_riss_table<HFr>(n, t, own, impl, &L);
    if (w.size() != L.words) return 3;
    std::printf("riss %zu %zu %zu %zu %zu %zu %d\n", L.coef, L.red, L.coef2, L.words, L.Tn, L.ncols, L.has2 ? 1 : 0);
    return put_raw(w);
}
int main(int argc, char** argv) {
    if (argc >= 3 && std::strcmp(argv[1], "sqrt") == 0) {
        const int impl = impl_of(argv[2]);
        return impl < 0 ? 1 : run_sqrt(impl);
    }
    if (argc >= 6 && std::strcmp(argv[1], "riss") == 0) {
        const int impl = impl_of(argv[2]);
        return impl < 0 ? 1 : run_riss(impl, std::strtoul(argv[3], nullptr, 10), std::strtoul(argv[4], nullptr, 10), std::strtol(argv[5], nullptr, 10));
    }
    if (argc < 6) return 1;
    const size_t n = std::strtoul(argv[2], nullptr, 10), d = std::strtoul(argv[3], nullptr, 10), t = std::strtoul(argv[4], nullptr, 10);
    std::vector<size_t> ids;
    for (char* p = std::strtok(argv[5], ","); p; p = std::strtok(nullptr, ",")) ids.push_back(std::strtoul(p, nullptr, 10));
    if (ids.size() < d + t + 1) return 1;
    const bool full = argc > 6 && std::strcmp(argv[6], "full") == 0;
    return std::strcmp(argv[1], "gl") == 0 ? run<HGl>(n, d, t, ids, full) : run<HFr>(n, d, t, ids, full);
}
