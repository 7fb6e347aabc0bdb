// TEST INFRASTRUCTURE (tests/test_host_layer.py): the shared host layer of the three libraries, mpc-code_amd/csrc/mpc_host.hpp, exercised without a
// GPU - no HIP call is made.  Built with the host side under AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process:
//   host_layer_check BLOCK_IN UNPADDED_OUT
// BLOCK_IN holds a gathered block [world = 2][n = 2][dim = 3][Bs = 128] of doubles; its un-padding for B = 65 is written to UNPADDED_OUT.
#include "mpc_host.hpp"

#include <cstdlib>
#include <cstring>

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int soa_round_trips()
{
    for (int B : {1, 63, 64, 65, 130})
        for (int d : {0, 1, 3}) {
            const size_t Bs = pad64(B);
            CHECK(Bs % 64 == 0 && Bs >= (size_t)B && Bs < (size_t)B + 64);
            std::vector<double> src((size_t)B * d), soa((size_t)d * Bs, -7.0), back((size_t)B * d, -9.0);
            for (size_t i = 0; i < src.size(); i++) src[i] = 1.0 + (double)i;
            to_soa(src.data(), B, d, Bs, soa.data());
            for (int i = 0; i < d; i++) {
                for (int b = 0; b < B; b++) CHECK(soa[(size_t)i * Bs + b] == src[(size_t)b * d + i]);
                for (size_t b = B; b < Bs; b++) CHECK(soa[(size_t)i * Bs + b] == 0.0);      // the padding lanes
            }
            from_soa(soa.data(), B, d, Bs, back.data());
            CHECK(back == src);
        }
    return 0;
}

// the closed forms of mpc_loop_alloc / nmpc_alloc / enmpc_alloc: float64 log j at sum_{i<j} max_steps * dim_i * Bs over the logs the caller enables
// (a log of dimension zero is left out by the caller), int32 log i at i * max_steps * Bs
static int layout_and_ranges()
{
    const char *names[] = {"U", "X_HAT", "XS", "US", "YS", "Xp", "D_HAT"};
    const int dims[] = {2, 3, 3, 2, 0, 3, 1};      // (YS of dimension zero: skipped, the logs behind it move up)
    const std::vector<const char *> ints = {"STATUS_DYN", "STATUS_SS", "ITERS_DYN", "SQP_DYN", "SQP_SS"};
    const int ms = 7; const size_t Bs = 128;
    std::vector<std::pair<const char *, int>> dlogs;
    for (int i = 0; i < 7; i++) if (dims[i] > 0) dlogs.push_back({names[i], dims[i]});
    LogTab t;
    t.layout(dlogs, ints, ms, Bs);
    size_t off = 0;
    for (int i = 0; i < 7; i++) {
        const LogTab::Entry *e = t.find(names[i]);
        if (dims[i] == 0) { CHECK(e == nullptr); continue; }
        CHECK(e && e->off == off && e->dim == dims[i]);
        off += (size_t)ms * dims[i] * Bs;
    }
    CHECK(t.n_dbl == off && off == (size_t)ms * 14 * Bs);
    for (size_t i = 0; i < ints.size(); i++) { const LogTab::Entry *e = t.find(ints[i]); CHECK(e && e->dim == 0 && e->off == i * ms * Bs); }
    CHECK(t.n_int == ints.size() * ms * Bs && t.max_steps == ms && t.Bs == Bs);
    CHECK(t.find("SL") == nullptr && t.dev("SL") == nullptr);
    // no int32 logs (the linear library below MPC_LOG_U), no float64 logs either
    LogTab none;
    none.layout({}, {}, ms, Bs);
    CHECK(none.n_dbl == 0 && none.n_int == 0 && none.find("U") == nullptr);
    // laying out again forgets the previous table
    t.layout({{"U", 2}}, {}, 3, 64);
    CHECK(t.find("X_HAT") == nullptr && t.find("STATUS_DYN") == nullptr && t.n_dbl == 3 * 2 * 64 && t.n_int == 0);

    // addresses and the range check of steps [k0, k0 + n), on a host array standing for the device's
    t.layout(dlogs, ints, ms, Bs);
    std::vector<double> mem(t.n_dbl); std::vector<int32_t> memi(t.n_int);
    t.dbl.p = mem.data(); t.ints.p = memi.data();      // (never released: not the table's to free)
    const LogTab::Entry *xs = t.find("XS");
    CHECK(t.dev("XS") == mem.data() + xs->off && t.dev("XS", 2) == mem.data() + xs->off + 2 * 3 * Bs);
    CHECK(t.dev("ITERS_DYN", 4) == memi.data() + 2 * ms * Bs + 4 * Bs);
    const double *src = nullptr; size_t n = 0;
    CHECK(t.slice(*xs, 0, ms, &src, &n) == 0 && src == mem.data() + xs->off && n == (size_t)ms * 3 * Bs);
    CHECK(t.slice(*xs, 5, 2, &src, &n) == 0 && src == mem.data() + xs->off + 5 * 3 * Bs && n == 2 * 3 * Bs);
    g_err[0] = 0;
    CHECK(t.slice(*xs, -1, 2, &src, &n) == -1 && !std::strcmp(g_err, "steps out of range"));
    CHECK(t.slice(*xs, 0, 0, &src, &n) == -1 && t.slice(*xs, 3, -2, &src, &n) == -1);
    CHECK(t.slice(*xs, 6, 2, &src, &n) == -1 && t.slice(*xs, 0, ms + 1, &src, &n) == -1 && t.slice(*xs, ms, 1, &src, &n) == -1);
    CHECK(fail(-12, "code %d", 5) == -12 && !std::strcmp(g_err, "code 5"));
    t.dbl.p = nullptr; t.ints.p = nullptr;
    return 0;
}

static int unpad_file(const char *in, const char *out)
{
    const int world = 2, n = 2, dim = 3, B = 65; const size_t Bs = 128;
    std::vector<double> blk((size_t)world * n * dim * Bs), res((size_t)world * n * B * dim);
    FILE *f = std::fopen(in, "rb");
    CHECK(f && std::fread(blk.data(), 8, blk.size(), f) == blk.size());
    std::fclose(f);
    LogTab::unpad(blk.data(), (size_t)world * n, dim, B, Bs, res.data());
    f = std::fopen(out, "wb");
    CHECK(f && std::fwrite(res.data(), 8, res.size(), f) == res.size());
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s BLOCK_IN UNPADDED_OUT\n", argv[0]); return 2; }
    if (soa_round_trips() || layout_and_ranges() || unpad_file(argv[1], argv[2])) return 1;
    std::puts("host layer ok");
    return 0;
}
