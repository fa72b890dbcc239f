// hist_harness.cpp — the host side of include/vr/vr_hist.h (csrc/vr_hist_host.h: edges, the bin
// of a value, the percentile window) as a stand-alone program, built with -fsanitize=address,
// undefined by tests/test_hist_cpu.py.  It checks the closed forms itself (exit status 1 on a
// mismatch) and prints the edges' and windows' bits, which the test compares with tests/hist_ref.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../volumetric-renderer_amd/csrc/vr_hist_host.h"

using namespace vr;

static int g_bad = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            std::printf("FAILED line %d: %s\n", __LINE__, #x);    \
            ++g_bad;                                              \
        }                                                         \
    } while (0)

static uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

struct Counts {
    std::vector<uint64_t> bins;
    uint64_t below = 0, above = 0, nan = 0;
};

// what hist_kernel does with each voxel
static Counts count(const std::vector<float> &v, float lo, float hi, uint32_t nbins)
{
    Counts c;
    c.bins.assign(nbins, 0);
    std::vector<float> e(nbins);
    hist_edges(lo, hi, nbins, e.data());
    const double scale = hist_scale(lo, hi, nbins);
    for (float x : v) {
        if (x != x)
            ++c.nan;
        else if (x < lo)
            ++c.below;
        else if (x > hi)
            ++c.above;
        else
            ++c.bins[hist_bin(x, e.data(), nbins, lo, scale)];
    }
    return c;
}

// every edge, its predecessor, hi and hi's successor: each bin 2, one below, one above
static void edge_values(float lo, float hi, uint32_t nbins)
{
    std::vector<float> e(nbins), v;
    hist_edges(lo, hi, nbins, e.data());
    CHECK(bits(e[0]) == bits(lo));
    for (uint32_t b = 0; b < nbins; ++b) {
        if (b) CHECK(e[b] > e[b - 1]);
        v.push_back(e[b]);
        v.push_back(std::nextafterf(e[b], -INFINITY));
    }
    v.push_back(hi);
    v.push_back(std::nextafterf(hi, INFINITY));
    const Counts c = count(v, lo, hi, nbins);
    CHECK(c.below == 1 && c.above == 1 && c.nan == 0);
    for (uint32_t b = 0; b < nbins; ++b) CHECK(c.bins[b] == 2);
    std::printf("edges %a %a %u:", lo, hi, nbins);
    for (uint32_t b = 0; b < nbins; b += nbins / 8 ? nbins / 8 : 1) std::printf(" %08x", bits(e[b]));
    std::printf(" %08x\n", bits(e[nbins - 1]));
}

static void print_window(const std::vector<uint64_t> &bins, float lo, float hi, double p0, double p1)
{
    float a = -7.0f, b = -7.0f;
    const bool ok = hist_window(bins.data(), (uint32_t)bins.size(), lo, hi, p0, p1, &a, &b);
    if (!ok) CHECK(a == -7.0f && b == -7.0f);
    std::printf("window %a %a %zu %.17g %.17g: %d %08x %08x\n", lo, hi, bins.size(), p0, p1, (int)ok,
                bits(a), bits(b));
}

int main()
{
    edge_values(-1.3f, 2.7f, 1000);
    edge_values(0.0f, 65535.0f, 4096);
    edge_values(-3.0e38f, 3.0e38f, 4096);  // hi - lo overflows f32: the guess is formed in double

    {  // duplicate edges: of several equal edges the last one takes the value
        const float lo = 1.0f, hi = std::nextafterf(1.0f, 2.0f);
        float e[4];
        hist_edges(lo, hi, 4, e);
        CHECK(e[0] == lo && e[1] == lo && e[3] == hi);
        const Counts c = count({lo, hi, lo, std::nextafterf(lo, 0.0f), std::nextafterf(hi, 2.0f)}, lo, hi, 4);
        uint32_t last_lo = 0;
        for (uint32_t b = 0; b < 4; ++b)
            if (e[b] == lo) last_lo = b;
        for (uint32_t b = 0; b < 4; ++b)
            CHECK(c.bins[b] == (b == last_lo ? 2u : 0u) + (b == 3 ? 1u : 0u));
        CHECK(c.below == 1 && c.above == 1);
    }
    {  // NaN, infinities, -0.0 with lo = 0, a denormal
        const float den = std::numeric_limits<float>::denorm_min();
        const Counts c = count({NAN, INFINITY, -INFINITY, -0.0f, 0.0f, den, -den, 1.0f, 0.5f}, 0.0f, 1.0f, 2);
        CHECK(c.nan == 1 && c.above == 1 && c.below == 2);
        CHECK(c.bins[0] == 3 && c.bins[1] == 2);
    }
    {  // a byte volume over (0, 256, 256): the identity
        std::vector<float> v;
        for (int i = 0; i < 256; ++i)
            for (int k = 0; k <= i % 3; ++k) v.push_back((float)i);
        const Counts c = count(v, 0.0f, 256.0f, 256);
        for (int i = 0; i < 256; ++i) CHECK(c.bins[i] == (uint64_t)(i % 3 + 1));
    }
    {  // the window rule and every refusal
        std::vector<uint64_t> bins(64, 0);
        for (uint32_t b = 0; b < 64; ++b) bins[b] = (b * 37u) % 11u + (b == 20 ? 1000u : 0u);
        print_window(bins, -1.0f, 3.0f, 0.0, 1.0);
        print_window(bins, -1.0f, 3.0f, 0.01, 0.99);
        print_window(bins, -1.0f, 3.0f, 0.3, 0.31);
        std::vector<uint64_t> one(16, 0);
        one[5] = 9;
        print_window(one, 0.0f, 16.0f, 0.0, 1.0);
        print_window(one, 0.0f, 16.0f, 0.01, 0.99);
        one[5] = 0;
        one[15] = 1ull << 33;
        print_window(one, 0.0f, 16.0f, 0.5, 1.0);
        float a = 0, b = 0;
        CHECK(!hist_window(nullptr, 16, 0, 1, 0, 1, &a, &b));
        CHECK(!hist_window(one.data(), 16, 0, 1, 0, 1, nullptr, &b));
        CHECK(!hist_window(one.data(), 16, 0, 1, 0, 1, &a, nullptr));
        CHECK(!hist_window(one.data(), 0, 0, 1, 0, 1, &a, &b));
        CHECK(!hist_window(one.data(), 16, 1, 1, 0, 1, &a, &b));
        CHECK(!hist_window(one.data(), 16, 0, NAN, 0, 1, &a, &b));
        CHECK(!hist_window(one.data(), 16, 0, INFINITY, 0, 1, &a, &b));
        CHECK(!hist_window(one.data(), 16, 0, 1, -0.1, 1, &a, &b));
        CHECK(!hist_window(one.data(), 16, 0, 1, 0.5, 0.5, &a, &b));
        CHECK(!hist_window(one.data(), 16, 0, 1, 0, 1.5, &a, &b));
        CHECK(!hist_window(one.data(), 16, 0, 1, NAN, 1, &a, &b));
        one[15] = 0;
        CHECK(!hist_window(one.data(), 16, 0, 1, 0, 1, &a, &b));  // N == 0
        CHECK(a == 0 && b == 0);
    }
    std::printf(g_bad ? "hist harness: %d FAILED\n" : "hist harness ok\n", g_bad);
    return g_bad ? 1 : 0;
}
