// hist_harness.cpp — the host side of include/vr/vr_hist.h (csrc/vr_hist_host.h: edges, the bin
// of a value, the percentile window; csrc/vr_box_host.h: the request box and its bricks) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_hist_cpu.py.  It checks
// the closed forms itself (exit status 1 on a mismatch) and prints the edges' and windows' bits,
// which the test compares with tests/hist_ref.py, and the resolved boxes, which the test compares
// with its own statement of the rule.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../volumetric-renderer_amd/csrc/vr_hist_host.h"
#include "harness_check.h"

using namespace vr;

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

// a request's box on a dims volume: what the shared rule (vr_box_host.h, which vr_histogram uses as
// it is) says, printed for the test in the label harness's format
static void box_case(uint32_t use_box, const uint32_t lo[3], const uint32_t hi[3], const uint32_t dims[3])
{
    // the arrays sit at the very end of heap blocks: a read past [2] is an ASan report
    std::vector<uint32_t> mn(lo, lo + 3), mx(hi, hi + 3), dm(dims, dims + 3);
    VoxelBox b;
    std::memset(&b, 0x77, sizeof b);
    const VoxelBox before = b;
    const BoxError e = box_resolve(use_box, mn.data(), mx.data(), dm.data(), &b);
    bool want = use_box <= 1;
    unsigned __int128 vox = 1;
    for (int a = 0; a < 3 && want; ++a) {
        const uint32_t l = use_box ? lo[a] : 0u, h = use_box ? hi[a] : dims[a];
        want = l < h && h <= dims[a];
        if (want) vox *= h - l;
    }
    CHECK((e == kBoxOk) == want && (e == kBoxUse) == (use_box > 1));
    if (e) CHECK(std::memcmp(&b, &before, sizeof b) == 0);  // untouched
    unsigned long long nwork = 0;
    if (!e) {
        for (int a = 0; a < 3; ++a) {
            CHECK(b.lo[a] == (use_box ? lo[a] : 0u) && b.hi[a] == (use_box ? hi[a] : dims[a]));
            CHECK(b.ext[a] == b.hi[a] - b.lo[a]);
        }
        CHECK(vox >> 64 ? b.voxels == ~0ull : b.voxels == (unsigned long long)vox);  // saturates
        const uint32_t cells[3] = {7, 8, 8};
        uint32_t b0[3] = {0, 0, 0}, nb[3] = {0, 0, 0};
        nwork = box_brick_range(b, cells, 2, b0, nb);
        for (int a = 0; a < 3; ++a) {
            // every padded voxel index of the box lies in the bricks b0 .. b0 + nb - 1
            const unsigned long long first = (unsigned long long)b.lo[a] + 2, last = (unsigned long long)b.hi[a] + 1;
            CHECK(first / cells[a] == b0[a] && last / cells[a] == (unsigned long long)b0[a] + nb[a] - 1);
        }
        const unsigned __int128 prod = (unsigned __int128)nb[0] * nb[1] * nb[2];
        CHECK(nwork >= 1 && (prod >> 64 ? nwork == ~0ull : nwork == (unsigned long long)prod));
    }
    std::printf("box %u  %u %u %u  %u %u %u on %u %u %u: %d  %llu  %llu\n", use_box, lo[0], lo[1], lo[2], hi[0], hi[1],
                hi[2], dims[0], dims[1], dims[2], (int)(e == kBoxOk), e ? 0ull : (unsigned long long)b.voxels, nwork);
}

int main()
{
    {  // the request box: the label harness's cases but those of its 2^32 - 1 bound
        const uint32_t M = 0xFFFFFFFFu;
        const uint32_t dims[3] = {19, 17, 21}, big[3] = {M, M, M}, zero3[3] = {0, 0, 0};
        struct {
            uint32_t use, lo[3], hi[3];
        } cases[] = {
            {0, {0, 0, 0}, {0, 0, 0}},      // the whole volume: the box is not read for sense
            {0, {9, 9, 9}, {1, 1, 1}},
            {1, {0, 0, 0}, {19, 17, 21}},
            {1, {3, 2, 5}, {15, 13, 18}},
            {1, {3, 2, 5}, {4, 13, 18}},    // one voxel along x
            {1, {18, 16, 20}, {19, 17, 21}},
            {1, {0, 0, 0}, {20, 17, 21}},   // beyond, by one
            {1, {0, 0, 0}, {19, 18, 21}},
            {1, {0, 0, 0}, {19, 17, 22}},
            {1, {3, 3, 3}, {3, 4, 4}},      // empty
            {1, {3, 5, 3}, {4, 4, 4}},      // min above max
            {1, {0, 0, M}, {1, 1, 1}},
            {1, {0, 0, 0}, {1, M, 1}},
            {2, {0, 0, 0}, {1, 1, 1}},      // use_box
            {M, {0, 0, 0}, {1, 1, 1}},
        };
        for (const auto &c : cases) box_case(c.use, c.lo, c.hi, dims);
        box_case(0, zero3, zero3, zero3);  // no volume
        box_case(0, zero3, zero3, big);    // no bound here: the voxel product passes 64 bits and saturates
        box_case(1, zero3, big, big);
    }
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
    return harness_done("hist");
}
