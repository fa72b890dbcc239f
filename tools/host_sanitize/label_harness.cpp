// label_harness.cpp — the host side of include/vr/vr_label.h (csrc/vr_label_host.h: what a request
// is refused for, the voxel box it resolves to and its 2^32 - 1 bound, the seed and capacity checks
// and the bricks a launch walks) as a stand-alone program, built with -fsanitize=address,undefined
// by tests/test_label_cpu.py.  It checks every rule itself (exit status 1 on a mismatch) and prints
// the resolved boxes, which the test compares with its own statement of the rule.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/vr/vr_label.h"
#include "../../volumetric-renderer_amd/csrc/vr_label_host.h"
#include "harness_check.h"

using namespace vr;

static_assert(sizeof(vr_label_request) == 40, "vr_label_request is 40 bytes");
static_assert(sizeof(vr_label_component) == kLabelComponentBytes && kLabelComponentBytes == 64,
              "vr_label_component is 64 bytes");
static_assert(sizeof(vr_label_info) == 40, "vr_label_info is 40 bytes");
static_assert(VR_ENOSPC == -28, "VR_ENOSPC");

// a request's box on a dims volume: what label_box_resolve says, printed for the test
static void box_case(uint32_t use_box, const uint32_t lo[3], const uint32_t hi[3], const uint32_t dims[3])
{
    // the arrays sit at the very end of heap blocks: a read past [2] is an ASan report
    std::vector<uint32_t> mn(lo, lo + 3), mx(hi, hi + 3), dm(dims, dims + 3);
    LabelBox b;
    std::memset(&b, 0x77, sizeof b);
    const LabelBox before = b;
    const char *m = label_box_resolve(use_box, mn.data(), mx.data(), dm.data(), &b);
    bool want = use_box <= 1;
    unsigned __int128 vox = 1;
    for (int a = 0; a < 3 && want; ++a) {
        const uint32_t l = use_box ? lo[a] : 0u, h = use_box ? hi[a] : dims[a];
        want = l < h && h <= dims[a];
        if (want) vox *= h - l;
    }
    want = want && vox <= (unsigned __int128)0xFFFFFFFFull;
    CHECK((m == nullptr) == want);
    if (m) CHECK(std::memcmp(&b, &before, sizeof b) == 0);  // untouched
    unsigned long long nwork = 0;
    if (!m) {
        for (int a = 0; a < 3; ++a) {
            CHECK(b.lo[a] == (use_box ? lo[a] : 0u) && b.hi[a] == (use_box ? hi[a] : dims[a]));
            CHECK(b.ext[a] == b.hi[a] - b.lo[a]);
        }
        CHECK(b.voxels == (unsigned long long)vox && b.voxels <= kLabelMaxVoxels);
        const uint32_t cells[3] = {7, 8, 8};
        uint32_t b0[3] = {0, 0, 0}, nb[3] = {0, 0, 0};
        nwork = box_brick_range(b, cells, 2, b0, nb);  // (vr_box_host.h: the shared rule)
        for (int a = 0; a < 3; ++a) {
            // every padded voxel index of the box lies in the bricks b0 .. b0 + nb - 1
            const unsigned long long first = (unsigned long long)b.lo[a] + 2, last = (unsigned long long)b.hi[a] + 1;
            CHECK(first / cells[a] == b0[a] && last / cells[a] == (unsigned long long)b0[a] + nb[a] - 1);
        }
        const unsigned __int128 prod = (unsigned __int128)nb[0] * nb[1] * nb[2];
        CHECK(nwork >= 1 && (prod >> 64 ? nwork == ~0ull : nwork == (unsigned long long)prod));
        // the seed rule and the box-linear index, at the box's corners and just outside
        const uint32_t first[3] = {b.lo[0], b.lo[1], b.lo[2]}, last[3] = {b.hi[0] - 1, b.hi[1] - 1, b.hi[2] - 1};
        CHECK(label_seed_ok(b, first) && label_seed_ok(b, last));
        CHECK(label_linear(b, first) == 0u && label_linear(b, last) == (uint32_t)(b.voxels - 1));
        for (int a = 0; a < 3; ++a) {
            std::vector<uint32_t> s(last, last + 3);
            s[a] = b.hi[a];
            CHECK(!label_seed_ok(b, s.data()));
            s[a] = b.lo[a] - 1u;  // (wraps to 2^32 - 1 at 0: outside as well)
            CHECK(!label_seed_ok(b, s.data()));
        }
        CHECK(label_capacity_ok(b.voxels, b.voxels) && !label_capacity_ok(b.voxels - 1, b.voxels) &&
              label_capacity_ok(~0ull, b.voxels));
    }
    std::printf("box %u  %u %u %u  %u %u %u on %u %u %u: %d  %llu  %llu\n", use_box, lo[0], lo[1], lo[2], hi[0], hi[1],
                hi[2], dims[0], dims[1], dims[2], (int)(m == nullptr), m ? 0ull : (unsigned long long)b.voxels, nwork);
}

int main()
{
    {  // the window, the connectivity and use_box
        const float inf = std::numeric_limits<float>::infinity(), big = std::numeric_limits<float>::max();
        CHECK(label_request_error(NAN, 1.0f, 6, 0) != nullptr && label_request_error(0.0f, NAN, 6, 0) != nullptr);
        CHECK(label_request_error(NAN, NAN, 26, 1) != nullptr);
        CHECK(label_request_error(1.0f, 0.5f, 6, 0) != nullptr && label_request_error(inf, -inf, 6, 0) != nullptr);
        CHECK(label_request_error(inf, big, 26, 0) != nullptr);
        const float good[][2] = {{0.0f, 0.0f}, {-0.0f, 0.0f}, {0.0f, -0.0f}, {-inf, inf}, {0.25f, inf}, {-inf, -1.0f},
                                 {inf, inf}, {-inf, -inf}, {-big, big}};
        for (const auto &g : good)
            CHECK(label_request_error(g[0], g[1], 6, 0) == nullptr && label_request_error(g[0], g[1], 26, 1) == nullptr);
        const uint32_t M = 0xFFFFFFFFu;
        for (uint32_t c : {0u, 1u, 4u, 5u, 7u, 8u, 18u, 25u, 27u, 0x10006u, M})
            CHECK(label_request_error(0.0f, 1.0f, c, 0) != nullptr);
        for (uint32_t u : {2u, 3u, M}) CHECK(label_request_error(0.0f, 1.0f, 6, u) != nullptr);
    }
    {  // a device label buffer is 4-byte aligned
        alignas(8) static const unsigned char buf[8] = {0};
        CHECK(label_pointer_ok(buf) && label_pointer_ok(buf + 4) && label_pointer_ok(nullptr));
        CHECK(!label_pointer_ok(buf + 1) && !label_pointer_ok(buf + 2) && !label_pointer_ok(buf + 3));
    }
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
    box_case(0, zero3, zero3, big);    // far more than 2^32 - 1 voxels: the product passes 64 bits
    box_case(1, zero3, big, big);
    {  // the 2^32 - 1 bound, from both sides
        const uint32_t c5[3] = {8192, 1024, 1024}, half[3] = {4096, 1024, 1024}, under[3] = {4096, 1024, 1023};
        box_case(0, zero3, zero3, c5);      // 2^33
        box_case(1, zero3, half, c5);       // 2^32: one too many
        box_case(1, zero3, under, c5);      // 2^32 - 2^22
        const uint32_t line[3] = {M, 1, 1}, line2[3] = {M, 2, 1}, sq[3] = {65536, 65536, 1}, sq1[3] = {65535, 65537, 1};
        box_case(0, zero3, zero3, line);    // 2^32 - 1 exactly
        box_case(0, zero3, zero3, line2);
        box_case(0, zero3, zero3, sq);      // 2^32
        box_case(0, zero3, zero3, sq1);     // 2^32 - 1
        const uint32_t lo[3] = {1, 0, 0};
        box_case(1, lo, line2, line2);      // (2^32 - 2) * 2
    }
    return harness_done("label");
}
