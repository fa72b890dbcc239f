// hit_harness.cpp — the host side of include/vr/vr_hit.h (csrc/vr_hit_host.h: what a request is
// refused for, and the rectangle it resolves to) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_hit_cpu.py.  It checks every rule itself (exit
// status 1 on a mismatch) and prints the resolved rectangles, which the test compares with its
// own statement of the rule.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/vr/vr_hit.h"
#include "../../volumetric-renderer_amd/csrc/vr_hit_host.h"
#include "harness_check.h"

using namespace vr;

static_assert(sizeof(vr_hit_request) == 28, "vr_hit_request is 28 bytes");
static_assert(sizeof(vr_hit) == kHitRecordBytes && kHitRecordBytes == 24, "vr_hit is 24 bytes");
static_assert(kHitEntry == VR_HIT_ENTRY && kHitOpacity == VR_HIT_OPACITY && kHitMax == VR_HIT_MAX &&
                  kHitMin == VR_HIT_MIN && kHitIso == VR_HIT_ISO && kHitKinds == VR_HIT_ISO + 1,
              "the kinds are enum vr_hit_kind");

// a request's rectangle on a W x H framebuffer: what hit_rect_resolve says, printed for the test
static void rect_case(uint32_t use_rect, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t W,
                      uint32_t H)
{
    // the rectangle sits at the very end of a heap block: a read past rect[3] is an ASan report
    std::vector<uint32_t> r{x0, y0, w, h};
    HitRect out{7, 7, 7, 7};
    const char *m = hit_rect_resolve(use_rect, r.data(), W, H, &out);
    // the rule, restated: 64-bit sums, nothing empty
    const bool want = use_rect <= 1 && W > 0 && H > 0 &&
                      (!use_rect || (w >= 1 && h >= 1 && (unsigned long long)x0 + w <= W &&
                                     (unsigned long long)y0 + h <= H));
    CHECK((m == nullptr) == want);
    if (m) {
        CHECK(out.x0 == 7 && out.y0 == 7 && out.w == 7 && out.h == 7);  // untouched
    } else if (use_rect) {
        CHECK(out.x0 == x0 && out.y0 == y0 && out.w == w && out.h == h);
    } else {
        CHECK(out.x0 == 0 && out.y0 == 0 && out.w == W && out.h == H);
    }
    if (!m) CHECK(hit_bytes(out) == 24ull * out.w * out.h);
    std::printf("rect %u %u %u %u %u on %u %u: %d %u %u %u %u\n", use_rect, x0, y0, w, h, W, H,
                (int)(m == nullptr), out.x0, out.y0, out.w, out.h);
}

int main()
{
    {  // kinds and thresholds
        for (int k = -2; k <= 7; ++k) CHECK((hit_kind_error(k, 0.5f) == nullptr) == (k >= 0 && k <= 4));
        CHECK(hit_kind_error(std::numeric_limits<int32_t>::min(), 0.5f) != nullptr);
        CHECK(hit_kind_error(std::numeric_limits<int32_t>::max(), 0.5f) != nullptr);
        const float bad[] = {NAN, 0.0f, -0.0f, -1.0f, std::nextafterf(1.0f, 2.0f), 2.0f, INFINITY, -INFINITY};
        for (float t : bad) {
            CHECK(hit_kind_error(kHitOpacity, t) != nullptr);
            for (int k : {kHitEntry, kHitMax, kHitMin, kHitIso}) CHECK(hit_kind_error(k, t) == nullptr);
        }
        const float good[] = {std::numeric_limits<float>::denorm_min(), 0.25f, 0.9f,
                              std::nextafterf(1.0f, 0.0f), 1.0f};
        for (float t : good) CHECK(hit_kind_error(kHitOpacity, t) == nullptr);
    }
    const uint32_t M = 0xFFFFFFFFu;
    rect_case(0, 0, 0, 0, 0, 45, 35);      // the whole frame: the rectangle is not read for sense
    rect_case(0, 99, 99, 99, 99, 45, 35);
    rect_case(1, 0, 0, 45, 35, 45, 35);
    rect_case(1, 13, 7, 20, 18, 45, 35);
    rect_case(1, 44, 34, 1, 1, 45, 35);
    rect_case(1, 45, 34, 1, 1, 45, 35);    // beyond, by one
    rect_case(1, 44, 35, 1, 1, 45, 35);
    rect_case(1, 44, 34, 2, 1, 45, 35);
    rect_case(1, 44, 34, 1, 2, 45, 35);
    rect_case(1, 0, 0, 0, 1, 45, 35);      // empty
    rect_case(1, 0, 0, 1, 0, 45, 35);
    rect_case(1, 1, 0, M, 1, 45, 35);      // x0 + w wraps in 32 bits
    rect_case(1, 0, 2, 1, M - 1, 45, 35);
    rect_case(1, M, M, M, M, M, M);
    rect_case(1, 0, 0, M, M, M, M);        // the largest there is
    rect_case(2, 0, 0, 1, 1, 45, 35);      // use_rect
    rect_case(M, 0, 0, 1, 1, 45, 35);
    rect_case(0, 0, 0, 1, 1, 0, 35);       // no framebuffer
    rect_case(1, 0, 0, 1, 1, 45, 0);
    {  // vr_pick's pixel
        HitRect r{7, 7, 7, 7};
        CHECK(hit_pick_resolve(45, 0, 45, 35, &r) != nullptr && hit_pick_resolve(0, 35, 45, 35, &r) != nullptr);
        CHECK(hit_pick_resolve(M, M, 45, 35, &r) != nullptr && hit_pick_resolve(0, 0, 0, 0, &r) != nullptr);
        CHECK(r.x0 == 7 && r.y0 == 7 && r.w == 7 && r.h == 7);
        CHECK(hit_pick_resolve(44, 34, 45, 35, &r) == nullptr);
        CHECK(r.x0 == 44 && r.y0 == 34 && r.w == 1 && r.h == 1 && hit_bytes(r) == 24);
    }
    return harness_done("hit");
}
