// vr_hit_host.h — the host side of include/vr/vr_hit.h: what a hit request is refused for, and
// the pixel rectangle it resolves to on a W x H framebuffer.  Plain C++ without HIP, so a
// stand-alone program can run it (under a sanitizer, tests/test_hit_cpu.py); vr_api_hit.hip includes
// it for vr_hit_render, vr_hit_render_device, vr_hit_count_work and vr_pick.
#pragma once

#include <stdint.h>

namespace vr {

constexpr int kHitEntry = 0, kHitOpacity = 1, kHitMax = 2, kHitMin = 3, kHitIso = 4;  // vr_hit_kind
constexpr int kHitKinds = 5;
constexpr uint32_t kHitRecordBytes = 24;  // sizeof(vr_hit)

struct HitRect {
    uint32_t x0, y0, w, h;
};

// nullptr: the kind and (for OPACITY) the threshold are what vr_hit.h allows; else what is wrong.
// !(t > 0 && t <= 1) refuses a NaN as well.
inline const char *hit_kind_error(int32_t kind, float threshold)
{
    if (kind < 0 || kind >= kHitKinds) return "unknown hit kind";
    if (kind == kHitOpacity && !(threshold > 0.0f && threshold <= 1.0f))
        return "hit threshold must be in (0, 1]";
    return nullptr;
}

// The rectangle of a request on a W x H framebuffer into *r; nullptr, or what is wrong (*r is
// then untouched).  The sums are formed in 64 bits: x0 + w may pass 2^32.
inline const char *hit_rect_resolve(uint32_t use_rect, const uint32_t rect[4], uint32_t W, uint32_t H,
                                    HitRect *r)
{
    if (use_rect > 1) return "hit use_rect must be 0 or 1";
    if (W == 0 || H == 0) return "hit rectangle is empty or beyond the framebuffer";
    if (!use_rect) {
        *r = HitRect{0, 0, W, H};
        return nullptr;
    }
    if (rect[2] == 0 || rect[3] == 0 || (uint64_t)rect[0] + rect[2] > (uint64_t)W ||
        (uint64_t)rect[1] + rect[3] > (uint64_t)H)
        return "hit rectangle is empty or beyond the framebuffer";
    *r = HitRect{rect[0], rect[1], rect[2], rect[3]};
    return nullptr;
}

// vr_pick's pixel: the 1 x 1 rectangle at (px, py).
inline const char *hit_pick_resolve(uint32_t px, uint32_t py, uint32_t W, uint32_t H, HitRect *r)
{
    if (px >= W || py >= H) return "pick pixel is beyond the framebuffer";
    *r = HitRect{px, py, 1, 1};
    return nullptr;
}

// Bytes of a resolved rectangle's records.  (The rectangle lies inside the caller's framebuffer,
// which bounds w * h far below 2^64 / 24.)
inline uint64_t hit_bytes(const HitRect &r) { return (uint64_t)r.w * r.h * kHitRecordBytes; }

}  // namespace vr
