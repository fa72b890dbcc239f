// vr_label_host.h — the host side of include/vr/vr_label.h: what a label request is refused for,
// the voxel box it resolves to on an nx x ny x nz volume, the 2^32 - 1 bound, the seed and capacity
// checks (the bricks a launch walks: vr_box_host.h).  Plain C++ without HIP, so a stand-alone program
// can run it (under a sanitizer, tests/test_label_cpu.py); vr_api_label.hip includes it for
// vr_label_* and vr_region_grow*.
#pragma once

#include <stdint.h>

#include <cmath>

#include "vr_box_host.h"

namespace vr {

constexpr uint32_t kLabelComponentBytes = 64;          // sizeof(vr_label_component)
constexpr uint64_t kLabelMaxVoxels = 0xFFFFFFFFull;    // a label is 1 + a box-linear index, in 32 bits

using LabelBox = VoxelBox;  // (vr_box_host.h)

// nullptr: lo, hi, connectivity and use_box are what vr_label.h allows; else what is wrong.
inline const char *label_request_error(float lo, float hi, uint32_t connectivity, uint32_t use_box)
{
    if (std::isnan(lo) || std::isnan(hi)) return "label window bounds must not be NaN";
    if (lo > hi) return "label window needs lo <= hi";
    if (connectivity != 6 && connectivity != 26) return "label connectivity must be 6 or 26";
    if (use_box > 1) return "label use_box must be 0 or 1";
    return nullptr;
}

// The box of a request on a volume of dims voxels into *b; nullptr, or what is wrong (*b is then
// untouched).  The shared rule (box_resolve), and at most 2^32 - 1 voxels, so that every label fits.
inline const char *label_box_resolve(uint32_t use_box, const uint32_t box_min[3], const uint32_t box_max[3],
                                     const uint32_t dims[3], LabelBox *b)
{
    LabelBox r;
    switch (box_resolve(use_box, box_min, box_max, dims, &r)) {
        case kBoxUse: return "label use_box must be 0 or 1";
        case kBoxEmpty: return "label box is empty or beyond the volume";
        case kBoxOk: break;
    }
    if (r.voxels > kLabelMaxVoxels) return "label box holds more than 2^32 - 1 voxels: label it box by box";
    *b = r;
    return nullptr;
}

// The seed is a volume voxel index inside the box.
inline bool label_seed_ok(const LabelBox &b, const uint32_t seed[3])
{
    for (int a = 0; a < 3; ++a)
        if (seed[a] < b.lo[a] || seed[a] >= b.hi[a]) return false;
    return true;
}

// Box-linear index of volume voxel v, a voxel of the box.
inline uint32_t label_linear(const LabelBox &b, const uint32_t v[3])
{
    return (v[0] - b.lo[0]) + b.ext[0] * ((v[1] - b.lo[1]) + b.ext[1] * (v[2] - b.lo[2]));
}

// The kernels store labels as 32-bit words (and with 32-bit atomics): a device label buffer is
// 4-byte aligned.
inline bool label_pointer_ok(const void *labels) { return (reinterpret_cast<uintptr_t>(labels) & 3u) == 0; }

// A buffer of cap records holds the n of a result.
inline bool label_capacity_ok(uint64_t cap, uint64_t n) { return cap >= n; }

}  // namespace vr
