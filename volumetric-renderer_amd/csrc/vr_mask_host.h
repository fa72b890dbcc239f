// vr_mask_host.h — the one statement of the grid rule of the mask families (include/vr/vr_morph.h,
// vr_maskcc.h, vr_mstat.h, vr_mview.h): the grid a request resolves to, its two bounds, and what an array or an
// output of a call is refused for.  Like vr_box_host.h it answers with a reason code; each family
// (vr_<family>_host.h) owns the texts, its further request fields and its geometry.  Plain C++
// without HIP, so a stand-alone program can run it (under a sanitizer, tests/test_mask_host_cpu.py).
#pragma once

#include <stdint.h>

namespace vr {

constexpr uint32_t kMaskMaxExtent = 32768u;         // VR_MORPH_MAX_EXTENT, VR_MASKCC_MAX_EXTENT, VR_MSTAT_MAX_EXTENT, VR_MVIEW_MAX_EXTENT
constexpr uint64_t kMaskMaxVoxels = 0xFFFFFFFFull;  // a box-linear index, and 1 + it, fits 32 bits
constexpr int kMaskOk = 0, kMaskEinval = -22, kMaskEnospc = -28;  // VR_OK, VR_EINVAL, VR_ENOSPC

// What a check found; a family's text table is indexed by it (kMaskFine: no text).
enum MaskReason {
    kMaskFine = 0,
    kMaskExtent,     // an extent outside [1, kMaskMaxExtent]
    kMaskVoxels,     // more than kMaskMaxVoxels voxels
    kMaskElemBytes,  // elem_bytes neither 1 nor 4
    kMaskAlign,      // a 4-byte array in device memory that is not 4-byte aligned
    kMaskOverlap,    // the output shares a byte with an input
    kMaskShort,      // the output holds fewer elements than a full-size call writes
    kMaskReasons
};

// ext voxels whose voxel (0, 0, 0) is the volume voxel `origin` (zero where a family has none).
struct MaskGrid {
    uint32_t ext[3];
    uint32_t origin[3];
    uint64_t voxels;
};

// The grid of ext at origin 0 into *g; kMaskFine, or kMaskExtent or kMaskVoxels with *g untouched.
inline MaskReason mask_grid_resolve(const uint32_t ext[3], MaskGrid *g)
{
    uint64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        if (ext[a] < 1 || ext[a] > kMaskMaxExtent) return kMaskExtent;
        n *= ext[a];  // (at most 2^45)
    }
    if (n > kMaskMaxVoxels) return kMaskVoxels;
    for (int a = 0; a < 3; ++a) {
        g->ext[a] = ext[a];
        g->origin[a] = 0;
    }
    g->voxels = n;
    return kMaskFine;
}

// [a, a + na) and [b, b + nb) share a byte.
inline bool mask_overlap(const void *a, uint64_t na, const void *b, uint64_t nb)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb ? pb - pa < na : pa - pb < nb;
}

inline bool mask_aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// A refusal: its text into *msg, its code returned.
inline int mask_refuse(const char **msg, const char *text, int code)
{
    *msg = text;
    return code;
}

// An input array (NULL where the call allows none): kMaskFine, kMaskElemBytes or kMaskAlign.  The
// alignment binds device memory only: a host array is copied byte by byte.
inline MaskReason mask_check_array(const void *array, uint32_t elem_bytes, bool device)
{
    if (elem_bytes != 1 && elem_bytes != 4) return kMaskElemBytes;
    return device && elem_bytes == 4 && !mask_aligned4(array) ? kMaskAlign : kMaskFine;
}

// An output of cap elements of out_elem bytes, where a full-size call writes `full`, against the
// in_bytes bytes of an input (NULL: none).  kMaskOverlap for what a full-size call would touch,
// min(cap, full) elements; then kMaskShort for cap < full; kMaskFine.
inline MaskReason mask_check_output(const void *in, uint64_t in_bytes, const void *out, uint32_t out_elem, uint64_t cap,
                                    uint64_t full)
{
    const uint64_t n = cap < full ? cap : full;
    if (in && n && mask_overlap(in, in_bytes, out, n * out_elem)) return kMaskOverlap;
    return cap < full ? kMaskShort : kMaskFine;
}

// The end of a request check that found no kMaskEinval: r into *g, then kMaskEnospc with `text`
// for an output that is kMaskShort (the caller reports g->voxels), or kMaskOk.
inline int mask_resolved(const MaskGrid &r, MaskReason output, const char *text, MaskGrid *g, const char **msg)
{
    *g = r;
    return output == kMaskShort ? mask_refuse(msg, text, kMaskEnospc) : kMaskOk;
}

}  // namespace vr
