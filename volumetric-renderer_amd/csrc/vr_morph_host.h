// vr_morph_host.h — the host side of include/vr/vr_morph.h: what a distance-transform or morphology
// request is refused for (the grid rule is vr_mask_host.h's, the texts and the request's own fields
// are here) and how one axis pass is cut into workgroup tiles.  Plain C++ without HIP, so a stand-alone program can run it (under a sanitizer,
// tests/test_morph_cpu.py); vr_api_morph.hip includes it for vr_edt_squared* and vr_mask_morph*,
// vr_morph_kernels.hip for the tiling.
#pragma once

#include <stdint.h>

#include "vr_mask_host.h"

namespace vr {

constexpr uint32_t kMorphNone = 0xFFFFFFFFu;        // VR_EDT_NONE
constexpr uint32_t kMorphOps = 4, kMorphTargets = 2;  // enum vr_morph_op, enum vr_edt_target

// The family's texts for the shared rule (vr_mask_host.h MaskReason; the outputs' are below).
constexpr const char *kMorphTexts[kMaskAlign + 1] = {
    nullptr, "morph extent must lie in [1, 32768]", "morph grid holds more than 2^32 - 1 voxels",
    "morph elem_bytes must be 1 or 4", "a 4-byte mask must be 4-byte aligned"};

// What both calls share: the NULL arguments, the grid, the element width, the mask's alignment,
// the overlap of an output of out_elem bytes per voxel with the mask, and the capacity.  kMaskOk
// with *g resolved; kMaskEinval (*g untouched); or kMaskEnospc with *g resolved (the caller reports
// g->voxels).  *msg names a refusal.
inline int morph_check_common(const uint32_t *ext, const void *mask, uint32_t elem_bytes, const void *out,
                              uint32_t out_elem, uint64_t cap, const void *info, bool device, MaskGrid *g,
                              const char **msg)
{
    *msg = nullptr;
    if (!ext || !mask || !out || !info) return mask_refuse(msg, "NULL argument", kMaskEinval);
    MaskGrid r;
    if (MaskReason why = mask_grid_resolve(ext, &r)) return mask_refuse(msg, kMorphTexts[why], kMaskEinval);
    if (MaskReason why = mask_check_array(mask, elem_bytes, device)) return mask_refuse(msg, kMorphTexts[why], kMaskEinval);
    if (device && out_elem == 4 && !mask_aligned4(out))
        return mask_refuse(msg, "dist2_dev must be 4-byte aligned", kMaskEinval);
    const MaskReason o = mask_check_output(mask, r.voxels * elem_bytes, out, out_elem, cap, r.voxels);
    if (o == kMaskOverlap) return mask_refuse(msg, "the output overlaps the mask", kMaskEinval);
    return mask_resolved(r, o, "the output buffer is smaller than the grid (see the info's voxels)", g, msg);
}

inline int morph_check_edt(const uint32_t *ext, const void *mask, uint32_t elem_bytes, uint32_t target,
                           const void *dist2, uint64_t dcap, const void *info, bool device, MaskGrid *g,
                           const char **msg)
{
    const int rc = morph_check_common(ext, mask, elem_bytes, dist2, 4, dcap, info, device, g, msg);
    if (rc == kMaskEinval) return rc;
    if (target >= kMorphTargets) return mask_refuse(msg, "edt target must be VR_EDT_TO_SET or VR_EDT_TO_UNSET", kMaskEinval);
    return rc;
}

inline int morph_check_morph(const uint32_t *ext, uint32_t op, uint32_t r2, const void *mask, uint32_t elem_bytes,
                             const void *out, uint64_t mcap, const void *info, bool device, MaskGrid *g,
                             const char **msg)
{
    const int rc = morph_check_common(ext, mask, elem_bytes, out, 1, mcap, info, device, g, msg);
    if (rc == kMaskEinval) return rc;
    if (op >= kMorphOps) return mask_refuse(msg, "morph op must be one of enum vr_morph_op", kMaskEinval);
    if (r2 == kMorphNone) return mask_refuse(msg, "morph r2 must be below VR_EDT_NONE", kMaskEinval);
    return rc;
}

// ---- one axis pass, cut into tiles (vr_morph_kernels.hip morph_edt_axis_kernel) ----
// The pass along y sees bz slabs of by lines of bx voxels; the pass along z one slab of bz lines
// of bx * by voxels.  A workgroup stages a tile of `width` neighbouring columns, all `n` voxels of
// each, in LDS: width is the largest power of two up to 64 with width * n <= words, and 1 for a
// column longer than that (n <= words always: kMorphLdsWordsLong holds the longest column).
constexpr uint32_t kMorphLdsWords = 16384;      // 64 KiB: two workgroups a CU
constexpr uint32_t kMorphLdsWordsLong = 32768;  // 128 KiB: columns of more than 16384 voxels

struct MorphAxis {
    uint32_t n;            // voxels of a column
    uint32_t width_log2;   // log2 of the columns in a tile
    uint64_t line;         // voxels of a line, the stride between a column's voxels
    uint64_t slabs;        // independent slabs, slab * line * n voxels apart
    uint64_t tiles_line;   // tiles across a line
    uint64_t tiles;        // slabs * tiles_line
    uint32_t lds_words;    // kMorphLdsWords or kMorphLdsWordsLong
};

inline MorphAxis morph_axis(const MaskGrid &g, int axis /* 1: y, 2: z */)
{
    MorphAxis A;
    A.n = g.ext[axis];
    A.line = axis == 1 ? g.ext[0] : (uint64_t)g.ext[0] * g.ext[1];
    A.slabs = axis == 1 ? g.ext[2] : 1;
    A.lds_words = A.n > kMorphLdsWords ? kMorphLdsWordsLong : kMorphLdsWords;
    uint32_t lg = 6;
    while (lg > 0 && ((uint64_t)A.n << lg) > A.lds_words) --lg;
    A.width_log2 = lg;
    A.tiles_line = (A.line + (1ull << lg) - 1) >> lg;
    A.tiles = A.slabs * A.tiles_line;
    return A;
}

}  // namespace vr
