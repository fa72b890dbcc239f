// vr_morph_host.h — the host side of include/vr/vr_morph.h: what a distance-transform or morphology
// request is refused for, the grid it resolves to, and how one axis pass is cut into workgroup
// tiles.  Plain C++ without HIP, so a stand-alone program can run it (under a sanitizer,
// tests/test_morph_cpu.py); vr_api_morph.hip includes it for vr_edt_squared* and vr_mask_morph*,
// vr_morph_kernels.hip for the tiling.
#pragma once

#include <stdint.h>

namespace vr {

constexpr uint32_t kMorphNone = 0xFFFFFFFFu;        // VR_EDT_NONE
constexpr uint32_t kMorphMaxExtent = 32768u;        // VR_MORPH_MAX_EXTENT
constexpr uint64_t kMorphMaxVoxels = 0xFFFFFFFFull;  // a box-linear index fits 32 bits
constexpr int kMorphOk = 0, kMorphEinval = -22, kMorphEnospc = -28;  // VR_OK, VR_EINVAL, VR_ENOSPC
constexpr uint32_t kMorphOps = 4, kMorphTargets = 2;  // enum vr_morph_op, enum vr_edt_target

struct MorphGrid {
    uint32_t ext[3];
    uint64_t voxels;
};

// The grid of ext into *g; nullptr, or what is wrong (*g is then untouched).
inline const char *morph_grid_resolve(const uint32_t ext[3], MorphGrid *g)
{
    uint64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        if (ext[a] < 1 || ext[a] > kMorphMaxExtent) return "morph extent must lie in [1, 32768]";
        n *= ext[a];  // (at most 2^45)
    }
    if (n > kMorphMaxVoxels) return "morph grid holds more than 2^32 - 1 voxels";
    for (int a = 0; a < 3; ++a) g->ext[a] = ext[a];
    g->voxels = n;
    return nullptr;
}

// [a, a + na) and [b, b + nb) share a byte.
inline bool morph_overlap(const void *a, uint64_t na, const void *b, uint64_t nb)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb ? pb - pa < na : pa - pb < nb;
}

inline bool morph_aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// A refusal: its text into *msg, its code returned.
inline int morph_refuse(const char **msg, const char *text, int code)
{
    *msg = text;
    return code;
}

// What both calls share: the NULL arguments, the grid, the element width, the mask's alignment
// (device memory only: a host array is copied byte by byte), the overlap of an output of out_elem
// bytes per voxel with the mask, and the capacity.  kMorphOk with *g resolved; kMorphEinval;
// or kMorphEnospc with *g resolved (the caller reports g->voxels).  *msg names a refusal.
inline int morph_check_common(const uint32_t *ext, const void *mask, uint32_t elem_bytes, const void *out,
                              uint32_t out_elem, uint64_t cap, const void *info, bool device, MorphGrid *g,
                              const char **msg)
{
    *msg = nullptr;
    if (!ext || !mask || !out || !info) return morph_refuse(msg, "NULL argument", kMorphEinval);
    MorphGrid r;
    if (const char *m = morph_grid_resolve(ext, &r)) return morph_refuse(msg, m, kMorphEinval);
    if (elem_bytes != 1 && elem_bytes != 4) return morph_refuse(msg, "morph elem_bytes must be 1 or 4", kMorphEinval);
    if (device && elem_bytes == 4 && !morph_aligned4(mask))
        return morph_refuse(msg, "a 4-byte mask must be 4-byte aligned", kMorphEinval);
    if (device && out_elem == 4 && !morph_aligned4(out))
        return morph_refuse(msg, "dist2_dev must be 4-byte aligned", kMorphEinval);
    // the overlap of what a full-size call would touch: min(cap, voxels) elements of the output
    const uint64_t out_n = cap < r.voxels ? cap : r.voxels;
    if (morph_overlap(mask, r.voxels * elem_bytes, out, out_n * out_elem) && out_n)
        return morph_refuse(msg, "the output overlaps the mask", kMorphEinval);
    *g = r;
    if (cap < r.voxels)
        return morph_refuse(msg, "the output buffer is smaller than the grid (see the info's voxels)", kMorphEnospc);
    return kMorphOk;
}

inline int morph_check_edt(const uint32_t *ext, const void *mask, uint32_t elem_bytes, uint32_t target,
                           const void *dist2, uint64_t dcap, const void *info, bool device, MorphGrid *g,
                           const char **msg)
{
    const int rc = morph_check_common(ext, mask, elem_bytes, dist2, 4, dcap, info, device, g, msg);
    if (rc == kMorphEinval) return rc;
    if (target >= kMorphTargets) return morph_refuse(msg, "edt target must be VR_EDT_TO_SET or VR_EDT_TO_UNSET", kMorphEinval);
    return rc;
}

inline int morph_check_morph(const uint32_t *ext, uint32_t op, uint32_t r2, const void *mask, uint32_t elem_bytes,
                             const void *out, uint64_t mcap, const void *info, bool device, MorphGrid *g,
                             const char **msg)
{
    const int rc = morph_check_common(ext, mask, elem_bytes, out, 1, mcap, info, device, g, msg);
    if (rc == kMorphEinval) return rc;
    if (op >= kMorphOps) return morph_refuse(msg, "morph op must be one of enum vr_morph_op", kMorphEinval);
    if (r2 == kMorphNone) return morph_refuse(msg, "morph r2 must be below VR_EDT_NONE", kMorphEinval);
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

inline MorphAxis morph_axis(const MorphGrid &g, int axis /* 1: y, 2: z */)
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
