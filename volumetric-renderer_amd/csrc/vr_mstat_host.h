// vr_mstat_host.h — the host side of include/vr/vr_mstat.h: what a request is refused for (the grid
// rule is vr_mask_host.h's, the texts, the origin and the request's own fields are here), the launch
// geometry and scratch layout of its passes, and the voxel-to-element addressing of the base
// bricks, which the kernels share.  Plain C++ without HIP, so a stand-alone
// program can run it (under a sanitizer, tests/test_mstat_cpu.py); vr_api_mstat.hip includes it for
// the entry points, vr_mstat_kernels.hip for the geometry and the addressing.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "vr_hist_host.h"  // hist_range_ok, and with it vr_box_host.h
#include "vr_mask_host.h"

#if defined(__HIPCC__)
#define VR_MSTAT_HD __host__ __device__
#else
#define VR_MSTAT_HD
#endif

namespace vr {

constexpr uint64_t kMstatMaxTable = 0xFFFFFFFFull;   // a record slot is 32 bits, as a box-linear index
constexpr uint32_t kMstatNone = 0xFFFFFFFFu;         // VR_MSTAT_NONE
constexpr uint32_t kMstatRecordBytes = 64;           // sizeof(vr_mstat_region), sizeof(vr_label_component)
constexpr uint32_t kMstatAccBytes = 48;              // one region's accumulators (vr_mstat_kernels.h MstatAcc)
constexpr uint32_t kMstatTileX = 64, kMstatTileY = 4;  // a workgroup's tile: a wave per row, 64 voxels of it
constexpr uint32_t kMstatMaxGrid = 4096;             // workgroups of a launch: the rest is strided
constexpr uint32_t kMstatCounters = 8;               // 64-bit words (vr_mstat_kernels.h MstatCounter)

// ---- the base bricks (vr_internal.h, restated: nothing of it is host-only) ----
// A layout a context can hold: its brick's cells and elements per axis, the elements a brick is
// padded to, and the values an element holds (component 0 is the voxel's own).
struct MstatLayout {
    uint32_t bx, by, bz;  // cells of a brick
    uint32_t ex, ey;      // elements of a brick row and of a brick column
    uint32_t elems;       // elements of a brick
    uint32_t vpe;         // values per element
};
enum MstatKind { kMstatF32 = 0, kMstatQuad16 = 1, kMstatQuad8 = 2, kMstatPlain8 = 3, kMstatKinds = 4 };
constexpr uint32_t kMstatPad = 2;  // kPad

VR_MSTAT_HD constexpr MstatLayout mstat_layout(int kind)
{
    // GeomWide: 8^3 cells, 9^3 elements; GeomByte: 7 x 8 x 8 cells, 8 x 9 x 9 elements
    return kind == kMstatPlain8 ? MstatLayout{7, 8, 8, 8, 9, 648, 1}
                                : MstatLayout{8, 8, 8, 9, 9, 729, kind == kMstatF32 ? 2u : 4u};
}

// bricks_for (no brick groups)
VR_MSTAT_HD constexpr uint32_t mstat_bricks(uint32_t n, uint32_t cells) { return (n + 3u) / cells + 1u; }

// The element of volume voxel (x, y, z) in the base bricks of an nbx x nby x * brick grid: hist_kernel's
// addressing.  The voxel's value is component 0 of it, base[element * vpe].
VR_MSTAT_HD constexpr uint64_t mstat_element(const MstatLayout &L, uint32_t nbx, uint32_t nby, uint32_t x, uint32_t y,
                                             uint32_t z)
{
    const uint32_t px = x + kMstatPad, py = y + kMstatPad, pz = z + kMstatPad;
    const uint32_t bx = px / L.bx, by = py / L.by, bz = pz / L.bz;
    const uint32_t xl = px - bx * L.bx, yl = py - by * L.by, zl = pz - bz * L.bz;
    const uint64_t slot = ((uint64_t)bz * nby + by) * nbx + bx;  // brick_slot
    return slot * L.elems + ((zl * L.ey + yl) * L.ex + xl);
}

// ---- the grid ----
// The family's texts for the shared rule (vr_mask_host.h MaskReason; the outputs' are below).
constexpr const char *kMstatTexts[kMaskAlign + 1] = {
    nullptr, "grid extent must lie in [1, 32768]", "grid holds more than 2^32 - 1 voxels", "elem_bytes must be 1 or 4",
    "a 4-byte array must be 4-byte aligned"};

// What every call shares: the extents, the origin, the element width and the array's alignment
// (array may be NULL where the call allows it).
inline int mstat_check_grid(const uint32_t *ext, const uint32_t *origin, const void *array, uint32_t elem_bytes,
                            bool device, MaskGrid *r, const char **msg)
{
    if (MaskReason why = mask_grid_resolve(ext, r)) return mask_refuse(msg, kMstatTexts[why], kMaskEinval);
    for (int a = 0; a < 3; ++a) r->origin[a] = origin[a];
    if (MaskReason why = mask_check_array(array, elem_bytes, device)) return mask_refuse(msg, kMstatTexts[why], kMaskEinval);
    return kMaskOk;
}

// The grid against the volume (after the context lookup): origin[a] + ext[a] <= dims[a].
inline const char *mstat_origin_error(const MaskGrid &g, const uint32_t dims[3])
{
    constexpr const char *text = "origin + ext lies beyond the volume";
    uint32_t hi[3];
    for (int a = 0; a < 3; ++a) {
        if ((uint64_t)g.origin[a] + g.ext[a] > 0xFFFFFFFFull) return text;
        hi[a] = g.origin[a] + g.ext[a];
    }
    VoxelBox b;  // the shared rule: the grid is the request box [origin, origin + ext)
    return box_resolve(1, g.origin, hi, dims, &b) == kBoxOk ? nullptr : text;
}

// vr_mask_stats*: kMaskOk with *g resolved, or kMaskEinval (*g untouched).  have_hist: the request
// is not NULL, and then (use_box, lo, hi, nbins) are its fields.
inline int mstat_check_stats(const uint32_t *ext, const uint32_t *origin, const void *mask, uint32_t elem_bytes,
                             bool have_hist, uint32_t use_box, float lo, float hi, uint32_t nbins, const void *bins,
                             const void *hinfo, const void *region, bool device, MaskGrid *g, const char **msg)
{
    *msg = nullptr;
    if (!ext || !origin || !mask || !region) return mask_refuse(msg, "NULL argument", kMaskEinval);
    if (have_hist ? (!bins || !hinfo) : (bins || hinfo))
        return mask_refuse(msg, "bins and hinfo are NULL exactly when the histogram request is", kMaskEinval);
    MaskGrid r;
    if (int rc = mstat_check_grid(ext, origin, mask, elem_bytes, device, &r, msg)) return rc;
    if (have_hist) {
        if (use_box != 0) return mask_refuse(msg, "a mask histogram takes no box: use_box must be 0", kMaskEinval);
        if (!hist_range_ok(lo, hi, nbins))
            return mask_refuse(msg, "histogram needs finite lo < hi and 1 <= nbins <= 4096", kMaskEinval);
    }
    *g = r;
    return kMaskOk;
}

// vr_label_stats*: kMaskOk, kMaskEinval (*g untouched), or kMaskEnospc for rcap below ntable with
// *g resolved (the caller reports g->voxels).  A full-size call writes ntable records.
inline int mstat_check_labels(const uint32_t *ext, const uint32_t *origin, const void *labels, const void *table,
                              uint64_t ntable, const void *regions, uint64_t rcap, const void *info, bool device,
                              MaskGrid *g, const char **msg)
{
    *msg = nullptr;
    if (!ext || !origin || !labels || !table || !regions || !info) return mask_refuse(msg, "NULL argument", kMaskEinval);
    MaskGrid r;
    if (int rc = mstat_check_grid(ext, origin, labels, 4, device, &r, msg)) return rc;
    if (ntable > kMstatMaxTable) return mask_refuse(msg, "the table holds more than 2^32 - 1 records", kMaskEinval);
    if (mask_check_output(labels, r.voxels * 4, regions, kMstatRecordBytes, rcap, ntable) == kMaskOverlap)
        return mask_refuse(msg, "the region buffer overlaps the labels", kMaskEinval);
    const MaskReason o = mask_check_output(table, ntable * kMstatRecordBytes, regions, kMstatRecordBytes, rcap, ntable);
    if (o == kMaskOverlap) return mask_refuse(msg, "the region buffer overlaps the table", kMaskEinval);
    return mask_resolved(r, o, "the region buffer is smaller than the table (see the info's regions)", g, msg);
}

// vr_mask_window*: the same for the byte output and the window (vr_label.h's); mask may be NULL.
inline int mstat_check_window(const uint32_t *ext, const uint32_t *origin, const void *mask, uint32_t elem_bytes,
                              float lo, float hi, const void *out, uint64_t mcap, const void *info, bool device,
                              MaskGrid *g, const char **msg)
{
    *msg = nullptr;
    if (!ext || !origin || !out || !info) return mask_refuse(msg, "NULL argument", kMaskEinval);
    MaskGrid r;
    if (int rc = mstat_check_grid(ext, origin, mask, elem_bytes, device, &r, msg)) return rc;
    if (std::isnan(lo) || std::isnan(hi)) return mask_refuse(msg, "window bounds must not be NaN", kMaskEinval);
    if (lo > hi) return mask_refuse(msg, "window needs lo <= hi", kMaskEinval);
    const MaskReason o = mask_check_output(mask, r.voxels * elem_bytes, out, 1, mcap, r.voxels);
    if (o == kMaskOverlap) return mask_refuse(msg, "the output overlaps the mask", kMaskEinval);
    return mask_resolved(r, o, "the output buffer is smaller than the grid (see the info's voxels)", g, msg);
}

// ---- the launch geometry and the scratch of one call (vr_mstat_kernels.hip) ----
// The voxel passes walk tiles of kMstatTileX x kMstatTileY voxels of one z, a workgroup a tile and a
// wave a row of it, tiles x-fastest; grids beyond kMstatMaxGrid workgroups are strided.  The record
// passes (gather, finalize) give a thread a record.  The scratch: the counters, the histogram's
// counts and edges, then per record its accumulators, its 64-byte record and its compacted label.
struct MstatGeom {
    uint32_t tiles_x, tiles_y;
    uint64_t tiles;       // tiles_x * tiles_y * bz: at most the voxel count
    uint32_t grid;        // workgroups of a voxel pass
    uint32_t rec_grid;    // workgroups of a record pass (256 records each a round)
    size_t cnt, bins, edges, acc, rec, lab, bytes;  // offsets into the scratch block and its size
};

inline MstatGeom mstat_geometry(const MaskGrid &g, uint64_t nrec)
{
    MstatGeom G;
    G.tiles_x = (g.ext[0] + kMstatTileX - 1) / kMstatTileX;
    G.tiles_y = (g.ext[1] + kMstatTileY - 1) / kMstatTileY;
    G.tiles = (uint64_t)G.tiles_x * G.tiles_y * g.ext[2];
    G.grid = (uint32_t)(G.tiles < kMstatMaxGrid ? G.tiles : kMstatMaxGrid);
    const uint64_t per = (nrec + 255) / 256;
    G.rec_grid = (uint32_t)(per < 1 ? 1 : (per < kMstatMaxGrid ? per : kMstatMaxGrid));
    G.cnt = 0;
    G.bins = G.cnt + kMstatCounters * 8;
    G.edges = G.bins + (size_t)kHistMaxBins * 8;
    G.acc = G.edges + (size_t)kHistMaxBins * 4;
    G.rec = G.acc + (size_t)nrec * kMstatAccBytes;
    G.lab = G.rec + (size_t)nrec * kMstatRecordBytes;
    G.bytes = G.lab + (size_t)nrec * 4;
    return G;
}

}  // namespace vr
