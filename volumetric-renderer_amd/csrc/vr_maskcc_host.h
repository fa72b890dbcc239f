// vr_maskcc_host.h — the host side of include/vr/vr_maskcc.h: what a labelling or selection request
// is refused for (the grid rule is vr_mask_host.h's, the texts and the request's own fields are
// here), and the launch geometry and scratch layout of its passes.
// Plain C++ without HIP, so a stand-alone program can run it (under a sanitizer, tests/
// test_maskcc_cpu.py); vr_api_maskcc.hip includes it for vr_mask_label* and vr_mask_select*,
// vr_maskcc_kernels.hip for the geometry.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "vr_mask_host.h"

namespace vr {

constexpr uint32_t kMccRules = 4;                  // enum vr_mask_rule
constexpr uint32_t kMccKeepLargest = 0, kMccKeepMinVoxels = 1, kMccKeepSeed = 2, kMccFillHoles = 3;
constexpr uint32_t kMccRecordBytes = 64;           // sizeof(vr_label_component)
constexpr uint32_t kMccChunk = 8192;               // voxels a flatten workgroup walks: 128 ballot words
constexpr uint32_t kMccChunkWords = kMccChunk / 64u;
constexpr uint32_t kMccRowWaves = 4;               // rows a workgroup walks at a time, a wave each
constexpr uint32_t kMccMaxGrid = 8192;             // workgroups of a launch: the rest is strided
constexpr uint32_t kMccCounters = 8;               // 64-bit words (vr_maskcc_kernels.h MccArgs::cnt)

// The family's texts for the shared rule (vr_mask_host.h MaskReason; the outputs' are below).
constexpr const char *kMccTexts[kMaskAlign + 1] = {
    nullptr, "mask extent must lie in [1, 32768]", "mask grid holds more than 2^32 - 1 voxels",
    "mask elem_bytes must be 1 or 4", "a 4-byte mask must be 4-byte aligned"};

// What both calls share but the capacity: the grid, the element width, the connectivity and the
// mask's alignment, in this order.  kMaskOk with *r resolved, or kMaskEinval.
inline int mcc_check_mask(const uint32_t *ext, const void *mask, uint32_t elem_bytes, uint32_t connectivity,
                          bool device, MaskGrid *r, const char **msg)
{
    if (MaskReason why = mask_grid_resolve(ext, r)) return mask_refuse(msg, kMccTexts[why], kMaskEinval);
    const MaskReason why = mask_check_array(mask, elem_bytes, device);
    if (why == kMaskElemBytes) return mask_refuse(msg, kMccTexts[why], kMaskEinval);
    if (connectivity != 6 && connectivity != 26) return mask_refuse(msg, "mask connectivity must be 6 or 26", kMaskEinval);
    return why ? mask_refuse(msg, kMccTexts[why], kMaskEinval) : kMaskOk;
}

// vr_mask_label*: kMaskOk with *g resolved; kMaskEinval (*g untouched); or kMaskEnospc for lcap below
// the voxel count, with *g resolved (the caller reports g->voxels).  *msg names a refusal.  A grid
// has at most as many components as voxels; ccap is held against the count the call finds.
inline int mcc_check_label(const uint32_t *ext, const void *mask, uint32_t elem_bytes, uint32_t connectivity,
                           const void *labels, uint64_t lcap, const void *comps, uint64_t ccap, const void *info,
                           bool device, MaskGrid *g, const char **msg)
{
    *msg = nullptr;
    if (!ext || !mask || !labels || !comps || !info) return mask_refuse(msg, "NULL argument", kMaskEinval);
    MaskGrid r;
    if (int rc = mcc_check_mask(ext, mask, elem_bytes, connectivity, device, &r, msg)) return rc;
    if (device && !mask_aligned4(labels)) return mask_refuse(msg, "labels_dev must be 4-byte aligned", kMaskEinval);
    const MaskReason lo = mask_check_output(mask, r.voxels * elem_bytes, labels, 4, lcap, r.voxels);
    if (lo == kMaskOverlap) return mask_refuse(msg, "the label buffer overlaps the mask", kMaskEinval);
    if (mask_check_output(mask, r.voxels * elem_bytes, comps, kMccRecordBytes, ccap, r.voxels) == kMaskOverlap)
        return mask_refuse(msg, "the record buffer overlaps the mask", kMaskEinval);
    return mask_resolved(r, lo, "the label buffer is smaller than the grid (see the info's voxels)", g, msg);
}

// vr_mask_select*: the same for the byte output and the request's fields (req_seed: 3 words).
inline int mcc_check_select(const uint32_t *ext, bool have_req, uint32_t rule, uint32_t connectivity,
                            const uint32_t *req_seed, const void *mask, uint32_t elem_bytes, const void *out,
                            uint64_t mcap, const void *info, bool device, MaskGrid *g, const char **msg)
{
    *msg = nullptr;
    if (!ext || !have_req || !mask || !out || !info) return mask_refuse(msg, "NULL argument", kMaskEinval);
    MaskGrid r;
    if (int rc = mcc_check_mask(ext, mask, elem_bytes, connectivity, device, &r, msg)) return rc;
    if (rule >= kMccRules) return mask_refuse(msg, "mask rule must be one of enum vr_mask_rule", kMaskEinval);
    if (rule == kMccKeepSeed)
        for (int a = 0; a < 3; ++a)
            if (req_seed[a] >= r.ext[a]) return mask_refuse(msg, "seed lies outside the grid", kMaskEinval);
    const MaskReason o = mask_check_output(mask, r.voxels * elem_bytes, out, 1, mcap, r.voxels);
    if (o == kMaskOverlap) return mask_refuse(msg, "the output overlaps the mask", kMaskEinval);
    return mask_resolved(r, o, "the output buffer is smaller than the grid (see the info's voxels)", g, msg);
}

// Box-linear index of grid voxel v.
inline uint32_t mcc_linear(const MaskGrid &g, const uint32_t v[3])
{
    return v[0] + g.ext[0] * (v[1] + g.ext[1] * v[2]);  // below 2^32 - 1 (mask_grid_resolve)
}

// ---- the launch geometry and the scratch of one call (vr_maskcc_kernels.hip) ----
// The row passes (rows, links, records) give a wave a row, kMccRowWaves rows a workgroup; the
// flatten pass gives a workgroup a chunk of kMccChunk voxels; the selection sweep gives a thread a
// voxel.  Grids beyond kMccMaxGrid workgroups are strided, but the flatten pass, whose workgroup
// is its chunk (at most 2^32 / 8192 of them).  The root table: a bit per voxel in 64-bit words,
// the count of the chunk's roots before each word, the roots before each chunk; then the counters.
struct MccGeom {
    uint64_t rows;         // by * bz
    uint32_t row_words;    // 64-voxel words of a row
    uint32_t row_grid;     // workgroups of a row pass
    uint32_t nwords;       // 64-bit words of the root table
    uint32_t nchunks;      // flatten workgroups
    uint32_t sweep_grid;   // workgroups of the selection sweep (256 threads, a voxel each a round)
    size_t bits, wpre, chunk, cnt, bytes;  // offsets into the scratch block and its size
};

inline MccGeom mcc_geometry(const MaskGrid &g)
{
    MccGeom G;
    G.rows = (uint64_t)g.ext[1] * g.ext[2];
    G.row_words = (g.ext[0] + 63u) / 64u;
    const uint64_t groups = (G.rows + kMccRowWaves - 1) / kMccRowWaves;
    G.row_grid = (uint32_t)(groups < kMccMaxGrid ? groups : kMccMaxGrid);
    G.nwords = (uint32_t)((g.voxels + 63) / 64);
    G.nchunks = (uint32_t)((g.voxels + kMccChunk - 1) / kMccChunk);
    const uint64_t sweep = (g.voxels + 255) / 256;
    G.sweep_grid = (uint32_t)(sweep < kMccMaxGrid ? sweep : kMccMaxGrid);
    G.bits = 0;
    G.wpre = G.bits + (size_t)G.nwords * 8;
    G.chunk = G.wpre + (size_t)G.nwords * 4;
    G.cnt = (G.chunk + (size_t)G.nchunks * 4 + 7) & ~(size_t)7;
    G.bytes = G.cnt + kMccCounters * 8;
    return G;
}

}  // namespace vr
