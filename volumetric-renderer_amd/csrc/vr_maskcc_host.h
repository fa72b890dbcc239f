// vr_maskcc_host.h — the host side of include/vr/vr_maskcc.h: what a labelling or selection request
// is refused for, the grid it resolves to, and the launch geometry and scratch layout of its passes.
// Plain C++ without HIP, so a stand-alone program can run it (under a sanitizer, tests/
// test_maskcc_cpu.py); vr_api_maskcc.hip includes it for vr_mask_label* and vr_mask_select*,
// vr_maskcc_kernels.hip for the geometry.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace vr {

constexpr uint32_t kMccMaxExtent = 32768u;         // VR_MASKCC_MAX_EXTENT
constexpr uint64_t kMccMaxVoxels = 0xFFFFFFFFull;  // a label is 1 + a box-linear index, in 32 bits
constexpr int kMccOk = 0, kMccEinval = -22, kMccEnospc = -28;  // VR_OK, VR_EINVAL, VR_ENOSPC
constexpr uint32_t kMccRules = 4;                  // enum vr_mask_rule
constexpr uint32_t kMccKeepLargest = 0, kMccKeepMinVoxels = 1, kMccKeepSeed = 2, kMccFillHoles = 3;
constexpr uint32_t kMccRecordBytes = 64;           // sizeof(vr_label_component)
constexpr uint32_t kMccChunk = 8192;               // voxels a flatten workgroup walks: 128 ballot words
constexpr uint32_t kMccChunkWords = kMccChunk / 64u;
constexpr uint32_t kMccRowWaves = 4;               // rows a workgroup walks at a time, a wave each
constexpr uint32_t kMccMaxGrid = 8192;             // workgroups of a launch: the rest is strided
constexpr uint32_t kMccCounters = 8;               // 64-bit words (vr_maskcc_kernels.h MccArgs::cnt)

struct MccGrid {
    uint32_t ext[3];
    uint64_t voxels;
};

// The grid of ext into *g; nullptr, or what is wrong (*g is then untouched).  vr_morph.h's rule.
inline const char *mcc_grid_resolve(const uint32_t ext[3], MccGrid *g)
{
    uint64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        if (ext[a] < 1 || ext[a] > kMccMaxExtent) return "mask extent must lie in [1, 32768]";
        n *= ext[a];  // (at most 2^45)
    }
    if (n > kMccMaxVoxels) return "mask grid holds more than 2^32 - 1 voxels";
    for (int a = 0; a < 3; ++a) g->ext[a] = ext[a];
    g->voxels = n;
    return nullptr;
}

// [a, a + na) and [b, b + nb) share a byte.
inline bool mcc_overlap(const void *a, uint64_t na, const void *b, uint64_t nb)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb ? pb - pa < na : pa - pb < nb;
}

inline bool mcc_aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// A refusal: its text into *msg, its code returned.
inline int mcc_refuse(const char **msg, const char *text, int code)
{
    *msg = text;
    return code;
}

// What both calls share but the capacity: the grid, the element width, the connectivity and the
// mask's alignment (device memory only: a host array is copied byte by byte).  kMccOk with *r
// resolved, or kMccEinval.
inline int mcc_check_mask(const uint32_t *ext, const void *mask, uint32_t elem_bytes, uint32_t connectivity,
                          bool device, MccGrid *r, const char **msg)
{
    if (const char *m = mcc_grid_resolve(ext, r)) return mcc_refuse(msg, m, kMccEinval);
    if (elem_bytes != 1 && elem_bytes != 4) return mcc_refuse(msg, "mask elem_bytes must be 1 or 4", kMccEinval);
    if (connectivity != 6 && connectivity != 26) return mcc_refuse(msg, "mask connectivity must be 6 or 26", kMccEinval);
    if (device && elem_bytes == 4 && !mcc_aligned4(mask))
        return mcc_refuse(msg, "a 4-byte mask must be 4-byte aligned", kMccEinval);
    return kMccOk;
}

// vr_mask_label*: kMccOk with *g resolved; kMccEinval (*g untouched); or kMccEnospc for lcap below
// the voxel count, with *g resolved (the caller reports g->voxels).  *msg names a refusal.  The
// overlap is that of what a full-size call would touch: min(cap, voxels) elements of an output (a
// grid has at most as many components as voxels).
inline int mcc_check_label(const uint32_t *ext, const void *mask, uint32_t elem_bytes, uint32_t connectivity,
                           const void *labels, uint64_t lcap, const void *comps, uint64_t ccap, const void *info,
                           bool device, MccGrid *g, const char **msg)
{
    *msg = nullptr;
    if (!ext || !mask || !labels || !comps || !info) return mcc_refuse(msg, "NULL argument", kMccEinval);
    MccGrid r;
    if (int rc = mcc_check_mask(ext, mask, elem_bytes, connectivity, device, &r, msg)) return rc;
    if (device && !mcc_aligned4(labels)) return mcc_refuse(msg, "labels_dev must be 4-byte aligned", kMccEinval);
    const uint64_t ln = lcap < r.voxels ? lcap : r.voxels, cn = ccap < r.voxels ? ccap : r.voxels;
    if (ln && mcc_overlap(mask, r.voxels * elem_bytes, labels, ln * 4))
        return mcc_refuse(msg, "the label buffer overlaps the mask", kMccEinval);
    if (cn && mcc_overlap(mask, r.voxels * elem_bytes, comps, cn * kMccRecordBytes))
        return mcc_refuse(msg, "the record buffer overlaps the mask", kMccEinval);
    *g = r;
    if (lcap < r.voxels)
        return mcc_refuse(msg, "the label buffer is smaller than the grid (see the info's voxels)", kMccEnospc);
    return kMccOk;
}

// vr_mask_select*: the same for the byte output and the request's fields (req_seed: 3 words).
inline int mcc_check_select(const uint32_t *ext, bool have_req, uint32_t rule, uint32_t connectivity,
                            const uint32_t *req_seed, const void *mask, uint32_t elem_bytes, const void *out,
                            uint64_t mcap, const void *info, bool device, MccGrid *g, const char **msg)
{
    *msg = nullptr;
    if (!ext || !have_req || !mask || !out || !info) return mcc_refuse(msg, "NULL argument", kMccEinval);
    MccGrid r;
    if (int rc = mcc_check_mask(ext, mask, elem_bytes, connectivity, device, &r, msg)) return rc;
    if (rule >= kMccRules) return mcc_refuse(msg, "mask rule must be one of enum vr_mask_rule", kMccEinval);
    if (rule == kMccKeepSeed)
        for (int a = 0; a < 3; ++a)
            if (req_seed[a] >= r.ext[a]) return mcc_refuse(msg, "seed lies outside the grid", kMccEinval);
    const uint64_t on = mcap < r.voxels ? mcap : r.voxels;
    if (on && mcc_overlap(mask, r.voxels * elem_bytes, out, on))
        return mcc_refuse(msg, "the output overlaps the mask", kMccEinval);
    *g = r;
    if (mcap < r.voxels)
        return mcc_refuse(msg, "the output buffer is smaller than the grid (see the info's voxels)", kMccEnospc);
    return kMccOk;
}

// Box-linear index of grid voxel v.
inline uint32_t mcc_linear(const MccGrid &g, const uint32_t v[3])
{
    return v[0] + g.ext[0] * (v[1] + g.ext[1] * v[2]);  // below 2^32 - 1 (mcc_grid_resolve)
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

inline MccGeom mcc_geometry(const MccGrid &g)
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
