// vr_mmesh_host.h — the host side of include/vr/vr_mmesh.h: what a request is refused for (the grid
// rule is vr_mask_host.h's; the texts and the request's own fields are here) and the node, cell,
// word and scratch geometry, which the kernels share.  Plain C++ without HIP, so a stand-alone
// program can run it (under a sanitizer, tests/test_mmesh_cpu.py); vr_api_mmesh.hip includes it for
// the entry points, vr_mmesh_kernels.hip for the geometry.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "vr_mask_host.h"

#if defined(__HIPCC__)
#define VR_MMESH_HD __host__ __device__
#else
#define VR_MMESH_HD
#endif

namespace vr {

constexpr uint32_t kMmeshMaxIters = 64;            // VR_MMESH_MAX_ITERS
constexpr uint32_t kMmeshAny = 0, kMmeshLabel = 1;  // vr_mview_select
constexpr uint32_t kMmeshVertexBytes = 24;         // sizeof(vr_mesh_vertex)
constexpr uint32_t kMmeshTriBytes = 12;            // three uint32_t
constexpr uint64_t kMmeshMaxVertices = 0xFFFFFFFFull;
constexpr uint32_t kMmeshWord = 64;                // nodes, and cells, of one x row in a word: a wave's lanes
constexpr uint32_t kMmeshBlock = 256;              // threads of every workgroup: four waves
constexpr uint32_t kMmeshWaves = kMmeshBlock / 64;
constexpr uint32_t kMmeshMaxGroups = 1024;         // workgroups a launch has at most; the loops stride
constexpr uint32_t kMmeshScanTile = kMmeshBlock;   // cell words one step of a scan workgroup covers
constexpr uint32_t kMmeshSpanTiles = 4;            // a scan workgroup's span is a multiple of this many tiles

// vr_mmesh_request, field for field (vr_api_mmesh.hip asserts the layout).
struct MmeshRequest {
    uint32_t ext[3], origin[3];
    uint32_t elem_bytes, select, label, closed, normals, smooth_iters;
    float relax;
    uint32_t reserved;
    const void *array;
};

// ---- the geometry ----
// Nodes: the grid's voxels and, closed, one ring around them: nn[a] = ext[a] + 2 ring.  Cells:
// nc[a] = nn[a] - 1 (0 on an axis: no cell at all).  A node row (all x of one y, z) is packed into
// nw = ceil(nn[0] / 64) words of 64 bits, bit x & 63 of word x >> 6; a cell row into
// cw = ceil(nc[0] / 64) words the same way.  Node word (w, y, z) has index w + nw * (y + nn[1] * z),
// cell word (w, y, z) index w + cw * (y + nc[1] * z): cell-linear word order, the order of the
// output.  The classify and scan workgroup g owns the cell words [g * span, (g + 1) * span).
struct MmeshGeom {
    uint32_t ring;
    uint32_t nn[3], nc[3];
    uint32_t nw, cw;
    uint64_t node_rows, node_words, cells, cell_words;
    uint32_t groups, span;
};

VR_MMESH_HD inline MmeshGeom mmesh_geom(const uint32_t ext[3], uint32_t closed)
{
    MmeshGeom G;
    G.ring = closed ? 1u : 0u;
    for (int a = 0; a < 3; ++a) {
        G.nn[a] = ext[a] + 2 * G.ring;
        G.nc[a] = G.nn[a] - 1;
    }
    G.nw = (G.nn[0] + kMmeshWord - 1) / kMmeshWord;
    G.cw = (G.nc[0] + kMmeshWord - 1) / kMmeshWord;
    G.node_rows = (uint64_t)G.nn[1] * G.nn[2];
    G.node_words = G.node_rows * G.nw;
    G.cells = (uint64_t)G.nc[0] * G.nc[1] * G.nc[2];
    G.cell_words = (uint64_t)G.cw * G.nc[1] * G.nc[2];
    const uint64_t unit = (uint64_t)kMmeshScanTile * kMmeshSpanTiles;
    uint64_t groups = (G.cell_words + unit - 1) / unit;
    if (groups > kMmeshMaxGroups) groups = kMmeshMaxGroups;
    if (groups < 1) groups = 1;
    G.groups = (uint32_t)groups;
    const uint64_t per = (G.cell_words + groups - 1) / groups;
    G.span = (uint32_t)(((per + unit - 1) / unit) * unit);
    if (G.span == 0) G.span = (uint32_t)unit;
    return G;
}

// The context's scratch of a call, in bytes from the start of its block, each part 8-byte aligned:
// the inside bits (8 B a node word), the active bits (8 B a cell word), the triangle prefix (8 B a
// cell word), the vertex prefix (4 B a cell word; the packed counts before the scan), the two sums
// of every workgroup and the matching counter.  Per cell of a long row: 1 bit + (8 + 8 + 4) / 64 B,
// 0.44 B; the worst case is a grid one to 62 voxels wide in x, whose every row pads to a whole word.
struct MmeshScratch {
    uint64_t bits, active, pre_t, pre_v, gsum, matching, bytes;
};

VR_MMESH_HD inline MmeshScratch mmesh_scratch(const MmeshGeom &G)
{
    MmeshScratch S;
    S.bits = 0;
    S.active = S.bits + G.node_words * 8;
    S.pre_t = S.active + G.cell_words * 8;
    S.pre_v = S.pre_t + G.cell_words * 8;
    S.gsum = S.pre_v + ((G.cell_words * 4 + 7) & ~7ull);
    S.matching = S.gsum + (uint64_t)kMmeshMaxGroups * 16;
    S.bytes = S.matching + 8;
    return S;
}

// The two `local` arrays of the smoothing sweeps: 12 B a vertex each, the second 8-byte aligned.
VR_MMESH_HD inline uint64_t mmesh_local_stride(uint64_t vertices) { return (vertices * 12 + 7) & ~7ull; }

// The most records a call can write: a vertex per cell, three edges of two triangles per cell.
VR_MMESH_HD inline uint64_t mmesh_max_vertices(const MmeshGeom &G) { return G.cells; }
VR_MMESH_HD inline uint64_t mmesh_max_triangles(const MmeshGeom &G) { return G.cells * 6; }

// ---- the texts ----
constexpr const char *kMmeshTexts[kMaskAlign + 1] = {
    nullptr, "mask mesh: grid extent must lie in [1, 32768]", "mask mesh: grid holds more than 2^32 - 1 voxels",
    "mask mesh: elem_bytes must be 1 or 4", "mask mesh: a 4-byte array must be 4-byte aligned"};
constexpr const char *kMmeshNull = "mask mesh: NULL argument";
constexpr const char *kMmeshSelect = "mask mesh: select must be VR_MVIEW_ANY or VR_MVIEW_LABEL";
constexpr const char *kMmeshLabelZero = "mask mesh: VR_MVIEW_LABEL needs a non-zero label";
constexpr const char *kMmeshClosed = "mask mesh: closed must be 0 or 1";
constexpr const char *kMmeshNormals = "mask mesh: normals must be 0 or 1";
constexpr const char *kMmeshIters = "mask mesh: smooth_iters must be at most 64";
constexpr const char *kMmeshRelax = "mask mesh: relax must be finite and in [0, 1]";
constexpr const char *kMmeshReserved = "mask mesh: reserved must be 0";
constexpr const char *kMmeshOutAlign = "mask mesh: an output must be 4-byte aligned";
constexpr const char *kMmeshOverArray = "mask mesh: an output overlaps the array";
constexpr const char *kMmeshOverOutput = "mask mesh: the outputs overlap each other";
constexpr const char *kMmeshOverInfo = "mask mesh: an output overlaps the info";
constexpr const char *kMmeshOrigin = "mask mesh: origin + ext lies beyond the volume";
constexpr const char *kMmeshNoVolume = "mask mesh: no volume";
constexpr const char *kMmeshTooMany = "mask mesh: more than 2^32 - 1 vertices";
constexpr const char *kMmeshShort = "mask mesh: a buffer is smaller than the mesh (see the info's counts)";

// ---- the request ----
// What the four calls share.  device: the array lives in device memory (its alignment binds).
// kMaskOk with *g resolved, or kMaskEinval with *g untouched.
inline int mmesh_check_request(const MmeshRequest *q, const void *info, bool device, MaskGrid *g, const char **msg)
{
    *msg = nullptr;
    if (!q || !q->array || !info) return mask_refuse(msg, kMmeshNull, kMaskEinval);
    MaskGrid r;
    if (MaskReason why = mask_grid_resolve(q->ext, &r)) return mask_refuse(msg, kMmeshTexts[why], kMaskEinval);
    for (int a = 0; a < 3; ++a) r.origin[a] = q->origin[a];
    if (MaskReason why = mask_check_array(q->array, q->elem_bytes, device))
        return mask_refuse(msg, kMmeshTexts[why], kMaskEinval);
    if (q->select != kMmeshAny && q->select != kMmeshLabel) return mask_refuse(msg, kMmeshSelect, kMaskEinval);
    if (q->select == kMmeshLabel && q->label == 0) return mask_refuse(msg, kMmeshLabelZero, kMaskEinval);
    if (q->closed > 1) return mask_refuse(msg, kMmeshClosed, kMaskEinval);
    if (q->normals > 1) return mask_refuse(msg, kMmeshNormals, kMaskEinval);
    if (q->smooth_iters > kMmeshMaxIters) return mask_refuse(msg, kMmeshIters, kMaskEinval);
    if (!std::isfinite(q->relax) || !(q->relax >= 0.0f) || q->relax > 1.0f) return mask_refuse(msg, kMmeshRelax, kMaskEinval);
    if (q->reserved != 0) return mask_refuse(msg, kMmeshReserved, kMaskEinval);
    *g = r;
    return kMaskOk;
}

// An extraction: the request, then its two outputs.  The counts are not known before the count
// pass, so an output stands for what it could hold at most: min(cap, the grid's most) records.
inline int mmesh_check_extract(const MmeshRequest *q, const void *verts, uint64_t vcap, const void *tris, uint64_t tcap,
                               const void *info, uint64_t info_bytes, bool device, MaskGrid *g, const char **msg)
{
    *msg = nullptr;
    if (!q || !q->array || !verts || !tris || !info) return mask_refuse(msg, kMmeshNull, kMaskEinval);
    MaskGrid r;
    if (int rc = mmesh_check_request(q, info, device, &r, msg)) return rc;
    if (device && (!mask_aligned4(verts) || !mask_aligned4(tris))) return mask_refuse(msg, kMmeshOutAlign, kMaskEinval);
    const MmeshGeom G = mmesh_geom(r.ext, q->closed);
    const uint64_t vmost = mmesh_max_vertices(G), tmost = mmesh_max_triangles(G);
    const uint64_t vn = vcap < vmost ? vcap : vmost, tn = tcap < tmost ? tcap : tmost;
    const uint64_t in_bytes = r.voxels * q->elem_bytes;
    if (mask_check_output(q->array, in_bytes, verts, kMmeshVertexBytes, vcap, vmost) == kMaskOverlap ||
        mask_check_output(q->array, in_bytes, tris, kMmeshTriBytes, tcap, tmost) == kMaskOverlap)
        return mask_refuse(msg, kMmeshOverArray, kMaskEinval);
    if (vn && tn && mask_overlap(verts, vn * kMmeshVertexBytes, tris, tn * kMmeshTriBytes))
        return mask_refuse(msg, kMmeshOverOutput, kMaskEinval);
    if (!device && (mask_check_output(info, info_bytes, verts, kMmeshVertexBytes, vcap, vmost) == kMaskOverlap ||
                    mask_check_output(info, info_bytes, tris, kMmeshTriBytes, tcap, tmost) == kMaskOverlap))
        return mask_refuse(msg, kMmeshOverInfo, kMaskEinval);
    *g = r;
    return kMaskOk;
}

// The grid against the volume (after the context lookup): origin[a] + ext[a] <= dims[a].
inline const char *mmesh_origin_error(const MaskGrid &g, const uint32_t dims[3])
{
    for (int a = 0; a < 3; ++a)
        if ((uint64_t)g.origin[a] + g.ext[a] > (uint64_t)dims[a]) return kMmeshOrigin;
    return nullptr;
}

// After the count pass: kMaskEinval for more vertices than an index holds, kMaskEnospc for a
// capacity below its count, kMaskOk.
inline int mmesh_check_counts(uint64_t vertices, uint64_t triangles, bool extract, uint64_t vcap, uint64_t tcap,
                              const char **msg)
{
    *msg = nullptr;
    if (vertices > kMmeshMaxVertices) return mask_refuse(msg, kMmeshTooMany, kMaskEinval);
    if (extract && (vcap < vertices || tcap < triangles)) return mask_refuse(msg, kMmeshShort, kMaskEnospc);
    return kMaskOk;
}

}  // namespace vr
