/*
 * vr_mmesh.h — the surface of a device mask, or of one label of a label array, as an indexed
 * triangle mesh (an addition beside vr.h and the other family headers; VR_ABI_VERSION, vr_params
 * and vr_stats are unchanged).  The entry points live in lib/libvr_amd_mmesh.so, a sixth library
 * beside libvr_amd.so, libvr_amd_morph.so, libvr_amd_maskcc.so, libvr_amd_mstat.so and
 * libvr_amd_mview.so on the same context: link it with libvr_amd.so.
 *
 * vr_label.h grows a region from a click, vr_morph.h and vr_maskcc.h clean it up, vr_mstat.h
 * measures it, vr_mview.h shows it; every one of those calls ends in a mask or a label array in
 * device memory.  These calls take the surface of that array out as geometry without a read-back:
 * to save for a printer or a mesh tool (vr_host.h vr_mesh_write_ply takes the result unchanged), to
 * draw with the host's rasteriser, to measure by area.  vr_mesh.h meshes a threshold of the
 * resident volume; this meshes an array the caller holds.  A voxel mask's surface is a staircase,
 * so the calls also relax it: each vertex moves toward its neighbours while it stays in its cell.
 *
 * Request.  ext, origin, elem_bytes and array are vr_mstat.h's grid: ext[3] = (bx, by, bz) voxels,
 * every extent in [1, 32768], at most 2^32 - 1 voxels, box-linear order l = i + bx * (j + by * k);
 * origin[3] is the VOLUME voxel of grid voxel (0, 0, 0), origin[a] + ext[a] <= dims[a];
 * elem_bytes is 1 or 4, and a 4-byte array in device memory must be 4-byte aligned (a byte mask
 * may have any address).  select and label are vr_mview.h's rule: an element MATCHES iff it is
 * non-zero (VR_MVIEW_ANY; label is ignored) or iff it equals `label` (VR_MVIEW_LABEL; label
 * non-zero).  closed, normals: 0 or 1.  smooth_iters: 0 .. VR_MMESH_MAX_ITERS.  relax: finite, in
 * [0, 1].  reserved: 0.
 *
 * All arithmetic is f32, no contraction, every division and square root correctly rounded: each
 * operation written below is one IEEE operation, in the written order.
 *
 * Nodes.  Node (i, j, k) of the grid is grid voxel (i, j, k); it is INSIDE iff its element
 * matches.  closed = 1 adds one ring of nodes that are never inside on every side of the grid; the
 * ring is never read from memory.  The cell set, the corner index dx + 2 dy + 4 dz, "active", and
 * the quads with their four cells C0 .. C3 and their winding are vr_mesh.h's, word for word, over
 * these nodes: per axis a the cells are c[a] in [0, ext[a] - 2] open and [-1, ext[a] - 1] closed,
 * in grid coordinates.
 *
 * Vertex.  Each active cell of the cell set gives one vertex.  local is vr_mesh.h's vertex
 * arithmetic with the node values 1.0f (inside) and 0.0f (outside) and iso = 0.5f: every crossing
 * edge has t = 0.5f exactly, s is a sum of multiples of 0.5f, and local = s / (float)n lies
 * strictly inside (0, 1).
 *
 * Smoothing.  smooth_iters Jacobi sweeps: every vertex of a sweep reads the previous sweep's local.
 * For the vertex of cell c, with local and relax:
 *
 *     q = (0, 0, 0); cnt = 0
 *     for o in (-1,0,0) (+1,0,0) (0,-1,0) (0,+1,0) (0,0,-1) (0,0,+1), in this order:
 *         the neighbour c + o COUNTS iff it is in the cell set and the four nodes of the face the
 *         two cells share are not all alike (both cells are then active)
 *         if it counts: t[a] = local_n[a] + (float)o[a];  q[a] = q[a] + t[a];  cnt = cnt + 1
 *     if cnt > 0, for a = 0, 1, 2:
 *         m = q[a] / (float)cnt;  v = local[a] + relax * (m - local[a])
 *         if !(v >= 0) v = 0;  if (v > 1) v = 1;  local'[a] = v
 *     else local' = local
 *
 * so a vertex never leaves its cell.  Connectivity never changes: the triangles are the same for
 * every smooth_iters and relax.
 *
 * Position.  pos[a] = (((float)C[a] + 0.5f) + local[a]) / (float)dims[a], with C = origin + c as a
 * signed integer (a ring cell is origin - 1) and dims the VOLUME's: a vertex shares vr_hit.pos's
 * and vr_mesh.h's coordinates.
 *
 * Normal.  normals = 1: G[a] = sum over the cell's eight corners of (2 d_a - 1) * inside, an
 * integer in [-4, 4]; g2 = (float)(G . G); if g2 > 0: r = 1.0f / sqrtf(g2) in two IEEE roundings
 * and normal[a] = (float)(-G[a]) * r.  Otherwise, and with normals = 0, the three floats are +0.0f.
 * The normal points from the set side to the unset side; smoothing does not change it.
 *
 * Order.  Specified, unlike vr_mesh.h's.  Vertices follow their cells in cell-linear order, x
 * fastest, then y, then z, over the cell set.  Triangles follow the owner cell C2 = P in the same
 * order, then the edge axis x, y, z, two triangles each in vr_mesh.h's order.  The output is a
 * function of the request and the array alone.
 *
 * Info.  voxels: the grid's voxel count.  matching: the matching voxels of the grid (ring nodes do
 * not count).  vertices, triangles: the mesh's counts.  Capacities and counts are in records: a
 * vertex is a vr_mesh_vertex of 24 bytes, a triangle three uint32_t vertex indices.
 *
 * Forms.  The _device forms take a device array and device buffers, work on `stream` and return
 * when their outputs are complete: the host needs the counts before the emit passes.  The host
 * forms take a host array and host buffers, stage them through the context's scratch and are
 * synchronous.
 *
 * Errors.  Every refusal leaves every output untouched, VR_ENOSPC's info excepted.  VR_EINVAL for a
 * NULL argument (the stream may be NULL), an extent outside [1, 32768], more than 2^32 - 1 voxels,
 * an elem_bytes other than 1 or 4, a misaligned 4-byte array in device memory, a select other than
 * 0 or 1, VR_MVIEW_LABEL with label 0, closed or normals other than 0 or 1, smooth_iters above
 * VR_MMESH_MAX_ITERS, a relax that is not finite or outside [0, 1], reserved != 0, a device output
 * that is not 4-byte aligned, an output that overlaps the array, the other output or (host forms)
 * the info, an origin or grid beyond the volume (or no volume), and a mesh of more than 2^32 - 1
 * vertices.  VR_ENOSPC (vr_mesh.h's) for vcap or tcap below the count: unlike the other mask
 * families this is known only after the count pass, so *info then holds all four fields -- the
 * needed sizes -- and no buffer is touched.  VR_ENOMEM when the scratch cannot be allocated.
 *
 * State.  vr_mview.h's: the calls build, evict and downgrade nothing (vr_memory_report is
 * unchanged) and leave every setting alone: a frame rendered before and after them has identical
 * bytes.  Scratch lives in the context and is freed by vr_destroy.  vr_timing_* brackets each call
 * as one interval.  vr_mmesh_last_kernel_name names the family's last kernel on the context (""
 * before the first).  A multi-device context (vr_create_mask) computes on its lowest device, where
 * the buffers must live.
 */
#ifndef VR_VR_MMESH_H
#define VR_VR_MMESH_H

#include "vr.h"
#include "vr_mesh.h"  /* VR_ENOSPC, vr_mesh_vertex */
#include "vr_mview.h" /* VR_MVIEW_ANY, VR_MVIEW_LABEL */

#ifdef __cplusplus
extern "C" {
#endif

#define VR_MMESH_MAX_EXTENT 32768u
#define VR_MMESH_MAX_ITERS 64u

typedef struct vr_mmesh_request {
    uint32_t ext[3], origin[3]; /* vr_mstat.h's grid: origin + ext <= dims */
    uint32_t elem_bytes;        /* 1 or 4 */
    uint32_t select, label;     /* vr_mview.h's rule: ANY = non-zero; LABEL = equals label (non-zero) */
    uint32_t closed;            /* 1: a ring of unset nodes around the grid; 0: open, with a rim */
    uint32_t normals;           /* 0 or 1 */
    uint32_t smooth_iters;      /* 0 .. VR_MMESH_MAX_ITERS */
    float    relax;             /* finite, in [0, 1] */
    uint32_t reserved;          /* 0 */
    const void *array;          /* box-linear, l = i + bx*(j + by*k); device memory (device forms), host (host forms) */
} vr_mmesh_request;             /* 64 bytes */

typedef struct vr_mmesh_info {
    uint64_t voxels, vertices, triangles, matching;
} vr_mmesh_info; /* 32 bytes */

/* The counts alone, of a device array, on `stream`; returns when they are known. */
int vr_mask_mesh_count_device(vr_ctx *ctx, const vr_mmesh_request *req, vr_mmesh_info *info, void *stream);
/* The same of a host array. */
int vr_mask_mesh_count(vr_ctx *ctx, const vr_mmesh_request *req, vr_mmesh_info *info);
/* vcap vertex records into verts_dev, tcap triangles (3 uint32_t each) into tris_dev, on `stream`;
   returns when both buffers are complete. */
int vr_mask_mesh_extract_device(vr_ctx *ctx, const vr_mmesh_request *req, void *verts_dev, uint64_t vcap,
                                void *tris_dev, uint64_t tcap, vr_mmesh_info *info, void *stream);
/* The same from a host array into host buffers. */
int vr_mask_mesh_extract(vr_ctx *ctx, const vr_mmesh_request *req, vr_mesh_vertex *verts_host, uint64_t vcap,
                         uint32_t *tris_host, uint64_t tcap, vr_mmesh_info *info);
/* The last kernel this family launched on the context. */
const char *vr_mmesh_last_kernel_name(const vr_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_MMESH_H */
