/*
 * vr_mesh.h — the isosurface as an indexed triangle mesh, extracted on the device (an addition
 * beside vr.h, vr_modes.h, vr_iso.h, vr_mpr.h, vr_hist.h and vr_hit.h; VR_ABI_VERSION, vr_params
 * and vr_stats are unchanged).
 *
 * VR_MODE_ISO draws a surface and vr_hit.h names one point of it.  These calls hand the surface
 * itself out as geometry -- to save for a mesh tool or a printer (vr_host.h vr_mesh_write_ply), to
 * draw with the host's rasteriser beside the volume, to measure by enclosed volume and area -- and
 * count the voxels at or above the threshold on the way.  Nothing is read back to the host first:
 * the kernels walk the resident base bricks.
 *
 * The method: surface nets on the voxel lattice.  One vertex per lattice cell the surface crosses,
 * one quad (two triangles) per lattice edge it crosses: an indexed mesh by construction, about half
 * of marching cubes' triangles, no case table.  The known limit is the one vertex per cell: thin
 * sheets and ambiguous faces give non-manifold edges (an edge shared by four triangles, never an
 * odd number in a closed mesh).
 *
 * Nodes.  Node (i, j, k) is voxel (i, j, k); its value is f = (float)stored, the value the sampler
 * uses; its position is the texel centre ((i + 0.5)/nx, (j + 0.5)/ny, (k + 0.5)/nz) in texture
 * coordinates, so a vertex and a vr_hit.pos share a coordinate system.
 * The node set N is the whole volume, or the half-open voxel box of the request (use_box,
 * box_min, box_max: vr_hist_request's convention and errors).
 * closed = 1: one ring of extra nodes surrounds N on every side, each of value +0.0f -- the
 * sampler's border value, so a surface cut by a face of the cube closes the way an ISO frame shows
 * it, and a surface cut by an interior box face is capped there.  (A ring node's value comes from
 * the box test, in N ? stored : 0.0f, never from what the bricks hold there.)
 *
 * Cells.  Cell c has the corner nodes c + (dx, dy, dz), dx, dy, dz in {0, 1}, corner index
 * dx + 2 dy + 4 dz.  The cell set is every cell whose eight corners are nodes: per axis a,
 * c[a] in [lo[a], hi[a] - 2] open and [lo[a] - 1, hi[a] - 1] closed (lo, hi: the box).
 * A node is inside iff f >= iso (a NaN is never inside, as VR_MODE_ISO's d >= iso); a cell is
 * active iff its eight corners are not all alike.
 *
 * Vertex.  Each active cell of the cell set gives one vertex.  All arithmetic is f32, no
 * contraction, every division correctly rounded:
 *
 *     edges, in this order, as corner pairs (A, B):
 *       x: (0,1) (2,3) (4,5) (6,7)   y: (0,2) (1,3) (4,6) (5,7)   z: (0,4) (1,5) (2,6) (3,7)
 *     s = (0,0,0); n = 0
 *     for each edge with inside(A) != inside(B):
 *         t = (iso - vA) / (vB - vA);  if !(t >= 0) t = 0;  if (t > 1) t = 1     (NaN -> 0)
 *         p = A's (dx,dy,dz) as floats, with the edge's own axis component replaced by t
 *         s = s + p (per component);  n = n + 1
 *     local = s / (float)n                                   per component
 *     pos[a] = (((float)c[a] + 0.5f) + local[a]) / (float)dims[a]
 *
 * Normal.  normals = 1: g is the f32 central-difference gradient at pos, vr_iso.h's g (the
 * trilinear filter of the per-voxel differences, sampled from the volume through the sampler: it
 * ignores the box and the ring).  w = g * dims, g2 = w . w; if g2 > 0: r = 1.0f / sqrtf(g2) in two
 * IEEE roundings and normal[a] = -(w[a] * r) -- outward, toward lower values.  Otherwise, and with
 * normals = 0, the three floats are +0.0f.
 *
 * Quads.  Every lattice edge P -> Q = P + e_a with both ends nodes, inside(P) != inside(Q) and all
 * four cells around it in the cell set gives two triangles.  With b = (a+1) % 3, c = (a+2) % 3 the
 * four cells are C0 = P - e_b - e_c, C1 = P - e_c, C2 = P, C3 = P - e_b (all active by
 * construction).  inside(P): (C0, C1, C2) and (C0, C2, C3); inside(Q): (C0, C2, C1) and
 * (C0, C3, C2).  An edge that lacks one of the four cells gives nothing: the open mesh's rim.
 * A closed mesh has every directed edge matched by its reverse; its signed volume is positive.
 *
 * Order.  The order of vertices and triangles is a deterministic function of the volume and the
 * request and of nothing else -- no grid size, no kernel variant; two calls write the same bytes.
 * It is otherwise unspecified (DESIGN.md 4.11 says what it is today); do not rely on it.
 *
 * Units.  Capacities (vcap, tcap) and counts are in records: a vertex is 24 bytes, a triangle
 * three uint32_t vertex indices.  inside_voxels counts the nodes of N with f >= iso (ring nodes do
 * not count): times the voxel volume, the usual segmentation volume.  iso is a field of the
 * request, in density units, as the hit kind is; the context's isovalue is not read.
 *
 * Errors: VR_EINVAL, with the outputs untouched, for a NULL argument (the stream may be NULL), a
 * non-finite iso, closed, normals or use_box other than 0 or 1, a box that is empty or beyond the
 * volume, no volume, and more than 2^32 - 1 vertices.  VR_ENOSPC for a capacity below the count:
 * *info holds the needed counts and both buffers are untouched.  VR_ENOMEM when the per-call device
 * scratch cannot be allocated.
 *
 * State.  The calls read the volume's base bricks only (every storage type and layout): they
 * build, evict and downgrade nothing (vr_memory_report is unchanged) and leave render mode,
 * isovalue, slice box, TF and window alone -- a frame rendered before and after them has identical
 * bytes.  The scratch lives in the context and is freed by vr_destroy.  vr_timing_* brackets the
 * passes: the classify pass with its scans is one timed interval, the two emit passes of an
 * extraction another.  vr_debug_last_kernel_name names the classify kernel.  A
 * multi-device context (vr_create_mask) computes on its lowest device.
 * vr_mesh_count and vr_mesh_extract are synchronous.  vr_mesh_extract_device works on `stream`
 * and returns when the buffers are complete: the host needs the counts before the emit passes, as
 * vr_set_volume_device returns after its kernel.
 */
#ifndef VR_VR_MESH_H
#define VR_VR_MESH_H

#include "vr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VR_ENOSPC (-28)

typedef struct vr_mesh_request {
    float    iso;         /* density units, finite */
    uint32_t closed;      /* 1: the ring of +0.0f nodes around N (a closed mesh); 0: open, with a rim */
    uint32_t normals;     /* 1: the normalised negative gradient per vertex; 0: +0.0f */
    uint32_t use_box;     /* 0: the whole volume; 1: the voxel box below */
    uint32_t box_min[3];  /* voxels, half open: box_min[a] < box_max[a] <= dims[a] */
    uint32_t box_max[3];
} vr_mesh_request;        /* 40 bytes */

typedef struct vr_mesh_vertex {
    float pos[3];     /* texture coordinates, as vr_hit.pos */
    float normal[3];  /* unit length, outward; +0.0f where the gradient vanishes or normals = 0 */
} vr_mesh_vertex;     /* 24 bytes */

typedef struct vr_mesh_info {
    uint64_t vertices, triangles, inside_voxels, reserved;  /* reserved: 0 */
} vr_mesh_info;

/* The counts alone. */
int vr_mesh_count(vr_ctx *ctx, const vr_mesh_request *req, vr_mesh_info *info);
/* vcap vertex records into verts_host, tcap triangles (3 uint32_t each) into tris_host. */
int vr_mesh_extract(vr_ctx *ctx, const vr_mesh_request *req, vr_mesh_vertex *verts_host, uint64_t vcap,
                    uint32_t *tris_host, uint64_t tcap, vr_mesh_info *info);
/* The same into device memory, on `stream`; returns when both buffers are complete. */
int vr_mesh_extract_device(vr_ctx *ctx, const vr_mesh_request *req, void *verts_dev, uint64_t vcap,
                           void *tris_dev, uint64_t tcap, vr_mesh_info *info, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_MESH_H */
