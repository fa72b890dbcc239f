/*
 * vr_label.h — connected-component labelling of a value window and seeded region growing, on the
 * device (an addition beside vr.h, vr_modes.h, vr_iso.h, vr_mpr.h, vr_hist.h, vr_hit.h and
 * vr_mesh.h; VR_ABI_VERSION, vr_params and vr_stats are unchanged).
 *
 * vr_hit.h names the point a caller clicked and vr_mesh.h hands out the surface at its value.
 * These calls answer which voxels belong to the thing that was clicked: the components of a value
 * window (keep the largest, drop the islands) and the component under a seed.  Nothing is read
 * back to the host first: the kernels walk the resident base bricks.
 *
 * Nodes.  N is the whole volume, or the half-open voxel box of the request (use_box, box_min,
 * box_max: vr_hist_request's convention and errors).  A voxel's value is f = (float)stored, the
 * value the sampler uses.
 *
 * In.  A voxel is in iff lo <= f && f <= hi, compared in f32.  A NaN is never in; -0.0 compares as
 * 0; lo and hi may be infinite, so [iso, +inf] is vr_mesh.h's `inside`.  NaN bounds and lo > hi
 * are errors.
 *
 * Connectivity.  6: two in-voxels of N are neighbours when they differ by one step along one
 * axis.  26: when they differ by at most one along every axis and are not equal.  Only voxels of N
 * connect: a structure cut by a box face becomes whatever pieces lie inside the box, and nothing
 * outside N is read for connectivity.  A component is a class of the transitive closure.
 *
 * Box-linear index.  With bx, by, bz the box's extents (the volume's, without a box), voxel
 * (i, j, k) of N has l = (i - box_min.x) + bx * ((j - box_min.y) + by * (k - box_min.z)): for the
 * whole volume the usual x-fastest index.
 *
 * Label.  A uint32_t: 0 for a voxel that is not in, otherwise 1 + the smallest l over the voxel's
 * component.  This is a function of the volume and the request and of nothing else -- no order of
 * execution, grid size or brick layout: two calls write identical bytes, and any correct
 * implementation writes the same bytes.  Labels are delivered in box-linear order, lcap of them.
 * So that a label fits, a box of more than 2^32 - 1 voxels is VR_EINVAL: a larger volume (8192 x
 * 1024 x 1024 is 2^33 voxels) is labelled box by box.
 *
 * Components.  One record per component, sorted by ascending label.  bbox_min / bbox_max and the
 * sums are in VOLUME voxel indices whatever the box (bbox half open, like the request's box);
 * the centroid is sum / voxels per axis.  labels_dev must be 4-byte aligned (a misaligned one is
 * VR_EINVAL); comps_dev and mask_dev need no alignment.
 *
 * Info.  voxels: the count of N.  in_voxels: the voxels that are in.  components: the records.
 * largest_label / largest_voxels: the component with the most voxels, ties to the smallest label;
 * 0 and 0 when there is none.
 *
 * Region growing.  seed is a volume voxel index inside N (outside N: VR_EINVAL).  The mask is one
 * byte per voxel of N in box-linear order: 1 for the voxels of the seed's component, 0 elsewhere;
 * *comp_out is that component's record.  A seed that is not in gives an all-zero mask, an all-zero
 * record and VR_OK.
 *
 * Errors.  VR_EINVAL, with the outputs untouched, for a NULL argument (the stream may be NULL),
 * NaN bounds, lo > hi, a connectivity other than 6 or 26, use_box other than 0 or 1, a box that is
 * empty or beyond the volume, a seed outside N, a misaligned labels_dev, and more than 2^32 - 1
 * voxels in N.  (There is no "no volume" error: a context always holds a volume, a fresh one the
 * one-voxel placeholder of value 0 it is created with, and the calls label that.)
 * VR_ENOSPC (vr_mesh.h's) in two forms.  lcap or mcap below the voxels of N is known on the host:
 * it is refused before any kernel, no buffer is touched, and info->voxels is set (the other info
 * fields 0; vr_region_grow* have no info and touch nothing).  ccap below the component count:
 * *info is complete, the component buffer is untouched and the label buffer holds the complete
 * valid labels, the expensive part.  VR_ENOMEM when the device scratch cannot be allocated.
 *
 * State.  The calls read the volume's base bricks only (every storage type and layout): they
 * build, evict and downgrade nothing (vr_memory_report is unchanged) and leave render mode,
 * isovalue, slice box, TF and window alone -- a frame rendered before and after them has identical
 * bytes.  Scratch lives in the context and is freed by vr_destroy: vr_label_count and
 * vr_region_grow* keep their labels there, 4 bytes per voxel of N (the device call labels straight
 * into the caller's buffer); every call keeps 3/16 byte per voxel of N for the root table and 64
 * bytes per component.  vr_timing_* brackets the passes: the labelling passes (local, seam,
 * flatten, scan) are one timed interval, the component table another, the mask pass of a region
 * grow a third (vr_debug.h vr_debug_label_pass_ms splits them kernel by kernel).  vr_debug_last_kernel_name names the kernel that reads the bricks,
 * label_local_kernel<VT, CONN>.  A multi-device context (vr_create_mask) computes on its lowest
 * device.  vr_label_count, vr_label_components and vr_region_grow are synchronous.  The device
 * forms work on `stream` and return when their buffers are complete: the host needs the component
 * count before it sizes the table, as vr_mesh_extract_device needs its counts.
 */
#ifndef VR_VR_LABEL_H
#define VR_VR_LABEL_H

#include "vr.h"
#include "vr_mesh.h" /* VR_ENOSPC */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vr_label_request {
    float    lo, hi;        /* the window, density units: in iff lo <= f && f <= hi */
    uint32_t connectivity;  /* 6 or 26 */
    uint32_t use_box;       /* 0: the whole volume; 1: the voxel box below */
    uint32_t box_min[3];    /* voxels, half open: box_min[a] < box_max[a] <= dims[a] */
    uint32_t box_max[3];
} vr_label_request;         /* 40 bytes */

typedef struct vr_label_component {
    uint32_t label;        /* 1 + smallest box-linear index of its voxels */
    uint32_t reserved;     /* 0 */
    uint64_t voxels;
    uint32_t bbox_min[3];  /* VOLUME voxel indices, half open like the request's box */
    uint32_t bbox_max[3];
    uint64_t sum[3];       /* sums of the voxels' volume indices x, y, z: centroid = sum / voxels */
} vr_label_component;      /* 64 bytes */

typedef struct vr_label_info {
    uint64_t voxels;          /* the count of N */
    uint64_t in_voxels;
    uint64_t components;
    uint64_t largest_voxels;
    uint32_t largest_label;   /* most voxels, ties to the smallest label; 0 and 0 when none */
    uint32_t reserved;        /* 0 */
} vr_label_info;              /* 40 bytes */

/* The counts alone. */
int vr_label_count(vr_ctx *ctx, const vr_label_request *req, vr_label_info *info);
/* lcap labels into labels_host (box-linear order), ccap records into comps_host. */
int vr_label_components(vr_ctx *ctx, const vr_label_request *req, uint32_t *labels_host, uint64_t lcap,
                        vr_label_component *comps_host, uint64_t ccap, vr_label_info *info);
/* The same into device memory, on `stream`; returns when both buffers are complete. */
int vr_label_components_device(vr_ctx *ctx, const vr_label_request *req, void *labels_dev, uint64_t lcap,
                               void *comps_dev, uint64_t ccap, vr_label_info *info, void *stream);
/* The seed's component: mcap mask bytes (box-linear order) and its record. */
int vr_region_grow(vr_ctx *ctx, const vr_label_request *req, const uint32_t seed[3], uint8_t *mask_host,
                   uint64_t mcap, vr_label_component *comp_out);
/* The same with the mask in device memory, on `stream`; returns when the mask is complete. */
int vr_region_grow_device(vr_ctx *ctx, const vr_label_request *req, const uint32_t seed[3], void *mask_dev,
                          uint64_t mcap, vr_label_component *comp_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_LABEL_H */
