/*
 * vr_maskcc.h — the connected components of a device mask: canonical labels and records, a
 * selection pass (keep the largest component, the components of at least n voxels, the component
 * at a seed) and hole filling (an addition beside vr.h and the other family headers;
 * VR_ABI_VERSION, vr_params and vr_stats are unchanged).  The entry points live in
 * lib/libvr_amd_maskcc.so, a third library beside libvr_amd.so and libvr_amd_morph.so on the same
 * context: link it with libvr_amd.so.
 *
 * vr_label.h labels a value window of the volume and grows the region under a click; vr_morph.h
 * cleans that mask.  These calls look at the components of the mask afterwards: an opening cuts a
 * bridge, and the caller keeps the piece that was clicked, or the largest, or drops everything under
 * 50 voxels; a grown region has cavities, and hole filling closes exactly those without welding
 * neighbours together as a closing would.
 *
 * Grid and mask.  vr_morph.h's.  ext[3] = (bx, by, bz) voxels, every extent in [1, 32768], at most
 * 2^32 - 1 voxels, box-linear order l = i + bx * (j + by * k).  elem_bytes is 1 or 4; a voxel is
 * SET iff its element is non-zero: a label array with many labels is one set, its distinct labels
 * are not told apart.  A 4-byte mask and every uint32_t output in device memory must be 4-byte
 * aligned; a 1-byte mask and the byte and record outputs may have any alignment.  No output may
 * overlap the mask.  Only the voxels of the grid exist.
 *
 * Connectivity.  6 or 26, with vr_label.h's definitions.
 *
 * Labels.  vr_label.h's: 0 for a voxel that is not set, otherwise 1 + the smallest box-linear
 * index of the voxel's component.  A function of the mask and the connectivity alone: two calls
 * write identical bytes, and any correct implementation writes the same bytes.
 *
 * Records.  vr_label_components sorted by ascending label, `reserved` 0.  bbox_min, bbox_max (half
 * open) and sum are in GRID indices: a mask carries no origin.  The info is a vr_label_info with
 * vr_label.h's meanings (in_voxels: the set voxels).
 *
 * Selection.  The output is one byte per voxel, 0 or 1.  For the three KEEP rules `components`
 * counts the components of the set voxels under `connectivity`, `kept` how many of them the rule
 * keeps, and the output is their union.
 *   VR_MASK_KEEP_LARGEST     the component with the most voxels, ties to the smallest label (the
 *                            label info's largest_label); an empty mask: all zero, kept 0.
 *   VR_MASK_KEEP_MIN_VOXELS  every component with voxels >= min_voxels; 0 keeps all of them.
 *   VR_MASK_KEEP_SEED        the component of the grid voxel seed = (i, j, k).  A seed that is not
 *                            set: all zero, kept 0 and VR_OK, as vr_region_grow.  A seed outside
 *                            the grid is VR_EINVAL.
 *   VR_MASK_FILL_HOLES       `connectivity` is that of the UNSET voxels.  A hole is a component of
 *                            unset voxels that holds no voxel on the grid's border (an index 0 or
 *                            ext[a] - 1 along some axis): exactly a record whose bbox touches no
 *                            face.  The output is the set voxels plus every hole; `components`
 *                            counts the unset components and `kept` the holes.  A grid with an
 *                            extent of 1 has no holes.
 * vr_mask_select_info: voxels; in_set, the set voxels of the mask; out_set, those of the output;
 * components and kept as above.
 *
 * Host forms.  vr_mask_label and vr_mask_select take host arrays, stage them through the context's
 * scratch and are synchronous.  The device forms work on `stream` and return when their buffers
 * are complete (the host needs the component count before it sizes the table).
 *
 * Errors.  VR_EINVAL, with every output untouched, for a NULL argument (the stream may be NULL),
 * an extent outside [1, 32768], more than 2^32 - 1 voxels, an elem_bytes other than 1 or 4, a
 * misaligned 4-byte mask or uint32_t output in device memory, an output that overlaps the mask, a
 * connectivity other than 6 or 26, an unknown rule, and a seed outside the grid (VR_MASK_KEEP_SEED).
 * VR_ENOSPC (vr_mesh.h's) in vr_label.h's two forms: lcap or mcap, counted in elements, below the
 * voxel count is refused before any kernel, no buffer touched, info->voxels set and the info's
 * other fields 0; ccap below the component count leaves the info complete and the labels complete,
 * the record buffer untouched.  VR_ENOMEM when the scratch cannot be allocated.
 *
 * State.  The calls read no volume; they build, evict and downgrade nothing (vr_memory_report is
 * unchanged) and leave every setting alone: a frame rendered before and after them has identical
 * bytes.  Scratch lives in the context and is freed by vr_destroy: 3/16 byte per voxel for the
 * root table, 65 bytes per component, the host forms' device copies of their arrays, and for
 * vr_mask_select* its labels, 4 bytes per voxel (vr_mask_label_device labels straight into the
 * caller's buffer).  vr_timing_* brackets the labelling passes (rows, links, flatten, scan) as one
 * interval, the records as a second (none when there is no component) and the selection pass as a
 * third.  vr_maskcc_last_kernel_name names the family's last kernel on the context ("" before the
 * first).  A multi-device context (vr_create_mask) computes on its lowest device, where the
 * buffers must live.
 */
#ifndef VR_VR_MASKCC_H
#define VR_VR_MASKCC_H

#include "vr.h"
#include "vr_label.h" /* vr_label_component, vr_label_info */
#include "vr_mesh.h"  /* VR_ENOSPC */

#ifdef __cplusplus
extern "C" {
#endif

#define VR_MASKCC_MAX_EXTENT 32768u

enum vr_mask_rule {
    VR_MASK_KEEP_LARGEST = 0,
    VR_MASK_KEEP_MIN_VOXELS = 1,
    VR_MASK_KEEP_SEED = 2,
    VR_MASK_FILL_HOLES = 3
};

typedef struct vr_mask_select_request {
    uint32_t rule;          /* enum vr_mask_rule */
    uint32_t connectivity;  /* 6 or 26 */
    uint64_t min_voxels;    /* VR_MASK_KEEP_MIN_VOXELS only */
    uint32_t seed[3];       /* VR_MASK_KEEP_SEED only: a grid voxel (i, j, k) */
    uint32_t reserved;      /* not read */
} vr_mask_select_request;   /* 32 bytes */

typedef struct vr_mask_select_info {
    uint64_t voxels;
    uint64_t in_set;      /* set voxels of the mask */
    uint64_t out_set;     /* set voxels of the output */
    uint64_t components;  /* of the set voxels; VR_MASK_FILL_HOLES: of the unset ones */
    uint64_t kept;        /* components the rule keeps; VR_MASK_FILL_HOLES: the holes */
} vr_mask_select_info;    /* 40 bytes */

/* lcap labels (uint32_t, box-linear order) into labels_dev and ccap records into comps_dev, on
 * `stream`; returns when both buffers are complete. */
int vr_mask_label_device(vr_ctx *ctx, const uint32_t ext[3], const void *mask_dev, uint32_t elem_bytes,
                         uint32_t connectivity, void *labels_dev, uint64_t lcap, void *comps_dev, uint64_t ccap,
                         vr_label_info *info, void *stream);
/* The same from a host mask into host arrays. */
int vr_mask_label(vr_ctx *ctx, const uint32_t ext[3], const void *mask_host, uint32_t elem_bytes,
                  uint32_t connectivity, uint32_t *labels_host, uint64_t lcap, vr_label_component *comps_host,
                  uint64_t ccap, vr_label_info *info);
/* mcap mask bytes (0 or 1, box-linear order) into out_dev, on `stream`; returns when complete. */
int vr_mask_select_device(vr_ctx *ctx, const uint32_t ext[3], const vr_mask_select_request *req,
                          const void *mask_dev, uint32_t elem_bytes, void *out_dev, uint64_t mcap,
                          vr_mask_select_info *info, void *stream);
/* The same from a host mask into a host array. */
int vr_mask_select(vr_ctx *ctx, const uint32_t ext[3], const vr_mask_select_request *req, const void *mask_host,
                   uint32_t elem_bytes, uint8_t *out_host, uint64_t mcap, vr_mask_select_info *info);
/* The last kernel this family launched on the context. */
const char *vr_maskcc_last_kernel_name(const vr_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_MASKCC_H */
