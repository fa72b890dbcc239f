/*
 * vr_morph.h — the exact Euclidean distance transform of a device mask and ball morphology on it
 * (an addition beside vr.h and the other family headers; VR_ABI_VERSION, vr_params and vr_stats are
 * unchanged).  The entry points live in lib/libvr_amd_morph.so, a second library beside
 * libvr_amd.so on the same context: link both.
 *
 * vr_label.h hands out the component under a click as a device mask and the labels of a value
 * window.  These calls clean such a mask and measure it: close a leak before growing, open away a
 * bridge, drop a shell of partial-volume voxels, find the thickest point of a vessel, turn a mask
 * into a margin.  All of them are one primitive, the squared distance to the nearest voxel of a
 * target set; dilation, erosion, opening and closing with a ball are thresholds of it.
 *
 * Grid.  ext[3] = (bx, by, bz) voxels, in box-linear order, l = i + bx * (j + by * k): exactly the
 * order in which vr_label.h delivers its labels and masks.  Only the voxels of the grid exist:
 * nothing outside it is set, unset or read.  Every extent lies in [1, 32768], so that the largest
 * distance, 3 * 32767^2, stays below the sentinel, and the grid holds at most 2^32 - 1 voxels, so
 * that an index fits 32 bits.  Distances are in isotropic voxel units (the project has no voxel
 * spacing).
 *
 * Mask in.  A device buffer of elem_bytes 1 or 4 per voxel: 1 is a region-grow mask, 4 a label
 * array.  A voxel is SET iff its element is non-zero.  A 1-byte mask may have any alignment; a
 * 4-byte mask and every uint32_t output in device memory must be 4-byte aligned.  No output may
 * overlap the mask.
 *
 * Squared distance.  vr_edt_squared_device writes one uint32_t per voxel in box-linear order: the
 * minimum of |p - q|^2 over the target voxels q of the grid, target being the set voxels
 * (VR_EDT_TO_SET) or the unset ones (VR_EDT_TO_UNSET).  An exact integer, 0 on the target voxels;
 * VR_EDT_NONE everywhere when the grid has no target voxel.  The result is a function of the mask
 * alone: two calls write identical bytes, and any correct implementation writes the same bytes.
 * vr_edt_info: voxels, the grid's count; target_voxels; max_dist2 and max_index, the largest finite
 * value and the smallest box-linear index that holds it (VR_EDT_NONE and 0 when no value is
 * finite).
 *
 * Morphology.  The structuring element is the ball of integer squared radius r2, 0 <= r2 <
 * VR_EDT_NONE: the offsets d with |d|^2 <= r2.  The output is one byte per voxel, 0 or 1.
 *   dilate(M) = {p : some q in M has |p - q|^2 <= r2}
 *   erode(M)  = {p in M : every grid voxel q with |p - q|^2 <= r2 is in M}
 * so the grid's border erodes nothing; open = dilate(erode(M)), close = erode(dilate(M)).  r2 = 0
 * returns M as 0/1 for every op.  vr_morph_info: voxels, in_set (the set voxels of the mask) and
 * out_set (those of the output).
 *
 * Host forms.  vr_edt_squared and vr_mask_morph take host arrays, stage them through the context's
 * scratch and are synchronous.  The device forms work on `stream` and return when their buffer is
 * complete (the info needs the counts).
 *
 * Errors.  VR_EINVAL, with every output untouched, for a NULL argument (the stream may be NULL), an
 * extent outside [1, 32768], more than 2^32 - 1 voxels, an elem_bytes other than 1 or 4, an unknown
 * target or op, r2 = VR_EDT_NONE, a misaligned 4-byte mask or uint32_t output in device memory, and
 * an output that overlaps the mask.  VR_ENOSPC (vr_mesh.h's) when dcap or mcap, counted in
 * elements, is below the voxel count: refused before any kernel, no buffer touched, info->voxels
 * set and the info's other fields 0.  VR_ENOMEM when the scratch cannot be allocated.
 *
 * State.  The calls read no volume; they build, evict and downgrade nothing (vr_memory_report is
 * unchanged) and leave every setting alone: a frame rendered before and after them has identical
 * bytes.  Scratch lives in the context and is freed by vr_destroy: 4 bytes per voxel for the
 * morphology's distance (vr_edt_squared_device transforms in place in the caller's buffer and
 * takes none), 1 byte per voxel for the intermediate mask of open and close, eight words of
 * counters, and the host forms' device copies of their arrays.  vr_timing_* brackets one interval
 * per transform: one for a squared distance, a dilation or an erosion, two for an opening or a
 * closing.  vr_morph_last_kernel_name names the family's last kernel on the context ("" before
 * the first).  A multi-device context (vr_create_mask) computes on its lowest device, where the
 * buffers must live.
 */
#ifndef VR_VR_MORPH_H
#define VR_VR_MORPH_H

#include "vr.h"
#include "vr_mesh.h" /* VR_ENOSPC */

#ifdef __cplusplus
extern "C" {
#endif

#define VR_EDT_NONE 0xFFFFFFFFu /* the distance where the grid has no target voxel */
#define VR_MORPH_MAX_EXTENT 32768u

enum vr_edt_target { VR_EDT_TO_SET = 0, VR_EDT_TO_UNSET = 1 };
enum vr_morph_op { VR_MORPH_DILATE = 0, VR_MORPH_ERODE = 1, VR_MORPH_OPEN = 2, VR_MORPH_CLOSE = 3 };

typedef struct vr_edt_info {
    uint64_t voxels;        /* bx * by * bz */
    uint64_t target_voxels;
    uint32_t max_dist2;     /* the largest finite value; VR_EDT_NONE when there is none */
    uint32_t max_index;     /* the smallest box-linear index that holds it; 0 when there is none */
} vr_edt_info;              /* 24 bytes */

typedef struct vr_morph_info {
    uint64_t voxels;
    uint64_t in_set;        /* set voxels of the mask */
    uint64_t out_set;       /* set voxels of the output */
} vr_morph_info;            /* 24 bytes */

/* dcap distances (uint32_t, box-linear order) into dist2_dev, on `stream`; returns when complete. */
int vr_edt_squared_device(vr_ctx *ctx, const uint32_t ext[3], const void *mask_dev, uint32_t elem_bytes,
                          uint32_t target, void *dist2_dev, uint64_t dcap, vr_edt_info *info, void *stream);
/* The same from a host mask into a host array. */
int vr_edt_squared(vr_ctx *ctx, const uint32_t ext[3], const void *mask_host, uint32_t elem_bytes,
                   uint32_t target, uint32_t *dist2_host, uint64_t dcap, vr_edt_info *info);
/* mcap mask bytes (0 or 1, box-linear order) into out_dev, on `stream`; returns when complete. */
int vr_mask_morph_device(vr_ctx *ctx, const uint32_t ext[3], uint32_t op, uint32_t r2, const void *mask_dev,
                         uint32_t elem_bytes, void *out_dev, uint64_t mcap, vr_morph_info *info, void *stream);
/* The same from a host mask into a host array. */
int vr_mask_morph(vr_ctx *ctx, const uint32_t ext[3], uint32_t op, uint32_t r2, const void *mask_host,
                  uint32_t elem_bytes, uint8_t *out_host, uint64_t mcap, vr_morph_info *info);
/* The last kernel this family launched on the context. */
const char *vr_morph_last_kernel_name(const vr_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_MORPH_H */
