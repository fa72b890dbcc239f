/*
 * vr_mstat.h — the volume under a device mask or label array: the statistics and the histogram of
 * the voxels a mask selects, one statistics record per label of a label array, and a value-window
 * pass that writes or refines a mask (an addition beside vr.h and the other family headers;
 * VR_ABI_VERSION, vr_params and vr_stats are unchanged).  The entry points live in
 * lib/libvr_amd_mstat.so, a fourth library beside libvr_amd.so, libvr_amd_morph.so and
 * libvr_amd_maskcc.so on the same context: link it with libvr_amd.so.
 *
 * vr_label.h, vr_morph.h and vr_maskcc.h take a caller from a click to a clean segmentation; every
 * one of their calls ends in a mask or a label array.  These calls bring that array back to the
 * data without a read-back: the mean and the extremes of the lesion, its histogram, an intensity
 * record per component, the intersection of a mask with a value window.  They read the resident
 * base bricks (as vr_histogram does) and an array in device memory (as vr_morph.h does).
 *
 * Grid and array.  vr_morph.h's.  ext[3] = (bx, by, bz) voxels, every extent in [1, 32768], at most
 * 2^32 - 1 voxels, box-linear order l = i + bx * (j + by * k).  elem_bytes is 1 or 4 (also where
 * vr_mask_window*'s mask is NULL); a voxel is SET iff its element is non-zero.  A label array is
 * uint32_t.  A 4-byte array in device memory must be 4-byte aligned; a 1-byte mask, the byte output,
 * the table and the region records may have any alignment.  No output may overlap an input.
 *
 * Origin.  origin[3] is the VOLUME voxel index of grid voxel (0, 0, 0): grid voxel (i, j, k) is
 * volume voxel origin + (i, j, k), and origin[a] + ext[a] <= dims[a].  For a mask made by
 * vr_region_grow* or vr_label_components* with a box, origin is that box_min; otherwise zero.
 *
 * Values.  A voxel's value is f = (float)stored, the sampler's value, as in vr_hist.h and
 * vr_label.h.  Only the base bricks are read, never a derived structure.
 *
 * Records.  A vr_mstat_region describes the grid voxels of one region: `voxels` of them, `nan` of
 * them NaN; vmin / vmax over the others (infinities count; none: +INFINITY / -INFINITY; the sign of
 * a zero extreme is unspecified, as in vr_hist.h; -0.0 == 0); min_index / max_index, the smallest
 * box-linear index with f == vmin / f == vmax (VR_MSTAT_NONE when there is none); sum and sum2 of f
 * and f * f over the non-NaN voxels (+0.0 when none).  Everything but sum and sum2 on f32 storage is
 * a function of the volume, the array and the request alone: two calls, and any correct
 * implementation, write the same bytes (up to the sign of a zero extreme).
 *
 * Sums.  On integer storage (vr_debug_volume_info's storage u8 / i8 / u16 / i16, which includes a
 * 32- or 64-bit upload that VR_KNOB_NARROW narrowed) they are the exact integer sums, accumulated
 * in 64 bits -- sum as int64, sum2 as uint64: 65535^2 * (2^32 - 1) < 2^64 -- and converted to double
 * once: bytes too.  On f32 storage the terms are (double)f and the exact product
 * (double)f * (double)f, added in double in an unspecified order: with n terms and A the sum of
 * their magnitudes, |sum - S| <= (n - 1) * 2^-52 * A (the bound gamma(n-1) * A with
 * gamma(k) <= 2k * 2^-53, which holds for every order), and the same for sum2.  Opposite infinities
 * give NaN, as IEEE addition does.  A zero term counts as +0.0 whatever its sign, so a sum is never
 * -0.0: a region whose voxels are all -0.0 has sum +0.0.  This is the only place where two calls may differ: the kernels
 * add these two fields with the hardware's double add on device memory.
 *
 * vr_mask_stats*.  The set voxels are one region with label 1, into *region_out (host memory).  With
 * `hist` the bins follow vr_hist.h's binning exactly over the set voxels (lo, hi, nbins; use_box
 * must be 0: the grid is the box), and *hinfo has vr_hist.h's meanings over them: hinfo->voxels ==
 * region_out->voxels.  hist, bins_host and hinfo are NULL together or not at all.
 *
 * vr_label_stats*.  The table is ntable 64-byte vr_label_component records as either labeller writes
 * them (vr_label_components*, vr_mask_label*); only .label is read: labels strictly ascending and
 * non-zero.  Region i describes the voxels whose element equals table[i].label, in table order; an
 * empty one has voxels 0.  A non-zero element whose value is not in the table counts in
 * info->unlisted and in no record; info->set counts the non-zero elements, info->regions is ntable,
 * which may be 0.  A table that is not ascending makes the records unspecified, but every access
 * stays inside the buffers and the call returns.
 *
 * vr_mask_window*.  The out byte is 1 iff the voxel is set (mask NULL: always) and lo <= f && f <= hi,
 * compared in f32: vr_label.h's window.  A NaN is never in; the bounds may be infinite.  The info is
 * a vr_morph_info: voxels, in_set (the grid's count when the mask is NULL) and out_set.
 *
 * Host forms.  vr_mask_stats, vr_label_stats and vr_mask_window take host arrays, stage them through
 * the context's scratch and are synchronous.  The device forms work on `stream` and return when
 * their outputs are complete.
 *
 * Errors.  VR_EINVAL, with every output untouched, for a NULL argument (the stream, hist with its
 * two outputs, and vr_mask_window*'s mask may be NULL), an extent outside [1, 32768], more than
 * 2^32 - 1 voxels, an origin or grid beyond the volume (or no volume), an elem_bytes other than 1 or
 * 4, a misaligned 4-byte array in device memory, an output that overlaps an input, hist->use_box
 * other than 0 or a lo / hi / nbins that vr_hist.h refuses, NaN window bounds or lo > hi, and ntable
 * above 2^32 - 1.  VR_ENOSPC (vr_mesh.h's) before any kernel for rcap below ntable or mcap below
 * the voxel count: info->voxels set and the info's other fields 0, no buffer touched.  VR_ENOMEM
 * when the scratch cannot be allocated.
 *
 * State.  vr_hist.h's: the calls build, evict and downgrade nothing (vr_memory_report is unchanged)
 * and leave every setting alone: a frame rendered before and after them has identical bytes.
 * Scratch lives in the context and is freed by vr_destroy: 116 bytes per table record, 48 KiB for
 * the counters and the histogram, and the host forms' device copies of their arrays.  vr_timing_*
 * brackets each call's passes as one interval.  vr_mstat_last_kernel_name names the family's last
 * kernel on the context ("" before the first).  A multi-device context (vr_create_mask) computes on
 * its lowest device, where the buffers must live.
 */
#ifndef VR_VR_MSTAT_H
#define VR_VR_MSTAT_H

#include "vr.h"
#include "vr_hist.h"  /* vr_hist_request, vr_hist_info */
#include "vr_label.h" /* vr_label_component */
#include "vr_mesh.h"  /* VR_ENOSPC */
#include "vr_morph.h" /* vr_morph_info */

#ifdef __cplusplus
extern "C" {
#endif

#define VR_MSTAT_MAX_EXTENT 32768u
#define VR_MSTAT_NONE 0xFFFFFFFFu

typedef struct vr_mstat_region {
    uint32_t label;                /* the table's label; 1 for vr_mask_stats* */
    uint32_t reserved;             /* 0 */
    uint64_t voxels;               /* grid voxels of the region */
    uint64_t nan;                  /* of them, NaN */
    float    vmin, vmax;           /* over the non-NaN voxels, infinities count; none: +INF / -INF */
    uint32_t min_index, max_index; /* smallest box-linear index with f == vmin / f == vmax;
                                      VR_MSTAT_NONE when there is none */
    double   sum, sum2;            /* of f and of f*f over the non-NaN voxels; +0.0 when none */
    uint64_t reserved2;            /* 0 */
} vr_mstat_region;                 /* 64 bytes */

typedef struct vr_mstat_info {
    uint64_t voxels;    /* bx * by * bz */
    uint64_t set;       /* non-zero elements */
    uint64_t unlisted;  /* of them, those whose value the table does not hold */
    uint64_t regions;   /* ntable */
} vr_mstat_info;        /* 32 bytes */

/* The region of the set voxels into *region_out and, with hist, hist->nbins counts into bins_host
 * and the rest into *hinfo (all host memory), on `stream`; returns when they are complete. */
int vr_mask_stats_device(vr_ctx *ctx, const uint32_t ext[3], const uint32_t origin[3], const void *mask_dev,
                         uint32_t elem_bytes, const vr_hist_request *hist, uint64_t *bins_host, vr_hist_info *hinfo,
                         vr_mstat_region *region_out, void *stream);
/* The same from a host mask. */
int vr_mask_stats(vr_ctx *ctx, const uint32_t ext[3], const uint32_t origin[3], const void *mask_host,
                  uint32_t elem_bytes, const vr_hist_request *hist, uint64_t *bins_host, vr_hist_info *hinfo,
                  vr_mstat_region *region_out);
/* ntable records into regions_dev (rcap records), on `stream`; returns when they are complete. */
int vr_label_stats_device(vr_ctx *ctx, const uint32_t ext[3], const uint32_t origin[3], const void *labels_dev,
                          const void *table_dev, uint64_t ntable, void *regions_dev, uint64_t rcap,
                          vr_mstat_info *info, void *stream);
/* The same from host arrays into a host array. */
int vr_label_stats(vr_ctx *ctx, const uint32_t ext[3], const uint32_t origin[3], const uint32_t *labels_host,
                   const vr_label_component *table_host, uint64_t ntable, vr_mstat_region *regions_host,
                   uint64_t rcap, vr_mstat_info *info);
/* mcap mask bytes (0 or 1, box-linear order) into out_dev, on `stream`; returns when complete. */
int vr_mask_window_device(vr_ctx *ctx, const uint32_t ext[3], const uint32_t origin[3], const void *mask_dev,
                          uint32_t elem_bytes, float lo, float hi, void *out_dev, uint64_t mcap,
                          vr_morph_info *info, void *stream);
/* The same from a host mask (or NULL) into a host array. */
int vr_mask_window(vr_ctx *ctx, const uint32_t ext[3], const uint32_t origin[3], const void *mask_host,
                   uint32_t elem_bytes, float lo, float hi, uint8_t *out_host, uint64_t mcap,
                   vr_morph_info *info);
/* The last kernel this family launched on the context. */
const char *vr_mstat_last_kernel_name(const vr_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_MSTAT_H */
