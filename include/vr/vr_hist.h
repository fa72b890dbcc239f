/*
 * vr_hist.h — the value histogram of the resident volume, the exact data range that comes with
 * it, a percentile window from a histogram, and a setter that applies a value window without
 * touching the voxels (an addition beside vr.h, vr_modes.h, vr_iso.h and vr_mpr.h;
 * VR_ABI_VERSION, vr_params and vr_stats are unchanged).
 *
 * Every frame mode and every MPR image turns a density into a colour through
 * t = (v - vmin) / (vmax - vmin) and the transfer function.  These calls give a caller what it
 * needs to choose that window: the distribution of the voxels (computed on the device from the
 * base bricks, so a volume uploaded from device memory needs no host copy), their exact minimum
 * and maximum, and vr_set_value_range to apply a window without a re-upload.
 *
 * Binning.  A voxel's value is v = (float)stored, the value the sampler uses (an integer volume
 * that was narrowed to 8 or 16 bits gives the same v).  The lower edges of the bins are
 *
 *     e[b] = (float)( (double)lo + ((double)b * ((double)hi - (double)lo)) / (double)nbins )
 *                                  b = 0 .. nbins-1, evaluated left to right in double and
 *                                  rounded to f32 once
 *
 * They are non-decreasing and e[0] == lo exactly; vr_hist_edges returns exactly these.  A voxel
 * with lo <= v <= hi counts in the LARGEST b with e[b] <= v: v == hi lands in the last bin, and
 * of several equal edges the last one takes the value (np.searchsorted(e, v, side="right") - 1).
 * v < lo counts in `below`, v > hi in `above`, a NaN in `nan`; -0.0 compares as 0.  Counts are
 * exact integers: the result depends neither on the kernel variant, nor on the brick layout, nor
 * on the order of accumulation.
 *
 * vr_histogram is synchronous.  It reads the volume's base bricks only (every storage type and
 * layout), each voxel once through its own element: it builds, evicts and downgrades nothing
 * (vr_memory_report is unchanged) and leaves render mode, isovalue, slice box, TF and window
 * alone -- a frame rendered before and after it has identical bytes.  vr_timing_* brackets its
 * kernel like a frame kernel, and vr_debug_last_kernel_name names it.  A multi-device context
 * (vr_create_mask) computes on its lowest device, which holds a replica of the volume; nothing
 * goes through vr_dist.
 * Errors: VR_EINVAL, with the outputs untouched and before any HIP call, for a NULL argument, a
 * non-finite lo or hi, lo >= hi, nbins 0 or above VR_HIST_MAX_BINS, and use_box other than 0 or
 * 1; and (after the context lookup) for an empty box or one beyond the volume's dimensions.
 *
 * vr_hist_window (pure host): with c[b] the running sum of bins and N = c[nbins-1],
 *     b0 = the smallest b with c[b] >  (uint64_t)floor(p_lo * (double)N)
 *     b1 = the smallest b with c[b] >= max(1, (uint64_t)ceil(p_hi * (double)N))
 *     *vmin_out = e[b0];   *vmax_out = (b1 == nbins-1) ? hi : e[b1+1]
 * VR_EINVAL, with the outputs untouched, for a NULL argument, a bad lo / hi / nbins, N == 0, and
 * anything other than 0 <= p_lo < p_hi <= 1.
 *
 * vr_set_value_range replaces vmin / vmax exactly as an upload of the same voxels with these
 * values would: it validates what vr_set_volume validates (a NULL context only; vmin == vmax keeps
 * its texel-0 meaning), waits for the device(s) first as a volume or TF change does, and
 * invalidates the skip-empty distance field (built from the window); the per-brick ranges and the
 * difference fields do not depend on the window and stay.  A multi-device context forwards it to
 * every member.  vr_debug_volume_info reports the new values.
 */
#ifndef VR_VR_HIST_H
#define VR_VR_HIST_H

#include "vr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VR_HIST_MAX_BINS 4096

typedef struct vr_hist_request {
    float lo, hi;        /* finite, lo < hi */
    uint32_t nbins;      /* 1 .. VR_HIST_MAX_BINS */
    uint32_t use_box;    /* 0: the whole volume; 1: the voxel box below */
    uint32_t box_min[3]; /* voxel indices, x y z; the box is half open: */
    uint32_t box_max[3]; /* box_min[a] <= i < box_max[a] <= dims[a], not empty */
} vr_hist_request;       /* 40 bytes */

typedef struct vr_hist_info {
    uint64_t voxels;             /* voxels in the box = sum(bins) + below + above + nan */
    uint64_t below, above, nan;  /* v < lo;  v > hi;  v != v */
    float vmin, vmax;            /* over the box's non-NaN voxels (infinities count);
                                    none: +INFINITY / -INFINITY.  The sign of a zero
                                    extreme is unspecified (compare with ==) */
} vr_hist_info;                  /* 40 bytes */

/* Synchronous: req->nbins counts into bins_host, the rest into *info. */
int vr_histogram(vr_ctx *ctx, const vr_hist_request *req, uint64_t *bins_host, vr_hist_info *info);
/* Pure host helpers, no context. */
int vr_hist_edges(float lo, float hi, uint32_t nbins, float *edges_out /* nbins floats */);
int vr_hist_window(const uint64_t *bins, uint32_t nbins, float lo, float hi,
                   double p_lo, double p_hi, float *vmin_out, float *vmax_out);
/* The value window of every later frame and MPR image; the voxels stay. */
int vr_set_value_range(vr_ctx *ctx, float vmin, float vmax);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_HIST_H */
