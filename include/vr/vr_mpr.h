/*
 * vr_mpr.h — multi-planar reformat (MPR): oblique slices and thick slabs through the volume (an
 * addition beside vr.h, vr_modes.h and vr_iso.h; VR_ABI_VERSION, vr_params and vr_stats are
 * unchanged).
 *
 * An MPR image shows a plane through the data -- axial, coronal, sagittal or oblique -- thin, or
 * thickened into a slab that is projected along the plane's normal with the maximum, the minimum
 * or the mean.  It is the image a viewer puts beside the 3D frame.  MPR is an entry point of its
 * own, not a render mode: it takes no camera, its image has its own size (independent of the
 * context's framebuffer), and the context's render mode and isovalue neither matter to it nor are
 * touched by it -- a frame rendered before and after an MPR call has identical bytes.
 *
 * The plane is given in texture coordinates, the [0,1]^3 cube the march's `pos` lives in (x, y, z
 * = the volume's axes; world +z is screen-up in this renderer).  The rays are parallel and
 * short: one per pixel, nsamples positions along dn, centred on the plane.
 *
 * MPR semantics (the filter, the operators' NaN rules, the transfer-function lookup, the one-step
 * composite epilogue and both output formats are those of vr_modes.h):
 *
 *     for pixel (px, py), row 0 = top, and slab sample s = 0 .. nsamples-1, in this order:
 *         cx = (double)px + 0.5 - 0.5*(double)width;   cy = (double)py + 0.5 - 0.5*(double)height
 *         t  = (double)s - 0.5*(double)(nsamples - 1)          the slab is centred on the plane
 *         q[a] = (float)( (double)origin[a] + cx*(double)du[a] + cy*(double)dv[a] + t*(double)dn[a] )
 *                                 evaluated left to right in double, rounded to f32 once
 *         if any q[a] > 1 or < 0: not a step                   the march's bounds test
 *         steps++
 *         if q strictly inside the context's slice box (the march's strict slab test):
 *             d = trilinear(q)        the composite's filter, same lerp nesting;   samples++
 *             MAX:  m = fmaxf(m, d) from -INFINITY     MIN: m = fminf(m, d) from +INFINITY
 *                                                      (a NaN sample leaves m unchanged)
 *             MEAN: sum = sum + d (f32, from +0, in s order); n++      (a NaN sample propagates)
 *     no sample taken: pixel = clear colour (all four channels)
 *     else: v = m, or sum / (float)n (the correctly rounded f32 quotient)
 *           t = (v - vmin) / (vmax - vmin);  s = tf(t)          (a NaN t reads texel 0)
 *           C = (s.rgb * s.a) * 1;  T = 1 * (1 - s.a)           one composite step from T = 1
 *           A = 1 - T;  out.rgb = C A + clear.rgb (1 - A);  out.a = A A + clear.a (1 - A)
 *
 * The positions are computed in double and rounded once, as the frame kernels' pixel rays are:
 * each product of an f32 with a small half-integer is exact in double, so the result does not
 * depend on whether a compiler contracts to FMA, and a sample's position does not depend on the
 * samples before it.  Unlike a march the loop does not end at the first position outside the
 * cube: a slab whose centre plane lies outside still shows the samples that lie inside.  With
 * nsamples == 1 the three operators give the same pixel (for a NaN sample each by its own rule).
 *
 * vr_params: validated as in every mode; only clear_color is used.  step, ray_dist, shading,
 * ert_eps, skip_empty and the scheduling fields are ignored.
 * vr_stats from vr_mpr_count_work: rays = pixels with at least one step; steps and samples as in
 * the loop above; shaded_samples = skipped_samples = 0.
 *
 * MPR reads the volume's base bricks only (every storage type): it builds and evicts no derived
 * structure and counts no downgrade.  vr_timing_* brackets the MPR kernel like a frame kernel, and
 * vr_debug_last_kernel_name names it.  A multi-device context (vr_create_mask) renders the whole
 * image on its lowest device, which holds a replica of the volume: no row shares, nothing goes
 * through vr_dist.
 *
 * Errors: VR_EINVAL, with the output untouched, for a NULL argument; a non-finite component in
 * origin, du, dv or dn; width or height 0 (vr_resize accepts every other size, and so does MPR
 * as long as the image's 16x16-pixel tiles number less than 2^31); nsamples 0 or above
 * VR_MPR_MAX_SAMPLES; an unknown op or out_format; and whatever vr_params every mode refuses.
 */
#ifndef VR_VR_MPR_H
#define VR_VR_MPR_H

#include "vr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum vr_mpr_op { VR_MPR_MAX = 0, VR_MPR_MIN = 1, VR_MPR_MEAN = 2 };

#define VR_MPR_MAX_SAMPLES 4096

typedef struct vr_mpr_plane {
    float origin[3];    /* texture coordinates (the [0,1]^3 cube the march's `pos` lives in) of the image centre */
    float du[3];        /* texture-space step of one pixel to the right */
    float dv[3];        /* texture-space step of one pixel down (row 0 = top) */
    float dn[3];        /* texture-space step between consecutive slab samples */
    uint32_t width, height;  /* the image; independent of the context's framebuffer size */
    uint32_t nsamples;  /* 1 = thin slice; up to VR_MPR_MAX_SAMPLES */
    int32_t  op;        /* vr_mpr_op; with nsamples == 1 all three give the same pixel */
} vr_mpr_plane;

/* Synchronous: width * height pixels of out_format (vr_out_format) into host memory. */
int vr_mpr_render(vr_ctx *ctx, const vr_mpr_plane *plane, const vr_params *params, void *out_host,
                  int out_format);
/* The same pixels into device memory of the context's device (a multi-device context: its lowest
 * device), asynchronous on `stream` (NULL: the default stream). */
int vr_mpr_render_device(vr_ctx *ctx, const vr_mpr_plane *plane, const vr_params *params,
                         void *out_dev, int out_format, void *stream);
/* The loop's counters for the whole image (synchronous; writes no pixel). */
int vr_mpr_count_work(vr_ctx *ctx, const vr_mpr_plane *plane, const vr_params *params,
                      vr_stats *out);
/* Pure host helper, no context: an axis-aligned plane showing the whole cross-section, computed
 * in f32.  origin is 0.5 on the two in-plane axes and `position` on `axis`; dn is `spacing` along
 * `axis`; the image spans the whole face:
 *   axis 2 (axial):    right = +x, du.x = 1.0f / width;  down = +y, dv.y = 1.0f / height
 *   axis 1 (coronal):  right = +x;                       down = -z, dv.z = -(1.0f / height)
 *   axis 0 (sagittal): right = +y, du.y = 1.0f / width;  down = -z
 * VR_EINVAL (*out untouched): NULL out, an axis outside 0..2, a non-finite position or spacing,
 * and the size, sample-count and operator errors above. */
int vr_mpr_axis_plane(int axis, float position, uint32_t width, uint32_t height,
                      uint32_t nsamples, float spacing, int op, vr_mpr_plane *out);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_MPR_H */
