/*
 * vr_modes.h — render modes of a context (an addition beside vr.h; VR_ABI_VERSION and
 * vr_params are unchanged).
 *
 * A context renders in one of five modes.  The mode is context state, like the slice box: it
 * applies to every frame issued after the call, through vr_render, vr_render_device (row shares
 * included), vr_prepare, vr_count_work, vr_timing_*, vr_kernel_name and vr_dist_render.
 *
 *   VR_MODE_COMPOSITE  (default) the reference's front-to-back transfer-function composite
 *                      (volume.frag), everything vr.h describes.
 *   VR_MODE_MIP        maximum-intensity projection: the pixel shows the largest density
 *                      sample of its ray, looked up in the transfer function once.
 *   VR_MODE_ISO        first-hit isosurface: the first point of the ray whose density reaches
 *                      the context's isovalue, drawn as a lit opaque surface (vr_iso.h has the
 *                      isovalue's entry points and the semantics).
 *   VR_MODE_MINIP      minimum-intensity projection: the pixel shows the smallest density
 *                      sample of its ray (the thin-slab view of airways and other low-density
 *                      structures; meant to be used with the slice box, see below).
 *   VR_MODE_MEAN       mean-intensity projection: the average of the ray's density samples,
 *                      looked up in the transfer function once (the "X-ray" / thick-slab look).
 *
 * The values 2 and 5 are unassigned: vr_set_render_mode refuses them like any unknown mode.
 *
 * MIP semantics.  The ray is the composite's: the same pixel ray and entry point, nsteps =
 * int(ray_dist / step), the position update p = p + dir * step in f32, the bounds break and the
 * strict slab test.  Per covered pixel:
 *
 *     m = -INFINITY; any = false
 *     for each step that passes the bounds test and the strict slab test:
 *         d = trilinear(pos)                  the composite's filter, same lerp nesting
 *         m = fmaxf(m, d); any = true         a NaN sample leaves m unchanged
 *     if !any: pixel = clear colour           (as every uncovered pixel)
 *     else:
 *         t = (m - vmin) / (vmax - vmin)      as the composite (vmin == vmax: NaN, texel 0)
 *         s = tf(t)
 *         C = (s.rgb * s.a) * 1;  T = 1 * (1 - s.a)        one composite step from T = 1
 *         A = 1 - T;  out.rgb = C A + clear.rgb (1 - A);  out.a = A A + clear.a (1 - A)
 *
 * Both output formats are supported.  The maximum does not depend on the order the samples are
 * taken in, so every kernel variant renders the same bytes.
 *
 * vr_params in MIP mode:
 *   used unchanged   step, ray_dist, clear_color, depth_zero_to_one, tile_order, wave_shape,
 *                    frames_in_flight
 *   ignored          shading, ambient, diffuse, specular, spec_power, exact_gradient, ert_eps
 *                    (still validated as in composite mode)
 *   skip_empty = 1   range skipping: a sample in a brick whose stored maximum is not above the
 *                    ray's running maximum is not fetched (same pixels).  It needs the per-brick
 *                    value ranges only, which a transfer-function change does not invalidate;
 *                    when the memory budget refuses them the frame fetches every sample and
 *                    vr_memory_report counts a downgrade (VR_DERIVED_SKIP).
 * vr_stats from vr_count_work: rays, steps, samples (fetched), skipped_samples (in-slab samples
 * range skipping leaves out); shaded_samples is 0.
 *
 * MIP reads the volume's base bricks only: it builds and evicts no difference field and no
 * alternative copy.
 *
 * MinIP and mean semantics.  The ray, the filter, the epilogue, both output formats and the
 * vr_params table are MIP's; what is kept along the ray differs.  Per covered pixel:
 *
 *     MinIP:  m = +INFINITY; any = false
 *             each in-slab step:  d = trilinear(pos);  m = fminf(m, d);  any = true
 *                                                      (a NaN sample leaves m unchanged)
 *             v = m
 *     Mean:   sum = 0.0f; n = 0
 *             each in-slab step, in step order:  d = trilinear(pos);  sum = sum + d;  n = n + 1
 *                                 (one f32 addition per sample, so the order is part of the
 *                                 result; a NaN or infinite sample propagates as IEEE addition says)
 *             any = n > 0;  v = sum / (float)n         the correctly rounded f32 quotient
 *     both:   if !any: pixel = clear colour
 *             else: t = (v - vmin) / (vmax - vmin);  s = tf(t)      (a NaN t reads texel 0)
 *                   one composite step from T = 1, then the blend over the clear colour, as MIP
 *
 * Every kernel variant renders the same bytes: the minimum does not depend on the order, and the
 * mean's additions are made in step order whatever the number of samples in flight.
 *
 *   skip_empty = 1   range skipping, same pixels, from the per-brick value ranges alone (as MIP:
 *                    no transfer-function dependence, VR_DERIVED_SKIP downgrade over the budget).
 *                    MinIP: a sample in a brick whose stored minimum is not below the ray's
 *                    running minimum is not fetched.  Mean: a sample in a brick whose values are
 *                    all one finite number c is not fetched and adds c (it still counts in n).
 * vr_stats from vr_count_work: as MIP; samples + skipped_samples is the number of in-slab steps.
 *
 * One wart: the sampler is the composite's CLAMP_TO_BORDER, so a sample within half a voxel of a
 * cube face blends with 0.  A MinIP over the whole cube is therefore dominated by its entry and
 * exit samples: use MinIP with a slice box inset by at least half a voxel on every side.
 *
 * Like MIP, both read the base bricks only: no difference field, no alternative copy, nothing
 * evicted.
 */
#ifndef VR_VR_MODES_H
#define VR_VR_MODES_H

#include "vr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum vr_render_mode { VR_MODE_COMPOSITE = 0, VR_MODE_MIP = 1, VR_MODE_ISO = 3,
                      VR_MODE_MINIP = 4, VR_MODE_MEAN = 6 /* 2, 5: unassigned */ };

/* Set the mode of the frames issued from now on (frames already issued keep theirs; a
 * multi-device context forwards it to every device once its issued frames are done).
 * VR_EINVAL: NULL ctx or unknown mode (the mode is unchanged). */
int vr_set_render_mode(vr_ctx *ctx, int mode);
/* VR_EINVAL: NULL ctx or NULL mode. */
int vr_get_render_mode(const vr_ctx *ctx, int *mode);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_MODES_H */
