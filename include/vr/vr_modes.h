/*
 * vr_modes.h — render modes of a context (an addition beside vr.h; VR_ABI_VERSION and
 * vr_params are unchanged).
 *
 * A context renders in one of three modes.  The mode is context state, like the slice box: it
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
 *
 * The value 2 is unassigned: vr_set_render_mode refuses it like any unknown mode.
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
 */
#ifndef VR_VR_MODES_H
#define VR_VR_MODES_H

#include "vr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum vr_render_mode { VR_MODE_COMPOSITE = 0, VR_MODE_MIP = 1, VR_MODE_ISO = 3 /* 2: unassigned */ };

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
