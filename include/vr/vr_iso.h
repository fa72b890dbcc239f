/*
 * vr_iso.h — first-hit isosurface rendering, the third render mode (an addition beside vr.h and
 * vr_modes.h; VR_ABI_VERSION and vr_params are unchanged).
 *
 * In VR_MODE_ISO (vr_modes.h, value 3; 2 is unassigned) the pixel shows the first point of its
 * ray at which the density reaches the context's isovalue, drawn as an opaque, optionally
 * Phong-lit surface.  The isovalue is context state, like the mode and the slice box: it is in
 * the volume's own density units (those of vmin / vmax), defaults to 0.0f, survives volume,
 * transfer-function and mode changes, applies to the frames issued after the call, and matters
 * only in VR_MODE_ISO.  A multi-device context forwards it to every device, as the mode.
 *
 * ISO semantics.  The ray is the composite's: the same pixel ray and entry point, nsteps =
 * int(ray_dist / step), the position update p = p + dir * step in f32, the bounds break and the
 * strict slab test.  Per covered pixel:
 *
 *     hit = false; prev = false
 *     for each step k < nsteps:
 *         if any component of pos is > 1 or < 0: break
 *         steps++
 *         if pos strictly inside the slice box:
 *             d = trilinear(pos)                  the composite's filter, same lerp nesting
 *             samples++
 *             if d >= iso: hit = true; break      a NaN sample never hits
 *             prev = true; q = pos
 *         else:
 *             prev = false
 *         pos = pos + dir * step                  f32, as the composite
 *     if !hit: pixel = clear colour               (all four channels, as every uncovered pixel)
 *     else:
 *         hi = pos
 *         if prev:                                refine between q (below) and pos (at or above)
 *             lo = q
 *             repeat 4 times:
 *                 mid = (lo + hi) * 0.5f          per component: an f32 add, then the exact halving
 *                 if trilinear(mid) >= iso: hi = mid  else: lo = mid
 *         c = tf((iso - vmin) / (vmax - vmin)).rgb    the composite's division and lookup; the
 *                                                 transfer function's alpha is ignored
 *         if params.shading:
 *             g = the exact f32 central-difference gradient at hi (the composite's
 *                 exact_gradient = 1 gradient: never the binary16 field)
 *             w = g * dims; g2 = w . w
 *             if g2 > 0: ndl = |(w . dir) / sqrt(g2)|
 *                        c = c * (ambient + diffuse * ndl) + specular * ndl^spec_power
 *         pixel = (c.r, c.g, c.b, 1.0f)           opaque: no blend with the clear colour
 *
 * A hit at the ray's first in-slab sample (prev == false) is a cap -- the surface cut open by
 * the slice box or the cube face -- and is shown at that sample without refinement.  The four
 * midpoints need no slab test: they lie between two in-slab points of a convex box.
 *
 * Both output formats are supported.  Every kernel variant renders the same bytes.
 *
 * vr_params in ISO mode:
 *   used unchanged   step, ray_dist, clear_color, depth_zero_to_one, shading, ambient, diffuse,
 *                    specular, spec_power, tile_order, wave_shape, frames_in_flight
 *   ignored          ert_eps, exact_gradient (still validated as in composite mode)
 *   skip_empty = 1   range skipping: a search sample in a brick whose stored maximum is below
 *                    the isovalue is not fetched (same pixels).  It needs the per-brick value
 *                    ranges only, which neither a transfer-function change nor an isovalue change
 *                    invalidates; when the memory budget refuses them the frame fetches every
 *                    sample and vr_memory_report counts a downgrade (VR_DERIVED_SKIP).
 * vr_stats from vr_count_work: rays, steps, samples (search samples fetched), skipped_samples
 * (in-slab search samples range skipping leaves out; samples + skipped_samples is the `samples`
 * of the loop above); refinement fetches are not counted; shaded_samples is the number of rays
 * whose surface point was shaded (0 with shading = 0).
 *
 * ISO reads the volume's base bricks only: it builds and evicts no difference field and no
 * alternative copy.
 */
#ifndef VR_VR_ISO_H
#define VR_VR_ISO_H

#include "vr_modes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Set the isovalue of the frames issued from now on (frames already issued keep theirs; a
 * multi-device context forwards it to every device once its issued frames are done).
 * VR_EINVAL: NULL ctx or a non-finite value (the isovalue is unchanged). */
int vr_set_isovalue(vr_ctx *ctx, float v);
/* VR_EINVAL: NULL ctx or NULL v (*v is untouched). */
int vr_get_isovalue(const vr_ctx *ctx, float *v);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_ISO_H */
