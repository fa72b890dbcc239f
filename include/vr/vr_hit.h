/*
 * vr_hit.h — per-pixel hit records of the 3D frame, and picking (an addition beside vr.h,
 * vr_modes.h, vr_iso.h, vr_mpr.h and vr_hist.h; VR_ABI_VERSION, vr_params and vr_stats are
 * unchanged).
 *
 * A frame is colour only.  These calls say where in the volume a pixel of a frame comes from: the
 * texture coordinates of the point its ray "finds", the distance from the camera to it, the
 * density there and the step that found it -- for a 3D cursor (a click on a vessel in the MIP
 * frame places the MPR planes through hit.pos, vr_mpr_axis_plane), for measuring between two
 * picked points, and for a host that draws geometry beside the volume and needs a depth per
 * pixel.  What "finds" means is the request's kind, which a caller chooses to match the frame it
 * shows; it is a field of the request and not the context's render mode, as MPR is independent of
 * the mode.  VR_HIT_ISO uses the context's isovalue (vr_set_isovalue).
 *
 * The output holds w * h records of 24 bytes, row-major; row 0 is the top row of the rectangle,
 * or of the framebuffer when use_rect is 0.
 *
 * The walk.  The ray is the composite's, exactly as vr_iso.h states it: the same pixel ray and
 * entry point -- for pixel (x0 + i, y0 + j) of the full W x H framebuffer --, nsteps =
 * int(ray_dist / step), the position update pos = pos + dir * step in f32, the bounds break and
 * the strict slab test, d = trilinear(pos) with the composite's filter.  Per covered pixel, with
 * k the loop index:
 *
 *     ENTRY    the first in-slab sample: hit at k, pos, value = d (NaN allowed; the sign and
 *              payload of a NaN value are unspecified, here and in OPACITY)
 *     OPACITY  T = 1.0f; per in-slab sample, in step order:
 *                  t = (d - vmin) / (vmax - vmin);  a = tf(t).a   the composite's division, lookup
 *                  T = T * (1.0f - a)
 *                  if (1.0f - T) >= threshold: hit at k, pos, value = d; stop
 *              (shading and ert_eps are ignored: neither changes a frame's alpha before the
 *              march terminates.  As in the composite frame, a NaN or infinite d reads texel 0
 *              when the window is one the kernels divide by with a reciprocal)
 *     MAX      m = -INFINITY; per in-slab sample: if d > m: m = d, remember k, pos.
 *              After the ray: hit iff some sample updated m; value = m.  So the record is the
 *              FIRST sample equal to the ray's maximum; NaN samples never update; a ray of only
 *              NaN / -inf samples misses.
 *     MIN      the mirror image: from +INFINITY with d < m.  (The border-blend wart of
 *              vr_modes.h applies: use an inset slice box.)
 *     ISO      the search and the 4-step bisection of vr_iso.h, verbatim.  step = k of the first
 *              sample with d >= iso; pos = the refined `hi` (a cap: the sample itself);
 *              value = trilinear(hi)
 *     an uncovered pixel, or no hit: the miss record {0,0,0, +INFINITY, 0, 0xFFFFFFFF}
 *
 *     depth = (float) sqrt(dx*dx + dy*dy + dz*dz),  d_a = ((double)pos[a] - 0.5) - (double)cam.position[a]
 *             evaluated left to right in double (no contraction), rounded to f32 once: the
 *             Euclidean distance camera -> point in world units (the volume is the unit cube
 *             centred on the origin).
 *
 * vr_params: step, ray_dist, depth_zero_to_one and wave_shape are used unchanged; everything
 * else (skip_empty, tile_order and frames_in_flight included) is validated as in every mode and
 * then ignored.  Every kernel variant (VR_KNOB_HIT_INFLIGHT) writes the same bytes.
 *
 * vr_stats from vr_hit_count_work: rays = covered pixels; steps and samples count up to and
 * including the step and sample that ended the walk (MAX and MIN walk the whole ray; ISO's
 * refinement fetches and its value fetch are not counted); shaded_samples = pixels with a hit;
 * skipped_samples = 0.
 *
 * Errors: VR_EINVAL, with the output untouched, for a NULL argument, an unknown kind, for
 * VR_HIT_OPACITY a threshold that is NaN, <= 0 or > 1, use_rect other than 0 or 1, an empty
 * rectangle or one beyond the framebuffer, for vr_pick px >= W or py >= H, and whatever
 * vr_params and the camera every mode refuses.
 *
 * State.  The calls read the volume's base bricks only (every storage type and layout) and the
 * transfer function: they build, evict and downgrade nothing (vr_memory_report is unchanged) and
 * leave render mode, isovalue, slice box, TF and window alone -- a frame rendered before and
 * after them has identical bytes.  vr_timing_* brackets the kernel like a frame kernel, and
 * vr_debug_last_kernel_name names it.  A multi-device context (vr_create_mask) computes on its
 * lowest device, which holds a replica of the volume; nothing goes through vr_dist.
 * vr_hit_render_device is asynchronous on `stream`, as vr_mpr_render_device; the other three are
 * synchronous.
 */
#ifndef VR_VR_HIT_H
#define VR_VR_HIT_H

#include "vr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum vr_hit_kind { VR_HIT_ENTRY = 0, VR_HIT_OPACITY = 1, VR_HIT_MAX = 2, VR_HIT_MIN = 3, VR_HIT_ISO = 4 };

typedef struct vr_hit_request {
    int32_t  kind;        /* vr_hit_kind */
    float    threshold;   /* VR_HIT_OPACITY only: accumulated opacity in (0, 1]; ignored otherwise */
    uint32_t use_rect;    /* 0: the whole framebuffer; 1: the pixel rectangle below */
    uint32_t rect[4];     /* x0, y0, w, h: w, h >= 1, x0 + w <= W, y0 + h <= H */
} vr_hit_request;         /* 28 bytes */

typedef struct vr_hit {
    float    pos[3];  /* texture coordinates of the point: the march's f32 `pos`, bit for bit */
    float    depth;   /* distance camera -> point, world units (above); miss: +INFINITY */
    float    value;   /* the density the kind found there (above) */
    uint32_t step;    /* loop index k of the sample that made the hit; miss: 0xFFFFFFFF */
} vr_hit;             /* 24 bytes; a miss is {0,0,0, +INFINITY, 0, 0xFFFFFFFF} exactly */

/* Synchronous: w * h records into out_host. */
int vr_hit_render(vr_ctx *ctx, const vr_camera *cam, const vr_params *params,
                  const vr_hit_request *req, vr_hit *out_host);
/* Asynchronous on `stream`: w * h records into device memory. */
int vr_hit_render_device(vr_ctx *ctx, const vr_camera *cam, const vr_params *params,
                         const vr_hit_request *req, void *out_dev, void *stream);
int vr_hit_count_work(vr_ctx *ctx, const vr_camera *cam, const vr_params *params,
                      const vr_hit_request *req, vr_stats *out);
/* One pixel: the record of (px, py); the rectangle in *req is ignored.  Launches one tile, not a
 * frame. */
int vr_pick(vr_ctx *ctx, const vr_camera *cam, const vr_params *params, const vr_hit_request *req,
            uint32_t px, uint32_t py, vr_hit *out);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_HIT_H */
