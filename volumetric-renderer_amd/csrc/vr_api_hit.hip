// vr_api_hit.hip — hit records and picking (include/vr/vr_hit.h) on the host scaffold of vr_ctx.h.
#include "vr_ctx.h"
#include "vr_hit_host.h"

namespace {
// What vr_hit.h refuses before it looks at the context: the NULL arguments and the request's own
// fields (csrc/vr_hit_host.h); no HIP call.
int check_hit_request(vr_ctx *c, const vr_camera *cam, const vr_params *p, const vr_hit_request *req,
                      const void *out)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    if (!cam || !p || !req || !out) return fail(c, VR_EINVAL, "NULL argument");
    if (const char *m = hit_kind_error(req->kind, req->threshold)) return fail(c, VR_EINVAL, m);
    if (req->use_rect > 1) return fail(c, VR_EINVAL, "hit use_rect must be 0 or 1");
    return VR_OK;
}

// The kernel arguments of rectangle r; c is a single-device context.  build_params does the
// camera and parameter checks and the ray constants of the whole framebuffer; the rectangle then
// replaces the image the tiles cover (vr_internal.h HitArgs).  The view facts build_params notes
// for the next frame's policy are put back: a hit image is no frame.
int build_hit(vr_ctx *c, const vr_camera *cam, const vr_params *p, const vr_hit_request *req,
              const HitRect &r, void *out, MarchParams &P, HitArgs &A)
{
    const bool dense_rows = c->dense_rows;
    const double pixel_span = c->pixel_span, axis_align = c->axis_align, row_align = c->row_align;
    const int ray_axis = c->ray_axis;
    const int rc = build_params(c, cam, p, nullptr, VR_OUT_RGBA8, 16, 0, 1, RowShare{1, 1}, P);
    c->dense_rows = dense_rows;
    c->pixel_span = pixel_span;
    c->axis_align = axis_align;
    c->row_align = row_align;
    c->ray_axis = ray_axis;
    if (rc) return rc;
    if ((unsigned long long)((r.w + 15ull) / 16) * ((r.h + kMarchRows - 1ull) / kMarchRows) >= 1ull << 31)
        return fail(c, VR_EINVAL, "hit rectangle too large");
    P.W = r.w;
    P.H = r.h;
    P.local_rows = r.h;
    P.out_bytes = 0;
    P.tiles_x = (r.w + 15) / 16;
    P.tiles_y = (r.h + kMarchRows - 1) / kMarchRows;
    P.tile_order = 3;  // the static super-tiles: the adaptive order's cost table is the frames'
    P.supers_x = (P.tiles_x + kSuper - 1) / kSuper;
    P.supers_total = P.supers_x * ((P.tiles_y + kSuper - 1) / kSuper);
    P.pipelined = 0;
    A.out = out;
    A.out_bytes = hit_bytes(r);
    A.threshold = req->threshold;
    A.iso = c->isovalue;
    A.x0 = r.x0;
    A.y0 = r.y0;
    return VR_OK;
}

int hit_inflight(const vr_ctx *c, int kind)
{
    return c->knobs.hit_inflight == 1 || c->knobs.hit_inflight == 2 ? c->knobs.hit_inflight
                                                                      : kHitDefaultInFlight(kind);
}

// The hit launch on `stream`, bracketed by the timing events like a frame kernel.  It reads the
// base bricks and the TF only (a swap of either waits for the device first), so it takes part in
// no build, eviction or frame fence.
int hit_launch(vr_ctx *c, const vr_camera *cam, const vr_params *p, const vr_hit_request *req,
               const HitRect &r, void *out_dev, hipStream_t s)
{
    MarchParams P;
    HitArgs A;
    if (int rc = build_hit(c, cam, p, req, r, out_dev, P, A)) return rc;
    HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    Interval timed;
    if (int rc = timed.begin(c, s)) return rc;
    std::string name;
    HIP_TRY(c, launch_hit(c->layout, req->kind, false, hit_inflight(c, req->kind), P, A, s, &name),
            "hit kernel launch");
    c->last_mpr_name = name;
    return timed.end();
}

// The synchronous calls: the records of r through the context's own device buffer into out.
int hit_to_host(vr_ctx *c, const vr_camera *cam, const vr_params *p, const vr_hit_request *req,
                const HitRect &r, vr_hit *out)
{
    {  // the camera and parameter checks, before the buffer is sized by the rectangle
        MarchParams P;
        HitArgs A;
        if (int rc = build_hit(c, cam, p, req, r, nullptr, P, A)) return rc;
    }
    HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t bytes = (size_t)hit_bytes(r);
    // (no wait: its last records were copied out synchronously)
    if (int rc = reserve(c, c->hit_dev, bytes, "hipMalloc(hit records)", nullptr)) return rc;
    if (int rc = hit_launch(c, cam, p, req, r, c->hit_dev.p, nullptr)) return rc;
    HIP_TRY(c, hipMemcpy(out, c->hit_dev.p, bytes, hipMemcpyDeviceToHost), "hipMemcpy(hit records)");
    return VR_OK;
}
}  // namespace

extern "C" {

int vr_hit_render_device(vr_ctx *c, const vr_camera *cam, const vr_params *p, const vr_hit_request *req,
                         void *out_dev, void *stream)
{
    if (int rc = check_hit_request(c, cam, p, req, out_dev)) return rc;
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) { return vr_hit_render_device(m, cam, p, req, out_dev, stream); });
    HitRect r;
    if (const char *m = hit_rect_resolve(req->use_rect, req->rect, c->width, c->height, &r))
        return fail(c, VR_EINVAL, m);
    return hit_launch(c, cam, p, req, r, out_dev, static_cast<hipStream_t>(stream));
}

int vr_hit_render(vr_ctx *c, const vr_camera *cam, const vr_params *p, const vr_hit_request *req,
                  vr_hit *out)
{
    if (int rc = check_hit_request(c, cam, p, req, out)) return rc;
    if (is_group(c)) return on_replica(c, [&](vr_ctx *m) { return vr_hit_render(m, cam, p, req, out); });
    HitRect r;
    if (const char *m = hit_rect_resolve(req->use_rect, req->rect, c->width, c->height, &r))
        return fail(c, VR_EINVAL, m);
    return hit_to_host(c, cam, p, req, r, out);
}

int vr_pick(vr_ctx *c, const vr_camera *cam, const vr_params *p, const vr_hit_request *req,
            uint32_t px, uint32_t py, vr_hit *out)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    if (!cam || !p || !req || !out) return fail(c, VR_EINVAL, "NULL argument");
    // (the request's rectangle is ignored, use_rect with it)
    if (const char *m = hit_kind_error(req->kind, req->threshold)) return fail(c, VR_EINVAL, m);
    if (is_group(c)) return on_replica(c, [&](vr_ctx *m) { return vr_pick(m, cam, p, req, px, py, out); });
    HitRect r;
    if (const char *m = hit_pick_resolve(px, py, c->width, c->height, &r)) return fail(c, VR_EINVAL, m);
    return hit_to_host(c, cam, p, req, r, out);
}

int vr_hit_count_work(vr_ctx *c, const vr_camera *cam, const vr_params *p, const vr_hit_request *req,
                      vr_stats *out)
{
    if (int rc = check_hit_request(c, cam, p, req, out)) return rc;
    if (is_group(c)) return on_replica(c, [&](vr_ctx *m) { return vr_hit_count_work(m, cam, p, req, out); });
    HitRect r;
    if (const char *m = hit_rect_resolve(req->use_rect, req->rect, c->width, c->height, &r))
        return fail(c, VR_EINVAL, m);
    MarchParams P;
    HitArgs A;  // (the counting kernel writes no record)
    if (int rc = build_hit(c, cam, p, req, r, nullptr, P, A)) return rc;
    HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    HIP_TRY(c, hipMemset(c->counters, 0, 8 * sizeof(unsigned long long)), "hipMemset(counters)");
    std::string name;
    HIP_TRY(c, launch_hit(c->layout, req->kind, true, 1, P, A, nullptr, &name), "hit (count) launch");
    c->last_mpr_name = name;
    return read_counters(c, out);
}

}  // extern "C"
