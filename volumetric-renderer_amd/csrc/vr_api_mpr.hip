// vr_api_mpr.hip — multi-planar reformat (include/vr/vr_mpr.h) on the host scaffold of vr_ctx.h.
#include "vr_ctx.h"

namespace {
// the plane's own errors (vr_mpr.h); c may be NULL (vr_mpr_axis_plane)
int check_plane_shape(vr_ctx *c, uint32_t width, uint32_t height, uint32_t nsamples, int op)
{
    if (width == 0 || height == 0) return fail(c, VR_EINVAL, "mpr image size must be non-zero");
    if ((unsigned long long)((width + 15ull) / 16) * ((height + 15ull) / 16) >= 1ull << 31)
        return fail(c, VR_EINVAL, "mpr image too large");
    if (nsamples == 0 || nsamples > VR_MPR_MAX_SAMPLES)
        return fail(c, VR_EINVAL, "mpr nsamples must be in [1, 4096]");
    if (op != VR_MPR_MAX && op != VR_MPR_MIN && op != VR_MPR_MEAN)
        return fail(c, VR_EINVAL, "unknown mpr op");
    return VR_OK;
}

// Everything vr_mpr.h refuses, then the kernel's argument; c is a single-device context.
int build_mpr(vr_ctx *c, const vr_mpr_plane *pl, const vr_params *p, void *out, int out_format,
              MprArgs &A)
{
    if (!pl) return fail(c, VR_EINVAL, "plane is NULL");
    if (int rc = check_params(c, p)) return rc;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(pl->origin[a]) || !std::isfinite(pl->du[a]) || !std::isfinite(pl->dv[a]) ||
            !std::isfinite(pl->dn[a]))
            return fail(c, VR_EINVAL, "mpr plane vectors must be finite");
    if (int rc = check_plane_shape(c, pl->width, pl->height, pl->nsamples, pl->op)) return rc;
    if (out_format != VR_OUT_RGBA8 && out_format != VR_OUT_RGBA32F)
        return fail(c, VR_EINVAL, "unknown out_format");
    std::memset(&A, 0, sizeof(A));
    A.vol = c->bricks;
    A.vol_bytes = c->brick_bytes;
    A.tf = c->tf;
    A.out = out;
    A.counters = c->counters;
    for (int a = 0; a < 3; ++a) {
        A.origin[a] = (double)pl->origin[a];
        A.du[a] = (double)pl->du[a];
        A.dv[a] = (double)pl->dv[a];
        A.dn[a] = (double)pl->dn[a];
        A.smin[a] = c->smin[a];
        A.smax[a] = c->smax[a];
    }
    A.half_w = 0.5 * (double)pl->width;
    A.half_h = 0.5 * (double)pl->height;
    A.half_n = 0.5 * (double)(pl->nsamples - 1);
    A.nbx = bricks_for(c->nx, 0, c->layout);
    A.nby = bricks_for(c->ny, 1, c->layout);
    A.fnx = (float)c->nx;
    A.fny = (float)c->ny;
    A.fnz = (float)c->nz;
    A.vmin = c->vmin;
    A.range = c->vmax - c->vmin;
    // (the frames' reciprocal division domain, build_params)
    A.div_fast = A.range >= 0x1p-40f && A.range < 0x1p100f && std::fabs(c->vmin) < 0x1p100f &&
                 std::fabs(c->vmax) < 0x1p100f;
    A.inv_range = A.div_fast ? 1.0f / A.range : 0.0f;
    A.tf_n = (int32_t)c->tf_n;
    A.tf_nf = (float)c->tf_n;
    for (int k = 0; k < 4; ++k) A.clear[k] = p->clear_color[k];
    A.W = pl->width;
    A.H = pl->height;
    A.nsamples = pl->nsamples;
    A.tiles_x = (pl->width + 15) / 16;
    A.tiles_y = (pl->height + 15) / 16;
    A.tile_order = c->knobs.tile_order == 1 || c->knobs.tile_order == 3 ? (uint32_t)c->knobs.tile_order
                                                                         : kMprTileOrder(pl->nsamples);
    A.supers_x = (A.tiles_x + kSuper - 1) / kSuper;
    A.supers_total = A.supers_x * ((A.tiles_y + kSuper - 1) / kSuper);
    A.out_format = out_format;
    A.op = pl->op;
    A.out_bytes = (unsigned long long)pl->width * pl->height * (out_format == VR_OUT_RGBA32F ? 16 : 4);
    return VR_OK;
}

// The MPR launch on `stream`, bracketed by the timing events like a frame kernel.  It reads the
// base bricks and the TF only (a swap of either waits for the device first), so it takes part in
// no build, eviction or frame fence.
int mpr_render_device_impl(vr_ctx *c, const vr_mpr_plane *pl, const vr_params *p, void *out_dev,
                           int out_format, void *stream)
{
    MprArgs A;
    if (int rc = build_mpr(c, pl, p, out_dev, out_format, A)) return rc;
    HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Interval timed;
    if (int rc = timed.begin(c, s)) return rc;
    std::string name;
    HIP_TRY(c, launch_mpr(c->layout, false, A, s, &name), "mpr kernel launch");
    c->last_mpr_name = name;
    return timed.end();
}
}  // namespace

extern "C" {

int vr_mpr_render_device(vr_ctx *c, const vr_mpr_plane *pl, const vr_params *p, void *out_dev,
                         int out_format, void *stream)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    if (!out_dev) return fail(c, VR_EINVAL, "output buffer is NULL");
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) { return vr_mpr_render_device(m, pl, p, out_dev, out_format, stream); });
    return mpr_render_device_impl(c, pl, p, out_dev, out_format, stream);
}

int vr_mpr_render(vr_ctx *c, const vr_mpr_plane *pl, const vr_params *p, void *out, int out_format)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    if (!out) return fail(c, VR_EINVAL, "output buffer is NULL");
    if (is_group(c)) return on_replica(c, [&](vr_ctx *m) { return vr_mpr_render(m, pl, p, out, out_format); });
    MprArgs A;  // the argument checks, before the staging image is sized by the plane
    if (int rc = build_mpr(c, pl, p, out, out_format, A)) return rc;
    HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t bytes = (size_t)A.out_bytes;
    // (no wait: its last image was copied out synchronously)
    if (int rc = reserve(c, c->mpr_dev, bytes, "hipMalloc(mpr image)", nullptr)) return rc;
    if (int rc = mpr_render_device_impl(c, pl, p, c->mpr_dev.p, out_format, nullptr)) return rc;
    HIP_TRY(c, hipMemcpy(out, c->mpr_dev.p, bytes, hipMemcpyDeviceToHost), "hipMemcpy(mpr image)");
    return VR_OK;
}

int vr_mpr_count_work(vr_ctx *c, const vr_mpr_plane *pl, const vr_params *p, vr_stats *out)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    if (!out) return fail(c, VR_EINVAL, "stats is NULL");
    if (is_group(c)) return on_replica(c, [&](vr_ctx *m) { return vr_mpr_count_work(m, pl, p, out); });
    MprArgs A;  // (the counting kernel writes no pixel: no output, any format)
    if (int rc = build_mpr(c, pl, p, nullptr, VR_OUT_RGBA8, A)) return rc;
    HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    HIP_TRY(c, hipMemset(c->counters, 0, 8 * sizeof(unsigned long long)), "hipMemset(counters)");
    std::string name;
    HIP_TRY(c, launch_mpr(c->layout, true, A, nullptr, &name), "mpr (count) launch");
    c->last_mpr_name = name;
    return read_counters(c, out);
}

int vr_mpr_axis_plane(int axis, float position, uint32_t width, uint32_t height, uint32_t nsamples,
                      float spacing, int op, vr_mpr_plane *out)
{
    if (!out) return fail(nullptr, VR_EINVAL, "plane is NULL");
    if (axis < 0 || axis > 2) return fail(nullptr, VR_EINVAL, "mpr axis must be 0, 1 or 2");
    if (!std::isfinite(position) || !std::isfinite(spacing))
        return fail(nullptr, VR_EINVAL, "mpr position and spacing must be finite");
    if (int rc = check_plane_shape(nullptr, width, height, nsamples, op)) return rc;
    vr_mpr_plane pl;
    std::memset(&pl, 0, sizeof pl);
    for (int a = 0; a < 3; ++a) pl.origin[a] = a == axis ? position : 0.5f;
    pl.dn[axis] = spacing;
    const float ru = 1.0f / (float)width, rv = 1.0f / (float)height;
    if (axis == 2) {  // axial: right +x, down +y
        pl.du[0] = ru;
        pl.dv[1] = rv;
    } else {  // coronal: right +x; sagittal: right +y; both down -z (world +z is screen-up)
        pl.du[axis == 1 ? 0 : 1] = ru;
        pl.dv[2] = -rv;
    }
    pl.width = width;
    pl.height = height;
    pl.nsamples = nsamples;
    pl.op = op;
    *out = pl;
    return VR_OK;
}

}  // extern "C"
