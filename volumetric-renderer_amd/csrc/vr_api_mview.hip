// vr_api_mview.hip — the view of a device mask or label array (include/vr/vr_mview.h): its occupancy
// words, its first-hit records, the pick and the slice, on the host scaffold of vr_ctx.h and
// vr_mask_call.h.  Built into lib/libvr_amd_mview.so, which takes the scaffold (fail, hip_fail,
// reserve, pooled_event, build_params, the group's wait) from libvr_amd.so.
#include "vr_mask_call.h"
#include "../../include/vr/vr_mview.h"
#include "vr_mview_kernels.h"

#include <cstddef>

namespace {
static_assert(VR_MVIEW_MAX_EXTENT == kMaskMaxExtent && VR_MVIEW_CELL == kMviewCell && VR_MVIEW_ANY == kMviewAny &&
                  VR_MVIEW_LABEL == kMviewLabel && sizeof(vr_mask_hit) == kMviewHitBytes && sizeof(vr_mview_info) == 48 &&
                  sizeof(vr_mview_occ_info) == 32 && VR_MPR_MAX_SAMPLES == kMviewMaxSamples,
              "vr_mview.h");
static_assert(sizeof(vr_mview_source) == sizeof(MviewSource) && offsetof(vr_mview_source, origin) == offsetof(MviewSource, origin) &&
                  offsetof(vr_mview_source, elem_bytes) == offsetof(MviewSource, elem_bytes) &&
                  offsetof(vr_mview_source, select) == offsetof(MviewSource, select) &&
                  offsetof(vr_mview_source, label) == offsetof(MviewSource, label) &&
                  offsetof(vr_mview_source, reserved) == offsetof(MviewSource, reserved) &&
                  offsetof(vr_mview_source, array) == offsetof(MviewSource, array) &&
                  offsetof(vr_mview_source, occupancy) == offsetof(MviewSource, occupancy),
              "vr_mview_source");
static_assert(sizeof(vr_mpr_plane) == sizeof(MviewPlane) && offsetof(vr_mpr_plane, du) == offsetof(MviewPlane, du) &&
                  offsetof(vr_mpr_plane, dv) == offsetof(MviewPlane, dv) && offsetof(vr_mpr_plane, dn) == offsetof(MviewPlane, dn) &&
                  offsetof(vr_mpr_plane, width) == offsetof(MviewPlane, width) &&
                  offsetof(vr_mpr_plane, height) == offsetof(MviewPlane, height) &&
                  offsetof(vr_mpr_plane, nsamples) == offsetof(MviewPlane, nsamples) &&
                  offsetof(vr_mpr_plane, op) == offsetof(MviewPlane, op),
              "vr_mpr_plane");

const MviewSource *as_source(const vr_mview_source *s) { return reinterpret_cast<const MviewSource *>(s); }
const MviewPlane *as_plane(const vr_mpr_plane *p) { return reinterpret_cast<const MviewPlane *>(p); }

// The context's blocks of this family grow behind a wait for the device (reserve's idle_first).
constexpr const char *kMviewIdle = "hipDeviceSynchronize (mview scratch)";

// One call's kernel on stream s; c is a single-device context.  The timing events bracket the
// counters' memset and the kernel as one interval.
struct MviewRun {
    vr_ctx *c;
    hipStream_t s;
    MaskGrid g;
    HitRect r{0, 0, 0, 0};
    MarchParams P;
    Interval timed;

    // What needs the context: a volume, and the grid inside it.  Before any output or scratch.
    int admit()
    {
        if (!c->bricks) return fail(c, VR_EINVAL, "mask view: no volume");
        const uint32_t dims[3] = {c->nx, c->ny, c->nz};
        if (const char *m = mview_origin_error(g, dims)) return fail(c, VR_EINVAL, m);
        return VR_OK;
    }
    // admit(), then the camera and parameter checks and the ray constants of the whole framebuffer.
    // The view facts build_params notes for the next frame's policy are put back: a hit image is no
    // frame (csrc/vr_api_hit.hip).
    int admit_view(const vr_camera *cam, const vr_params *p)
    {
        if (int rc = admit()) return rc;
        const bool dense_rows = c->dense_rows;
        const double pixel_span = c->pixel_span, axis_align = c->axis_align, row_align = c->row_align;
        const int ray_axis = c->ray_axis;
        const int rc = build_params(c, cam, p, nullptr, VR_OUT_RGBA8, 16, 0, 1, RowShare{1, 1}, P);
        c->dense_rows = dense_rows;
        c->pixel_span = pixel_span;
        c->axis_align = axis_align;
        c->row_align = row_align;
        c->ray_axis = ray_axis;
        return rc;
    }
    MviewArray array_of(const vr_mview_source *src, const void *array, const void *occ) const
    {
        MviewArray S;
        std::memset(&S, 0, sizeof S);
        S.array = array;
        S.occ = static_cast<const uint32_t *>(occ);
        const uint32_t dims[3] = {c->nx, c->ny, c->nz};
        for (int a = 0; a < 3; ++a) {
            S.ext[a] = g.ext[a];
            S.origin[a] = g.origin[a];
            S.dims[a] = dims[a];
            S.fn[a] = (float)dims[a];
        }
        const MviewCells C = mview_cells(g.ext);
        S.c0 = C.c[0];
        S.c1 = C.c[1];
        S.select = src->select;
        S.label = src->label;
        return S;
    }
    // The counters zeroed on s, inside the interval: work the call needs.
    int begin(unsigned long long **cnt)
    {
        HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
        if (int rc = reserve(c, c->mview_cnt_dev, kMviewCounters * 8, "hipMalloc(mview counters)", kMviewIdle)) return rc;
        *cnt = static_cast<unsigned long long *>(c->mview_cnt_dev.p);
        if (int rc = timed.begin(c, s)) return rc;
        HIP_TRY(c, hipMemsetAsync(*cnt, 0, kMviewCounters * 8, s), "hipMemset(mview counters)");
        return VR_OK;
    }
    // The interval closed and the counters on the host (waits for s).
    int end(unsigned long long *cnt, unsigned long long h[kMviewCounters])
    {
        if (int rc = timed.end()) return rc;
        HIP_TRY(c, hipMemcpyAsync(h, cnt, kMviewCounters * 8, hipMemcpyDeviceToHost, s), "hipMemcpy(mview counters)");
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(mview)");
        return VR_OK;
    }

    int occupancy(const vr_mview_source *src, void *occ_dev, vr_mview_occ_info *I)
    {
        MviewOccArgs A;
        std::memset(&A, 0, sizeof A);
        A.S = array_of(src, src->array, nullptr);
        const MviewCells C = mview_cells(g.ext);
        A.words = static_cast<uint32_t *>(occ_dev);
        A.ncells = (uint32_t)C.cells;
        A.nwords = (uint32_t)C.words;
        if (int rc = begin(&A.cnt)) return rc;
        HIP_TRY(c, launch_mview_occupancy(src->elem_bytes, A, s, &c->mview_last_name), "mview occupancy launch");
        unsigned long long h[kMviewCounters];
        if (int rc = end(A.cnt, h)) return rc;
        std::memset(I, 0, sizeof *I);
        I->voxels = g.voxels;
        I->cells = C.cells;
        I->cells_set = h[kMviewCntCellsSet];
        I->matching = h[kMviewCntMatching];
        return VR_OK;
    }
    // The records of rectangle r; array, occ and out in device memory.  I may be NULL (the pick).
    int hits(const vr_mview_source *src, const void *array, const void *occ, void *out, vr_mview_info *I)
    {
        MviewHitArgs A;
        std::memset(&A, 0, sizeof A);
        A.S = array_of(src, array, occ);
        A.out = out;
        A.x0 = r.x0;
        A.y0 = r.y0;
        A.w = r.w;
        A.h = r.h;
        A.tiles_x = (r.w + 15) / 16;
        if (int rc = begin(&A.cnt)) return rc;
        HIP_TRY(c, launch_mview_hit(src->elem_bytes, P, A, (r.h + 15) / 16, s, &c->mview_last_name), "mview hit launch");
        unsigned long long h[kMviewCounters];
        if (int rc = end(A.cnt, h)) return rc;
        if (I) fill(I, (uint64_t)r.w * r.h, h);
        return VR_OK;
    }
    int slice(const vr_mpr_plane *pl, const vr_mview_source *src, const void *array, const void *occ, void *out,
              vr_mview_info *I)
    {
        MviewSliceArgs A;
        std::memset(&A, 0, sizeof A);
        A.S = array_of(src, array, occ);
        A.out = static_cast<uint32_t *>(out);
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
        A.W = pl->width;
        A.H = pl->height;
        A.nsamples = pl->nsamples;
        A.tiles_x = (pl->width + 15) / 16;
        if (int rc = begin(&A.cnt)) return rc;
        HIP_TRY(c, launch_mview_slice(src->elem_bytes, A, (pl->height + 15) / 16, s, &c->mview_last_name),
                "mview slice launch");
        unsigned long long h[kMviewCounters];
        if (int rc = end(A.cnt, h)) return rc;
        fill(I, (uint64_t)pl->width * pl->height, h);
        return VR_OK;
    }
    void fill(vr_mview_info *I, uint64_t pixels, const unsigned long long h[kMviewCounters]) const
    {
        std::memset(I, 0, sizeof *I);
        I->voxels = g.voxels;
        I->pixels = pixels;
        I->covered = h[kMviewCntCovered];
        I->hits = h[kMviewCntHits];
        I->steps = h[kMviewCntSteps];
        I->samples = h[kMviewCntSamples];
    }
};

}  // namespace

extern "C" {

uint64_t vr_mview_occupancy_words(const uint32_t ext[3]) { return mview_occupancy_words(ext); }

int vr_mask_occupancy_device(vr_ctx *c, const vr_mview_source *src, void *occ_dev, uint64_t ocap_words,
                             vr_mview_occ_info *info, void *stream)
{
    MviewRun R{c, static_cast<hipStream_t>(stream)};
    return mask_call(
        c, R.g, info, [&](const char **msg) { return mview_check_occupancy(as_source(src), occ_dev, ocap_words, info, &R.g, msg); },
        [&](vr_ctx *m) { return vr_mask_occupancy_device(m, src, occ_dev, ocap_words, info, stream); },
        [&] { return R.admit(); }, [&](vr_mview_occ_info *I) { return R.occupancy(src, occ_dev, I); });
}

int vr_mask_hit_render_device(vr_ctx *c, const vr_camera *cam, const vr_params *p, const vr_mview_source *src,
                              const uint32_t *rect, void *out_dev, uint64_t rcap, vr_mview_info *info, void *stream)
{
    MviewRun R{c, static_cast<hipStream_t>(stream)};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mview_check_hit(as_source(src), cam, p, rect, c->width, c->height, out_dev, rcap, info, sizeof *info, true,
                                   &R.g, &R.r, msg);
        },
        [&](vr_ctx *m) { return vr_mask_hit_render_device(m, cam, p, src, rect, out_dev, rcap, info, stream); },
        [&] { return R.admit_view(cam, p); },
        [&](vr_mview_info *I) { return R.hits(src, src->array, src->occupancy, out_dev, I); });
}

int vr_mask_hit_render(vr_ctx *c, const vr_camera *cam, const vr_params *p, const vr_mview_source *src,
                       const uint32_t *rect, vr_mask_hit *out_host, uint64_t rcap, vr_mview_info *info)
{
    MviewRun R{c, nullptr};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mview_check_hit(as_source(src), cam, p, rect, c->width, c->height, out_host, rcap, info, sizeof *info, false,
                                   &R.g, &R.r, msg);
        },
        [&](vr_ctx *m) { return vr_mask_hit_render(m, cam, p, src, rect, out_host, rcap, info); },
        [&] { return R.admit_view(cam, p); },
        [&](vr_mview_info *I) {
            MaskStage S{c};
            if (int rc = S.begin(c->mview_io_dev, "hipMalloc(mview staging)", kMviewIdle,
                                 {src->array, (size_t)R.g.voxels * src->elem_bytes, "hipMemcpy(array)"}, {},
                                 (size_t)R.r.w * R.r.h * kMviewHitBytes))
                return rc;
            if (int rc = R.hits(src, S.in[0], nullptr, S.out, I)) return rc;
            return S.finish(out_host, "hipMemcpy(mask hit records)");
        });
}

// vr_mask_pick: no info struct and no VR_ENOSPC, so written out on the pieces mask_call is made of.
int vr_mask_pick(vr_ctx *c, const vr_camera *cam, const vr_params *p, const vr_mview_source *src, uint32_t px,
                 uint32_t py, vr_mask_hit *out_host)
{
    if (!c) return null_ctx();
    MviewRun R{c, nullptr};
    const char *msg;
    if (int rc = mview_check_pick(as_source(src), cam, p, px, py, c->width, c->height, out_host, &R.g, &R.r, &msg))
        return fail(c, rc, msg);
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) { return vr_mask_pick(m, cam, p, src, px, py, out_host); });
    if (int rc = R.admit_view(cam, p)) return rc;
    MaskStage S{c};  // (no input: the array is the caller's device memory)
    if (int rc = S.begin(c->mview_io_dev, "hipMalloc(mview staging)", kMviewIdle, {}, {}, kMviewHitBytes)) return rc;
    if (int rc = R.hits(src, src->array, nullptr, S.out, nullptr)) return rc;
    return S.finish(out_host, "hipMemcpy(mask hit record)");
}

int vr_mask_slice_device(vr_ctx *c, const vr_mpr_plane *pl, const vr_mview_source *src, void *out_dev, uint64_t pcap,
                         vr_mview_info *info, void *stream)
{
    MviewRun R{c, static_cast<hipStream_t>(stream)};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mview_check_slice(as_source(src), as_plane(pl), out_dev, pcap, info, sizeof *info, true, &R.g, msg);
        },
        [&](vr_ctx *m) { return vr_mask_slice_device(m, pl, src, out_dev, pcap, info, stream); }, [&] { return R.admit(); },
        [&](vr_mview_info *I) { return R.slice(pl, src, src->array, src->occupancy, out_dev, I); });
}

int vr_mask_slice(vr_ctx *c, const vr_mpr_plane *pl, const vr_mview_source *src, uint32_t *out_host, uint64_t pcap,
                  vr_mview_info *info)
{
    MviewRun R{c, nullptr};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mview_check_slice(as_source(src), as_plane(pl), out_host, pcap, info, sizeof *info, false, &R.g, msg);
        },
        [&](vr_ctx *m) { return vr_mask_slice(m, pl, src, out_host, pcap, info); }, [&] { return R.admit(); },
        [&](vr_mview_info *I) {
            MaskStage S{c};
            if (int rc = S.begin(c->mview_io_dev, "hipMalloc(mview staging)", kMviewIdle,
                                 {src->array, (size_t)R.g.voxels * src->elem_bytes, "hipMemcpy(array)"}, {},
                                 (size_t)pl->width * pl->height * 4))
                return rc;
            if (int rc = R.slice(pl, src, S.in[0], nullptr, S.out, I)) return rc;
            return S.finish(out_host, "hipMemcpy(mask slice)");
        });
}

const char *vr_mview_last_kernel_name(const vr_ctx *c) { return mask_last_kernel_name(c, &vr_ctx::mview_last_name); }

}  // extern "C"
