// vr_api_morph.hip — the exact distance transform of a mask and ball morphology (include/vr/
// vr_morph.h) on the host scaffold of vr_ctx.h and vr_mask_call.h.  Built into lib/libvr_amd_morph.so, which takes
// the scaffold (fail, hip_fail, reserve, pooled_event, the group's wait) from libvr_amd.so.
#include "vr_mask_call.h"
#include "../../include/vr/vr_morph.h"
#include "vr_morph_kernels.h"

namespace {
static_assert(VR_EDT_NONE == kMorphNone && VR_MORPH_MAX_EXTENT == kMaskMaxExtent && VR_MORPH_CLOSE + 1 == kMorphOps &&
                  VR_EDT_TO_UNSET + 1 == kMorphTargets && sizeof(vr_edt_info) == 24 && sizeof(vr_morph_info) == 24,
              "vr_morph.h");

// The context's blocks of this family grow behind a wait for the device: an earlier call's passes
// may still read the old block on another stream (reserve's idle_first).
constexpr const char *kMorphIdle = "hipDeviceSynchronize (morph scratch)";
constexpr size_t kMorphCntBytes = 8 * sizeof(unsigned long long);  // two transforms' four words

// One call's transforms on stream s; c is a single-device context.
struct MorphRun {
    vr_ctx *c;
    hipStream_t s;
    MaskGrid g;
    Interval timed;
    int runs = 0;  // transforms so far: transform r counts into words 4 r ..

    int begin()
    {
        HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
        if (int rc = reserve(c, c->morph_cnt_dev, kMorphCntBytes, "hipMalloc(morph counters)", kMorphIdle)) return rc;
        HIP_TRY(c, hipMemsetAsync(c->morph_cnt_dev.p, 0, kMorphCntBytes, s), "hipMemset(morph counters)");
        return VR_OK;
    }
    // One transform, a timed interval: the distance to the set (or unset) voxels of `mask` into dist;
    // fin kMorphEdt leaves it there, kMorphThresh writes (dist2 <= limit) != invert into out.
    int transform(const void *mask, uint32_t elem_bytes, bool to_unset, uint32_t limit, void *dist, MorphFinal fin,
                  void *out, bool invert)
    {
        MorphArgs A;
        std::memset(&A, 0, sizeof A);
        A.mask = mask;
        A.dist = static_cast<uint32_t *>(dist);
        A.out = static_cast<uint8_t *>(out);
        A.cnt = static_cast<unsigned long long *>(c->morph_cnt_dev.p) + 4 * runs++;
        for (int a = 0; a < 3; ++a) A.ext[a] = g.ext[a];
        A.elem_bytes = elem_bytes;
        A.to_unset = to_unset;
        A.limit = limit;
        A.invert = invert;
        if (int rc = timed.begin(c, s)) return rc;
        HIP_TRY(c, launch_morph_edt_x(A, g, s, &c->morph_last_name), "morph launch (x)");
        HIP_TRY(c, launch_morph_edt_axis(A, g, 1, kMorphStore, s, &c->morph_last_name), "morph launch (y)");
        HIP_TRY(c, launch_morph_edt_axis(A, g, 2, fin, s, &c->morph_last_name), "morph launch (z)");
        return timed.end();
    }
    // The counters to the host (waits for s).
    int counts(unsigned long long h[8])
    {
        HIP_TRY(c, hipMemcpyAsync(h, c->morph_cnt_dev.p, kMorphCntBytes, hipMemcpyDeviceToHost, s),
                "hipMemcpy(morph counters)");
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(morph)");
        return VR_OK;
    }

    int edt(const void *mask, uint32_t elem_bytes, uint32_t target, void *dist, vr_edt_info *I)
    {
        if (int rc = begin()) return rc;
        if (int rc = transform(mask, elem_bytes, target == VR_EDT_TO_UNSET, kMorphNone - 1u, dist, kMorphEdt, nullptr,
                               false))
            return rc;
        unsigned long long h[8];
        if (int rc = counts(h)) return rc;
        std::memset(I, 0, sizeof *I);
        I->voxels = g.voxels;
        I->target_voxels = target == VR_EDT_TO_UNSET ? g.voxels - h[0] : h[0];
        I->max_dist2 = h[1] ? (uint32_t)(h[1] >> 32) : VR_EDT_NONE;  // (a key is never 0: an index is below 2^32 - 1)
        I->max_index = h[1] ? ~(uint32_t)h[1] : 0u;
        return VR_OK;
    }

    int morph(uint32_t op, uint32_t r2, const void *mask, uint32_t elem_bytes, void *out, vr_morph_info *I)
    {
        if (int rc = begin()) return rc;
        if (int rc = reserve(c, c->morph_dist_dev, (size_t)g.voxels * 4, "hipMalloc(morph distance)", kMorphIdle))
            return rc;
        void *dist = c->morph_dist_dev.p;
        // a dilation thresholds the distance to the set voxels, an erosion that to the unset ones
        const bool erode_first = op == VR_MORPH_ERODE || op == VR_MORPH_OPEN;
        if (op == VR_MORPH_DILATE || op == VR_MORPH_ERODE) {
            if (int rc = transform(mask, elem_bytes, erode_first, r2, dist, kMorphThresh, out, erode_first)) return rc;
        } else {
            if (int rc = reserve(c, c->morph_tmp_dev, (size_t)g.voxels, "hipMalloc(morph intermediate mask)", kMorphIdle))
                return rc;
            void *tmp = c->morph_tmp_dev.p;
            if (int rc = transform(mask, elem_bytes, erode_first, r2, dist, kMorphThresh, tmp, erode_first)) return rc;
            if (int rc = transform(tmp, 1, !erode_first, r2, dist, kMorphThresh, out, !erode_first)) return rc;
        }
        unsigned long long h[8];
        if (int rc = counts(h)) return rc;
        std::memset(I, 0, sizeof *I);
        I->voxels = g.voxels;
        I->in_set = h[0];
        I->out_set = h[4 * (runs - 1) + 2];
        return VR_OK;
    }
};

}  // namespace

extern "C" {

int vr_edt_squared_device(vr_ctx *c, const uint32_t ext[3], const void *mask_dev, uint32_t elem_bytes,
                          uint32_t target, void *dist2_dev, uint64_t dcap, vr_edt_info *info, void *stream)
{
    MorphRun R{c, static_cast<hipStream_t>(stream)};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return morph_check_edt(ext, mask_dev, elem_bytes, target, dist2_dev, dcap, info, true, &R.g, msg);
        },
        [&](vr_ctx *m) {
            return vr_edt_squared_device(m, ext, mask_dev, elem_bytes, target, dist2_dev, dcap, info, stream);
        },
        nullptr, [&](vr_edt_info *I) { return R.edt(mask_dev, elem_bytes, target, dist2_dev, I); });
}

int vr_edt_squared(vr_ctx *c, const uint32_t ext[3], const void *mask_host, uint32_t elem_bytes, uint32_t target,
                   uint32_t *dist2_host, uint64_t dcap, vr_edt_info *info)
{
    MorphRun R{c, nullptr};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return morph_check_edt(ext, mask_host, elem_bytes, target, dist2_host, dcap, info, false, &R.g, msg);
        },
        [&](vr_ctx *m) { return vr_edt_squared(m, ext, mask_host, elem_bytes, target, dist2_host, dcap, info); }, nullptr,
        [&](vr_edt_info *I) {
            MaskStage S{c};
            if (int rc = S.begin(c->morph_io_dev, "hipMalloc(morph staging)", kMorphIdle,
                                 {mask_host, (size_t)R.g.voxels * elem_bytes, "hipMemcpy(mask)"}, {},
                                 (size_t)R.g.voxels * 4))
                return rc;
            if (int rc = R.edt(S.in[0], elem_bytes, target, S.out, I)) return rc;
            return S.finish(dist2_host, "hipMemcpy(dist2)");
        });
}

int vr_mask_morph_device(vr_ctx *c, const uint32_t ext[3], uint32_t op, uint32_t r2, const void *mask_dev,
                         uint32_t elem_bytes, void *out_dev, uint64_t mcap, vr_morph_info *info, void *stream)
{
    MorphRun R{c, static_cast<hipStream_t>(stream)};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return morph_check_morph(ext, op, r2, mask_dev, elem_bytes, out_dev, mcap, info, true, &R.g, msg);
        },
        [&](vr_ctx *m) { return vr_mask_morph_device(m, ext, op, r2, mask_dev, elem_bytes, out_dev, mcap, info, stream); },
        nullptr, [&](vr_morph_info *I) { return R.morph(op, r2, mask_dev, elem_bytes, out_dev, I); });
}

int vr_mask_morph(vr_ctx *c, const uint32_t ext[3], uint32_t op, uint32_t r2, const void *mask_host,
                  uint32_t elem_bytes, uint8_t *out_host, uint64_t mcap, vr_morph_info *info)
{
    MorphRun R{c, nullptr};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return morph_check_morph(ext, op, r2, mask_host, elem_bytes, out_host, mcap, info, false, &R.g, msg);
        },
        [&](vr_ctx *m) { return vr_mask_morph(m, ext, op, r2, mask_host, elem_bytes, out_host, mcap, info); }, nullptr,
        [&](vr_morph_info *I) {
            MaskStage S{c};
            if (int rc = S.begin(c->morph_io_dev, "hipMalloc(morph staging)", kMorphIdle,
                                 {mask_host, (size_t)R.g.voxels * elem_bytes, "hipMemcpy(mask)"}, {}, (size_t)R.g.voxels))
                return rc;
            if (int rc = R.morph(op, r2, S.in[0], elem_bytes, S.out, I)) return rc;
            return S.finish(out_host, "hipMemcpy(morph mask)");
        });
}

const char *vr_morph_last_kernel_name(const vr_ctx *c) { return mask_last_kernel_name(c, &vr_ctx::morph_last_name); }

}  // extern "C"
