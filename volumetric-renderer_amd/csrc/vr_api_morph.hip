// vr_api_morph.hip — the exact distance transform of a mask and ball morphology (include/vr/
// vr_morph.h) on the host scaffold of vr_ctx.h.  Built into lib/libvr_amd_morph.so, which takes
// the scaffold (fail, hip_fail, reserve, pooled_event, the group's wait) from libvr_amd.so.
#include "vr_ctx.h"
#include "../../include/vr/vr_morph.h"
#include "vr_morph_kernels.h"

namespace {
static_assert(VR_EDT_NONE == kMorphNone && VR_MORPH_MAX_EXTENT == kMorphMaxExtent && VR_EINVAL == kMorphEinval &&
                  VR_ENOSPC == kMorphEnospc && VR_OK == kMorphOk && VR_MORPH_CLOSE + 1 == kMorphOps &&
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
    MorphGrid g;
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

// The host forms' device copies: the mask at the block's start, the result behind it, 4-byte aligned.
size_t io_result_offset(const MorphGrid &g, uint32_t elem_bytes) { return ((size_t)g.voxels * elem_bytes + 3) & ~(size_t)3; }
}  // namespace

extern "C" {

int vr_edt_squared_device(vr_ctx *c, const uint32_t ext[3], const void *mask_dev, uint32_t elem_bytes,
                          uint32_t target, void *dist2_dev, uint64_t dcap, vr_edt_info *info, void *stream)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    MorphRun R{c, static_cast<hipStream_t>(stream)};
    const char *msg;
    const int rc = morph_check_edt(ext, mask_dev, elem_bytes, target, dist2_dev, dcap, info, true, &R.g, &msg);
    if (rc == VR_ENOSPC) {
        *info = vr_edt_info{R.g.voxels};  // known on the host: the voxels alone, every other field 0
    }
    if (rc) return fail(c, rc, msg);
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) {
            return vr_edt_squared_device(m, ext, mask_dev, elem_bytes, target, dist2_dev, dcap, info, stream);
        });
    vr_edt_info I;
    if (int rc2 = R.edt(mask_dev, elem_bytes, target, dist2_dev, &I)) return rc2;
    *info = I;
    return VR_OK;
}

int vr_edt_squared(vr_ctx *c, const uint32_t ext[3], const void *mask_host, uint32_t elem_bytes, uint32_t target,
                   uint32_t *dist2_host, uint64_t dcap, vr_edt_info *info)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    MorphRun R{c, nullptr};
    const char *msg;
    const int rc = morph_check_edt(ext, mask_host, elem_bytes, target, dist2_host, dcap, info, false, &R.g, &msg);
    if (rc == VR_ENOSPC) *info = vr_edt_info{R.g.voxels};
    if (rc) return fail(c, rc, msg);
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) {
            return vr_edt_squared(m, ext, mask_host, elem_bytes, target, dist2_host, dcap, info);
        });
    HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t in_bytes = (size_t)R.g.voxels * elem_bytes, off = io_result_offset(R.g, elem_bytes);
    if (int rc2 = reserve(c, c->morph_io_dev, off + (size_t)R.g.voxels * 4, "hipMalloc(morph staging)", kMorphIdle))
        return rc2;
    char *io = static_cast<char *>(c->morph_io_dev.p);
    HIP_TRY(c, hipMemcpy(io, mask_host, in_bytes, hipMemcpyHostToDevice), "hipMemcpy(mask)");
    vr_edt_info I;
    if (int rc2 = R.edt(io, elem_bytes, target, io + off, &I)) return rc2;
    HIP_TRY(c, hipMemcpy(dist2_host, io + off, (size_t)R.g.voxels * 4, hipMemcpyDeviceToHost), "hipMemcpy(dist2)");
    *info = I;
    return VR_OK;
}

int vr_mask_morph_device(vr_ctx *c, const uint32_t ext[3], uint32_t op, uint32_t r2, const void *mask_dev,
                         uint32_t elem_bytes, void *out_dev, uint64_t mcap, vr_morph_info *info, void *stream)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    MorphRun R{c, static_cast<hipStream_t>(stream)};
    const char *msg;
    const int rc = morph_check_morph(ext, op, r2, mask_dev, elem_bytes, out_dev, mcap, info, true, &R.g, &msg);
    if (rc == VR_ENOSPC) *info = vr_morph_info{R.g.voxels};
    if (rc) return fail(c, rc, msg);
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) {
            return vr_mask_morph_device(m, ext, op, r2, mask_dev, elem_bytes, out_dev, mcap, info, stream);
        });
    vr_morph_info I;
    if (int rc2 = R.morph(op, r2, mask_dev, elem_bytes, out_dev, &I)) return rc2;
    *info = I;
    return VR_OK;
}

int vr_mask_morph(vr_ctx *c, const uint32_t ext[3], uint32_t op, uint32_t r2, const void *mask_host,
                  uint32_t elem_bytes, uint8_t *out_host, uint64_t mcap, vr_morph_info *info)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    MorphRun R{c, nullptr};
    const char *msg;
    const int rc = morph_check_morph(ext, op, r2, mask_host, elem_bytes, out_host, mcap, info, false, &R.g, &msg);
    if (rc == VR_ENOSPC) *info = vr_morph_info{R.g.voxels};
    if (rc) return fail(c, rc, msg);
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) {
            return vr_mask_morph(m, ext, op, r2, mask_host, elem_bytes, out_host, mcap, info);
        });
    HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t in_bytes = (size_t)R.g.voxels * elem_bytes, off = io_result_offset(R.g, elem_bytes);
    if (int rc2 = reserve(c, c->morph_io_dev, off + (size_t)R.g.voxels, "hipMalloc(morph staging)", kMorphIdle))
        return rc2;
    char *io = static_cast<char *>(c->morph_io_dev.p);
    HIP_TRY(c, hipMemcpy(io, mask_host, in_bytes, hipMemcpyHostToDevice), "hipMemcpy(mask)");
    vr_morph_info I;
    if (int rc2 = R.morph(op, r2, io, elem_bytes, io + off, &I)) return rc2;
    HIP_TRY(c, hipMemcpy(out_host, io + off, (size_t)R.g.voxels, hipMemcpyDeviceToHost), "hipMemcpy(morph mask)");
    *info = I;
    return VR_OK;
}

const char *vr_morph_last_kernel_name(const vr_ctx *c)
{
    if (!c) return "";
    if (is_group(c)) return vr_morph_last_kernel_name(c->members[0]);
    return c->morph_last_name;
}

}  // extern "C"
