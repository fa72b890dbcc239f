// vr_api_mmesh.hip — the surface of a device mask or label array as a triangle mesh
// (include/vr/vr_mmesh.h): the count pass, the capacity check that can only follow it, and the emit
// passes, on the host scaffold of vr_ctx.h and vr_mask_call.h.  Built into lib/libvr_amd_mmesh.so,
// which takes the scaffold (fail, hip_fail, reserve, pooled_event, the group's wait) from
// libvr_amd.so.
#include "vr_mask_call.h"
#include "../../include/vr/vr_mmesh.h"
#include "vr_mmesh_kernels.h"

#include <cstddef>

namespace {
static_assert(VR_MMESH_MAX_EXTENT == kMaskMaxExtent && VR_MMESH_MAX_ITERS == kMmeshMaxIters && VR_MVIEW_ANY == kMmeshAny &&
                  VR_MVIEW_LABEL == kMmeshLabel && sizeof(vr_mesh_vertex) == kMmeshVertexBytes && sizeof(vr_mmesh_info) == 32,
              "vr_mmesh.h");
static_assert(sizeof(vr_mmesh_request) == sizeof(MmeshRequest) && sizeof(vr_mmesh_request) == 64 &&
                  offsetof(vr_mmesh_request, origin) == offsetof(MmeshRequest, origin) &&
                  offsetof(vr_mmesh_request, elem_bytes) == offsetof(MmeshRequest, elem_bytes) &&
                  offsetof(vr_mmesh_request, select) == offsetof(MmeshRequest, select) &&
                  offsetof(vr_mmesh_request, label) == offsetof(MmeshRequest, label) &&
                  offsetof(vr_mmesh_request, closed) == offsetof(MmeshRequest, closed) &&
                  offsetof(vr_mmesh_request, normals) == offsetof(MmeshRequest, normals) &&
                  offsetof(vr_mmesh_request, smooth_iters) == offsetof(MmeshRequest, smooth_iters) &&
                  offsetof(vr_mmesh_request, relax) == offsetof(MmeshRequest, relax) &&
                  offsetof(vr_mmesh_request, reserved) == offsetof(MmeshRequest, reserved) &&
                  offsetof(vr_mmesh_request, array) == offsetof(MmeshRequest, array),
              "vr_mmesh_request");

const MmeshRequest *as_request(const vr_mmesh_request *q) { return reinterpret_cast<const MmeshRequest *>(q); }

// The context's blocks of this family grow behind a wait for the device (reserve's idle_first).
constexpr const char *kMmeshIdle = "hipDeviceSynchronize (mmesh scratch)";

// One call's passes on stream s; c is a single-device context.  One timed interval covers them all.
struct MmeshRun {
    vr_ctx *c;
    hipStream_t s;
    MaskGrid g;
    MmeshGeom G;
    MmeshArgs A;
    Interval timed;

    // What needs the context: a volume, and the grid inside it.  Before any output or scratch.
    int admit()
    {
        if (!c->bricks) return fail(c, VR_EINVAL, kMmeshNoVolume);
        const uint32_t dims[3] = {c->nx, c->ny, c->nz};
        if (const char *m = mmesh_origin_error(g, dims)) return fail(c, VR_EINVAL, m);
        return VR_OK;
    }

    // The count pass: the bits, the words with their counts, the scan; then the four fields of *I on
    // the host (waits for s).  The interval stays open for the emit passes.
    int count(const vr_mmesh_request *q, const void *array, vr_mmesh_info *I)
    {
        HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
        G = mmesh_geom(g.ext, q->closed);
        const MmeshScratch S = mmesh_scratch(G);
        if (G.node_words > 0xFFFFFFFFull || G.cell_words > 0xFFFFFFFFull) return fail(c, VR_EINVAL, kMmeshTexts[kMaskVoxels]);
        if (int rc = reserve(c, c->mmesh_aux_dev, (size_t)S.bytes, "hipMalloc(mmesh scratch)", kMmeshIdle)) return rc;
        char *base = static_cast<char *>(c->mmesh_aux_dev.p);
        std::memset(&A, 0, sizeof A);
        A.array = array;
        const uint32_t dims[3] = {c->nx, c->ny, c->nz};
        for (int a = 0; a < 3; ++a) {
            A.ext[a] = g.ext[a];
            A.origin[a] = g.origin[a];
            A.fdims[a] = (float)dims[a];
            A.nn[a] = G.nn[a];
            A.nc[a] = G.nc[a];
        }
        A.select = q->select;
        A.label = q->label;
        A.ring = G.ring;
        A.nw = G.nw;
        A.cw = G.cw;
        A.node_words = (uint32_t)G.node_words;
        A.cell_words = (uint32_t)G.cell_words;
        A.groups = G.groups;
        A.span = G.span;
        A.bits = reinterpret_cast<unsigned long long *>(base + S.bits);
        A.active = reinterpret_cast<unsigned long long *>(base + S.active);
        A.pre_t = reinterpret_cast<unsigned long long *>(base + S.pre_t);
        A.pre_v = reinterpret_cast<uint32_t *>(base + S.pre_v);
        A.gsum = reinterpret_cast<unsigned long long *>(base + S.gsum);
        A.matching = reinterpret_cast<unsigned long long *>(base + S.matching);
        A.normals = q->normals;
        A.relax = q->relax;

        if (int rc = timed.begin(c, s)) return rc;
        HIP_TRY(c, hipMemsetAsync(A.matching, 0, 8, s), "hipMemset(mmesh counter)");
        HIP_TRY(c, launch_mmesh_bits(q->elem_bytes, A, s, &c->mmesh_last_name), "mmesh bits launch");
        unsigned long long h[2 * kMmeshMaxGroups + 1] = {};
        if (A.cell_words) {
            HIP_TRY(c, launch_mmesh_classify(A, s, &c->mmesh_last_name), "mmesh classify launch");
            HIP_TRY(c, launch_mmesh_scan(A, s, &c->mmesh_last_name), "mmesh scan launch");
            HIP_TRY(c, hipMemcpyAsync(h, A.gsum, (size_t)G.groups * 16, hipMemcpyDeviceToHost, s), "hipMemcpy(mmesh sums)");
        }
        HIP_TRY(c, hipMemcpyAsync(&h[2 * kMmeshMaxGroups], A.matching, 8, hipMemcpyDeviceToHost, s), "hipMemcpy(mmesh counter)");
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(mmesh)");
        std::memset(I, 0, sizeof *I);
        I->voxels = g.voxels;
        I->matching = h[2 * kMmeshMaxGroups];
        if (A.cell_words)
            for (uint32_t k = 0; k < G.groups; ++k) {
                I->vertices += h[2 * k];
                I->triangles += h[2 * k + 1];
            }
        return VR_OK;
    }

    // What only the counts decide.  VR_ENOSPC: *info is the needed sizes, written here, since
    // mask_call hands an info out on VR_OK alone.
    int settle(const vr_mmesh_info &I, bool extract, uint64_t vcap, uint64_t tcap, vr_mmesh_info *info)
    {
        const char *msg;
        const int rc = mmesh_check_counts(I.vertices, I.triangles, extract, vcap, tcap, &msg);
        if (!rc) return VR_OK;
        if (int rc2 = timed.end()) return rc2;
        if (rc == VR_ENOSPC) *info = I;
        return fail(c, rc, msg);
    }

    // The emit passes of I.vertices > 0 vertices into device buffers that hold them.
    int emit(const vr_mmesh_request *q, const vr_mmesh_info &I, void *verts, void *tris)
    {
        A.verts = verts;
        A.tris = static_cast<uint32_t *>(tris);
        const uint32_t iters = q->smooth_iters;
        float *loc[2] = {nullptr, nullptr};
        if (iters) {
            const uint64_t stride = mmesh_local_stride(I.vertices);
            if (int rc = reserve(c, c->mmesh_loc_dev, (size_t)(2 * stride), "hipMalloc(mmesh locals)", kMmeshIdle)) return rc;
            loc[0] = reinterpret_cast<float *>(static_cast<char *>(c->mmesh_loc_dev.p));
            loc[1] = reinterpret_cast<float *>(static_cast<char *>(c->mmesh_loc_dev.p) + stride);
        }
        A.loc_out = loc[0];
        HIP_TRY(c, launch_mmesh_vertices(A, iters == 0, s, &c->mmesh_last_name), "mmesh vertex launch");
        for (uint32_t k = 0; k < iters; ++k) {
            A.loc_in = loc[k & 1];
            A.loc_out = loc[(k + 1) & 1];
            HIP_TRY(c, launch_mmesh_smooth(A, k + 1 == iters, s, &c->mmesh_last_name), "mmesh smooth launch");
        }
        if (I.triangles) HIP_TRY(c, launch_mmesh_triangles(A, s, &c->mmesh_last_name), "mmesh triangle launch");
        return VR_OK;
    }

    int finish()
    {
        if (int rc = timed.end()) return rc;
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(mmesh)");
        return VR_OK;
    }
};

}  // namespace

extern "C" {

int vr_mask_mesh_count_device(vr_ctx *c, const vr_mmesh_request *req, vr_mmesh_info *info, void *stream)
{
    MmeshRun R{c, static_cast<hipStream_t>(stream)};
    return mask_call(
        c, R.g, info, [&](const char **msg) { return mmesh_check_request(as_request(req), info, true, &R.g, msg); },
        [&](vr_ctx *m) { return vr_mask_mesh_count_device(m, req, info, stream); }, [&] { return R.admit(); },
        [&](vr_mmesh_info *I) {
            if (int rc = R.count(req, req->array, I)) return rc;
            if (int rc = R.settle(*I, false, 0, 0, info)) return rc;
            return R.finish();
        });
}

int vr_mask_mesh_count(vr_ctx *c, const vr_mmesh_request *req, vr_mmesh_info *info)
{
    MmeshRun R{c, nullptr};
    return mask_call(
        c, R.g, info, [&](const char **msg) { return mmesh_check_request(as_request(req), info, false, &R.g, msg); },
        [&](vr_ctx *m) { return vr_mask_mesh_count(m, req, info); }, [&] { return R.admit(); },
        [&](vr_mmesh_info *I) {
            MaskStage S{c};
            if (int rc = S.begin(c->mmesh_io_dev, "hipMalloc(mmesh staging)", kMmeshIdle,
                                 {req->array, (size_t)R.g.voxels * req->elem_bytes, "hipMemcpy(array)"}, {}, 0))
                return rc;
            if (int rc = R.count(req, S.in[0], I)) return rc;
            if (int rc = R.settle(*I, false, 0, 0, info)) return rc;
            return R.finish();
        });
}

int vr_mask_mesh_extract_device(vr_ctx *c, const vr_mmesh_request *req, void *verts_dev, uint64_t vcap, void *tris_dev,
                                uint64_t tcap, vr_mmesh_info *info, void *stream)
{
    MmeshRun R{c, static_cast<hipStream_t>(stream)};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mmesh_check_extract(as_request(req), verts_dev, vcap, tris_dev, tcap, info, sizeof *info, true, &R.g, msg);
        },
        [&](vr_ctx *m) { return vr_mask_mesh_extract_device(m, req, verts_dev, vcap, tris_dev, tcap, info, stream); },
        [&] { return R.admit(); },
        [&](vr_mmesh_info *I) {
            if (int rc = R.count(req, req->array, I)) return rc;
            if (int rc = R.settle(*I, true, vcap, tcap, info)) return rc;
            if (I->vertices)
                if (int rc = R.emit(req, *I, verts_dev, tris_dev)) return rc;
            return R.finish();
        });
}

int vr_mask_mesh_extract(vr_ctx *c, const vr_mmesh_request *req, vr_mesh_vertex *verts_host, uint64_t vcap,
                         uint32_t *tris_host, uint64_t tcap, vr_mmesh_info *info)
{
    MmeshRun R{c, nullptr};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mmesh_check_extract(as_request(req), verts_host, vcap, tris_host, tcap, info, sizeof *info, false, &R.g, msg);
        },
        [&](vr_ctx *m) { return vr_mask_mesh_extract(m, req, verts_host, vcap, tris_host, tcap, info); },
        [&] { return R.admit(); },
        [&](vr_mmesh_info *I) {
            MaskStage S{c};
            if (int rc = S.begin(c->mmesh_io_dev, "hipMalloc(mmesh staging)", kMmeshIdle,
                                 {req->array, (size_t)R.g.voxels * req->elem_bytes, "hipMemcpy(array)"}, {}, 0))
                return rc;
            if (int rc = R.count(req, S.in[0], I)) return rc;
            if (int rc = R.settle(*I, true, vcap, tcap, info)) return rc;
            if (!I->vertices) return R.finish();
            // the mesh in device memory: the vertex records, then the triangles (24 V is 8-byte aligned)
            const size_t vbytes = (size_t)I->vertices * kMmeshVertexBytes, tbytes = (size_t)I->triangles * kMmeshTriBytes;
            if (int rc = reserve(c, c->mmesh_out_dev, vbytes + tbytes, "hipMalloc(mmesh result)", kMmeshIdle)) return rc;
            char *out = static_cast<char *>(c->mmesh_out_dev.p);
            if (int rc = R.emit(req, *I, out, out + vbytes)) return rc;
            if (int rc = R.finish()) return rc;
            HIP_TRY(c, hipMemcpy(verts_host, out, vbytes, hipMemcpyDeviceToHost), "hipMemcpy(mask mesh vertices)");
            if (tbytes) HIP_TRY(c, hipMemcpy(tris_host, out + vbytes, tbytes, hipMemcpyDeviceToHost), "hipMemcpy(mask mesh triangles)");
            return VR_OK;
        });
}

const char *vr_mmesh_last_kernel_name(const vr_ctx *c) { return mask_last_kernel_name(c, &vr_ctx::mmesh_last_name); }

}  // extern "C"
