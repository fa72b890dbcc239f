// vr_api_mesh.hip — the isosurface mesh (include/vr/vr_mesh.h) on the host scaffold of vr_ctx.h.
#include "vr_ctx.h"
#include "vr_mesh_host.h"

namespace {
// What vr_mesh.h refuses before it looks at the context: the NULL arguments and the request's own
// fields (csrc/vr_mesh_host.h); no HIP call.
int check_mesh_request(vr_ctx *c, const vr_mesh_request *req, const void *info)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    if (!req || !info) return fail(c, VR_EINVAL, "NULL argument");
    if (const char *m = mesh_flags_error(req->iso, req->closed, req->normals, req->use_box))
        return fail(c, VR_EINVAL, m);
    return VR_OK;
}

// One call's passes on stream s; c is a single-device context.  The timing events bracket the
// classify pass with its scans as one interval and the two emit passes as another (the copy of
// the counts to the host and the host's wait for it lie between the two).
struct MeshRun {
    vr_ctx *c;
    hipStream_t s;
    MeshArgs A;
    Interval timed;

    // The classify pass and the scans, then the counts to the host (waits for s).  *I is written
    // only on VR_OK.
    int count(const vr_mesh_request *req, vr_mesh_info *I)
    {
        if (!c->bricks) return fail(c, VR_EINVAL, "no volume");
        const uint32_t dims[3] = {c->nx, c->ny, c->nz};
        MeshBox box;
        if (const char *m = mesh_box_resolve(req->use_box, req->box_min, req->box_max, req->closed, dims, &box))
            return fail(c, VR_EINVAL, m);
        std::memset(&A, 0, sizeof A);
        const uint32_t cells[3] = {(uint32_t)brick_cells(c->layout, 0), (uint32_t)brick_cells(c->layout, 1),
                                   (uint32_t)brick_cells(c->layout, 2)};
        const uint64_t nwork = mesh_brick_range(box, cells, (uint32_t)kPad, A.b0, A.nb);
        if (nwork >= 1ull << 31) return fail(c, VR_EINVAL, "mesh box holds too many bricks");
        for (int a = 0; a < 3; ++a) {
            A.dims[a] = dims[a];
            A.fdims[a] = (float)dims[a];
            A.lo[a] = box.lo[a];
            A.hi[a] = box.hi[a];
            A.clo[a] = (int32_t)box.clo[a];
            A.chi[a] = (int32_t)box.chi[a];
        }
        A.iso = req->iso;
        A.nwork = (uint32_t)nwork;
        A.nchunks = (A.nwork + kMeshChunk - 1) / kMeshChunk;
        A.nbx = bricks_for(c->nx, 0, c->layout);
        A.nby = bricks_for(c->ny, 1, c->layout);
        A.vol = c->bricks;
        HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
        const MeshScratch sc = mesh_scratch(nwork);
        // (behind a wait: an earlier call's passes may still read the old block on another stream)
        if (int rc = reserve(c, c->mesh_dev, sc.bytes, "hipMalloc(mesh scratch)", "hipDeviceSynchronize (mesh scratch)"))
            return rc;
        char *base = static_cast<char *>(c->mesh_dev.p);
        A.mask = reinterpret_cast<uint32_t *>(base + sc.mask);
        A.cnt = reinterpret_cast<uint2 *>(base + sc.cnt);
        A.pre = reinterpret_cast<uint2 *>(base + sc.pre);
        A.chunk = reinterpret_cast<unsigned long long *>(base + sc.chunk);
        A.out = reinterpret_cast<unsigned long long *>(base + sc.out);
        HIP_TRY(c, hipMemsetAsync(A.out, 0, 32, s), "hipMemset(mesh counts)");
        if (int rc = timed.begin(c, s)) return rc;
        std::string name;
        HIP_TRY(c, launch_mesh_classify(c->layout, A, s, &name), "mesh classify launch");
        c->last_mpr_name = name;
        if (int rc = timed.end()) return rc;
        unsigned long long h[3];
        HIP_TRY(c, hipMemcpyAsync(h, A.out, sizeof h, hipMemcpyDeviceToHost, s), "hipMemcpy(mesh counts)");
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(mesh counts)");
        if (h[0] > kMeshMaxVertices) return fail(c, VR_EINVAL, "mesh has more than 2^32 - 1 vertices");
        std::memset(I, 0, sizeof *I);
        I->vertices = h[0];
        I->triangles = 2 * h[1];
        I->inside_voxels = h[2];
        return VR_OK;
    }
    // The two emit passes into device buffers that hold I's counts.
    int emit(const vr_mesh_request *req, const vr_mesh_info &I, void *verts_dev, void *tris_dev)
    {
        A.verts = verts_dev;
        A.tris = static_cast<uint32_t *>(tris_dev);
        if (!I.vertices) return VR_OK;  // (no vertex, no triangle)
        if (int rc = timed.begin(c, s)) return rc;
        HIP_TRY(c, launch_mesh_vertices(c->layout, req->normals != 0, A, s), "mesh vertex launch");
        if (I.triangles) HIP_TRY(c, launch_mesh_quads(c->layout, A, s), "mesh quad launch");
        return timed.end();
    }
};
}  // namespace

extern "C" {

int vr_mesh_count(vr_ctx *c, const vr_mesh_request *req, vr_mesh_info *info)
{
    if (int rc = check_mesh_request(c, req, info)) return rc;
    if (is_group(c)) return on_replica(c, [&](vr_ctx *m) { return vr_mesh_count(m, req, info); });
    MeshRun R{c, nullptr};
    vr_mesh_info I;
    if (int rc = R.count(req, &I)) return rc;
    *info = I;
    return VR_OK;
}

int vr_mesh_extract_device(vr_ctx *c, const vr_mesh_request *req, void *verts_dev, uint64_t vcap,
                           void *tris_dev, uint64_t tcap, vr_mesh_info *info, void *stream)
{
    if (int rc = check_mesh_request(c, req, info)) return rc;
    if (!verts_dev || !tris_dev) return fail(c, VR_EINVAL, "NULL argument");
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) {
            return vr_mesh_extract_device(m, req, verts_dev, vcap, tris_dev, tcap, info, stream);
        });
    MeshRun R{c, static_cast<hipStream_t>(stream)};
    vr_mesh_info I;
    if (int rc = R.count(req, &I)) return rc;
    if (I.vertices > vcap || I.triangles > tcap) {
        *info = I;
        return fail(c, VR_ENOSPC, "mesh buffers are smaller than the mesh (see the info's counts)");
    }
    if (int rc = R.emit(req, I, verts_dev, tris_dev)) return rc;
    HIP_TRY(c, hipStreamSynchronize(R.s), "hipStreamSynchronize(mesh)");
    *info = I;
    return VR_OK;
}

int vr_mesh_extract(vr_ctx *c, const vr_mesh_request *req, vr_mesh_vertex *verts_host, uint64_t vcap,
                    uint32_t *tris_host, uint64_t tcap, vr_mesh_info *info)
{
    if (int rc = check_mesh_request(c, req, info)) return rc;
    if (!verts_host || !tris_host) return fail(c, VR_EINVAL, "NULL argument");
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) {
            return vr_mesh_extract(m, req, verts_host, vcap, tris_host, tcap, info);
        });
    MeshRun R{c, nullptr};
    vr_mesh_info I;
    if (int rc = R.count(req, &I)) return rc;
    if (I.vertices > vcap || I.triangles > tcap) {
        *info = I;
        return fail(c, VR_ENOSPC, "mesh buffers are smaller than the mesh (see the info's counts)");
    }
    // vertices, then (16-aligned) triangles, in the context's own device block
    const size_t vbytes = (size_t)I.vertices * kMeshVertexBytes, tbytes = (size_t)I.triangles * kMeshTriangleBytes;
    const size_t toff = (vbytes + 15) & ~(size_t)15, bytes = toff + tbytes;
    // (no wait: its last mesh was copied out synchronously)
    if (int rc = reserve(c, c->mesh_out_dev, bytes, "hipMalloc(mesh)", nullptr)) return rc;
    char *dev = static_cast<char *>(c->mesh_out_dev.p);
    if (int rc = R.emit(req, I, dev, dev + toff)) return rc;
    if (vbytes) HIP_TRY(c, hipMemcpy(verts_host, dev, vbytes, hipMemcpyDeviceToHost), "hipMemcpy(mesh vertices)");
    if (tbytes) HIP_TRY(c, hipMemcpy(tris_host, dev + toff, tbytes, hipMemcpyDeviceToHost), "hipMemcpy(mesh triangles)");
    HIP_TRY(c, hipDeviceSynchronize(), "hipDeviceSynchronize(mesh)");
    *info = I;
    return VR_OK;
}

}  // extern "C"
