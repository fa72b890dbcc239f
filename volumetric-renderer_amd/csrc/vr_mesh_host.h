// vr_mesh_host.h — the host side of include/vr/vr_mesh.h: what a mesh request is refused for, the
// node box and the cell range it resolves to on an nx x ny x nz volume, and the bricks a launch
// walks.  Plain C++ without HIP, so a stand-alone program can run it (under a sanitizer,
// tests/test_mesh_cpu.py); vr_api_mesh.hip includes it for vr_mesh_count, vr_mesh_extract and
// vr_mesh_extract_device.
#pragma once

#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "vr_box_host.h"

namespace vr {

constexpr uint32_t kMeshVertexBytes = 24;    // sizeof(vr_mesh_vertex)
constexpr uint32_t kMeshTriangleBytes = 12;  // three uint32_t
constexpr uint64_t kMeshMaxVertices = 0xFFFFFFFFull;  // an index is a uint32_t

// The node box [lo, hi) of a request and its cell range [clo, chi] (both ends included; logical
// cell indices, -1 allowed: the closed mesh's ring cell below voxel 0).  An axis of one node and
// closed = 0 has no cell: chi < clo there.
struct MeshBox : VoxelBox {
    int64_t clo[3], chi[3];
};

// nullptr: iso, closed, normals and use_box are what vr_mesh.h allows; else what is wrong.
inline const char *mesh_flags_error(float iso, uint32_t closed, uint32_t normals, uint32_t use_box)
{
    if (!std::isfinite(iso)) return "mesh iso must be finite";
    if (closed > 1) return "mesh closed must be 0 or 1";
    if (normals > 1) return "mesh normals must be 0 or 1";
    if (use_box > 1) return "mesh use_box must be 0 or 1";
    return nullptr;
}

// The box of a request on a volume of dims voxels into *b; nullptr, or what is wrong (*b is then
// untouched).  The shared rule (box_resolve).
inline const char *mesh_box_resolve(uint32_t use_box, const uint32_t box_min[3], const uint32_t box_max[3],
                                    uint32_t closed, const uint32_t dims[3], MeshBox *b)
{
    if (use_box > 1) return "mesh use_box must be 0 or 1";
    if (closed > 1) return "mesh closed must be 0 or 1";
    MeshBox r;
    if (box_resolve(use_box, box_min, box_max, dims, &r)) return "mesh box is empty or beyond the volume";
    for (int a = 0; a < 3; ++a) {
        r.clo[a] = closed ? (int64_t)r.lo[a] - 1 : (int64_t)r.lo[a];
        r.chi[a] = closed ? (int64_t)r.hi[a] - 1 : (int64_t)r.hi[a] - 2;
    }
    *b = r;
    return nullptr;
}

// The bricks a launch walks: those that hold the padded cells [clo + pad, hi - 1 + pad] per axis
// -- the cell set's, and in an open mesh also the cell of the box's last voxel, which is in no
// cell of the set but counts for inside_voxels (box_brick_range with clo as the first index).
inline uint64_t mesh_brick_range(const MeshBox &b, const uint32_t cells[3], uint32_t pad, uint32_t b0[3],
                                 uint32_t nb[3])
{
    const int64_t last[3] = {b.hi[0] - 1ll, b.hi[1] - 1ll, b.hi[2] - 1ll};
    return box_brick_range(b.clo, last, cells, pad, b0, nb);
}

// vr_host.h vr_mesh_write_ply: a binary little-endian PLY of nv vertex records (24 bytes: pos[3],
// normal[3]) and nt triangles (three uint32_t).  A vertex is written at pos * scale + offset per
// component in f32 (NULL: scale 1, offset 0), its normal unchanged.  0, -22 for a bad argument
// (a NULL path, a NULL array with a count, an index >= nv), -1 when the file cannot be written;
// *err (when not NULL) says which.  Nothing is left behind on -22.
inline int mesh_write_ply(const char *path, const void *verts, uint64_t nv, const uint32_t *tris, uint64_t nt,
                          const float scale[3], const float offset[3], const char **err)
{
    const char *dummy;
    if (!err) err = &dummy;
    *err = "";
    if (!path || (!verts && nv) || (!tris && nt)) return *err = "bad argument", -22;
    if (nv > kMeshMaxVertices) return *err = "more than 2^32 - 1 vertices", -22;
    for (uint64_t i = 0; i < 3 * nt; ++i)
        if (tris[i] >= nv) return *err = "triangle index beyond the vertices", -22;
    FILE *f = std::fopen(path, "wb");
    if (!f) return *err = "cannot write the file", -1;
    std::fprintf(f,
                 "ply\nformat binary_little_endian 1.0\ncomment written by vr_mesh_write_ply\n"
                 "element vertex %llu\nproperty float x\nproperty float y\nproperty float z\n"
                 "property float nx\nproperty float ny\nproperty float nz\n"
                 "element face %llu\nproperty list uchar uint vertex_indices\nend_header\n",
                 (unsigned long long)nv, (unsigned long long)nt);
    auto le32 = [](unsigned char *p, uint32_t w) {
        p[0] = (unsigned char)w;
        p[1] = (unsigned char)(w >> 8);
        p[2] = (unsigned char)(w >> 16);
        p[3] = (unsigned char)(w >> 24);
    };
    bool ok = true;
    const unsigned char *v = static_cast<const unsigned char *>(verts);
    for (uint64_t i = 0; i < nv && ok; ++i) {
        float r[6];
        std::memcpy(r, v + i * kMeshVertexBytes, sizeof r);
        unsigned char out[24];
        for (int a = 0; a < 6; ++a) {
            float x = r[a];
            if (a < 3) x = x * (scale ? scale[a] : 1.0f) + (offset ? offset[a] : 0.0f);
            uint32_t w;
            std::memcpy(&w, &x, 4);
            le32(out + 4 * a, w);
        }
        ok = std::fwrite(out, 1, sizeof out, f) == sizeof out;
    }
    for (uint64_t i = 0; i < nt && ok; ++i) {
        unsigned char out[13];
        out[0] = 3;
        for (int k = 0; k < 3; ++k) le32(out + 1 + 4 * k, tris[3 * i + k]);
        ok = std::fwrite(out, 1, sizeof out, f) == sizeof out;
    }
    ok = (std::fclose(f) == 0) && ok;
    return ok ? 0 : (*err = "short write", -1);
}

}  // namespace vr
