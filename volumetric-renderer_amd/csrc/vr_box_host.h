// vr_box_host.h — the request box every analysis call shares (vr_hist.h, vr_label.h, vr_mesh.h):
// the voxel box a request resolves to on an nx x ny x nz volume, and the bricks that hold a range
// of voxel indices.  Plain C++ without HIP, so a stand-alone program can run it (under a
// sanitizer, tools/host_sanitize/).  The rule is returned as a reason code: each family owns the
// texts of its refusals and adds its own bounds on top.
#pragma once

#include <stdint.h>

namespace vr {

// The voxel box [lo, hi) of a request, its extents and its voxel count (UINT64_MAX where the
// product of the three extents passes 64 bits).
struct VoxelBox {
    uint32_t lo[3], hi[3], ext[3];
    uint64_t voxels;
};

enum BoxError { kBoxOk = 0, kBoxUse, kBoxEmpty };  // use_box is not 0 or 1; empty or beyond the volume

// The box of a request on a volume of dims voxels into *b (untouched unless kBoxOk): the whole
// volume without use_box, else box_min < box_max <= dims per axis.
inline BoxError box_resolve(uint32_t use_box, const uint32_t box_min[3], const uint32_t box_max[3],
                            const uint32_t dims[3], VoxelBox *b)
{
    if (use_box > 1) return kBoxUse;
    VoxelBox r;
    r.voxels = 1;
    for (int a = 0; a < 3; ++a) {
        r.lo[a] = use_box ? box_min[a] : 0u;
        r.hi[a] = use_box ? box_max[a] : dims[a];
        if (r.lo[a] >= r.hi[a] || r.hi[a] > dims[a]) return kBoxEmpty;
        r.ext[a] = r.hi[a] - r.lo[a];
        r.voxels = r.voxels > UINT64_MAX / r.ext[a] ? UINT64_MAX : r.voxels * r.ext[a];
    }
    *b = r;
    return kBoxOk;
}

// The bricks that hold the padded indices first + pad .. last + pad per axis (first + pad >= 0;
// cells[a]: a brick's cells along a): the first brick and the count per axis; returns the counts'
// product (never 0; UINT64_MAX where it passes 64 bits: the caller bounds it).
inline uint64_t box_brick_range(const int64_t first[3], const int64_t last[3], const uint32_t cells[3],
                                uint32_t pad, uint32_t b0[3], uint32_t nb[3])
{
    uint64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        b0[a] = (uint32_t)((uint64_t)(first[a] + pad) / cells[a]);
        nb[a] = (uint32_t)((uint64_t)(last[a] + pad) / cells[a]) - b0[a] + 1;
        n = n > UINT64_MAX / nb[a] ? UINT64_MAX : n * nb[a];
    }
    return n;
}

// The bricks that hold the voxels of b.
inline uint64_t box_brick_range(const VoxelBox &b, const uint32_t cells[3], uint32_t pad, uint32_t b0[3],
                                uint32_t nb[3])
{
    const int64_t first[3] = {b.lo[0], b.lo[1], b.lo[2]}, last[3] = {b.hi[0] - 1ll, b.hi[1] - 1ll, b.hi[2] - 1ll};
    return box_brick_range(first, last, cells, pad, b0, nb);
}

}  // namespace vr
