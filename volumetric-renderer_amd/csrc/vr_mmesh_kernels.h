// vr_mmesh_kernels.h — what vr_api_mmesh.hip launches from vr_mmesh_kernels.hip (both in
// lib/libvr_amd_mmesh.so): the inside bits of a mask or label array, the active and edge words of
// its cells with their counts, the scan that turns the counts into vertex and triangle offsets, and
// the passes that write the vertices, smooth them and write the triangles.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_mmesh_host.h"

namespace vr {

// One call as its kernels see it.  Every word index fits 32 bits (vr_mmesh_host.h: at most about
// 2^30 node words); byte offsets are formed in size_t.
struct MmeshArgs {
    const void *array;  // box-linear, ELEM per voxel
    uint32_t ext[3], origin[3];
    float fdims[3];  // (float)dims of the volume
    uint32_t select, label, ring;
    uint32_t nn[3], nc[3], nw, cw;
    uint32_t node_words, cell_words;
    uint32_t groups, span;
    unsigned long long *bits;      // node_words
    unsigned long long *active;    // cell_words
    unsigned long long *pre_t;     // cell_words: triangles before the word
    uint32_t *pre_v;               // cell_words: vertices | triangles << 16 of the word, then vertices before it
    unsigned long long *gsum;      // per workgroup: its vertices, its triangles
    unsigned long long *matching;  // zero before the bits kernel
    const float *loc_in;           // the previous sweep's local, 3 floats a vertex
    float *loc_out;                // this pass's (a pass that is not the last)
    void *verts;                   // vr_mesh_vertex records
    uint32_t *tris;
    uint32_t normals;
    float relax;
};

// Each on `stream`; *name: the kernel launched.
hipError_t launch_mmesh_bits(uint32_t elem_bytes, const MmeshArgs &a, hipStream_t stream, const char **name);
hipError_t launch_mmesh_classify(const MmeshArgs &a, hipStream_t stream, const char **name);
hipError_t launch_mmesh_scan(const MmeshArgs &a, hipStream_t stream, const char **name);
// last: the pass writes pos into the records; otherwise local into loc_out.  The vertex pass writes
// the normals either way.
hipError_t launch_mmesh_vertices(const MmeshArgs &a, bool last, hipStream_t stream, const char **name);
hipError_t launch_mmesh_smooth(const MmeshArgs &a, bool last, hipStream_t stream, const char **name);
hipError_t launch_mmesh_triangles(const MmeshArgs &a, hipStream_t stream, const char **name);

}  // namespace vr
