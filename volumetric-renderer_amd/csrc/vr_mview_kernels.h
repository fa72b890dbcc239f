// vr_mview_kernels.h — what vr_api_mview.hip launches from vr_mview_kernels.hip (both in
// lib/libvr_amd_mview.so): the occupancy words of a mask or label array, its first-hit records along
// the frames' rays, and its elements on an MPR plane.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_internal.h"  // MarchParams (the exported build_params fills it)
#include "vr_mview_host.h"

namespace vr {

// The counters of a call, 64-bit words, zero before its kernel.
enum MviewCounter {
    kMviewCntCovered = 0,  // hit image: covered pixels; slice: pixels with a step
    kMviewCntHits = 1,     // hit records / non-zero pixels
    kMviewCntSteps = 2,
    kMviewCntSamples = 3,
    kMviewCntCellsSet = 0,  // occupancy: the set bits
    kMviewCntMatching = 1,  // and the matching voxels
    kMviewCounters = 4,
};

// The array as a kernel sees it: the grid inside the volume, the match rule and the words.
struct MviewArray {
    const void *array;    // box-linear, ELEM per voxel
    const uint32_t *occ;  // the occupancy words (OCC kernels), or NULL
    uint32_t ext[3], origin[3];
    uint32_t dims[3];     // the volume's
    float fn[3];          // (float)dims
    uint32_t c0, c1;      // cells along x and y
    uint32_t select, label;
};

// MarchParams describes the whole framebuffer (fw, fh, the unprojection, the ray constants and the
// slice box); the rectangle is here.
struct MviewHitArgs {
    MviewArray S;
    void *out;  // w * h records of kMviewHitBytes, 4-byte aligned
    unsigned long long *cnt;
    uint32_t x0, y0, w, h;
    uint32_t tiles_x;  // 16 x 16-pixel tiles in raster order, one per workgroup
};

struct MviewSliceArgs {
    MviewArray S;
    uint32_t *out;  // H x W elements
    unsigned long long *cnt;
    double origin[3], du[3], dv[3], dn[3];  // the plane's f32 vectors, widened (exact)
    double half_w, half_h, half_n;          // 0.5 W, 0.5 H, 0.5 (nsamples - 1)
    float smin[3], smax[3];
    uint32_t W, H, nsamples;
    uint32_t tiles_x;
};

struct MviewOccArgs {
    MviewArray S;
    uint32_t *words;
    unsigned long long *cnt;
    uint32_t ncells, nwords;
};

// Each on `stream`; *name: the kernel launched.  hipErrorInvalidValue for an elem_bytes that is
// neither 1 nor 4, before any launch.
hipError_t launch_mview_occupancy(uint32_t elem_bytes, const MviewOccArgs &a, hipStream_t stream, const char **name);
hipError_t launch_mview_hit(uint32_t elem_bytes, const MarchParams &p, const MviewHitArgs &a, uint32_t tiles_y,
                            hipStream_t stream, const char **name);
hipError_t launch_mview_slice(uint32_t elem_bytes, const MviewSliceArgs &a, uint32_t tiles_y, hipStream_t stream,
                              const char **name);

}  // namespace vr
