// vr_morph_kernels.h — what vr_api_morph.hip launches from vr_morph_kernels.hip (both in
// lib/libvr_amd_morph.so): one exact squared Euclidean distance transform as three passes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_morph_host.h"

namespace vr {

// What the last pass does with a voxel's distance.
enum MorphFinal {
    kMorphStore = 0,   // writes it (the pass along y)
    kMorphEdt = 1,     // writes it and folds max / index into cnt[1]
    kMorphThresh = 2,  // writes the byte (dist2 <= limit) != invert and counts the ones into cnt[2]
};

struct MorphArgs {
    const void *mask;         // elem_bytes per voxel, set iff non-zero
    uint32_t *dist;           // a uint32_t per voxel, transformed in place by the passes along y and z
    uint8_t *out;             // kMorphThresh: a byte per voxel
    unsigned long long *cnt;  // [0] set voxels of the mask, [1] dist2 << 32 | ~index (max), [2] ones of out
    uint32_t ext[3];
    uint32_t elem_bytes;      // 1 or 4
    uint32_t to_unset;        // the target voxels are the unset ones
    uint32_t limit;           // a distance above it is stored as kMorphNone (kMorphNone - 1: none is)
    uint32_t invert;          // kMorphThresh: erosion
};

// Pass 1, along x: dist[l] = the squared distance to the nearest target voxel of l's row (kMorphNone
// without one, or above limit); cnt[0] += the mask's set voxels.
hipError_t launch_morph_edt_x(const MorphArgs &a, const MaskGrid &g, hipStream_t stream, const char **name);
// Passes 2 and 3, along axis 1 (y) or 2 (z): the lower envelope of the columns, in place.
hipError_t launch_morph_edt_axis(const MorphArgs &a, const MaskGrid &g, int axis, MorphFinal fin,
                                 hipStream_t stream, const char **name);

}  // namespace vr
