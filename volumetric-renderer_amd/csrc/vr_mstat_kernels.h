// vr_mstat_kernels.h — what vr_api_mstat.hip launches from vr_mstat_kernels.hip (both in
// lib/libvr_amd_mstat.so): the statistics of the volume under a mask or under each label of a label
// array, and the value-window pass that writes a mask.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_mstat_host.h"

namespace vr {

// MstatArgs::cnt, 64-bit words, zero before a call's first pass
enum MstatCounter {
    kMstatCntSet = 0,       // the non-zero elements of the array
    kMstatCntUnlisted = 1,  // of them, those whose label the table does not hold
    kMstatCntBelow = 2,     // the histogram's below / above
    kMstatCntAbove = 3,
    kMstatCntOut = 4,       // the ones of the window pass's output
};

// One region's accumulators, all zero before the voxel pass: zero is the identity of every
// reduction (a key of a voxel is never 0).  sum, sum2: int64 / uint64 on integer storage, the bits
// of a double on f32 storage.
struct MstatAcc {
    unsigned long long count, nan;
    unsigned long long kmax;  // ordered(f) << 32 | ~index, reduced with max
    unsigned long long kmin;  // ~ordered(f) << 32 | ~index, reduced with max
    unsigned long long sum, sum2;
};
static_assert(sizeof(MstatAcc) == kMstatAccBytes, "vr_mstat_host.h");

struct MstatArgs {
    const void *vol;           // the base bricks (layout code `layout` of launch_mstat)
    const void *array;         // the mask (elem_bytes per voxel) or the labels (uint32_t); NULL: every voxel is set
    const void *table;         // ntable records of kMstatRecordBytes, any alignment: only .label is read
    uint32_t *labels;          // ntable labels, compacted from the table
    MstatAcc *acc;             // nrec accumulators
    void *rec;                 // nrec records of kMstatRecordBytes (vr_mstat_region), 8-byte aligned
    unsigned long long *cnt;   // kMstatCounters words
    unsigned long long *bins;  // nbins counts (the histogram)
    const float *edges;        // nbins lower edges
    uint8_t *out;              // the window pass: a byte per voxel
    double scale;              // hist_scale
    float lo, hi;              // the histogram's range, or the window
    uint32_t nbins;            // 0: no histogram
    uint32_t ext[3], origin[3];
    uint32_t nbx, nby;         // bricks_for of the volume's x and y
    uint32_t elem_bytes;       // 1 or 4
    uint32_t nrec;             // 1 for a mask, ntable for labels
};

enum MstatPass {
    kMstatGather = 0,    // labels[i] = table[i].label
    kMstatMask = 1,      // the accumulators of the one region of a mask, and the histogram
    kMstatLabels = 2,    // the accumulators of every listed label; cnt[kMstatCntSet], cnt[kMstatCntUnlisted]
    kMstatFinalize = 3,  // the records from the accumulators
    kMstatWindow = 4,    // out from the array and the window; cnt[kMstatCntSet], cnt[kMstatCntOut]
    kMstatPasses = 5,
};

// One pass on `stream` over the base bricks of layout code `layout`; *name: the kernel it launched.
// hipErrorInvalidValue for arguments the pass cannot run on, before any launch.
hipError_t launch_mstat(MstatPass pass, int layout, const MstatArgs &a, const MaskGrid &g, hipStream_t stream,
                        const char **name);

}  // namespace vr
