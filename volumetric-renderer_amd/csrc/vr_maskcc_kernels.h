// vr_maskcc_kernels.h — what vr_api_maskcc.hip launches from vr_maskcc_kernels.hip (both in
// lib/libvr_amd_maskcc.so): the components of a mask as row runs united through a lock-free
// union-find, their records, and the selection sweep.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_maskcc_host.h"

namespace vr {

// MccArgs::cnt, 64-bit words
enum MccCounter {
    kMccCntComps = 0,    // the components (the scan pass stores it)
    kMccCntIn = 1,       // the labelled voxels (the rows pass)
    kMccCntLargest = 2,  // voxels << 32 | ~label of the largest component
    kMccCntOnes = 3,     // the ones of the selection's output
    kMccCntKept = 4,     // the records the rule keeps
};

struct MccArgs {
    const void *mask;          // elem_bytes per voxel, set iff non-zero
    uint32_t *P;               // a label per voxel: the parent array of the union-find, parent + 1
    unsigned long long *bits;  // root table: a bit per voxel
    uint32_t *wpre;            //   the chunk's roots before each word
    uint32_t *chunk;           //   the chunk's roots, then (scan) the roots before each chunk
    unsigned long long *cnt;   // kMccCounters words, zero before the rows pass
    void *comps;               // ncomps records of kMccRecordBytes
    uint8_t *flags;            // ncomps bytes: the rule keeps the record
    uint8_t *out;              // the selection: a byte per voxel
    uint32_t ext[3];
    uint32_t nvox, nwords, nchunks, ncomps;
    uint32_t elem_bytes;       // 1 or 4
    uint32_t invert;           // label the unset voxels (hole filling)
    uint32_t rule;             // kMccKeep*, kMccFillHoles
    uint32_t seed;             // kMccKeepSeed: the seed's box-linear index
    unsigned long long min_voxels;
};

enum MccPass {
    kMccRows = 0,       // P[l] = 1 + the first voxel of l's run (0: not labelled); cnt[kMccCntIn]
    kMccLink = 1,       // unites the runs that touch across rows
    kMccFlatten = 2,    // P[l] = 1 + the root; the root table
    kMccScan = 3,       // the roots before each chunk; cnt[kMccCntComps]
    kMccTableInit = 4,  // the records' identities
    kMccAccum = 5,      // count, bounding box and index sums per record
    kMccLargest = 6,    // cnt[kMccCntLargest]
    kMccKeep = 7,       // flags from the rule; cnt[kMccCntKept]
    kMccSelect = 8,     // out from the flags; cnt[kMccCntOnes]
    kMccPasses = 9,
};

// One pass on `stream`; *name: the kernel it launched.  hipErrorInvalidValue for arguments the
// pass cannot run on, before any launch.
hipError_t launch_mcc(MccPass pass, const MccArgs &a, const MaskGrid &g, uint32_t connectivity, hipStream_t stream,
                      const char **name);

}  // namespace vr
