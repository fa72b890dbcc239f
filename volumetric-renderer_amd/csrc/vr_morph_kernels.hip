// vr_morph_kernels.hip — the exact squared Euclidean distance transform of a mask (include/vr/
// vr_morph.h), the one primitive behind vr_edt_squared* and vr_mask_morph*; the gfx950 code object
// of lib/libvr_amd_morph.so.  DESIGN.md §4.13.
//
// The transform is separable: along x the distance to the nearest target voxel of the row, then
// along y and along z the integer lower envelope D(i) = min_k F(k) + (i - k)^2 of every column, in
// place.  Rules (§4.12's): no workgroup waits for another -- order comes from kernel boundaries;
// every loop's bound can be read off the code; integer vector atomics only (atomicAdd and atomicMax
// on 64 bits); addresses are formed in 64 bits; kMorphNone terms are skipped, never added to; no
// scratch memory (make asm-morph).
#include "vr_morph_kernels.h"

namespace vr {
namespace {

constexpr uint32_t kXWaves = 4;                       // rows a workgroup walks at a time, a wave each
constexpr uint32_t kXWords = kMaskMaxExtent / 64u;    // 64-voxel words of the longest row
constexpr uint32_t kAxisThreads = 512;
constexpr uint32_t kMaxGrid = 8192;                   // workgroups of a launch: the rest is strided

// Pass 1.  A wave per row, a lane per voxel, 64 voxels a round.  Forward: the round's target voxels
// as one ballot word, kept in LDS beside the carry, the last target voxel of the words before it.
// Backward: a lane finds its nearest target voxel at or below it and at or above it with two bit
// scans of its word, and beyond the word in the carries from either side.
template <int EB>
__global__ __launch_bounds__(256) void morph_edt_x_kernel(const MorphArgs A, const uint64_t nrows)
{
    __shared__ unsigned long long s_bits[kXWaves][kXWords];
    __shared__ int s_left[kXWaves][kXWords];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t bx = A.ext[0], nwords = (bx + 63u) >> 6;  // at most kXWords
    const bool to_unset = A.to_unset != 0;
    unsigned long long nset = 0;  // (the same in every lane of the wave)
    // (row0 is the workgroup's: every wave runs every barrier)
    for (uint64_t row0 = (uint64_t)blockIdx.x * kXWaves; row0 < nrows; row0 += (uint64_t)gridDim.x * kXWaves) {
        const uint64_t row = row0 + wave;
        const bool live = row < nrows;
        const uint64_t base = row * bx;  // below the voxel count where live
        int carry = -1;
        for (uint32_t w = 0; w < nwords; ++w) {
            const uint32_t x = w * 64u + lane;
            const bool in = live && x < bx;
            bool set = false;
            if (in) {
                if (EB == 1)
                    set = static_cast<const uint8_t *>(A.mask)[base + x] != 0;
                else
                    set = static_cast<const uint32_t *>(A.mask)[base + x] != 0;
            }
            const unsigned long long m = __ballot(in && set != to_unset);
            nset += (unsigned long long)__popcll(__ballot(set));
            if (lane == 0) {
                s_bits[wave][w] = m;
                s_left[wave][w] = carry;
            }
            if (m) carry = (int)(w * 64u) + 63 - __clzll((long long)m);
        }
        __syncthreads();
        int right = -1;
        for (uint32_t ww = 0; ww < nwords; ++ww) {
            const uint32_t w = nwords - 1u - ww;
            const unsigned long long m = s_bits[wave][w];
            const uint32_t x = w * 64u + lane;
            const unsigned long long below = m & (~0ull >> (63u - lane));  // bits 0 .. lane
            const unsigned long long above = m & (~0ull << lane);          // bits lane .. 63
            const int pl = below ? (int)(w * 64u) + 63 - __clzll((long long)below) : s_left[wave][w];
            const int pr = above ? (int)(w * 64u) + __ffsll(above) - 1 : right;
            uint32_t d = kMorphNone;
            if (pl >= 0) d = x - (uint32_t)pl;
            if (pr >= 0) d = min(d, (uint32_t)pr - x);
            uint32_t d2 = kMorphNone;
            if (d != kMorphNone) {
                d2 = d * d;  // d < 32768
                if (d2 > A.limit) d2 = kMorphNone;
            }
            if (live && x < bx) A.dist[base + x] = d2;
            if (m) right = (int)(w * 64u) + __ffsll(m) - 1;
        }
        __syncthreads();  // (the next rows overwrite the words)
    }
    if (lane == 0 && nset) atomicAdd(&A.cnt[0], nset);
}

// Passes 2 and 3.  A workgroup stages a tile -- 2^width_log2 neighbouring columns, every voxel of
// each -- in LDS, lanes along the line so that the loads, the stores and the LDS reads of a wave
// are consecutive words; the transform is then in place.  A voxel searches outward from i.  The
// first kAxisNear offsets go one by one and stop at the first whose square reaches the best so far
// (or passes the limit): short wherever a target voxel is near.  What lies beyond goes by blocks of
// kAxisBlock voxels, whose minima the workgroup took first: a block is read only if its minimum
// plus the square of its nearest offset is below the best so far, and a side ends at the first
// block whose nearest offset's square reaches it.  Every skipped candidate is at least the best,
// so the result is exact.  F is at most 2 * 32767^2 and an offset's square at most 32767^2, so no
// sum wraps or reaches kMorphNone.
constexpr uint32_t kAxisNear = 16;
constexpr uint32_t kAxisBlockLog2 = 4, kAxisBlock = 1u << kAxisBlockLog2;

// The candidates of block b of column x: min over its voxels k of F(k) + (i - k)^2, and best.
__device__ inline uint32_t axis_scan_block(const uint32_t *s_f, uint32_t b, uint32_t x, uint32_t lg, uint32_t n,
                                           uint32_t i, uint32_t best)
{
    for (uint32_t t = 0; t < kAxisBlock; ++t) {
        const uint32_t k = (b << kAxisBlockLog2) + t;
        if (k >= n) break;
        const uint32_t f = s_f[(k << lg) | x];
        const uint32_t dd = k > i ? k - i : i - k;
        if (f != kMorphNone) best = min(best, f + dd * dd);
    }
    return best;
}

template <int FIN, int WORDS>
__global__ __launch_bounds__(kAxisThreads) void morph_edt_axis_kernel(const MorphArgs A, const MorphAxis X)
{
    __shared__ uint32_t s_f[WORDS];
    __shared__ uint32_t s_min[WORDS / kAxisBlock + 64];  // block b of column x at (b << lg) | x
    const uint32_t n = X.n, lg = X.width_log2, wmask = (1u << lg) - 1u;
    const uint32_t elems = n << lg;  // at most WORDS (morph_axis)
    const uint32_t nb = (n + kAxisBlock - 1u) >> kAxisBlockLog2;  // nb << lg is at most WORDS / kAxisBlock + 64
    const bool far = A.limit >= (kAxisNear + 1u) * (kAxisNear + 1u);  // an offset beyond the near steps can count
    unsigned long long acc = 0;      // kMorphEdt: the max key; kMorphThresh: the ones
    for (uint64_t tile = blockIdx.x; tile < X.tiles; tile += gridDim.x) {
        const uint64_t slab = tile / X.tiles_line;
        const uint64_t x0 = (tile - slab * X.tiles_line) << lg;
        const uint64_t base = slab * X.line * n + x0;
        for (uint32_t e = threadIdx.x; e < elems; e += kAxisThreads) {
            const uint32_t x = e & wmask, i = e >> lg;
            s_f[e] = x0 + x < X.line ? A.dist[base + x + (uint64_t)i * X.line] : kMorphNone;
        }
        __syncthreads();
        // (far is the launch's: a limit the near steps exhaust needs no minima and no second barrier)
        for (uint32_t q = threadIdx.x; far && q < (nb << lg); q += kAxisThreads) {
            const uint32_t x = q & wmask, b = q >> lg;
            uint32_t m = kMorphNone;
            for (uint32_t t = 0; t < kAxisBlock; ++t) {
                const uint32_t k = (b << kAxisBlockLog2) + t;
                if (k < n) m = min(m, s_f[(k << lg) | x]);
            }
            s_min[q] = m;
        }
        if (far) __syncthreads();
        for (uint32_t e = threadIdx.x; e < elems; e += kAxisThreads) {
            const uint32_t x = e & wmask, i = e >> lg;
            if (x0 + x >= X.line) continue;
            uint32_t best = s_f[e];
            // the offsets taken one by one: all of them unless blocks follow (far)
            const uint32_t dstop = far && kAxisNear + 1u < n ? kAxisNear + 1u : n;
            uint32_t d = 1;
#pragma unroll 1
            for (; d < dstop; ++d) {
                const uint32_t d2 = d * d;  // d < 32768
                if (d2 >= best || d2 > A.limit) break;
                if (d <= i) {
                    const uint32_t f = s_f[e - (d << lg)];
                    if (f != kMorphNone) best = min(best, f + d2);
                }
                if (d < n - i) {
                    const uint32_t f = s_f[e + (d << lg)];
                    if (f != kMorphNone) best = min(best, f + d2);
                }
            }
            if (d == dstop && dstop < n) {  // not stopped, and offsets left: far
                // (a block the near steps covered in part is read again: the minimum does not mind)
                const uint32_t ib = i >> kAxisBlockLog2;
                bool lo = true, hi = true;
                for (uint32_t j = 0; j < nb && (lo || hi); ++j) {
                    if (lo) {
                        if (j > ib) {
                            lo = false;
                        } else {
                            const uint32_t b = ib - j;
                            const uint32_t top = min((b << kAxisBlockLog2) + kAxisBlock - 1u, n - 1u);
                            const uint32_t dm = top >= i ? 0u : i - top;  // the block's nearest offset
                            const uint32_t dm2 = dm * dm;
                            if (dm2 >= best || dm2 > A.limit) {
                                lo = false;
                            } else {
                                const uint32_t fm = s_min[(b << lg) | x];
                                if (fm != kMorphNone && fm + dm2 < best) best = axis_scan_block(s_f, b, x, lg, n, i, best);
                            }
                        }
                    }
                    if (hi && j) {  // (j == 0 is the voxel's own block, read above)
                        const uint32_t b = ib + j;
                        if (b >= nb) {
                            hi = false;
                        } else {
                            const uint32_t dm = (b << kAxisBlockLog2) - i;  // above i: b > ib
                            const uint32_t dm2 = dm * dm;
                            if (dm2 >= best || dm2 > A.limit) {
                                hi = false;
                            } else {
                                const uint32_t fm = s_min[(b << lg) | x];
                                if (fm != kMorphNone && fm + dm2 < best) best = axis_scan_block(s_f, b, x, lg, n, i, best);
                            }
                        }
                    }
                }
            }
            if (best > A.limit) best = kMorphNone;
            const uint64_t l = base + x + (uint64_t)i * X.line;  // the box-linear index: below 2^32
            if (FIN == kMorphThresh) {
                const uint32_t one = (best != kMorphNone) != (A.invert != 0) ? 1u : 0u;
                A.out[l] = (uint8_t)one;
                acc += one;
            } else {
                A.dist[l] = best;
                if (FIN == kMorphEdt && best != kMorphNone) {
                    const unsigned long long key = (unsigned long long)best << 32 | (uint32_t)~(uint32_t)l;
                    acc = key > acc ? key : acc;
                }
            }
        }
        __syncthreads();  // (the next tile overwrites the columns)
    }
    if (FIN == kMorphStore) return;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(acc, o);
        if (FIN == kMorphEdt)
            acc = v > acc ? v : acc;
        else
            acc += v;
    }
    if ((threadIdx.x & 63u) == 0 && acc) {
        if (FIN == kMorphEdt)
            atomicMax(&A.cnt[1], acc);
        else
            atomicAdd(&A.cnt[2], acc);
    }
}

template <int FIN, int WORDS>
hipError_t launch_axis(const MorphArgs &a, const MorphAxis &X, hipStream_t stream)
{
    const uint32_t grid = (uint32_t)(X.tiles < kMaxGrid ? X.tiles : kMaxGrid);
    hipLaunchKernelGGL((morph_edt_axis_kernel<FIN, WORDS>), dim3(grid), dim3(kAxisThreads), 0, stream, a, X);
    return hipGetLastError();
}

bool args_ok(const MorphArgs &a, const MaskGrid &g)
{
    if (!a.dist || !a.cnt || (reinterpret_cast<uintptr_t>(a.dist) & 3u)) return false;
    for (int i = 0; i < 3; ++i)
        if (a.ext[i] != g.ext[i] || g.ext[i] < 1 || g.ext[i] > kMaskMaxExtent) return false;
    return g.voxels == (uint64_t)g.ext[0] * g.ext[1] * g.ext[2] && g.voxels <= kMaskMaxVoxels;
}

}  // namespace

hipError_t launch_morph_edt_x(const MorphArgs &a, const MaskGrid &g, hipStream_t stream, const char **name)
{
    if (!args_ok(a, g) || !a.mask || (a.elem_bytes != 1 && a.elem_bytes != 4)) return hipErrorInvalidValue;
    const uint64_t nrows = (uint64_t)g.ext[1] * g.ext[2];
    const uint64_t groups = (nrows + kXWaves - 1) / kXWaves;
    const uint32_t grid = (uint32_t)(groups < kMaxGrid ? groups : kMaxGrid);
    if (a.elem_bytes == 1) {
        hipLaunchKernelGGL(morph_edt_x_kernel<1>, dim3(grid), dim3(256), 0, stream, a, nrows);
        *name = "morph_edt_x_kernel<1>";
    } else {
        hipLaunchKernelGGL(morph_edt_x_kernel<4>, dim3(grid), dim3(256), 0, stream, a, nrows);
        *name = "morph_edt_x_kernel<4>";
    }
    return hipGetLastError();
}

hipError_t launch_morph_edt_axis(const MorphArgs &a, const MaskGrid &g, int axis, MorphFinal fin,
                                 hipStream_t stream, const char **name)
{
    if (!args_ok(a, g) || (axis != 1 && axis != 2) || (fin == kMorphThresh && !a.out)) return hipErrorInvalidValue;
    const MorphAxis X = morph_axis(g, axis);
    if (((uint64_t)X.n << X.width_log2) > X.lds_words) return hipErrorInvalidValue;
    const bool lng = X.lds_words == kMorphLdsWordsLong;
    switch (fin) {
        case kMorphStore:
            *name = lng ? "morph_edt_axis_kernel<0, 32768>" : "morph_edt_axis_kernel<0, 16384>";
            return lng ? launch_axis<kMorphStore, kMorphLdsWordsLong>(a, X, stream)
                       : launch_axis<kMorphStore, kMorphLdsWords>(a, X, stream);
        case kMorphEdt:
            *name = lng ? "morph_edt_axis_kernel<1, 32768>" : "morph_edt_axis_kernel<1, 16384>";
            return lng ? launch_axis<kMorphEdt, kMorphLdsWordsLong>(a, X, stream)
                       : launch_axis<kMorphEdt, kMorphLdsWords>(a, X, stream);
        case kMorphThresh:
            *name = lng ? "morph_edt_axis_kernel<2, 32768>" : "morph_edt_axis_kernel<2, 16384>";
            return lng ? launch_axis<kMorphThresh, kMorphLdsWordsLong>(a, X, stream)
                       : launch_axis<kMorphThresh, kMorphLdsWords>(a, X, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace vr
