// vr_mstat_kernels.hip — the statistics of the volume under a device mask or label array, and the
// value-window pass that writes a mask (include/vr/vr_mstat.h); the gfx950 code object of
// lib/libvr_amd_mstat.so.  DESIGN.md §4.15.
//
// The voxel passes walk the grid in box-linear order, a tile of kMstatTileX x kMstatTileY voxels a
// workgroup iteration and a row of it a wave, and read a voxel's element of the base bricks only
// where the array is non-zero: 64 voxels of a row are eight whole brick rows.  Rules (§4.12's): no
// workgroup waits for another -- order comes from kernel boundaries; every loop is a grid-stride
// loop, a loop over a wave's lanes, or a search bounded by log2 of the table; integer vector
// atomics only (atomicAdd and atomicMax on 32 and 64 bits), but the two sums on f32 storage, which
// take the hardware's double add on device memory after the wave and workgroup combine (never a
// compare-and-swap loop); indices are 32-bit and addresses are formed in 64 bits; no scratch memory
// (make asm-mstat).
#include "vr_mstat_kernels.h"

#include "vr_internal.h"  // read, never edited: the bricks' own constants, for the asserts below

namespace vr {
namespace {

// vr_mstat_host.h restates the brick addressing; these tie it to the bricks'.
static_assert(kGroupShift == 0 && brick_slot(3, 5, 7, 11, 13) == (7u * 13u + 5u) * 11u + 3u, "mstat_element: brick_slot");
static_assert(kPad == (int)kMstatPad && kF32VoxelsPerElement == 2 && VR_U8_PLAIN != 0, "mstat_layout");
constexpr bool layout_is(const MstatLayout &L, int bx, int by, int bz, int ex, int ey, int elems)
{
    return (int)L.bx == bx && (int)L.by == by && (int)L.bz == bz && (int)L.ex == ex && (int)L.ey == ey &&
           (int)L.elems == elems;
}
static_assert(layout_is(mstat_layout(kMstatF32), GeomWide::BX, GeomWide::BY, GeomWide::BZ, GeomWide::EX, GeomWide::EY,
                        GeomWide::Elems) &&
                  layout_is(mstat_layout(kMstatQuad16), GeomWide::BX, GeomWide::BY, GeomWide::BZ, GeomWide::EX,
                            GeomWide::EY, GeomWide::Elems) &&
                  layout_is(mstat_layout(kMstatQuad8), GeomWide::BX, GeomWide::BY, GeomWide::BZ, GeomWide::EX,
                            GeomWide::EY, GeomWide::Elems) &&
                  layout_is(mstat_layout(kMstatPlain8), GeomByte::BX, GeomByte::BY, GeomByte::BZ, GeomByte::EX,
                            GeomByte::EY, GeomByte::Elems),
              "mstat_layout: GeomWide, GeomByte");
static_assert(mstat_bricks(509, 8) == 65 && mstat_bricks(5, 7) == 2, "mstat_bricks: bricks_for");

using u64 = unsigned long long;

__device__ __forceinline__ uint32_t mstat_ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mstat_unorder(uint32_t o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int off)
{
    const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_down_u64(u64 v, int off)
{
    const uint32_t lo = __shfl_down((uint32_t)v, off, 64), hi = __shfl_down((uint32_t)(v >> 32), off, 64);
    return ((u64)hi << 32) | lo;
}

// What a lane, a wave or a workgroup has gathered for one region; all zero is the identity.  sum and
// sum2 hold integers (FLT 0) or the bits of doubles (FLT 1).
struct Part {
    uint32_t count, nan;
    u64 kmax, kmin, sum, sum2;
};
__device__ __forceinline__ Part part_zero() { return Part{0u, 0u, 0ull, 0ull, 0ull, 0ull}; }
template <bool FLT>
__device__ __forceinline__ u64 sum_add(u64 a, u64 b)
{
    if constexpr (FLT)
        return (u64)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
    else
        return a + b;
}
template <bool FLT>
__device__ __forceinline__ void part_merge(Part &a, const Part &b)
{
    a.count += b.count;
    a.nan += b.nan;
    a.kmax = b.kmax > a.kmax ? b.kmax : a.kmax;
    a.kmin = b.kmin > a.kmin ? b.kmin : a.kmin;
    a.sum = sum_add<FLT>(a.sum, b.sum);
    a.sum2 = sum_add<FLT>(a.sum2, b.sum2);
}
// voxel l with value f, once
template <bool FLT>
__device__ __forceinline__ Part part_of(float f, uint32_t l)
{
    Part p = part_zero();
    p.count = 1u;
    if (f != f) {
        p.nan = 1u;
        return p;
    }
    const uint32_t o = mstat_ordered(f == 0.0f ? 0.0f : f);  // -0.0 orders as 0
    p.kmax = ((u64)o << 32) | (u64)(~l);
    p.kmin = ((u64)(~o) << 32) | (u64)(~l);
    if constexpr (FLT) {
        const double d = f == 0.0f ? 0.0 : (double)f;  // a zero term is +0.0: no sum is -0.0
        p.sum = (u64)__double_as_longlong(d);
        p.sum2 = (u64)__double_as_longlong(d * d);  // exact: 48 bits of product
    } else {
        const long long v = (long long)f;  // exact: the stored integer
        p.sum = (u64)v;
        p.sum2 = (u64)(v * v);
    }
    return p;
}
__device__ __forceinline__ Part part_shfl_xor(const Part &p, int off)
{
    Part o;
    o.count = __shfl_xor(p.count, off, 64);
    o.nan = __shfl_xor(p.nan, off, 64);
    o.kmax = shfl_xor_u64(p.kmax, off);
    o.kmin = shfl_xor_u64(p.kmin, off);
    o.sum = shfl_xor_u64(p.sum, off);
    o.sum2 = shfl_xor_u64(p.sum2, off);
    return o;
}
__device__ __forceinline__ Part part_shfl_down(const Part &p, int off)
{
    Part o;
    o.count = __shfl_down(p.count, off, 64);
    o.nan = __shfl_down(p.nan, off, 64);
    o.kmax = shfl_down_u64(p.kmax, off);
    o.kmin = shfl_down_u64(p.kmin, off);
    o.sum = shfl_down_u64(p.sum, off);
    o.sum2 = shfl_down_u64(p.sum2, off);
    return o;
}
// p over the lanes with `member` (the others give the identity); every lane of the wave calls it
template <bool FLT>
__device__ __forceinline__ Part part_wave(const Part &p, bool member)
{
    Part r = part_zero();
    if (member) r = p;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part_merge<FLT>(r, part_shfl_xor(r, off));
    return r;
}
// p into a region's accumulators
template <bool FLT>
__device__ __forceinline__ void part_flush(MstatAcc *a, const Part &p)
{
    if (p.count == 0u) return;
    atomicAdd(&a->count, (u64)p.count);
    if (p.nan) atomicAdd(&a->nan, (u64)p.nan);
    if (p.kmax == 0ull) return;  // NaN only
    atomicMax(&a->kmax, p.kmax);
    atomicMax(&a->kmin, p.kmin);
    if constexpr (FLT) {
        unsafeAtomicAdd(reinterpret_cast<double *>(&a->sum), __longlong_as_double((long long)p.sum));
        unsafeAtomicAdd(reinterpret_cast<double *>(&a->sum2), __longlong_as_double((long long)p.sum2));
    } else {
        atomicAdd(&a->sum, p.sum);
        atomicAdd(&a->sum2, p.sum2);
    }
}

// The wave's voxel of tile t: grid voxel (x, j, k), inside the grid or not, and its box-linear index.
struct Voxel {
    uint32_t x, j, k, l;
    bool in;
};
__device__ __forceinline__ Voxel tile_voxel(const MstatArgs &A, uint32_t t, uint32_t tiles_x, uint32_t tiles_y)
{
    const uint32_t tx = t % tiles_x, r = t / tiles_x, ty = r % tiles_y;
    Voxel v;
    v.k = r / tiles_y;
    v.j = ty * kMstatTileY + (threadIdx.x >> 6);
    v.x = tx * kMstatTileX + (threadIdx.x & 63u);
    v.in = v.x < A.ext[0] && v.j < A.ext[1];
    v.l = v.in ? v.x + A.ext[0] * (v.j + A.ext[1] * v.k) : 0u;  // below 2^32 - 1 (mask_grid_resolve)
    return v;
}
// the array's element of voxel l is non-zero (a NULL array: every voxel is set)
__device__ __forceinline__ bool array_set(const MstatArgs &A, uint32_t l)
{
    if (!A.array) return true;
    if (A.elem_bytes == 1u) return static_cast<const uint8_t *>(A.array)[(size_t)l] != 0;
    return static_cast<const uint32_t *>(A.array)[(size_t)l] != 0u;
}
// f = (float)stored of the grid voxel: component 0 of its element
template <typename T, int KIND>
__device__ __forceinline__ float voxel_value(const MstatArgs &A, const Voxel &v)
{
    constexpr MstatLayout L = mstat_layout(KIND);
    const uint64_t e = mstat_element(L, A.nbx, A.nby, A.origin[0] + v.x, A.origin[1] + v.j, A.origin[2] + v.k);
    return (float)static_cast<const T *>(A.vol)[e * L.vpe];
}

// Pass: labels[i] = table[i].label, byte by byte (the table may have any alignment).
__global__ __launch_bounds__(256) void mstat_gather_kernel(const MstatArgs A)
{
    const uint8_t *tab = static_cast<const uint8_t *>(A.table);
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < (uint64_t)A.nrec; i += (uint64_t)gridDim.x * 256u) {
        const uint8_t *r = tab + i * kMstatRecordBytes;
        A.labels[i] = (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
    }
}

// Pass: the one region of a mask.  A lane gathers its voxels in registers; the waves combine by
// shuffles, the workgroup through LDS, and one thread adds to the accumulators.  HIST: the bins of
// vr_hist.h over the set voxels, hist_kernel's rule restated -- a first guess in double corrected
// against the edge table in LDS, 32-bit counters private to the workgroup (it sees far fewer than
// 2^32 voxels), flushed with one 64-bit atomic per non-zero bin.
template <typename T, int KIND, bool HIST>
__global__ __launch_bounds__(256) void mstat_mask_kernel(const MstatArgs A, const uint32_t tiles_x,
                                                         const uint32_t tiles_y, const uint64_t tiles)
{
    constexpr bool FLT = std::is_same<T, float>::value;
    __shared__ uint32_t s_bins[HIST ? kHistMaxBins : 1];
    __shared__ float s_edges[HIST ? kHistMaxBins : 1];
    __shared__ Part s_part[4];
    __shared__ uint32_t s_side[4][2];
    const uint32_t tid = threadIdx.x, nbins = A.nbins;
    if constexpr (HIST) {
        for (uint32_t i = tid; i < nbins; i += 256) {
            s_bins[i] = 0;
            s_edges[i] = A.edges[i];
        }
        __syncthreads();
    }
    const float lo = A.lo, hi = A.hi;
    const double dlo = (double)lo, scale = A.scale;
    Part acc = part_zero();
    uint32_t below = 0, above = 0;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const Voxel v = tile_voxel(A, (uint32_t)t, tiles_x, tiles_y);
        if (!v.in || !array_set(A, v.l)) continue;
        const float f = voxel_value<T, KIND>(A, v);
        part_merge<FLT>(acc, part_of<FLT>(f, v.l));
        if constexpr (HIST) {
            if (f == f) {
                const bool lt = f < lo, gt = f > hi;
                below += lt ? 1u : 0u;
                above += gt ? 1u : 0u;
                if (!lt && !gt) {
                    const double g = ((double)f - dlo) * scale;
                    uint32_t b = g >= (double)(nbins - 1) ? nbins - 1 : (g > 0.0 ? (uint32_t)g : 0u);
                    while (b + 1 < nbins && s_edges[b + 1] <= f) ++b;
                    while (b > 0 && s_edges[b] > f) --b;
                    atomicAdd(&s_bins[b], 1u);
                }
            }
        }
    }
    acc = part_wave<FLT>(acc, true);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        below += __shfl_xor(below, off, 64);
        above += __shfl_xor(above, off, 64);
    }
    if ((tid & 63u) == 0) {
        s_part[tid >> 6] = acc;
        s_side[tid >> 6][0] = below;
        s_side[tid >> 6][1] = above;
    }
    __syncthreads();
    if constexpr (HIST) {
        for (uint32_t i = tid; i < nbins; i += 256) {
            const uint32_t n = s_bins[i];
            if (n) atomicAdd(&A.bins[i], (u64)n);
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            part_merge<FLT>(acc, s_part[w]);
            below += s_side[w][0];
            above += s_side[w][1];
        }
        part_flush<FLT>(A.acc, acc);
        if (below) atomicAdd(&A.cnt[kMstatCntBelow], (u64)below);
        if (above) atomicAdd(&A.cnt[kMstatCntAbove], (u64)above);
    }
}

// The record slot of label lab: a binary search of the compacted labels, at most 32 steps, every
// probe inside [0, n) whatever the table holds.
__device__ __forceinline__ uint32_t label_slot(const uint32_t *__restrict__ labels, uint32_t n, uint32_t lab)
{
    uint32_t lo = 0, hi = n;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (labels[(size_t)mid] < lab)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo < n && labels[(size_t)lo] == lab ? lo : kMstatNone;
}

// Pass: one region per listed label.  A wave's 64 labels fall into runs of equal labels; the first
// lane of a run searches the run's slot once and hands it to the run's lanes, and a segmented
// reduction brings the run's voxels to that lane.  A lane keeps the sums of one slot in registers:
// a run of the same slot merges, and of two different ones the larger stays and the smaller goes to
// its accumulators, so a large region crossed by specks is not handed to its one contended record at
// every crossing (§4.14).  At the end the wave combines, kLabelRounds times, the lanes that share
// its first pending lane's slot; the workgroup merges these through LDS, and what is left goes
// singly.
constexpr int kLabelRounds = 2;
template <typename T, int KIND>
__global__ __launch_bounds__(256) void mstat_labels_kernel(const MstatArgs A, const uint32_t tiles_x,
                                                           const uint32_t tiles_y, const uint64_t tiles)
{
    constexpr bool FLT = std::is_same<T, float>::value;
    __shared__ Part s_part[4 * kLabelRounds];
    __shared__ uint32_t s_key[4 * kLabelRounds];
    __shared__ uint32_t s_side[4][2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t *__restrict__ labels = static_cast<const uint32_t *>(A.array);
    uint32_t key = kMstatNone, nset = 0, unlisted = 0;
    Part acc = part_zero();
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const Voxel v = tile_voxel(A, (uint32_t)t, tiles_x, tiles_y);
        const uint32_t lab = v.in ? labels[(size_t)v.l] : 0u;
        if (!__ballot(lab != 0u)) continue;  // wave-uniform
        const uint32_t prev = __shfl_up(lab, 1, 64);
        const bool start = lane == 0u || lab != prev;
        const u64 sm = __ballot(start);  // (bit 0 is set)
        const uint32_t head = 63u - (uint32_t)__clzll((long long)(sm & (~0ull >> (63u - lane))));
        const u64 above = lane == 63u ? 0ull : sm & ~((2ull << lane) - 1ull);
        const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 2u : 63u;  // the run's last lane
        uint32_t slot = kMstatNone;
        if (start && lab != 0u) slot = label_slot(A.labels, A.nrec, lab);
        slot = __shfl(slot, (int)head, 64);
        Part p = part_zero();
        if (lab != 0u) {
            ++nset;
            if (slot == kMstatNone)
                ++unlisted;
            else
                p = part_of<FLT>(voxel_value<T, KIND>(A, v), v.l);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const Part o = part_shfl_down(p, off);
            if (lane + (uint32_t)off <= end) part_merge<FLT>(p, o);
        }
        if (start && slot != kMstatNone) {
            if (key == slot) {
                part_merge<FLT>(acc, p);
            } else if (key != kMstatNone && acc.count > p.count) {
                part_flush<FLT>(A.acc + slot, p);
            } else {
                if (key != kMstatNone) part_flush<FLT>(A.acc + key, acc);
                acc = p;
                key = slot;
            }
        }
    }
    bool pend = key != kMstatNone;
#pragma unroll
    for (int round = 0; round < kLabelRounds; ++round) {
        const u64 todo = __ballot(pend);
        uint32_t lk = kMstatNone;
        Part r = part_zero();
        if (todo) {  // wave-uniform
            const int leader = __ffsll((long long)todo) - 1;
            lk = (uint32_t)__shfl((int)key, leader, 64);
            const bool same = pend && key == lk;
            r = part_wave<FLT>(acc, same);
            pend = pend && !same;
        }
        if (lane == 0u) {
            s_key[wave * kLabelRounds + round] = lk;
            s_part[wave * kLabelRounds + round] = r;
        }
    }
    if (pend) part_flush<FLT>(A.acc + key, acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nset += __shfl_xor(nset, off, 64);
        unlisted += __shfl_xor(unlisted, off, 64);
    }
    if (lane == 0u) {
        s_side[wave][0] = nset;
        s_side[wave][1] = unlisted;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 0; i < 4 * kLabelRounds; ++i) {
            const uint32_t k = s_key[i];
            if (k == kMstatNone) continue;
            Part r = s_part[i];
            for (int j = i + 1; j < 4 * kLabelRounds; ++j)
                if (s_key[j] == k) {
                    part_merge<FLT>(r, s_part[j]);
                    s_key[j] = kMstatNone;
                }
            part_flush<FLT>(A.acc + k, r);
        }
        for (int w = 1; w < 4; ++w) {
            nset += s_side[w][0];
            unlisted += s_side[w][1];
        }
        if (nset) atomicAdd(&A.cnt[kMstatCntSet], (u64)nset);
        if (unlisted) atomicAdd(&A.cnt[kMstatCntUnlisted], (u64)unlisted);
    }
}

// The record (vr_mstat_region, 64 bytes) as the finalize pass writes it.
struct MstatRecord {
    uint32_t label, reserved;
    u64 voxels, nan;
    float vmin, vmax;
    uint32_t min_index, max_index;
    double sum, sum2;
    u64 reserved2;
};
static_assert(sizeof(MstatRecord) == kMstatRecordBytes, "vr_mstat_region");

// Pass: the records from the accumulators.  Integer sums are converted to double here, once.
template <bool FLT>
__global__ __launch_bounds__(256) void mstat_finalize_kernel(const MstatArgs A)
{
    MstatRecord *rec = static_cast<MstatRecord *>(A.rec);
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < (uint64_t)A.nrec; i += (uint64_t)gridDim.x * 256u) {
        const MstatAcc a = A.acc[i];
        MstatRecord r;
        r.label = A.labels ? A.labels[i] : 1u;
        r.reserved = 0u;
        r.voxels = a.count;
        r.nan = a.nan;
        const bool any = a.kmax != 0ull;
        r.vmax = any ? mstat_unorder((uint32_t)(a.kmax >> 32)) : -INFINITY;
        r.vmin = any ? mstat_unorder(~(uint32_t)(a.kmin >> 32)) : INFINITY;
        r.max_index = any ? ~(uint32_t)a.kmax : kMstatNone;
        r.min_index = any ? ~(uint32_t)a.kmin : kMstatNone;
        if constexpr (FLT) {
            r.sum = __longlong_as_double((long long)a.sum);
            r.sum2 = __longlong_as_double((long long)a.sum2);
        } else {
            r.sum = (double)(long long)a.sum;
            r.sum2 = (double)a.sum2;
        }
        r.reserved2 = 0ull;
        rec[i] = r;
    }
}

// Pass: out = set && lo <= f && f <= hi, compared in f32 (a NaN is never in); the set voxels and the
// ones are counted.  The value is read only where the array is set.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void mstat_window_kernel(const MstatArgs A, const uint32_t tiles_x,
                                                           const uint32_t tiles_y, const uint64_t tiles)
{
    __shared__ uint32_t s_side[4][2];
    const uint32_t tid = threadIdx.x;
    const float lo = A.lo, hi = A.hi;
    uint32_t nset = 0, ones = 0;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const Voxel v = tile_voxel(A, (uint32_t)t, tiles_x, tiles_y);
        if (!v.in) continue;
        uint32_t one = 0u;
        if (array_set(A, v.l)) {
            ++nset;
            const float f = voxel_value<T, KIND>(A, v);
            one = lo <= f && f <= hi ? 1u : 0u;
        }
        A.out[(size_t)v.l] = (uint8_t)one;
        ones += one;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nset += __shfl_xor(nset, off, 64);
        ones += __shfl_xor(ones, off, 64);
    }
    if ((tid & 63u) == 0) {
        s_side[tid >> 6][0] = nset;
        s_side[tid >> 6][1] = ones;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            nset += s_side[w][0];
            ones += s_side[w][1];
        }
        if (nset) atomicAdd(&A.cnt[kMstatCntSet], (u64)nset);
        if (ones) atomicAdd(&A.cnt[kMstatCntOut], (u64)ones);
    }
}

bool args_ok(const MstatArgs &a, const MaskGrid &g)
{
    if (!a.cnt) return false;
    for (int i = 0; i < 3; ++i)
        if (a.ext[i] != g.ext[i] || a.origin[i] != g.origin[i] || g.ext[i] < 1 || g.ext[i] > kMaskMaxExtent) return false;
    return g.voxels == (uint64_t)g.ext[0] * g.ext[1] * g.ext[2] && g.voxels <= kMaskMaxVoxels;
}

// DO(T, KIND, "tag") for the kernel types of base layout code `layout`; `bad` for any other code.
#define MSTAT_FOR_LAYOUT(layout, DO, bad)                                \
    switch (layout) {                                                    \
        case ST_F32: DO(float, kMstatF32, "f32"); break;                 \
        case ST_U16: DO(uint16_t, kMstatQuad16, "u16"); break;           \
        case ST_I16: DO(int16_t, kMstatQuad16, "i16"); break;            \
        case ST_U8 | kQuadFlag: DO(uint8_t, kMstatQuad8, "quad_u8"); break; \
        case ST_I8 | kQuadFlag: DO(int8_t, kMstatQuad8, "quad_i8"); break;  \
        case ST_U8: DO(uint8_t, kMstatPlain8, "u8"); break;              \
        case ST_I8: DO(int8_t, kMstatPlain8, "i8"); break;               \
        default: bad;                                                    \
    }

}  // namespace

hipError_t launch_mstat(MstatPass pass, int layout, const MstatArgs &a, const MaskGrid &g, hipStream_t stream,
                        const char **name)
{
    if (!args_ok(a, g)) return hipErrorInvalidValue;
    const MstatGeom G = mstat_geometry(g, a.nrec);
    const dim3 vox(G.grid), recs(G.rec_grid), block(256);
    const bool voxel_pass = pass == kMstatMask || pass == kMstatLabels || pass == kMstatWindow;
    if (voxel_pass && (!a.vol || !a.nbx || !a.nby || (a.array && a.elem_bytes != 1 && a.elem_bytes != 4)))
        return hipErrorInvalidValue;
    const bool flt = layout == ST_F32;
    switch (pass) {
        case kMstatGather:
            if (!a.table || !a.labels || !a.nrec) return hipErrorInvalidValue;
            hipLaunchKernelGGL(mstat_gather_kernel, recs, block, 0, stream, a);
            *name = "mstat_gather_kernel";
            break;
        case kMstatMask:
            if (!a.array || !a.acc || a.nrec != 1 || (a.nbins && (!a.bins || !a.edges || a.nbins > kHistMaxBins)))
                return hipErrorInvalidValue;
#define MSTAT_DO(T, KIND, TAG)                                                                                     \
    if (a.nbins) {                                                                                                 \
        hipLaunchKernelGGL((mstat_mask_kernel<T, KIND, true>), vox, block, 0, stream, a, G.tiles_x, G.tiles_y, G.tiles); \
        *name = "mstat_mask_kernel<" TAG ", hist>";                                                                \
    } else {                                                                                                       \
        hipLaunchKernelGGL((mstat_mask_kernel<T, KIND, false>), vox, block, 0, stream, a, G.tiles_x, G.tiles_y, G.tiles); \
        *name = "mstat_mask_kernel<" TAG ">";                                                                      \
    }
            MSTAT_FOR_LAYOUT(layout, MSTAT_DO, return hipErrorInvalidValue)
#undef MSTAT_DO
            break;
        case kMstatLabels:
            // (an empty table: every non-zero element is unlisted)
            if (!a.array || a.elem_bytes != 4 || (a.nrec && (!a.acc || !a.labels))) return hipErrorInvalidValue;
#define MSTAT_DO(T, KIND, TAG)                                                                                  \
    hipLaunchKernelGGL((mstat_labels_kernel<T, KIND>), vox, block, 0, stream, a, G.tiles_x, G.tiles_y, G.tiles); \
    *name = "mstat_labels_kernel<" TAG ">";
            MSTAT_FOR_LAYOUT(layout, MSTAT_DO, return hipErrorInvalidValue)
#undef MSTAT_DO
            break;
        case kMstatFinalize:
            if (!a.acc || !a.rec || !a.nrec) return hipErrorInvalidValue;
            if (flt) {
                hipLaunchKernelGGL(mstat_finalize_kernel<true>, recs, block, 0, stream, a);
                *name = "mstat_finalize_kernel<f32>";
            } else {
                hipLaunchKernelGGL(mstat_finalize_kernel<false>, recs, block, 0, stream, a);
                *name = "mstat_finalize_kernel<int>";
            }
            break;
        case kMstatWindow:
            if (!a.out) return hipErrorInvalidValue;
#define MSTAT_DO(T, KIND, TAG)                                                                                  \
    hipLaunchKernelGGL((mstat_window_kernel<T, KIND>), vox, block, 0, stream, a, G.tiles_x, G.tiles_y, G.tiles); \
    *name = "mstat_window_kernel<" TAG ">";
            MSTAT_FOR_LAYOUT(layout, MSTAT_DO, return hipErrorInvalidValue)
#undef MSTAT_DO
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace vr
