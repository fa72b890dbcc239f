// vr_maskcc_kernels.hip — the connected components of a mask (include/vr/vr_maskcc.h): labels,
// records, the keep flags of a rule and the selection sweep; the gfx950 code object of
// lib/libvr_amd_maskcc.so.  DESIGN.md §4.14.
//
// The method is §4.12's lock-free union-find with the label array P as the parent array -- P[l] = 0
// for a voxel that is not labelled, else 1 + the index of a voxel of the same component that is not
// larger than l, l itself for a root -- fed by row runs instead of cells: the rows pass hangs every
// voxel under the first voxel of its run, the link pass unites each pair of runs that touch across
// two rows once, the flatten pass replaces every parent by the root, the component's smallest
// index.  Rules (§4.12's): no workgroup waits for another -- order comes from kernel boundaries;
// every loop is a grid-stride loop, a loop over a row's words, a strictly descending find or a
// unite whose retry strictly lowers a root; no load of P is relied on to be fresh; integer vector
// atomics only (atomicMin, atomicMax and atomicAdd on 32 and 64 bits); indices are 32-bit and
// addresses are formed in 64 bits; no scratch memory (make asm-maskcc).
#include "vr_maskcc_kernels.h"

namespace vr {
namespace {

constexpr uint32_t kNoRun = 0xFFFFFFFFu;

// parent + 1 of voxel x, as an agent-scope relaxed atomic load: served by the XCD's L2, which is not
// coherent with the other XCDs', so the value may be stale.  Nothing rests on its freshness: a stale
// parent is an older ancestor, and whether a word is zero never changes after the rows pass.
__device__ __forceinline__ uint32_t mcc_load(const uint32_t *P, uint64_t x)
{
    return __hip_atomic_load(P + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The root above labelled voxel x as far as this thread can see: still a voxel of x's component,
// and not below the true root.  A parent is smaller than its child, so the walk descends.
__device__ __forceinline__ uint32_t mcc_find(const uint32_t *P, uint32_t x)
{
    for (;;) {
        const uint32_t p = mcc_load(P, x) - 1u;
        if (p >= x) return x;  // (p == x: a root)
        x = p;
    }
}
// Unite the components of labelled voxels a and b.  atomicMin hangs the larger root under the
// smaller and returns what the word really held; where the larger one was no root any more (old !=
// hi + 1), the link to old - 1 that the minimum kept or replaced must not be lost: go on uniting
// old - 1 with lo.  hi falls on every retry.
__device__ __forceinline__ void mcc_unite(uint32_t *P, uint32_t a, uint32_t b)
{
    for (;;) {
        a = mcc_find(P, a);
        b = mcc_find(P, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicMin(P + (size_t)hi, lo + 1u);
        if (old == hi + 1u) return;
        a = old - 1u;
        b = lo;
    }
}

// Pass 1.  A wave per row, a lane per voxel, 64 voxels a round: the round's labelled voxels as one
// ballot word.  A labelled voxel stores 1 + the index of the first voxel of its run: the voxel
// after the highest clear bit below its own, or, where every bit below is set, the start of the
// run that reaches the word from the words before (the carry, the same in every lane).  INV
// labels the unset voxels.
template <int EB, int INV>
__global__ __launch_bounds__(256) void mcc_rows_kernel(const MccArgs A, const uint64_t nrows)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t bx = A.ext[0], nwords = (bx + 63u) >> 6;
    unsigned long long nin = 0;  // (the same in every lane of the wave)
    for (uint64_t row = (uint64_t)blockIdx.x * kMccRowWaves + wave; row < nrows;
         row += (uint64_t)gridDim.x * kMccRowWaves) {
        const uint64_t base = row * bx;  // base + x is below the voxel count
        uint32_t carry = kNoRun;
        for (uint32_t w = 0; w < nwords; ++w) {
            const uint32_t x = w * 64u + lane;
            const bool in = x < bx;
            bool set = false;
            if (in) {
                if (EB == 1)
                    set = (static_cast<const uint8_t *>(A.mask)[base + x] != 0) != (INV != 0);
                else
                    set = (static_cast<const uint32_t *>(A.mask)[base + x] != 0) != (INV != 0);
            }
            const unsigned long long m = __ballot(set);
            if (set) {
                const unsigned long long below = ~m & ((1ull << lane) - 1ull);  // the clear bits below the lane
                uint32_t start = w * 64u;
                if (below)
                    start += 64u - (uint32_t)__clzll((long long)below);
                else if (carry != kNoRun)
                    start = carry;
                A.P[base + x] = (uint32_t)base + start + 1u;
            } else if (in) {
                A.P[base + x] = 0u;
            }
            nin += (unsigned long long)__popcll(m);
            if (!(m >> 63))
                carry = kNoRun;
            else if (~m)
                carry = w * 64u + 64u - (uint32_t)__clzll((long long)~m);
            else if (carry == kNoRun)
                carry = w * 64u;
        }
    }
    if (lane == 0 && nin) atomicAdd(&A.cnt[kMccCntIn], nin);
}

// Pass 2.  A wave per row again.  The row's runs are united with the runs they touch in the rows
// before it in (z, y, x) order: rows (j - 1, k) and (j, k - 1) under 6, those two and (j - 1, k - 1)
// and (j + 1, k - 1) under 26, where a run also reaches one voxel further in x.  m and n are the
// ballot words of the two rows, ml and nl the same shifted by one voxel (bit c: the voxel at c - 1,
// across the word boundary from the word before).  Two runs overlap in one interval, and the lane
// of its first voxel unites them; under 26 two runs that do not overlap touch where one ends at
// c - 1 and the other starts at c, and lane c unites them.  So each pair of touching runs costs one
// unite, whatever its length.  Whether a word of P is zero is all that is read here but by unite.
template <int CONN>
__global__ __launch_bounds__(256) void mcc_link_kernel(const MccArgs A, const uint64_t nrows)
{
    constexpr int NR = CONN == 6 ? 2 : 4;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t bx = A.ext[0], by = A.ext[1], nwords = (bx + 63u) >> 6;
    const unsigned long long bit = 1ull << lane;
    uint32_t *P = A.P;
    for (uint64_t row = (uint64_t)blockIdx.x * kMccRowWaves + wave; row < nrows;
         row += (uint64_t)gridDim.x * kMccRowWaves) {
        const uint32_t k = (uint32_t)(row / by), j = (uint32_t)(row - (uint64_t)k * by);
        const uint64_t base = row * bx;
        bool have[NR];
        uint64_t nb[NR];  // the neighbour row's first voxel
        have[0] = j > 0;
        nb[0] = have[0] ? (row - 1) * bx : 0;
        have[1] = k > 0;
        nb[1] = have[1] ? (row - by) * bx : 0;
        if constexpr (NR == 4) {
            have[2] = j > 0 && k > 0;
            nb[2] = have[2] ? (row - by - 1) * bx : 0;
            have[3] = k > 0 && j + 1u < by;
            nb[3] = have[3] ? (row - by + 1) * bx : 0;
        }
        unsigned long long pm = 0, pn[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) pn[r] = 0;
        for (uint32_t w = 0; w < nwords; ++w) {
            const uint32_t x = w * 64u + lane;
            const bool in = x < bx;
            const unsigned long long m = __ballot(in && mcc_load(P, base + x) != 0u);
            const unsigned long long ml = (m << 1) | pm;
            pm = m >> 63;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                if (!have[r]) continue;  // (the wave's)
                const unsigned long long n = __ballot(in && mcc_load(P, nb[r] + x) != 0u);
                const unsigned long long nl = (n << 1) | pn[r];
                pn[r] = n >> 63;
                if (!((m | ml) & (n | nl))) continue;
                const uint32_t own = (uint32_t)(base + x), oth = (uint32_t)(nb[r] + x);
                if (m & n & ~(ml & nl) & bit) mcc_unite(P, own, oth);
                if (CONN == 26) {
                    if (m & ~ml & nl & ~n & bit) mcc_unite(P, own, oth - 1u);  // (c > 0: bit 0 of nl is 0 at c = 0)
                    if (n & ~nl & ml & ~m & bit) mcc_unite(P, own - 1u, oth);
                }
            }
        }
    }
}

// Pass 3.  A workgroup per chunk of kMccChunk voxels: P[l] = 1 + the root above l (a root keeps its
// own; writing a root over a parent leaves every concurrent find a valid ancestor), so P holds the
// labels.  On the way the roots -- P[l] == l + 1, which this pass never changes -- become the root
// table: a bit per voxel in 64-bit words (a ballot each), the count of the chunk's roots before
// each word, and the chunk's count.
__global__ __launch_bounds__(256) void mcc_flatten_kernel(const MccArgs A)
{
    static_assert(kMccChunk == 8192 && kMccChunkWords == 128, "32 rounds of 256 lanes, 128 ballots");
    __shared__ unsigned long long s_m[kMccChunkWords];
    __shared__ uint32_t s_tot[4];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * kMccChunk;
    uint32_t *P = A.P;
    for (uint32_t it = 0; it < 32u; ++it) {
        const uint64_t l64 = base + it * 256u + tid;
        bool root = false;
        if (l64 < (uint64_t)A.nvox) {
            const uint32_t l = (uint32_t)l64, p = mcc_load(P, l);
            if (p != 0u) {
                root = p == l + 1u;
                if (!root) P[(size_t)l] = mcc_find(P, p - 1u) + 1u;
            }
        }
        const unsigned long long b = __ballot(root);
        if (lane == 0) s_m[it * 4u + wave] = b;
    }
    __syncthreads();
    const unsigned long long m = tid < kMccChunkWords ? s_m[tid] : 0ull;
    const uint32_t cnt = (uint32_t)__popcll(m);
    uint32_t sc = cnt;  // inclusive over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t pv = __shfl_up(sc, off, 64);
        sc += (int)lane >= off ? pv : 0u;
    }
    if (lane == 63) s_tot[wave] = sc;
    __syncthreads();
    const uint32_t word = blockIdx.x * kMccChunkWords + tid;
    if (tid < kMccChunkWords && word < A.nwords) {
        A.bits[word] = m;
        A.wpre[word] = sc - cnt + (wave ? s_tot[0] : 0u);
    }
    if (tid == 0) A.chunk[blockIdx.x] = s_tot[0] + s_tot[1];
}

// Pass 4.  One workgroup: the chunks' root counts into their exclusive prefix, 256 chunks a round
// with a carry (at most 2^32 - 1 roots: 32 bits); the total, the components, into the counters.
__global__ __launch_bounds__(256) void mcc_scan_kernel(const MccArgs A)
{
    __shared__ uint32_t s_tot[2][4];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint32_t carry = 0, par = 0;
    for (uint32_t g0 = 0; g0 < A.nchunks; g0 += 256u, par ^= 1u) {
        const uint32_t g = g0 + tid;
        const uint32_t t = g < A.nchunks ? A.chunk[g] : 0u;
        uint32_t sc = t;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t pv = __shfl_up(sc, off, 64);
            sc += (int)lane >= off ? pv : 0u;
        }
        if (lane == 63) s_tot[par][wave] = sc;
        __syncthreads();
        uint32_t b = carry + (sc - t);
        for (uint32_t k = 0; k < wave; ++k) b += s_tot[par][k];
        if (g < A.nchunks) A.chunk[g] = b;
        carry += s_tot[par][0] + s_tot[par][1] + s_tot[par][2] + s_tot[par][3];
    }
    if (tid == 0) A.cnt[kMccCntComps] = carry;
}

// The record (vr_label_component, 64 bytes) as the table passes address it.
struct MccRecord {
    uint32_t label, reserved;
    unsigned long long voxels;
    uint32_t bmin[3], bmax[3];
    unsigned long long sum[3];
};
static_assert(sizeof(MccRecord) == kMccRecordBytes, "vr_label_component");
// What a lane or a wave has gathered for one label.
struct MccAcc {
    uint32_t cnt, mn[3], mx[3];
    unsigned long long sum[3];
};
__device__ __forceinline__ void mcc_acc_reset(MccAcc &a)
{
    a.cnt = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.mn[k] = 0xFFFFFFFFu;
        a.mx[k] = 0u;
        a.sum[k] = 0ull;
    }
}
__device__ __forceinline__ void mcc_acc_merge(MccAcc &a, const MccAcc &b)
{
    a.cnt += b.cnt;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.mn[k] = b.mn[k] < a.mn[k] ? b.mn[k] : a.mn[k];
        a.mx[k] = b.mx[k] > a.mx[k] ? b.mx[k] : a.mx[k];
        a.sum[k] += b.sum[k];
    }
}
__device__ __forceinline__ unsigned long long mcc_shfl_xor_u64(unsigned long long v, int off)
{
    const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}
// a over the lanes with `member` (the others give the identity); every lane of the wave calls it
__device__ __forceinline__ MccAcc mcc_acc_wave(const MccAcc &a, bool member)
{
    MccAcc r;
    mcc_acc_reset(r);
    if (member) r = a;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        MccAcc o;
        o.cnt = __shfl_xor(r.cnt, off, 64);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o.mn[k] = __shfl_xor(r.mn[k], off, 64);
            o.mx[k] = __shfl_xor(r.mx[k], off, 64);
            o.sum[k] = mcc_shfl_xor_u64(r.sum[k], off);
        }
        mcc_acc_merge(r, o);
    }
    return r;
}
// a into a record: integer atomics, mx already half open (index + 1).  (rec is null for a record
// index beyond the table, which no label of a flattened array has: nothing is written then.)
__device__ __forceinline__ void mcc_acc_flush(MccRecord *rec, const MccAcc &a)
{
    if (a.cnt == 0u || !rec) return;
    atomicAdd(&rec->voxels, (unsigned long long)a.cnt);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        atomicMin(&rec->bmin[k], a.mn[k]);
        atomicMax(&rec->bmax[k], a.mx[k]);
        atomicAdd(&rec->sum[k], a.sum[k]);
    }
}
// The record index of the component with label lab: the roots below its root, from the root table.
__device__ __forceinline__ uint32_t mcc_rank(const MccArgs &A, uint32_t lab)
{
    const uint32_t r = lab - 1u, w = r >> 6;
    return A.chunk[r / kMccChunk] + A.wpre[w] + (uint32_t)__popcll(A.bits[w] & ((1ull << (r & 63u)) - 1ull));
}
__device__ __forceinline__ MccRecord *mcc_record(const MccArgs &A, uint32_t lab)
{
    const uint32_t i = mcc_rank(A, lab);
    return i < A.ncomps ? static_cast<MccRecord *>(A.comps) + i : nullptr;
}

// Pass 5a.  The records before the sums: the identities of the reductions.
__global__ __launch_bounds__(256) void mcc_table_init_kernel(const MccArgs A)
{
    MccRecord *rec = static_cast<MccRecord *>(A.comps);
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < (uint64_t)A.ncomps;
         i += (uint64_t)gridDim.x * 256u) {
        MccRecord r;
        r.label = r.reserved = 0u;
        r.voxels = 0ull;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r.bmin[k] = 0xFFFFFFFFu;
            r.bmax[k] = 0u;
            r.sum[k] = 0ull;
        }
        rec[i] = r;
    }
}

// Pass 5b.  Count, bounding box and index sums per component, run by run: a wave per row, the
// row's labels as ballot words, and the lane of the first voxel of every run -- of its part in the
// word -- takes the whole part at once: its length from a bit scan, its x sum in closed form.  A
// lane keeps the sums of one label in registers.  A part of another label that is smaller than
// what the lane holds goes straight to its own record and the held sums stay: a large component,
// which a lane returns to after every speck it crosses, is not handed to its one contended record
// at each crossing (§4.12's first build paid that).  The second part in a row of the same other
// label (`miss`) takes the lane over, so that a lane which has moved into another large component
// gathers for it.  At the end the wave combines, twice, the lanes that share its first pending
// lane's label, and what is left goes singly.  There are no LDS slots.  Every sum is an integer,
// so no order shows in the result.  A root also stores its record's label.
constexpr int kMccWaveRounds = 2;
__global__ __launch_bounds__(256) void mcc_accum_kernel(const MccArgs A, const uint64_t nrows)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t bx = A.ext[0], by = A.ext[1], nwords = (bx + 63u) >> 6;
    const uint32_t *__restrict__ P = A.P;
    uint32_t key = 0, miss = 0;  // the label the lane gathers for, the last one it sent on alone; 0: none
    MccAcc acc;
    mcc_acc_reset(acc);
    for (uint64_t row = (uint64_t)blockIdx.x * kMccRowWaves + wave; row < nrows;
         row += (uint64_t)gridDim.x * kMccRowWaves) {
        const uint32_t k = (uint32_t)(row / by), j = (uint32_t)(row - (uint64_t)k * by);
        const uint64_t base = row * bx;
        for (uint32_t w = 0; w < nwords; ++w) {
            const uint32_t x = w * 64u + lane;
            const uint32_t lab = x < bx ? P[base + x] : 0u;
            const unsigned long long m = __ballot(lab != 0u);
            if ((m & ~(m << 1)) >> lane & 1ull) {  // the first voxel of a part
                const unsigned long long z = ~m >> lane;          // (bit 0 is clear: the lane's own voxel)
                const uint32_t len = z ? (uint32_t)__ffsll((long long)z) - 1u : 64u - lane;
                if (lab == (uint32_t)base + x + 1u)
                    if (MccRecord *own = mcc_record(A, lab)) own->label = lab;
                MccAcc t;
                t.cnt = len;
                t.mn[0] = x;
                t.mx[0] = x + len;
                t.mn[1] = j;
                t.mx[1] = j + 1u;
                t.mn[2] = k;
                t.mx[2] = k + 1u;
                t.sum[0] = (unsigned long long)(len * (2u * x + len - 1u) / 2u);  // x + .. + (x + len - 1)
                t.sum[1] = (unsigned long long)j * len;
                t.sum[2] = (unsigned long long)k * len;
                if (key == lab) {
                    mcc_acc_merge(acc, t);
                } else if (key != 0u && lab != miss && acc.cnt > len) {  // a speck crossed: its part goes alone
                    mcc_acc_flush(mcc_record(A, lab), t);
                    miss = lab;
                } else {
                    if (key != 0u) mcc_acc_flush(mcc_record(A, key), acc);
                    acc = t;
                    key = lab;
                    miss = 0u;
                }
            }
        }
    }
    bool pend = key != 0u;
#pragma unroll
    for (int round = 0; round < kMccWaveRounds; ++round) {
        const unsigned long long todo = __ballot(pend);
        if (!todo) break;  // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lk = (uint32_t)__shfl((int)key, leader, 64);
        const bool same = pend && key == lk;
        const MccAcc r = mcc_acc_wave(acc, same);
        if ((int)lane == leader) mcc_acc_flush(mcc_record(A, lk), r);
        pend = pend && !same;
    }
    if (pend) mcc_acc_flush(mcc_record(A, key), acc);
}

// Pass 5c.  The largest component: the maximum of voxels : ~label in 64 bits (most voxels, ties to
// the smallest label; a component has at most 2^32 - 1 voxels).
__global__ __launch_bounds__(256) void mcc_largest_kernel(const MccArgs A)
{
    const MccRecord *rec = static_cast<const MccRecord *>(A.comps);
    unsigned long long best = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < (uint64_t)A.ncomps;
         i += (uint64_t)gridDim.x * 256u) {
        const unsigned long long k = (rec[i].voxels << 32) | (unsigned long long)(~rec[i].label);
        best = k > best ? k : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = mcc_shfl_xor_u64(best, off);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63u) == 0 && best) atomicMax(&A.cnt[kMccCntLargest], best);
}

// Pass 6a.  One flag per record from the rule: its label against the largest component's or the
// seed's, its count against min_voxels, or its bounding box against the grid's faces (a hole
// touches none); the kept records are counted.
__global__ __launch_bounds__(256) void mcc_keep_kernel(const MccArgs A)
{
    const MccRecord *rec = static_cast<const MccRecord *>(A.comps);
    const uint32_t largest = ~(uint32_t)A.cnt[kMccCntLargest];
    const uint32_t seed_label = A.rule == kMccKeepSeed ? A.P[(size_t)A.seed] : 0u;
    uint32_t kept = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < (uint64_t)A.ncomps;
         i += (uint64_t)gridDim.x * 256u) {
        const MccRecord r = rec[i];
        bool keep;
        if (A.rule == kMccKeepLargest)
            keep = r.label == largest;
        else if (A.rule == kMccKeepMinVoxels)
            keep = r.voxels >= A.min_voxels;
        else if (A.rule == kMccKeepSeed)
            keep = r.label == seed_label;
        else
            keep = r.bmin[0] > 0u && r.bmin[1] > 0u && r.bmin[2] > 0u && r.bmax[0] < A.ext[0] && r.bmax[1] < A.ext[1] &&
                   r.bmax[2] < A.ext[2];
        A.flags[i] = keep ? (uint8_t)1 : (uint8_t)0;
        kept += keep ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kept += __shfl_xor(kept, off, 64);
    if ((threadIdx.x & 63u) == 0 && kept) atomicAdd(&A.cnt[kMccCntKept], (unsigned long long)kept);
}

// Pass 6b.  The sweep: each voxel's byte is its record's flag, looked up through the root table;
// a voxel without a label is 0, or 1 under FILL, where the labels are those of the unset voxels
// and an unlabelled voxel is a set one.  The ones are counted.
template <int FILL>
__global__ __launch_bounds__(256) void mcc_select_kernel(const MccArgs A)
{
    const uint32_t *__restrict__ P = A.P;
    uint32_t ones = 0;  // (a thread sees at most 2^32 / 256 voxels)
    for (uint64_t l = (uint64_t)blockIdx.x * 256u + threadIdx.x; l < (uint64_t)A.nvox; l += (uint64_t)gridDim.x * 256u) {
        const uint32_t lab = P[l];
        uint32_t one = FILL ? 1u : 0u;
        if (lab != 0u) {
            const uint32_t i = mcc_rank(A, lab);
            one = i < A.ncomps ? (uint32_t)A.flags[i] : 0u;
        }
        A.out[l] = (uint8_t)one;
        ones += one;
    }
    unsigned long long sum = ones;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += mcc_shfl_xor_u64(sum, off);
    if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(&A.cnt[kMccCntOnes], sum);
}

bool args_ok(const MccArgs &a, const MaskGrid &g, const MccGeom &G)
{
    if (!a.P || !a.bits || !a.wpre || !a.chunk || !a.cnt || (reinterpret_cast<uintptr_t>(a.P) & 3u)) return false;
    for (int i = 0; i < 3; ++i)
        if (a.ext[i] != g.ext[i] || g.ext[i] < 1 || g.ext[i] > kMaskMaxExtent) return false;
    if (g.voxels != (uint64_t)g.ext[0] * g.ext[1] * g.ext[2] || g.voxels > kMaskMaxVoxels) return false;
    return a.nvox == (uint32_t)g.voxels && a.nwords == G.nwords && a.nchunks == G.nchunks;
}

uint32_t record_grid(uint32_t ncomps)
{
    const uint32_t per = (ncomps + 255u) / 256u;
    return per < kMccMaxGrid ? per : kMccMaxGrid;
}

}  // namespace

hipError_t launch_mcc(MccPass pass, const MccArgs &a, const MaskGrid &g, uint32_t connectivity, hipStream_t stream,
                      const char **name)
{
    const MccGeom G = mcc_geometry(g);
    if (!args_ok(a, g, G)) return hipErrorInvalidValue;
    const bool records = pass >= kMccTableInit && pass <= kMccKeep;
    if (records && (!a.comps || a.ncomps == 0 || (uint64_t)a.ncomps > g.voxels)) return hipErrorInvalidValue;
    if (pass == kMccSelect && (!a.out || (a.ncomps && !a.flags))) return hipErrorInvalidValue;
    const dim3 rows(G.row_grid), block(256);
    switch (pass) {
        case kMccRows: {
            if (!a.mask || (a.elem_bytes != 1 && a.elem_bytes != 4)) return hipErrorInvalidValue;
            if (a.elem_bytes == 1 && !a.invert) {
                hipLaunchKernelGGL((mcc_rows_kernel<1, 0>), rows, block, 0, stream, a, G.rows);
                *name = "mcc_rows_kernel<1, 0>";
            } else if (a.elem_bytes == 1) {
                hipLaunchKernelGGL((mcc_rows_kernel<1, 1>), rows, block, 0, stream, a, G.rows);
                *name = "mcc_rows_kernel<1, 1>";
            } else if (!a.invert) {
                hipLaunchKernelGGL((mcc_rows_kernel<4, 0>), rows, block, 0, stream, a, G.rows);
                *name = "mcc_rows_kernel<4, 0>";
            } else {
                hipLaunchKernelGGL((mcc_rows_kernel<4, 1>), rows, block, 0, stream, a, G.rows);
                *name = "mcc_rows_kernel<4, 1>";
            }
            break;
        }
        case kMccLink:
            if (connectivity == 6) {
                hipLaunchKernelGGL(mcc_link_kernel<6>, rows, block, 0, stream, a, G.rows);
                *name = "mcc_link_kernel<6>";
            } else if (connectivity == 26) {
                hipLaunchKernelGGL(mcc_link_kernel<26>, rows, block, 0, stream, a, G.rows);
                *name = "mcc_link_kernel<26>";
            } else {
                return hipErrorInvalidValue;
            }
            break;
        case kMccFlatten:
            hipLaunchKernelGGL(mcc_flatten_kernel, dim3(G.nchunks), block, 0, stream, a);
            *name = "mcc_flatten_kernel";
            break;
        case kMccScan:
            hipLaunchKernelGGL(mcc_scan_kernel, dim3(1), block, 0, stream, a);
            *name = "mcc_scan_kernel";
            break;
        case kMccTableInit:
            hipLaunchKernelGGL(mcc_table_init_kernel, dim3(record_grid(a.ncomps)), block, 0, stream, a);
            *name = "mcc_table_init_kernel";
            break;
        case kMccAccum:
            hipLaunchKernelGGL(mcc_accum_kernel, rows, block, 0, stream, a, G.rows);
            *name = "mcc_accum_kernel";
            break;
        case kMccLargest:
            hipLaunchKernelGGL(mcc_largest_kernel, dim3(record_grid(a.ncomps)), block, 0, stream, a);
            *name = "mcc_largest_kernel";
            break;
        case kMccKeep:
            if (!a.flags || a.rule >= kMccRules || (a.rule == kMccKeepSeed && a.seed >= a.nvox)) return hipErrorInvalidValue;
            hipLaunchKernelGGL(mcc_keep_kernel, dim3(record_grid(a.ncomps)), block, 0, stream, a);
            *name = "mcc_keep_kernel";
            break;
        case kMccSelect:
            if (a.rule == kMccFillHoles) {
                hipLaunchKernelGGL(mcc_select_kernel<1>, dim3(G.sweep_grid), block, 0, stream, a);
                *name = "mcc_select_kernel<1>";
            } else {
                hipLaunchKernelGGL(mcc_select_kernel<0>, dim3(G.sweep_grid), block, 0, stream, a);
                *name = "mcc_select_kernel<0>";
            }
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace vr
