// vr_mmesh_kernels.hip — the kernels of include/vr/vr_mmesh.h, built into lib/libvr_amd_mmesh.so.
//
// The array is read once.  mmesh_bits_kernel packs "this node is inside" at one bit a node: a wave
// takes 64 consecutive nodes of one x row, a lane an element, and one ballot is the row's word (the
// ring's bits are 0 and are never read from memory).  Everything after it works on words: a cell
// row's active word is (OR of 8) & ~(AND of 8) over four node-row words and their one-bit shifts,
// the three "owned crossing edge" words are XORs of the same words, the counts are popcounts.
// The counts are scanned in cell-linear word order, which is the order of the output, so a cell's
// vertex is the prefix of its word plus the popcount of the active bits below it -- for the cell
// itself, for the four cells of a quad and for the six neighbours of a smoothing sweep alike.
// The emit passes give a wave a word and a lane a cell; they find the words that hold anything 64 at
// a time.  No float atomics: every result is a gather in a fixed order.
//
// Bounds.  Every word index is below node_words or cell_words by its loop; a vertex id is below the
// scanned total and a triangle offset below the triangle total, both of which the host has compared
// with the capacities before an emit pass is launched.
#include "vr_mmesh_kernels.h"

#pragma clang fp contract(off)

namespace vr {
namespace {

typedef unsigned long long u64;
constexpr int kBitsInFlight = 8;  // node words of a wave in flight in mmesh_bits_kernel

__device__ __forceinline__ uint32_t wave_first() { return __builtin_amdgcn_readfirstlane(blockIdx.x * kMmeshWaves + (threadIdx.x >> 6)); }
__device__ __forceinline__ uint32_t wave_count() { return gridDim.x * kMmeshWaves; }
__device__ __forceinline__ uint32_t pop64(u64 v) { return (uint32_t)__popcll(v); }

__device__ __forceinline__ u64 wave_sum(u64 v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}

// The sums of a and b over the workgroup, in every thread.  Every thread calls it.
__device__ __forceinline__ void block_sum2(u64 &a, u64 &b)
{
    __shared__ u64 s_sum[kMmeshWaves][2];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    a = wave_sum(a);
    b = wave_sum(b);
    __syncthreads();  // (an earlier call's readers are done)
    if (lane == 0) {
        s_sum[wave][0] = a;
        s_sum[wave][1] = b;
    }
    __syncthreads();
    a = b = 0;
#pragma unroll
    for (uint32_t w = 0; w < kMmeshWaves; ++w) {
        a += s_sum[w][0];
        b += s_sum[w][1];
    }
}

__device__ __forceinline__ uint32_t wave_inclusive(uint32_t x, uint32_t lane)
{
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    return x;
}

// ---- the inside bits ----
template <typename ELEM>
__global__ __launch_bounds__(kMmeshBlock) void mmesh_bits_kernel(MmeshArgs A)
{
    const uint32_t lane = threadIdx.x & 63u, nwaves = wave_count();
    const ELEM *__restrict__ arr = static_cast<const ELEM *>(A.array);
    u64 matching = 0;
    for (uint32_t t0 = wave_first(); t0 < A.node_words; t0 += nwaves * kBitsInFlight) {
        uint32_t e[kBitsInFlight];
        bool in[kBitsInFlight];
#pragma unroll
        for (int u = 0; u < kBitsInFlight; ++u) {
            const u64 task = (u64)t0 + (u64)u * nwaves;
            in[u] = false;
            e[u] = 0;
            if (task < A.node_words) {
                const uint32_t row = (uint32_t)task / A.nw, w = (uint32_t)task - row * A.nw;
                const uint32_t nz = row / A.nn[1], ny = row - nz * A.nn[1];
                // grid voxel of the node; a ring node wraps to a huge value and fails the compare
                const uint32_t gx = w * kMmeshWord + lane - A.ring, gy = ny - A.ring, gz = nz - A.ring;
                in[u] = gx < A.ext[0] && gy < A.ext[1] && gz < A.ext[2];
                if (in[u]) e[u] = (uint32_t)arr[(size_t)gx + (size_t)A.ext[0] * ((size_t)gy + (size_t)A.ext[1] * gz)];
            }
        }
#pragma unroll
        for (int u = 0; u < kBitsInFlight; ++u) {
            const u64 task = (u64)t0 + (u64)u * nwaves;
            if (task < A.node_words) {
                const bool m = in[u] && (A.select == kMmeshLabel ? e[u] == A.label : e[u] != 0u);
                const u64 word = __ballot(m);
                if (lane == 0) A.bits[task] = word;
                matching += pop64(word);
            }
        }
    }
    if (lane == 0 && matching) atomicAdd(A.matching, matching);
}

// ---- a cell word ----
// The node words around cell word i: r0 .. r3 are node rows (cy, cz), (cy + 1, cz), (cy, cz + 1),
// (cy + 1, cz + 1) at the cell's own x, s0 .. s3 the same rows one node on in x, so bit x of
// (r0, s0, r1, s1, r2, s2, r3, s3) is corner 0 .. 7 of cell x.  valid: the cells of the word.
struct CellWord {
    u64 r0, s0, r1, s1, r2, s2, r3, s3, valid;
    uint32_t w, cy, cz;
};

__device__ __forceinline__ void node_pair(const MmeshArgs &A, size_t at, bool more, u64 &r, u64 &s)
{
    const u64 lo = A.bits[at], hi = more ? A.bits[at + 1] : 0ull;
    r = lo;
    s = (lo >> 1) | (hi << 63);
}

__device__ __forceinline__ void load_cell_word(const MmeshArgs &A, uint32_t i, CellWord &W)
{
    const uint32_t row = i / A.cw;
    W.w = i - row * A.cw;
    W.cz = row / A.nc[1];
    W.cy = row - W.cz * A.nc[1];
    const bool more = W.w + 1 < A.nw;
    const size_t dy = A.nw, dz = (size_t)A.nn[1] * A.nw;
    const size_t at = ((size_t)W.cz * A.nn[1] + W.cy) * A.nw + W.w;
    node_pair(A, at, more, W.r0, W.s0);
    node_pair(A, at + dy, more, W.r1, W.s1);
    node_pair(A, at + dz, more, W.r2, W.s2);
    node_pair(A, at + dz + dy, more, W.r3, W.s3);
    const uint32_t rem = A.nc[0] - W.w * kMmeshWord;
    W.valid = rem >= kMmeshWord ? ~0ull : (1ull << rem) - 1ull;
}

__device__ __forceinline__ u64 active_of(const CellWord &W)
{
    const u64 any = W.r0 | W.s0 | W.r1 | W.s1 | W.r2 | W.s2 | W.r3 | W.s3;
    const u64 all = W.r0 & W.s0 & W.r1 & W.s1 & W.r2 & W.s2 & W.r3 & W.s3;
    return any & ~all & W.valid;
}

// The crossing edges P -> P + e_a that cell P owns: all four cells around the edge are in the set,
// so P is not in the first cell row or column across the edge.
__device__ __forceinline__ void edges_of(const CellWord &W, u64 &qx, u64 &qy, u64 &qz)
{
    const u64 y1 = W.cy >= 1 ? ~0ull : 0ull, z1 = W.cz >= 1 ? ~0ull : 0ull;
    const u64 x1 = W.w == 0 ? ~1ull : ~0ull;
    qx = (W.r0 ^ W.s0) & W.valid & y1 & z1;
    qy = (W.r0 ^ W.r1) & W.valid & z1 & x1;
    qz = (W.r0 ^ W.r2) & W.valid & x1 & y1;
}

__device__ __forceinline__ uint32_t corners_of(const CellWord &W, uint32_t lane)
{
    return (uint32_t)((W.r0 >> lane) & 1ull) | (uint32_t)((W.s0 >> lane) & 1ull) << 1 |
           (uint32_t)((W.r1 >> lane) & 1ull) << 2 | (uint32_t)((W.s1 >> lane) & 1ull) << 3 |
           (uint32_t)((W.r2 >> lane) & 1ull) << 4 | (uint32_t)((W.s2 >> lane) & 1ull) << 5 |
           (uint32_t)((W.r3 >> lane) & 1ull) << 6 | (uint32_t)((W.s3 >> lane) & 1ull) << 7;
}

__device__ __forceinline__ void group_range(const MmeshArgs &A, u64 &begin, u64 &end)
{
    begin = (u64)blockIdx.x * A.span;
    end = begin + A.span;
    if (end > A.cell_words) end = A.cell_words;
}

// ---- classify: the active words, the counts of every word, the sums of every workgroup ----
__global__ __launch_bounds__(kMmeshBlock) void mmesh_classify_kernel(MmeshArgs A)
{
    u64 begin, end;
    group_range(A, begin, end);
    u64 sv = 0, st = 0;
    for (u64 i = begin + threadIdx.x; i < end; i += kMmeshBlock) {
        CellWord W;
        load_cell_word(A, (uint32_t)i, W);
        const u64 act = active_of(W);
        u64 qx, qy, qz;
        edges_of(W, qx, qy, qz);
        const uint32_t v = pop64(act), t = 2u * (pop64(qx) + pop64(qy) + pop64(qz));
        A.active[i] = act;
        A.pre_v[i] = v | t << 16;  // v <= 64, t <= 384
        sv += v;
        st += t;
    }
    block_sum2(sv, st);
    if (threadIdx.x == 0) {
        A.gsum[2 * blockIdx.x] = sv;
        A.gsum[2 * blockIdx.x + 1] = st;
    }
}

// ---- scan: the counts of every word into the vertices and triangles before it ----
__global__ __launch_bounds__(kMmeshBlock) void mmesh_scan_kernel(MmeshArgs A)
{
    __shared__ uint32_t s_wave[kMmeshWaves][2];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    u64 bv = 0, bt = 0;  // before this workgroup's span, then before the tile
    for (uint32_t j = tid; j < blockIdx.x; j += kMmeshBlock) {
        bv += A.gsum[2 * j];
        bt += A.gsum[2 * j + 1];
    }
    block_sum2(bv, bt);
    u64 begin, end;
    group_range(A, begin, end);
    for (u64 base = begin; base < end; base += kMmeshScanTile) {
        const u64 i = base + tid;
        const bool in = i < end;
        const uint32_t p = in ? A.pre_v[i] : 0u;
        const uint32_t v = p & 0xFFFFu, t = p >> 16;
        const uint32_t iv = wave_inclusive(v, lane), it = wave_inclusive(t, lane);
        if (lane == 63) {
            s_wave[wave][0] = iv;
            s_wave[wave][1] = it;
        }
        __syncthreads();
        uint32_t ov = 0, ot = 0, tv = 0, tt = 0;
#pragma unroll
        for (uint32_t w = 0; w < kMmeshWaves; ++w) {
            const uint32_t a = s_wave[w][0], b = s_wave[w][1];
            if (w < wave) {
                ov += a;
                ot += b;
            }
            tv += a;
            tt += b;
        }
        if (in) {
            A.pre_v[i] = (uint32_t)(bv + ov + iv - v);
            A.pre_t[i] = bt + ot + it - t;
        }
        bv += tv;
        bt += tt;
        __syncthreads();
    }
}

// ---- the emit passes' walk ----
// f(i, act) for every cell word i with an active bit, the whole wave together: a wave loads 64
// active words at a time and visits those that are not zero.
template <class F>
__device__ __forceinline__ void for_each_active_word(const MmeshArgs &A, F f)
{
    const uint32_t lane = threadIdx.x & 63u;
    const u64 chunks = ((u64)A.cell_words + 63u) >> 6;
    for (u64 ch = wave_first(); ch < chunks; ch += wave_count()) {
        const u64 mine = (ch << 6) + lane;
        const u64 a = mine < A.cell_words ? A.active[mine] : 0ull;
        u64 todo = __ballot(a != 0ull);
        while (todo) {
            const uint32_t k = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint32_t lo = __shfl((uint32_t)a, k, 64), hi = __shfl((uint32_t)(a >> 32), k, 64);
            f((uint32_t)(ch << 6) + k, ((u64)hi << 32) | lo);
        }
    }
}

__device__ __forceinline__ u64 below(uint32_t lane) { return (1ull << lane) - 1ull; }

// The vertex of cell (x, y, z), which is active.
__device__ __forceinline__ uint32_t vertex_of(const MmeshArgs &A, uint32_t x, uint32_t y, uint32_t z)
{
    const size_t i = (size_t)(x >> 6) + (size_t)A.cw * ((size_t)y + (size_t)A.nc[1] * z);
    return A.pre_v[i] + pop64(A.active[i] & below(x & 63u));
}

// vr_mesh.h's vertex arithmetic with node values 1.0f and 0.0f and iso 0.5f: every crossing edge
// has t = 0.5f, every partial sum is a multiple of 0.5f (exact), and the division rounds once.
__device__ __forceinline__ void cell_local(uint32_t m, float &lx, float &ly, float &lz)
{
    constexpr int EA[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3};
    constexpr int EB[12] = {1, 3, 5, 7, 2, 3, 6, 7, 4, 5, 6, 7};
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    uint32_t n = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int axis = e >> 2, a = EA[e], b = EB[e];
        if (((m >> a) ^ (m >> b)) & 1u) {
            sx = sx + (axis == 0 ? 0.5f : (float)(a & 1));
            sy = sy + (axis == 1 ? 0.5f : (float)((a >> 1) & 1));
            sz = sz + (axis == 2 ? 0.5f : (float)(a >> 2));
            n = n + 1;
        }
    }
    const float fn = (float)n;
    lx = sx / fn;
    ly = sy / fn;
    lz = sz / fn;
}

__device__ __forceinline__ float pos_of(const MmeshArgs &A, int a, uint32_t c, float local)
{
    const int C = (int)A.origin[a] + (int)c - (int)A.ring;
    return (((float)C + 0.5f) + local) / A.fdims[a];
}

// ---- vertices: local of every active cell, its normal, and with LAST its position ----
template <bool LAST>
__global__ __launch_bounds__(kMmeshBlock) void mmesh_vertex_kernel(MmeshArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    for_each_active_word(A, [&](uint32_t i, u64 act) {
        if (!((act >> lane) & 1ull)) return;
        CellWord W;
        load_cell_word(A, i, W);
        const uint32_t m = corners_of(W, lane);
        const uint32_t vid = A.pre_v[i] + pop64(act & below(lane));
        float lx, ly, lz;
        cell_local(m, lx, ly, lz);
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (A.normals) {
            const int gx = (int)__popc(m & 0xAAu) - (int)__popc(m & 0x55u);
            const int gy = (int)__popc(m & 0xCCu) - (int)__popc(m & 0x33u);
            const int gz = (int)__popc(m & 0xF0u) - (int)__popc(m & 0x0Fu);
            const float g2 = (float)(gx * gx + gy * gy + gz * gz);
            if (g2 > 0.0f) {
                const float r = 1.0f / sqrtf(g2);
                nx = (float)(-gx) * r;
                ny = (float)(-gy) * r;
                nz = (float)(-gz) * r;
            }
        }
        float *rec = static_cast<float *>(A.verts) + (size_t)vid * 6;
        if (LAST) {
            rec[0] = pos_of(A, 0, W.w * kMmeshWord + lane, lx);
            rec[1] = pos_of(A, 1, W.cy, ly);
            rec[2] = pos_of(A, 2, W.cz, lz);
        } else {
            float *l = A.loc_out + (size_t)vid * 3;
            l[0] = lx;
            l[1] = ly;
            l[2] = lz;
        }
        rec[3] = nx;
        rec[4] = ny;
        rec[5] = nz;
    });
}

// ---- one Jacobi sweep: loc_in -> loc_out, or with LAST -> the records' positions ----
template <int OX, int OY, int OZ, uint32_t FACE>
__device__ __forceinline__ void neighbour(const MmeshArgs &A, bool in_set, uint32_t m, uint32_t x, uint32_t y, uint32_t z,
                                          float &q0, float &q1, float &q2, uint32_t &cnt)
{
    const uint32_t f = m & FACE;
    if (!in_set || f == 0u || f == FACE) return;
    const float *l = A.loc_in + (size_t)vertex_of(A, x + OX, y + OY, z + OZ) * 3;
    const float t0 = l[0] + (float)OX, t1 = l[1] + (float)OY, t2 = l[2] + (float)OZ;
    q0 = q0 + t0;
    q1 = q1 + t1;
    q2 = q2 + t2;
    cnt = cnt + 1;
}

__device__ __forceinline__ float relax_to(float local, float q, float fcnt, float relax)
{
    const float m = q / fcnt;
    const float d = m - local;
    const float s = relax * d;
    float v = local + s;
    if (!(v >= 0.0f)) v = 0.0f;
    if (v > 1.0f) v = 1.0f;
    return v;
}

template <bool LAST>
__global__ __launch_bounds__(kMmeshBlock) void mmesh_smooth_kernel(MmeshArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    for_each_active_word(A, [&](uint32_t i, u64 act) {
        if (!((act >> lane) & 1ull)) return;
        CellWord W;
        load_cell_word(A, i, W);
        const uint32_t m = corners_of(W, lane);
        const uint32_t vid = A.pre_v[i] + pop64(act & below(lane));
        const uint32_t x = W.w * kMmeshWord + lane, y = W.cy, z = W.cz;
        const float *l = A.loc_in + (size_t)vid * 3;
        float v0 = l[0], v1 = l[1], v2 = l[2];
        float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f;
        uint32_t cnt = 0;
        neighbour<-1, 0, 0, 0x55u>(A, x >= 1, m, x, y, z, q0, q1, q2, cnt);
        neighbour<1, 0, 0, 0xAAu>(A, x + 1 < A.nc[0], m, x, y, z, q0, q1, q2, cnt);
        neighbour<0, -1, 0, 0x33u>(A, y >= 1, m, x, y, z, q0, q1, q2, cnt);
        neighbour<0, 1, 0, 0xCCu>(A, y + 1 < A.nc[1], m, x, y, z, q0, q1, q2, cnt);
        neighbour<0, 0, -1, 0x0Fu>(A, z >= 1, m, x, y, z, q0, q1, q2, cnt);
        neighbour<0, 0, 1, 0xF0u>(A, z + 1 < A.nc[2], m, x, y, z, q0, q1, q2, cnt);
        if (cnt) {
            const float fcnt = (float)cnt;
            v0 = relax_to(v0, q0, fcnt, A.relax);
            v1 = relax_to(v1, q1, fcnt, A.relax);
            v2 = relax_to(v2, q2, fcnt, A.relax);
        }
        if (LAST) {
            float *rec = static_cast<float *>(A.verts) + (size_t)vid * 6;
            rec[0] = pos_of(A, 0, x, v0);
            rec[1] = pos_of(A, 1, y, v1);
            rec[2] = pos_of(A, 2, z, v2);
        } else {
            float *o = A.loc_out + (size_t)vid * 3;
            o[0] = v0;
            o[1] = v1;
            o[2] = v2;
        }
    });
}

// ---- triangles: two per owned crossing edge, in cell order, then x, y, z ----
__device__ __forceinline__ void quad(uint32_t *t, bool inside_p, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3)
{
    t[0] = c0;
    t[1] = inside_p ? c1 : c2;
    t[2] = inside_p ? c2 : c1;
    t[3] = c0;
    t[4] = inside_p ? c2 : c3;
    t[5] = inside_p ? c3 : c2;
}

__global__ __launch_bounds__(kMmeshBlock) void mmesh_triangle_kernel(MmeshArgs A)
{
    const uint32_t lane = threadIdx.x & 63u;
    for_each_active_word(A, [&](uint32_t i, u64 act) {
        CellWord W;
        load_cell_word(A, i, W);
        u64 qx, qy, qz;
        edges_of(W, qx, qy, qz);
        if (!(((qx | qy | qz) >> lane) & 1ull)) return;
        const u64 lo = below(lane);
        u64 at = A.pre_t[i] + 2ull * (pop64(qx & lo) + pop64(qy & lo) + pop64(qz & lo));
        const bool inside_p = (W.r0 >> lane) & 1ull;
        const uint32_t x = W.w * kMmeshWord + lane, y = W.cy, z = W.cz;
        const uint32_t c2 = A.pre_v[i] + pop64(act & lo);
        if ((qx >> lane) & 1ull) {  // b = y, c = z
            quad(A.tris + (size_t)at * 3, inside_p, vertex_of(A, x, y - 1, z - 1), vertex_of(A, x, y, z - 1), c2,
                 vertex_of(A, x, y - 1, z));
            at += 2;
        }
        if ((qy >> lane) & 1ull) {  // b = z, c = x
            quad(A.tris + (size_t)at * 3, inside_p, vertex_of(A, x - 1, y, z - 1), vertex_of(A, x - 1, y, z), c2,
                 vertex_of(A, x, y, z - 1));
            at += 2;
        }
        if ((qz >> lane) & 1ull) {  // b = x, c = y
            quad(A.tris + (size_t)at * 3, inside_p, vertex_of(A, x - 1, y - 1, z), vertex_of(A, x, y - 1, z), c2,
                 vertex_of(A, x - 1, y, z));
        }
    });
}

uint32_t walk_groups(const MmeshArgs &a)
{
    const uint64_t chunks = ((uint64_t)a.cell_words + 63) / 64;
    const uint64_t g = (chunks + kMmeshWaves - 1) / kMmeshWaves;
    return (uint32_t)(g > kMmeshMaxGroups ? kMmeshMaxGroups : g);
}

}  // namespace

hipError_t launch_mmesh_bits(uint32_t elem_bytes, const MmeshArgs &a, hipStream_t stream, const char **name)
{
    if ((elem_bytes != 1 && elem_bytes != 4) || a.node_words == 0) return hipErrorInvalidValue;
    const uint64_t g = ((uint64_t)a.node_words + kMmeshWaves - 1) / kMmeshWaves;
    const dim3 grid((uint32_t)(g > kMmeshMaxGroups ? kMmeshMaxGroups : g)), block(kMmeshBlock);
    if (elem_bytes == 1) {
        hipLaunchKernelGGL(mmesh_bits_kernel<uint8_t>, grid, block, 0, stream, a);
        *name = "mmesh_bits_kernel<u8>";
    } else {
        hipLaunchKernelGGL(mmesh_bits_kernel<uint32_t>, grid, block, 0, stream, a);
        *name = "mmesh_bits_kernel<u32>";
    }
    return hipGetLastError();
}

hipError_t launch_mmesh_classify(const MmeshArgs &a, hipStream_t stream, const char **name)
{
    if (a.cell_words == 0 || a.groups == 0 || a.groups > kMmeshMaxGroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mmesh_classify_kernel, dim3(a.groups), dim3(kMmeshBlock), 0, stream, a);
    *name = "mmesh_classify_kernel";
    return hipGetLastError();
}

hipError_t launch_mmesh_scan(const MmeshArgs &a, hipStream_t stream, const char **name)
{
    if (a.cell_words == 0 || a.groups == 0 || a.groups > kMmeshMaxGroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mmesh_scan_kernel, dim3(a.groups), dim3(kMmeshBlock), 0, stream, a);
    *name = "mmesh_scan_kernel";
    return hipGetLastError();
}

hipError_t launch_mmesh_vertices(const MmeshArgs &a, bool last, hipStream_t stream, const char **name)
{
    if (a.cell_words == 0) return hipErrorInvalidValue;
    const dim3 grid(walk_groups(a)), block(kMmeshBlock);
    if (last) {
        hipLaunchKernelGGL(mmesh_vertex_kernel<true>, grid, block, 0, stream, a);
        *name = "mmesh_vertex_kernel<last>";
    } else {
        hipLaunchKernelGGL(mmesh_vertex_kernel<false>, grid, block, 0, stream, a);
        *name = "mmesh_vertex_kernel<local>";
    }
    return hipGetLastError();
}

hipError_t launch_mmesh_smooth(const MmeshArgs &a, bool last, hipStream_t stream, const char **name)
{
    if (a.cell_words == 0) return hipErrorInvalidValue;
    const dim3 grid(walk_groups(a)), block(kMmeshBlock);
    if (last) {
        hipLaunchKernelGGL(mmesh_smooth_kernel<true>, grid, block, 0, stream, a);
        *name = "mmesh_smooth_kernel<last>";
    } else {
        hipLaunchKernelGGL(mmesh_smooth_kernel<false>, grid, block, 0, stream, a);
        *name = "mmesh_smooth_kernel<local>";
    }
    return hipGetLastError();
}

hipError_t launch_mmesh_triangles(const MmeshArgs &a, hipStream_t stream, const char **name)
{
    if (a.cell_words == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mmesh_triangle_kernel, dim3(walk_groups(a)), dim3(kMmeshBlock), 0, stream, a);
    *name = "mmesh_triangle_kernel";
    return hipGetLastError();
}

}  // namespace vr
