// vr_mview_kernels.hip — the kernels of include/vr/vr_mview.h, built into lib/libvr_amd_mview.so.
//
// A lookup is no filter: a sample is one element of the array, found by three f32 multiplies, a
// grid test and (with the occupancy words) one 4-byte load that says whether the array has to be
// read at all.  A ray stops at its first match, so almost every sample a frame walks lies in unset
// voxels; the words (at most 2 MiB) stay in L1 / L2 while the array (134 MB for a 512^3 byte mask)
// does not, so with them the scattered reads happen only near the surface.
//
// pixel_ray is vr_kernels.hip's, restated statement for statement (that unit is not shared): the
// double unprojection, the slab intersection, the entry-face snap, then the f32 direction.  The walk
// is hit_strip's: nsteps, the f32 position update, the bounds break, the strict slab test.  Positions
// are serial f32 additions, but the loads need not be: K samples of a lane are in flight, their
// positions formed first, their words loaded together, then their elements, and they are examined
// in step order, so the record is the same for every K.
#include "vr_mview_kernels.h"

#pragma clang fp contract(off)

namespace vr {
namespace {

typedef unsigned long long u64;
constexpr int kMviewInFlight = 4;   // samples of a lane in flight
constexpr uint32_t kMviewTile = 16;  // a workgroup: 16 x 16 pixels, a wave a 16 x 4 strip

__device__ __forceinline__ u64 wave_sum(u64 v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}

// The four counters of a workgroup of four waves: per wave, then across them in LDS, then one
// atomic per non-zero counter.  Every thread of the workgroup calls it.
__device__ __forceinline__ void flush_counters(u64 *cnt, u64 c0, u64 c1, u64 c2, u64 c3)
{
    __shared__ u64 s_cnt[4][kMviewCounters];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    c2 = wave_sum(c2);
    c3 = wave_sum(c3);
    if (lane == 0) {
        s_cnt[wave][0] = c0;
        s_cnt[wave][1] = c1;
        s_cnt[wave][2] = c2;
        s_cnt[wave][3] = c3;
    }
    __syncthreads();
    if (tid < (uint32_t)kMviewCounters) {
        const u64 v = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
        if (v) atomicAdd(&cnt[tid], v);
    }
}

template <typename ELEM>
__device__ __forceinline__ uint32_t load_elem(const void *__restrict__ array, uint32_t l)
{
    return (uint32_t) static_cast<const ELEM *>(array)[l];
}

__device__ __forceinline__ bool matches(const MviewArray &S, uint32_t e)
{
    return S.select == kMviewLabel ? e == S.label : e != 0u;
}

// vr_mview.h "voxel of a position": one f32 multiply, truncation, the clamp to n - 1.
__device__ __forceinline__ int voxel_of(float p, float fn, uint32_t n)
{
    const float t = p * fn;
    const int v = (int)t;
    return v > (int)n - 1 ? (int)n - 1 : v;
}

// The grid voxel of volume voxel (vx, vy, vz): false outside the grid (the unsigned compare takes a
// voxel below the origin, or outside the volume, with it); else its box-linear index and its cell.
__device__ __forceinline__ bool grid_voxel(const MviewArray &S, int vx, int vy, int vz, uint32_t &l, uint32_t &m)
{
    const uint32_t gx = (uint32_t)vx - S.origin[0], gy = (uint32_t)vy - S.origin[1], gz = (uint32_t)vz - S.origin[2];
    const bool in = vx >= 0 && vy >= 0 && vz >= 0 && gx < S.ext[0] && gy < S.ext[1] && gz < S.ext[2];
    l = in ? gx + S.ext[0] * (gy + S.ext[1] * gz) : 0u;
    m = in ? mview_cell_index(gx, gy, gz, S.c0, S.c1) : 0u;
    return in;
}

// One candidate sample of a lane: its element to examine, or none.
struct Lookup {
    uint32_t l, m, e;
    bool cand;
};

// The elements of K candidates: with OCC their words first, all K loads issued together, and the
// array only where the bit is set; then the K array loads together.
template <typename ELEM, bool OCC, int K>
__device__ __forceinline__ void fetch(const MviewArray &S, Lookup (&L)[K])
{
    if constexpr (OCC) {
        uint32_t w[K];
#pragma unroll
        for (int s = 0; s < K; ++s) w[s] = L[s].cand ? S.occ[L[s].m >> 5] : 0u;
#pragma unroll
        for (int s = 0; s < K; ++s) L[s].cand = L[s].cand && ((w[s] >> (L[s].m & 31u)) & 1u);
    }
#pragma unroll
    for (int s = 0; s < K; ++s) L[s].e = L[s].cand ? load_elem<ELEM>(S.array, L[s].l) : 0u;
}

// Pixel-centre ray -> cube entry: vr_kernels.hip's pixel_ray.
__device__ __forceinline__ bool mview_pixel_ray(const MarchParams &P, uint32_t px, uint32_t py, float tex[3],
                                                float dir[3])
{
    const double *m = P.inv;
    const double x = ((double)px + 0.5) / P.fw * 2.0 - 1.0;
    const double y = ((double)py + 0.5) / P.fh * 2.0 - 1.0;
    double h0[4], h1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        h0[r] = m[0 * 4 + r] * x + m[1 * 4 + r] * y + m[3 * 4 + r];
        h1[r] = h0[r] + m[2 * 4 + r];
    }
    double p0[3], d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        p0[r] = h0[r] / h0[3];
        d[r] = h1[r] / h1[3] - p0[r];
    }
    double te = -__builtin_inf(), tx = __builtin_inf();
    int axis = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double lo, hi;
        if (d[a] == 0.0) {
            if (p0[a] < -0.5 || p0[a] > 0.5) return false;
            lo = -__builtin_inf();
            hi = __builtin_inf();
        } else {
            const double t1 = (-0.5 - p0[a]) / d[a];
            const double t2 = (0.5 - p0[a]) / d[a];
            lo = t1 < t2 ? t1 : t2;
            hi = t1 < t2 ? t2 : t1;
        }
        if (lo > te) {
            te = lo;
            axis = a;
        }
        if (hi < tx) tx = hi;
    }
    if (!(te < tx) || te < 0.0 || te > 1.0) return false;
    float frag[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double e = p0[a] + te * d[a];
        frag[a] = (float)e;
        tex[a] = (float)(e + 0.5);
    }
    // the entry face's coordinate is constant over the face
    frag[axis] = d[axis] > 0.0 ? -0.5f : 0.5f;
    tex[axis] = d[axis] > 0.0 ? 0.0f : 1.0f;
    const float vx = frag[0] - P.cam[0];
    const float vy = frag[1] - P.cam[1];
    const float vz = frag[2] - P.cam[2];
    const float len = sqrtf(vx * vx + vy * vy + vz * vz);
    dir[0] = vx / len;
    dir[1] = vy / len;
    dir[2] = vz / len;
    return true;
}

// ---- the occupancy words ------------------------------------------------------------------------
// A workgroup owns one word, the 32 cells m = 32 b .. 32 b + 31, and writes it with a plain store:
// no word is shared, so nothing is memset and nothing is ORed.  Eight lanes hold a cell, lane t & 7
// its x column; a wave holds eight cells, which follow each other along x (but for the turn of a
// cell row), so a wave's load reads up to 64 consecutive elements of one voxel row, wherever the row
// starts.  A lane ORs its column over the cell's 64 rows, the ballot combines the eight lanes of a
// cell, LDS the four waves.  Cells beyond the grid, and voxels beyond a cut cell, set nothing: the
// unused bits of the last word are 0.
template <typename ELEM>
__global__ __launch_bounds__(256) void mview_occupancy_kernel(const MviewOccArgs A)
{
    __shared__ uint32_t s_bits[4];
    const MviewArray &S = A.S;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t m = blockIdx.x * 32u + (tid >> 3);
    uint32_t n = 0;  // this lane's matching voxels
    if (m < A.ncells) {
        const uint32_t ci = m % S.c0, r = m / S.c0, cj = r % S.c1, ck = r / S.c1;
        const uint32_t x = ci * kMviewCell + (tid & 7u);
        if (x < S.ext[0]) {
            const uint32_t y0 = cj * kMviewCell, z0 = ck * kMviewCell;
            const uint32_t ny = min(kMviewCell, S.ext[1] - y0), nz = min(kMviewCell, S.ext[2] - z0);
            for (uint32_t k = 0; k < nz; ++k)
                for (uint32_t j = 0; j < ny; ++j) {
                    const uint32_t l = x + S.ext[0] * ((y0 + j) + S.ext[1] * (z0 + k));
                    n += matches(S, load_elem<ELEM>(S.array, l)) ? 1u : 0u;
                }
        }
    }
    const u64 b = __ballot(n != 0u);
    uint32_t bits = 0;  // the wave's eight cells
#pragma unroll
    for (int c = 0; c < 8; ++c) bits |= ((b >> (8 * c)) & 0xFFull) ? 1u << c : 0u;
    if (lane == 0) s_bits[wave] = bits;
    __syncthreads();
    const uint32_t word = s_bits[0] | s_bits[1] << 8 | s_bits[2] << 16 | s_bits[3] << 24;
    if (tid == 0) A.words[blockIdx.x] = word;
    flush_counters(A.cnt, tid == 0 ? (u64)__popc(word) : 0ull, (u64)n, 0ull, 0ull);
}

// ---- the hit records ----------------------------------------------------------------------------
template <typename ELEM, bool OCC>
__global__ __launch_bounds__(256) void mview_hit_kernel(const MarchParams P, const MviewHitArgs A)
{
    constexpr int K = kMviewInFlight;
    const MviewArray &S = A.S;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t tile_x = blockIdx.x % A.tiles_x, tile_y = blockIdx.x / A.tiles_x;
    const uint32_t px = tile_x * kMviewTile + (lane & 15u);
    const uint32_t py = tile_y * kMviewTile + wave * 4u + (lane >> 4);
    const bool active = px < A.w && py < A.h;

    float tex[3] = {0.f, 0.f, 0.f}, dir[3] = {0.f, 0.f, 0.f};
    const bool covered = active && mview_pixel_ray(P, A.x0 + px, A.y0 + py, tex, dir);

    bool hit = false;
    float h0 = 0.f, h1 = 0.f, h2 = 0.f;  // the hit
    uint32_t he = 0, hl = kMviewMiss, hk = kMviewMiss;
    uint32_t n_steps = 0, n_samples = 0;  // (a ray has at most 1e8 steps: check_params)
    const int nsteps = covered ? P.nsteps : 0;
    float p0 = tex[0], p1 = tex[1], p2 = tex[2];
    const float d0 = dir[0], d1 = dir[1], d2 = dir[2];

    bool live = nsteps > 0;
    for (int it = 0; live; it += K) {
        Lookup L[K];
        float c0[K], c1[K], c2[K];
        bool lv[K], sl[K];
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const int k = it + s;
            // the first position outside ends the ray
            live = live && k < nsteps &&
                   !(p0 > 1.0f || p1 > 1.0f || p2 > 1.0f || p0 < 0.0f || p1 < 0.0f || p2 < 0.0f);
            // the strict slab test
            const bool slab = live && p0 < P.smax[0] && p1 < P.smax[1] && p2 < P.smax[2] && p0 > P.smin[0] &&
                              p1 > P.smin[1] && p2 > P.smin[2];
            lv[s] = live;
            sl[s] = slab;
            c0[s] = p0;
            c1[s] = p1;
            c2[s] = p2;
            const bool in = grid_voxel(S, voxel_of(p0, S.fn[0], S.dims[0]), voxel_of(p1, S.fn[1], S.dims[1]),
                                       voxel_of(p2, S.fn[2], S.dims[2]), L[s].l, L[s].m);
            L[s].cand = slab && in;
            p0 = p0 + d0 * P.step;
            p1 = p1 + d1 * P.step;
            p2 = p2 + d2 * P.step;
        }
        fetch<ELEM, OCC, K>(S, L);
#pragma unroll
        for (int s = 0; s < K; ++s) {  // in step order: the first match wins
            if (hit || !lv[s]) continue;
            ++n_steps;
            if (!sl[s]) continue;
            ++n_samples;
            if (L[s].cand && matches(S, L[s].e)) {
                hit = true;
                h0 = c0[s];
                h1 = c1[s];
                h2 = c2[s];
                he = L[s].e;
                hl = L[s].l;
                hk = (uint32_t)(it + s);
            }
        }
        live = live && !hit;
    }

    // the 26 neighbours of the hit voxel, once per hit pixel, from the array itself
    int n0 = 0, n1 = 0, n2 = 0;
    float depth = INFINITY;
    if (hit) {
        const int vx = voxel_of(h0, S.fn[0], S.dims[0]), vy = voxel_of(h1, S.fn[1], S.dims[1]),
                  vz = voxel_of(h2, S.fn[2], S.dims[2]);
#pragma unroll
        for (int oz = -1; oz <= 1; ++oz)
#pragma unroll
            for (int oy = -1; oy <= 1; ++oy)
#pragma unroll
                for (int ox = -1; ox <= 1; ++ox) {
                    if (ox == 0 && oy == 0 && oz == 0) continue;
                    uint32_t l, m;
                    if (!grid_voxel(S, vx + ox, vy + oy, vz + oz, l, m)) continue;
                    if (matches(S, load_elem<ELEM>(S.array, l))) {
                        n0 -= ox;
                        n1 -= oy;
                        n2 -= oz;
                    }
                }
        const double dx = ((double)h0 - 0.5) - (double)P.cam[0];
        const double dy = ((double)h1 - 0.5) - (double)P.cam[1];
        const double dz = ((double)h2 - 0.5) - (double)P.cam[2];
        depth = (float)sqrt(dx * dx + dy * dy + dz * dz);
    }
    if (active) {
        uint32_t *o = static_cast<uint32_t *>(A.out) + ((size_t)py * A.w + px) * (kMviewHitBytes / 4);
        o[0] = __float_as_uint(h0);
        o[1] = __float_as_uint(h1);
        o[2] = __float_as_uint(h2);
        o[3] = __float_as_uint(depth);
        o[4] = he;
        o[5] = hk;
        o[6] = hl;
        o[7] = ((uint32_t)n0 & 0xFFu) | ((uint32_t)n1 & 0xFFu) << 8 | ((uint32_t)n2 & 0xFFu) << 16;
    }
    flush_counters(A.cnt, covered ? 1ull : 0ull, hit ? 1ull : 0ull, (u64)n_steps, (u64)n_samples);
}

// ---- the slice ----------------------------------------------------------------------------------
// mpr_strip's positions: q = (float)(origin + cx du + cy dv + t dn), left to right in double, rounded
// once.  No position depends on the one before it; a position outside the cube is passed over.
template <typename ELEM, bool OCC>
__global__ __launch_bounds__(256) void mview_slice_kernel(const MviewSliceArgs A)
{
    constexpr int K = kMviewInFlight;
    const MviewArray &S = A.S;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t tile_x = blockIdx.x % A.tiles_x, tile_y = blockIdx.x / A.tiles_x;
    const uint32_t px = tile_x * kMviewTile + (lane & 15u);
    const uint32_t py = tile_y * kMviewTile + wave * 4u + (lane >> 4);
    const bool active = px < A.W && py < A.H;

    const double cx = (double)px + 0.5 - A.half_w, cy = (double)py + 0.5 - A.half_h;
    double b[3];  // the pixel's prefix of the position sum
#pragma unroll
    for (int a = 0; a < 3; ++a) b[a] = A.origin[a] + cx * A.du[a] + cy * A.dv[a];

    bool hit = false;
    uint32_t he = 0, n_steps = 0, n_samples = 0;
    const uint32_t ns = active ? A.nsamples : 0u;
    for (uint32_t it = 0; it < ns && !hit; it += K) {
        Lookup L[K];
        bool st[K], sl[K];
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const double t = (double)(it + (uint32_t)s) - A.half_n;
            const float q0 = (float)(b[0] + t * A.dn[0]);
            const float q1 = (float)(b[1] + t * A.dn[1]);
            const float q2 = (float)(b[2] + t * A.dn[2]);
            // the march's bounds test: a position outside is no step
            const bool step = it + (uint32_t)s < ns &&
                              !(q0 > 1.0f || q1 > 1.0f || q2 > 1.0f || q0 < 0.0f || q1 < 0.0f || q2 < 0.0f);
            // the march's strict slab test
            const bool slab = step && q0 < A.smax[0] && q1 < A.smax[1] && q2 < A.smax[2] && q0 > A.smin[0] &&
                              q1 > A.smin[1] && q2 > A.smin[2];
            st[s] = step;
            sl[s] = slab;
            const bool in = grid_voxel(S, voxel_of(q0, S.fn[0], S.dims[0]), voxel_of(q1, S.fn[1], S.dims[1]),
                                       voxel_of(q2, S.fn[2], S.dims[2]), L[s].l, L[s].m);
            L[s].cand = slab && in;
        }
        fetch<ELEM, OCC, K>(S, L);
#pragma unroll
        for (int s = 0; s < K; ++s) {  // in s order: the first match wins
            if (hit || !st[s]) continue;
            ++n_steps;
            if (!sl[s]) continue;
            ++n_samples;
            if (L[s].cand && matches(S, L[s].e)) {
                hit = true;
                he = L[s].e;
            }
        }
    }
    if (active) A.out[(size_t)py * A.W + px] = he;
    flush_counters(A.cnt, n_steps ? 1ull : 0ull, he ? 1ull : 0ull, (u64)n_steps, (u64)n_samples);
}

}  // namespace

hipError_t launch_mview_occupancy(uint32_t elem_bytes, const MviewOccArgs &a, hipStream_t stream, const char **name)
{
    if ((elem_bytes != 1 && elem_bytes != 4) || a.nwords == 0) return hipErrorInvalidValue;
    const dim3 grid(a.nwords), block(256);
    if (elem_bytes == 1) {
        hipLaunchKernelGGL(mview_occupancy_kernel<uint8_t>, grid, block, 0, stream, a);
        *name = "mview_occupancy_kernel<u8>";
    } else {
        hipLaunchKernelGGL(mview_occupancy_kernel<uint32_t>, grid, block, 0, stream, a);
        *name = "mview_occupancy_kernel<u32>";
    }
    return hipGetLastError();
}

hipError_t launch_mview_hit(uint32_t elem_bytes, const MarchParams &p, const MviewHitArgs &a, uint32_t tiles_y,
                            hipStream_t stream, const char **name)
{
    if ((elem_bytes != 1 && elem_bytes != 4) || a.tiles_x == 0 || tiles_y == 0) return hipErrorInvalidValue;
    const dim3 grid(a.tiles_x * tiles_y), block(256);
    const bool occ = a.S.occ != nullptr;
    if (elem_bytes == 1 && occ) {
        hipLaunchKernelGGL((mview_hit_kernel<uint8_t, true>), grid, block, 0, stream, p, a);
        *name = "mview_hit_kernel<u8, occ>";
    } else if (elem_bytes == 1) {
        hipLaunchKernelGGL((mview_hit_kernel<uint8_t, false>), grid, block, 0, stream, p, a);
        *name = "mview_hit_kernel<u8>";
    } else if (occ) {
        hipLaunchKernelGGL((mview_hit_kernel<uint32_t, true>), grid, block, 0, stream, p, a);
        *name = "mview_hit_kernel<u32, occ>";
    } else {
        hipLaunchKernelGGL((mview_hit_kernel<uint32_t, false>), grid, block, 0, stream, p, a);
        *name = "mview_hit_kernel<u32>";
    }
    return hipGetLastError();
}

hipError_t launch_mview_slice(uint32_t elem_bytes, const MviewSliceArgs &a, uint32_t tiles_y, hipStream_t stream,
                              const char **name)
{
    if ((elem_bytes != 1 && elem_bytes != 4) || a.tiles_x == 0 || tiles_y == 0) return hipErrorInvalidValue;
    const dim3 grid(a.tiles_x * tiles_y), block(256);
    const bool occ = a.S.occ != nullptr;
    if (elem_bytes == 1 && occ) {
        hipLaunchKernelGGL((mview_slice_kernel<uint8_t, true>), grid, block, 0, stream, a);
        *name = "mview_slice_kernel<u8, occ>";
    } else if (elem_bytes == 1) {
        hipLaunchKernelGGL((mview_slice_kernel<uint8_t, false>), grid, block, 0, stream, a);
        *name = "mview_slice_kernel<u8>";
    } else if (occ) {
        hipLaunchKernelGGL((mview_slice_kernel<uint32_t, true>), grid, block, 0, stream, a);
        *name = "mview_slice_kernel<u32, occ>";
    } else {
        hipLaunchKernelGGL((mview_slice_kernel<uint32_t, false>), grid, block, 0, stream, a);
        *name = "mview_slice_kernel<u32>";
    }
    return hipGetLastError();
}

}  // namespace vr
