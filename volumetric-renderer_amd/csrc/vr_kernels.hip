// vr_kernels.hip — gfx950 (CDNA4) kernels of the volume ray-marcher.
//
// The hot path is march_kernel: one lane per pixel, a 64-lane wavefront marches a 16x4
// pixel strip by default (vr_params.wave_shape), a 256-thread workgroup a 16x16 tile.  It
// restates the
// reference fragment shader res/shaders/volume.frag:21-52 plus the Vulkan fixed-function
// state it runs under (src/rendering/offscreen_pass.cpp: cube ray entry :55-90 + cull
// :680-681 + depth clip :701-712, border trilinear sampler :1014-1039, sRGB TF sampler
// :1076/:1125-1150, blend :715-725 over the clear colour :170-173, UNORM8 store :293).
//
// Design points (DESIGN.md has the roofline discussion):
//  * memory-bound gather, no MFMA: each density sample is a 2x2x2 trilinear footprint;
//  * bricked native-dtype volume with paired elements (vr_internal.h): f32 z-pairs (a sample
//    is 2 x 16-B loads), 8/16-bit yz-quads (one load); zero apron = CLAMP_TO_BORDER without
//    bounds tests; shaded f32 frames read a precomputed central-difference field;
//  * TF decoded to linear float4 (with forward differences) once per upload on the host and
//    staged in LDS;
//  * XCD-aware tile order (block_tile / order_tiles_kernel): tiles grouped in 64x64-pixel
//    super-tiles dealt over the 8 XCDs (balance); each XCD dispatches its tiles longest first
//    by the last launches' durations, stable within a duration octave (co-running tiles stay
//    neighbours in its L2);
//  * pipelined variant (two samples of a ray in flight) for shaded frames, small launches and
//    volumes >= 4 GiB; lane-group variant for small shaded launches with serial frames;
//  * fp contraction is OFF (pragma below + -ffp-contract=off): every fused multiply-add is
//    an explicit fmaf(), matching the CPU oracle's operation order bit for bit.
#include "vr_exact_math.h"
#include "vr_internal.h"

#include <array>
#include <cstdlib>
#include <tuple>
#include <type_traits>
#include <utility>

#pragma clang fp contract(off)

namespace vr {
namespace {

constexpr int kTile = 16;       // pixels per workgroup side
constexpr int kThreads = 256;   // lane-pair kernel workgroup: 4 waves
constexpr int kTfLut = 2 * (kTfLds + 2);  // float4s of the staged LUT (tf_lookup: + 2 sentinels)

__device__ __forceinline__ float lerpf(float a, float b, float w) { return fmaf(w, b - a, a); }

// Bounds-checking debug builds (-DVR_BOUNDS_CHECK): an out-of-range index is printed (the first
// 32 per process) and the access redirected to element 0.  Product builds compile it away.
#ifdef VR_BOUNDS_CHECK
__device__ unsigned int g_oob_reports;
__device__ __noinline__ void oob_report(int what, unsigned long long a, unsigned long long b)
{
    if (atomicAdd(&g_oob_reports, 1u) < 32u)
        printf("VR_OOB what=%d index=%llu limit=%llu block=%u thread=%u\n", what, a, b,
               (unsigned)blockIdx.x, (unsigned)threadIdx.x);
}
#define VR_OOB(what, a, b) ((unsigned long long)(a) >= (unsigned long long)(b) ? (oob_report((what), (a), (b)), true) : false)
#else
#define VR_OOB(what, a, b) false
#endif

// Two independent lerps in one packed-FP32 pair (v_pk_add_f32 + v_pk_fma_f32): the same IEEE
// operations per element as lerpf, so bit-identical to two scalar lerps.
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2v lerp2(f2v a, f2v b, float w)
{
    const f2v ww = {w, w};
    return __builtin_elementwise_fma(ww, b - a, a);
}

// Unaligned-capable vector types: element pairs are 4- or 8-byte aligned, and gfx950 global
// loads only need dword alignment, so these compile to single global_load_dwordx2/x4.
typedef float f2a __attribute__((ext_vector_type(2))) __attribute__((aligned(4)));
typedef float f4a __attribute__((ext_vector_type(4))) __attribute__((aligned(4)));
typedef uint32_t u2a __attribute__((ext_vector_type(2))) __attribute__((aligned(4)));
typedef uint32_t u4a __attribute__((ext_vector_type(4))) __attribute__((aligned(4)));

template <typename VT>
struct is_quad8 : std::false_type {};
template <typename T>
struct is_quad8<Quad8<T>> : std::true_type {};
// bytes per element; 32-bit words per element (quad layouts)
// VT is the voxel type, or Quad8<T> for 8-bit voxels in yz-quads (vr_internal.h kQuadFlag);
// Vox<VT> the voxel type either way
template <typename VT>
struct VoxOf {
    using type = VT;
};
template <typename T>
struct VoxOf<Quad8<T>> {
    using type = T;
};
template <>
struct VoxOf<F32Alt> {
    using type = float;
};
template <>
struct VoxOf<F32H> {
    using type = float;
};
template <>
struct VoxOf<F32P> {
    using type = float;
};
template <>
struct VoxOf<F32S> {
    using type = float;
};
template <>
struct VoxOf<F32Y> {
    using type = float;
};
template <>
struct VoxOf<F32HY> {
    using type = float;
};
template <typename VT>
using Vox = typename VoxOf<VT>::type;
template <typename VT>
constexpr bool kIsQuad8 = is_quad8<VT>::value;
// the f32 volume read with the binary16 difference field (MarchParams::grad_half)
template <typename VT>
constexpr bool kHalfField = std::is_same<VT, F32H>::value || std::is_same<VT, F32HY>::value;
// the y-major copy (vr_internal.h F32Y): y-pair elements, a brick's elements y-slowest
template <typename VT>
constexpr bool kYMajor = std::is_same<VT, F32Y>::value || std::is_same<VT, F32HY>::value;
// f32 pair elements: z-pairs (8^3 bricks, or GeomAlt bricks for F32Alt) or, kYMajor, y-pairs
template <typename VT>
constexpr bool kZPair = std::is_same<Vox<VT>, float>::value;
// f32 voxels one per element (the F32P copy, or every f32 volume in VR_F32_PLAIN builds)
template <typename VT>
constexpr bool kPlainF32 = std::is_same<VT, F32P>::value || std::is_same<VT, F32S>::value ||
                          (kZPair<VT> && VR_F32_PLAIN);
// the stencil copy (GeomStencil: gradient taps inside the brick)
template <typename VT>
constexpr bool kStencil = std::is_same<VT, F32S>::value;
// VR_STENCIL_WIDE = 1 (default): the stencil copy's density loads are 16 B from x - 1 (x - 1 ..
// x + 2 of each row), so a shaded sample's x differences need no further load.  0: 8-B density
// loads and one 16-B load per row at shade time (shaded default camera 0.240 -> 0.260 ms,
// profiles/r03/stencil_copy/)
#ifndef VR_STENCIL_WIDE
#define VR_STENCIL_WIDE 1
#endif
template <typename VT>
constexpr bool kStencilWide = kStencil<VT> && VR_STENCIL_WIDE;
// 8-bit volumes stored one voxel per element (VR_U8_PLAIN, vr_internal.h)
template <typename VT>
constexpr bool kPlainByte = sizeof(VT) == 1 && VR_U8_PLAIN && !kIsQuad8<VT>;
template <typename VT>
constexpr int kElemBytes = kZPair<VT> ? (kPlainF32<VT> ? 4 : 8)
                                      : (kPlainByte<VT> ? 1 : 4 * (int)sizeof(VT));
template <typename VT>
using GeomOf = std::conditional_t<kPlainByte<VT>, GeomByte,
                                  std::conditional_t<std::is_same<VT, F32Alt>::value, GeomAlt,
                                  std::conditional_t<std::is_same<VT, F32P>::value, GeomPlainRows,
                                  std::conditional_t<kStencil<VT>, GeomStencil, GeomWide>>>>;
template <typename VT>
constexpr int kQuadWords = sizeof(VT) == 1 ? 1 : 2;

// Element index of padded cell (pi, pj, pk) in the bricked layout (vr_internal.h).  64-bit:
// a 2048^3 volume has 257^3 x 729 elements.  (A 32-bit index with SGPR-base loads for
// volumes < 4 GiB measured slower on the shaded kernel and on the diagonal view.)
// (kYMajor: the last argument is nbz, the y-major structures' slot order, not nby)
template <typename VT>
__device__ __forceinline__ size_t cell_offset(int pi, int pj, int pk, uint32_t nbx, uint32_t nby)
{
    using G = GeomOf<VT>;
    const uint32_t ux = (uint32_t)pi, uy = (uint32_t)pj, uz = (uint32_t)pk;
    if constexpr (kYMajor<VT>) return ymajor_cell_offset(ux, uy, uz, nbx, nby);
    const uint32_t bx = ux / G::BX, by = uy / G::BY, bz = uz / G::BZ;
    const uint32_t l = ((uz - bz * G::BZ + G::Lo) * G::EY + (uy - by * G::BY + G::Lo)) * G::EX +
                       (ux - bx * G::BX + G::Lo);
    return (size_t)brick_slot(bx, by, bz, nbx, nby) * (size_t)G::Elems + l;
}

// Trilinear filter of a 2x2x2 cell given its voxels v[dz][dy][dx]: lerp x, then y, then z
// (the oracle's tri_cell operation order).  tri8x2: two independent cells at once (packed).
__device__ __forceinline__ float tri8(float v000, float v100, float v010, float v110, float v001,
                                      float v101, float v011, float v111, float ax, float ay,
                                      float az)
{
    // scalar: packing the z = 0 / z = 1 halves into v_pk_fma_f32 pairs (8 instructions for 14)
    // measured 2-7% slower (u8 C4 view sweep, profiles/r02/valu/packed_tri_ab.txt)
    const float c00 = lerpf(v000, v100, ax);
    const float c10 = lerpf(v010, v110, ax);
    const float c01 = lerpf(v001, v101, ax);
    const float c11 = lerpf(v011, v111, ax);
    const float c0 = lerpf(c00, c10, ay);
    const float c1 = lerpf(c01, c11, ay);
    return lerpf(c0, c1, az);
}
// element-wise: .x = tri8 of the .x voxels, .y = tri8 of the .y voxels
__device__ __forceinline__ f2v tri8x2(f2v v000, f2v v100, f2v v010, f2v v110, f2v v001,
                                      f2v v101, f2v v011, f2v v111, float ax, float ay, float az)
{
    const f2v c00 = lerp2(v000, v100, ax);
    const f2v c10 = lerp2(v010, v110, ax);
    const f2v c01 = lerp2(v001, v101, ax);
    const f2v c11 = lerp2(v011, v111, ax);
    const f2v c0 = lerp2(c00, c10, ay);
    const f2v c1 = lerp2(c01, c11, ay);
    return lerp2(c0, c1, az);
}

// Byte b of w as the voxel value (float of an 8-bit integer is exact).
template <typename VT>
__device__ __forceinline__ float byte_value(uint32_t w, int b)
{
    const uint32_t u = (w >> (8 * b)) & 0xFFu;
    if constexpr (std::is_signed<Vox<VT>>::value) return (float)(int)(int8_t)u;
    return (float)u;
}

// Component c of a yz-quad element held in 32-bit words w (c: 0 (y,z), 1 (y,z+1), 2 (y+1,z),
// 3 (y+1,z+1)); float(v) is exact for 8/16-bit voxels.
template <typename VT>
__device__ __forceinline__ float qc(const uint32_t *w, int c)
{
    if constexpr (sizeof(VT) == 1) {
        const uint32_t b = (w[0] >> (8 * c)) & 0xFFu;
        if constexpr (std::is_signed<Vox<VT>>::value) return (float)(int)(int8_t)b;
        return (float)b;
    } else {
        const uint32_t h = (w[c >> 1] >> (16 * (c & 1))) & 0xFFFFu;
        if constexpr (std::is_signed<Vox<VT>>::value) return (float)(int)(int16_t)h;
        return (float)h;
    }
}

// Load the elements at e and e + 1 (one 8-B or 16-B load) / the element at e alone.
template <typename VT>
__device__ __forceinline__ void quad_load2(const char *__restrict__ base, size_t e, uint32_t *w)
{
    const char *p = base + e * kElemBytes<VT>;
    if constexpr (sizeof(VT) == 1) {
        const u2a r = *reinterpret_cast<const u2a *>(p);
        w[0] = r.x;
        w[1] = r.y;
    } else {
        const u4a r = *reinterpret_cast<const u4a *>(p);
        w[0] = r.x;
        w[1] = r.y;
        w[2] = r.z;
        w[3] = r.w;
    }
}
template <typename VT>
__device__ __forceinline__ void quad_load1(const char *__restrict__ base, size_t e, uint32_t *w)
{
    const char *p = base + e * kElemBytes<VT>;
    if constexpr (sizeof(VT) == 1) {
        w[0] = *reinterpret_cast<const uint32_t *>(p);
    } else {
        const u2a r = *reinterpret_cast<const u2a *>(p);
        w[0] = r.x;
        w[1] = r.y;
    }
}
__device__ __forceinline__ f4a zpair_load2(const char *__restrict__ base, size_t e)
{
    return *reinterpret_cast<const f4a *>(base + e * 8);
}
__device__ __forceinline__ f2a zpair_load1(const char *__restrict__ base, size_t e)
{
    return *reinterpret_cast<const f2a *>(base + e * 8);
}

// The 8 voxels of the cell whose low corner element is e:
//   f32 z-pair: rows y and y+1, elements x and x+1 -> 2 x 16-B loads;
//   8/16-bit yz-quad: elements x and x+1 -> 1 x 8-B (u8) / 16-B (u16) load.
// The raw loaded words of one cell, decoded later.  The pipelined march keeps the words of the
// sample in flight in the Stage and decodes (byte extraction, int -> float) only when the
// sample is consumed, after the next sample's loads are issued: decoding at load time put the
// decode, and with it a wait for the loads, before the loop back-edge (vmcnt(0) right after
// issue), so only one sample per ray was really in flight.
template <typename VT, typename = void>
struct CellRaw {  // generic: the decoded cell itself (loaded and decoded together)
    float v[8];
};
template <typename VT>
struct CellRaw<VT, std::enable_if_t<kZPair<VT> && !kPlainF32<VT>>> {
    f4a r0, r1;  // rows y and y + 1: elements x, x + 1 as z-pairs (kYMajor: rows z, z + 1, y-pairs)
};
template <typename VT>
struct CellRaw<VT, std::enable_if_t<kStencilWide<VT>>> {
    f4a q[4];  // rows (y|y+1, z|z+1): elements x - 1 .. x + 2
};
template <typename VT>
struct CellRaw<VT, std::enable_if_t<kPlainByte<VT> && GeomByte::EX == 8>> {
    u4a q0, q1;    // slices z and z + 1: the 16 bytes from the 4-aligned address at or below e
    uint32_t sh;   // e mod 4
};

// (Cross-lane sharing of a cell's loads, VR_U8_SHARE for 8-bit and VR_F32_SHARE for f32 cells,
// measured 1.5-1.8x and 1.6x slower in round 5: tools/experiments/r05_pruned/.)

// the stencil copy with 16-B density loads keeps each row's x - 1 / x + 2 voxels for the
// gradient (row r = dy + 2 dz)
template <typename VT, typename = void>
struct CellTaps {};
template <typename VT>
struct CellTaps<VT, std::enable_if_t<kStencilWide<VT>>> {
    float xm[4], xp[4];
};
template <typename VT>
struct Cell8 : CellTaps<VT> {
    float v[8];  // index dx + 2 dy + 4 dz
    // issue the loads of the cell whose low corner element is e (decode() converts them)
    static __device__ __forceinline__ void issue(CellRaw<VT> &w, const char *__restrict__ base,
                                                 size_t e)
    {
        if constexpr (kZPair<VT> && !kPlainF32<VT>) {
            w.r0 = zpair_load2(base, e);
            w.r1 = zpair_load2(base, e + GeomOf<VT>::Row);  // (kYMajor: the row at z + 1)
        } else if constexpr (kStencilWide<VT>) {
            using G = GeomOf<VT>;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                w.q[r] = *reinterpret_cast<const f4a *>(
                    base + (e - 1 + (size_t)((r & 1) * G::Row + (r >> 1) * G::Slice)) * 4);
        } else if constexpr (kPlainByte<VT> && GeomByte::EX == 8) {
            const size_t a = e & ~(size_t)3;
            w.sh = (uint32_t)e & 3u;
            w.q0 = *reinterpret_cast<const u4a *>(base + a);
            w.q1 = *reinterpret_cast<const u4a *>(base + a + GeomByte::Slice);
        } else {
            Cell8 c;
            c.load(base, e);
#pragma unroll
            for (int i = 0; i < 8; ++i) w.v[i] = c.v[i];
        }
    }
    __device__ __forceinline__ void decode(const CellRaw<VT> &w)
    {
        if constexpr (kYMajor<VT>) {  // r0 = row z, r1 = row z + 1; .xy / .zw = y-pairs at x / x + 1
            v[0] = w.r0.x;
            v[2] = w.r0.y;
            v[1] = w.r0.z;
            v[3] = w.r0.w;
            v[4] = w.r1.x;
            v[6] = w.r1.y;
            v[5] = w.r1.z;
            v[7] = w.r1.w;
        } else if constexpr (kZPair<VT> && !kPlainF32<VT>) {
            v[0] = w.r0.x;
            v[4] = w.r0.y;
            v[1] = w.r0.z;
            v[5] = w.r0.w;
            v[2] = w.r1.x;
            v[6] = w.r1.y;
            v[3] = w.r1.z;
            v[7] = w.r1.w;
        } else if constexpr (kStencilWide<VT>) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                this->xm[r] = w.q[r].x;
                v[2 * r] = w.q[r].y;
                v[2 * r + 1] = w.q[r].z;
                this->xp[r] = w.q[r].w;
            }
        } else if constexpr (kPlainByte<VT> && GeomByte::EX == 8) {
            const uint32_t q[4] = {__builtin_amdgcn_alignbyte(w.q0.y, w.q0.x, w.sh),
                                   __builtin_amdgcn_alignbyte(w.q0.w, w.q0.z, w.sh),
                                   __builtin_amdgcn_alignbyte(w.q1.y, w.q1.x, w.sh),
                                   __builtin_amdgcn_alignbyte(w.q1.w, w.q1.z, w.sh)};
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // r = dy + 2 dz
                v[2 * r] = byte_value<VT>(q[r], 0);
                v[2 * r + 1] = byte_value<VT>(q[r], 1);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = w.v[i];
        }
    }
    __device__ __forceinline__ void load(const char *__restrict__ base, size_t e)
    {
        if constexpr (kStencilWide<VT> || kYMajor<VT>) {
            CellRaw<VT> w;
            issue(w, base, e);
            decode(w);
        } else if constexpr (kPlainF32<VT>) {  // rows (y, z), (y+1, z), (y, z+1), (y+1, z+1)
            using G = GeomOf<VT>;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f2a q = *reinterpret_cast<const f2a *>(
                    base + (e + (size_t)((r & 1) * G::Row + (r >> 1) * G::Slice)) * 4);
                v[2 * r] = q.x;
                v[2 * r + 1] = q.y;
            }
        } else if constexpr (kZPair<VT>) {
            const f4a r0 = zpair_load2(base, e);
            const f4a r1 = zpair_load2(base, e + GeomOf<VT>::Row);
            v[0] = r0.x;
            v[4] = r0.y;
            v[1] = r0.z;
            v[5] = r0.w;
            v[2] = r1.x;
            v[6] = r1.y;
            v[3] = r1.z;
            v[7] = r1.w;
        } else if constexpr (kPlainByte<VT> && GeomByte::EX == 4) {
            // 4-byte rows (3-cell-wide bricks): the row of the cell starts at the 4-aligned
            // address at or below e; one dwordx2 per slice holds rows y and y+1, the cell's
            // voxels at bytes s, s+1 of each dword (s = x <= 2)
            const size_t a = e & ~(size_t)3;
            const uint32_t sh = 8u * ((uint32_t)e & 3u);
            const u2a q0 = *reinterpret_cast<const u2a *>(base + a);
            const u2a q1 = *reinterpret_cast<const u2a *>(base + a + GeomByte::Slice);
            const uint32_t w[4] = {q0.x >> sh, q0.y >> sh, q1.x >> sh, q1.y >> sh};
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // r = dy + 2 dz
                v[2 * r] = byte_value<VT>(w[r], 0);
                v[2 * r + 1] = byte_value<VT>(w[r], 1);
            }
        } else if constexpr (kPlainByte<VT>) {
            // one dwordx4 per slice from the 4-aligned address at or below e (bricks and rows
            // are 4-aligned: s = e mod 4 = x mod 4): bytes s, s+1 = row y, s+8, s+9 = row y+1
            static_assert(GeomByte::EX == 8, "plain 8-bit rows are 4 or 8 bytes");
            const size_t a = e & ~(size_t)3;
            const uint32_t sh = (uint32_t)e & 3u;
            const u4a q0 = *reinterpret_cast<const u4a *>(base + a);
            const u4a q1 = *reinterpret_cast<const u4a *>(base + a + GeomByte::Slice);
            const uint32_t w[4] = {__builtin_amdgcn_alignbyte(q0.y, q0.x, sh),
                                   __builtin_amdgcn_alignbyte(q0.w, q0.z, sh),
                                   __builtin_amdgcn_alignbyte(q1.y, q1.x, sh),
                                   __builtin_amdgcn_alignbyte(q1.w, q1.z, sh)};
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // r = dy + 2 dz
                v[2 * r] = byte_value<VT>(w[r], 0);
                v[2 * r + 1] = byte_value<VT>(w[r], 1);
            }
        } else {
            constexpr int QW = kQuadWords<VT>;
            uint32_t w[2 * QW];
            quad_load2<VT>(base, e, w);
            v[0] = qc<VT>(w, 0);
            v[4] = qc<VT>(w, 1);
            v[2] = qc<VT>(w, 2);
            v[6] = qc<VT>(w, 3);
            v[1] = qc<VT>(w + QW, 0);
            v[5] = qc<VT>(w + QW, 1);
            v[3] = qc<VT>(w + QW, 2);
            v[7] = qc<VT>(w + QW, 3);
        }
    }
    __device__ __forceinline__ float tri(float ax, float ay, float az) const
    {
        return tri8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], ax, ay, az);
    }
};

// Central-difference gradient (extension): per axis e, the trilinear filter (the centre
// cell's weights, tri8's lerp order) of the per-voxel difference D_e(c) = v(c+e) - v(c-e)
// over the cell's 8 corners -- the oracle's grad_cell.  The differences need the 4-wide
// stencil's 24 outer voxels (10 loads for z-pair f32, 6 for yz-quads).  Taps one element
// below, or two above in z-pair x/y, may sit in the neighbouring brick (the apron covers
// +1): the per-axis deltas pick that brick.  Corner index: dx + 2 dy + 4 dz.
// PACKED: D_x / D_y and their filters as packed-FP32 pairs (fewer VALU, more VGPRs; the
// scalar form serves the register-tight skip-empty kernel).
template <bool PACKED>
__device__ __forceinline__ void grad_filter(const float *dx, const float *dy, const float *dz,
                                            float ax, float ay, float az, float &gx, float &gy,
                                            float &gz)
{
    if constexpr (PACKED) {
        const f2v g = tri8x2(f2v{dx[0], dy[0]}, f2v{dx[1], dy[1]}, f2v{dx[2], dy[2]},
                             f2v{dx[3], dy[3]}, f2v{dx[4], dy[4]}, f2v{dx[5], dy[5]},
                             f2v{dx[6], dy[6]}, f2v{dx[7], dy[7]}, ax, ay, az);
        gx = g.x;
        gy = g.y;
    } else {
        gx = tri8(dx[0], dx[1], dx[2], dx[3], dx[4], dx[5], dx[6], dx[7], ax, ay, az);
        gy = tri8(dy[0], dy[1], dy[2], dy[3], dy[4], dy[5], dy[6], dy[7], ax, ay, az);
    }
    gz = tri8(dz[0], dz[1], dz[2], dz[3], dz[4], dz[5], dz[6], dz[7], ax, ay, az);
}

template <typename VT, bool PACKED>
__device__ __forceinline__ void gradient(const char *__restrict__ base, size_t e,
                                         const Cell8<VT> &c, int pi, int pj, int pk,
                                         uint32_t nbx, uint32_t nby, long by_stride,
                                         long bz_stride, float ax, float ay, float az, float &gx,
                                         float &gy, float &gz)
{
    using G = GeomOf<VT>;
    constexpr long S = G::Row, S2 = G::Slice, B = G::Elems;
    constexpr long Lx = G::BX - 1, Ly = G::BY - 1, Lz = G::BZ - 1;
    const int lx = pi % G::BX, ly = pj % G::BY, lz = pk % G::BZ;
    // element-index deltas of the taps one element below / two above the cell's low corner;
    // a tap outside the brick reads the neighbouring brick (constant strides in x-fastest
    // brick order, the neighbour's slot otherwise)
    long dxm, dxp, dym, dyp, dzm, dzp;
    if constexpr (G::Lo == 1) {  // the stencil copy: every tap inside the brick
        dxm = -1;
        dxp = 2;
        dym = -S;
        dyp = 2 * S;
        dzm = -S2;
        dzp = 2 * S2;
    } else if constexpr (kGroupShift == 0) {
        dxm = lx > 0 ? -1 : (Lx - B);
        dxp = lx < Lx ? 2 : (B - (Lx - 1));
        dym = ly > 0 ? -S : (Ly * S - by_stride);
        dyp = ly < Ly ? 2 * S : (by_stride - (Ly - 1) * S);
        dzm = lz > 0 ? -S2 : (Lz * S2 - bz_stride);
        dzp = lz < Lz ? 2 * S2 : (bz_stride - (Lz - 1) * S2);
    } else {
        auto cross = [&](int ox, int oy, int oz) {
            return (long)cell_offset<VT>(pi + ox, pj + oy, pk + oz, nbx, nby) - (long)e;
        };
        dxm = lx > 0 ? -1 : cross(-1, 0, 0);
        dxp = lx < Lx ? 2 : cross(2, 0, 0);
        dym = ly > 0 ? -S : cross(0, -1, 0);
        dyp = ly < Ly ? 2 * S : cross(0, 2, 0);
        dzm = lz > 0 ? -S2 : cross(0, 0, -1);
        dzp = lz < Lz ? 2 * S2 : cross(0, 0, 2);
    }
    (void)dyp;
    (void)dzp;
    const float *v = c.v;
    float Dx[8], Dy[8], Dz[8];
    if constexpr (kPlainF32<VT>) {
        auto ld1 = [&](long o) { return *reinterpret_cast<const float *>(base + (e + o) * 4); };
        auto ld2 = [&](long o) { return *reinterpret_cast<const f2a *>(base + (e + o) * 4); };
#pragma unroll
        for (int dz_ = 0; dz_ < 2; ++dz_)
#pragma unroll
            for (int dy_ = 0; dy_ < 2; ++dy_) {
                const int o = 2 * dy_ + 4 * dz_;
                const long r = dy_ * S + dz_ * S2;
                if constexpr (kStencilWide<VT>) {  // taps kept by the density loads
                    Dx[o] = v[o + 1] - c.xm[dy_ + 2 * dz_];
                    Dx[o + 1] = c.xp[dy_ + 2 * dz_] - v[o];
                } else if constexpr (kStencil<VT>) {  // x - 1 .. x + 2 in one load
                    const f4a q = *reinterpret_cast<const f4a *>(base + (e - 1 + r) * 4);
                    Dx[o] = v[o + 1] - q.x;
                    Dx[o + 1] = q.w - v[o];
                } else {
                    Dx[o] = v[o + 1] - ld1(dxm + r);
                    Dx[o + 1] = ld1(dxp + r) - v[o];
                }
            }
#pragma unroll
        for (int dz_ = 0; dz_ < 2; ++dz_) {
            const f2a m = ld2(dym + dz_ * S2), q = ld2(dyp + dz_ * S2);
            const int o = 4 * dz_;
            Dy[o] = v[o + 2] - m.x;
            Dy[o + 1] = v[o + 3] - m.y;
            Dy[o + 2] = q.x - v[o];
            Dy[o + 3] = q.y - v[o + 1];
        }
#pragma unroll
        for (int dy_ = 0; dy_ < 2; ++dy_) {
            const f2a m = ld2(dzm + dy_ * S), q = ld2(dzp + dy_ * S);
            const int o = 2 * dy_;
            Dz[o] = v[o + 4] - m.x;
            Dz[o + 1] = v[o + 5] - m.y;
            Dz[o + 4] = q.x - v[o];
            Dz[o + 5] = q.y - v[o + 1];
        }
    } else if constexpr (kZPair<VT>) {
        // z-pairs (.x = z, .y = z + 1) of the x - 1 and x + 2 columns, rows y and y + 1
        const f2a xm0 = zpair_load1(base, e + dxm), xm1 = zpair_load1(base, e + dxm + S);
        const f2a xp0 = zpair_load1(base, e + dxp), xp1 = zpair_load1(base, e + dxp + S);
        // elements x, x + 1 of rows y - 1 and y + 2: (.x, .y) column x, (.z, .w) column x + 1
        const f4a ym = zpair_load2(base, e + dym), yp = zpair_load2(base, e + dyp);
        // elements x, x + 1 at z - 1 (pairs z - 1, z) and z + 1 (pairs z + 1, z + 2)
        const f4a zm0 = zpair_load2(base, e + dzm), zm1 = zpair_load2(base, e + dzm + S);
        const f4a zp0 = zpair_load2(base, e + S2), zp1 = zpair_load2(base, e + S2 + S);
        Dx[0] = v[1] - xm0.x; Dx[1] = xp0.x - v[0]; Dx[2] = v[3] - xm1.x; Dx[3] = xp1.x - v[2];
        Dx[4] = v[5] - xm0.y; Dx[5] = xp0.y - v[4]; Dx[6] = v[7] - xm1.y; Dx[7] = xp1.y - v[6];
        Dy[0] = v[2] - ym.x;  Dy[1] = v[3] - ym.z;  Dy[2] = yp.x - v[0];  Dy[3] = yp.z - v[1];
        Dy[4] = v[6] - ym.y;  Dy[5] = v[7] - ym.w;  Dy[6] = yp.y - v[4];  Dy[7] = yp.w - v[5];
        Dz[0] = v[4] - zm0.x; Dz[1] = v[5] - zm0.z; Dz[2] = v[6] - zm1.x; Dz[3] = v[7] - zm1.z;
        Dz[4] = zp0.y - v[0]; Dz[5] = zp0.w - v[1]; Dz[6] = zp1.y - v[2]; Dz[7] = zp1.w - v[3];
    } else if constexpr (kPlainByte<VT>) {
        // the 24 outer voxels one byte load each (8-bit shading is off the benchmarked path)
        auto ld = [&](long o) {
            return byte_value<VT>((uint32_t)*reinterpret_cast<const uint8_t *>(base + e + o), 0);
        };
#pragma unroll
        for (int dz_ = 0; dz_ < 2; ++dz_)
#pragma unroll
            for (int dy_ = 0; dy_ < 2; ++dy_) {
                const int o = 2 * dy_ + 4 * dz_;
                const long r = dy_ * S + dz_ * S2;
                Dx[o] = v[o + 1] - ld(dxm + r);
                Dx[o + 1] = ld(dxp + r) - v[o];
            }
#pragma unroll
        for (int dz_ = 0; dz_ < 2; ++dz_)
#pragma unroll
            for (int dx_ = 0; dx_ < 2; ++dx_) {
                const int o = dx_ + 4 * dz_;
                const long r = dx_ + dz_ * S2;
                Dy[o] = v[o + 2] - ld(dym + r);
                Dy[o + 2] = ld(dyp + r) - v[o];
            }
#pragma unroll
        for (int dy_ = 0; dy_ < 2; ++dy_)
#pragma unroll
            for (int dx_ = 0; dx_ < 2; ++dx_) {
                const int o = dx_ + 2 * dy_;
                const long r = dx_ + dy_ * S;
                Dz[o] = v[o + 4] - ld(dzm + r);
                Dz[o + 4] = ld(dzp + r) - v[o];
            }
    } else {
        constexpr int QW = kQuadWords<VT>;
        uint32_t xm[QW], xp[QW], ym[2 * QW], yp[2 * QW], zm[2 * QW], zp[2 * QW];
        quad_load1<VT>(base, e + dxm, xm);  // (x-1): comps (y,z) (y,z+1) (y+1,z) (y+1,z+1)
        quad_load1<VT>(base, e + dxp, xp);  // (x+2)
        quad_load2<VT>(base, e + dym, ym);  // (x, y-1), (x+1, y-1): comps 0,1 = y-1
        quad_load2<VT>(base, e + S, yp);    // (x, y+1), (x+1, y+1): comps 2,3 = y+2
        quad_load2<VT>(base, e + dzm, zm);  // (x, y, z-1), (x+1, y, z-1): comps 0,2 = z-1
        quad_load2<VT>(base, e + S2, zp);   // (x, y, z+1), (x+1, y, z+1): comps 1,3 = z+2
#pragma unroll
        for (int dz_ = 0; dz_ < 2; ++dz_)
#pragma unroll
            for (int dy_ = 0; dy_ < 2; ++dy_) {
                const int q = dz_ + 2 * dy_, o = 2 * dy_ + 4 * dz_;
                Dx[o] = v[o + 1] - qc<VT>(xm, q);
                Dx[o + 1] = qc<VT>(xp, q) - v[o];
            }
#pragma unroll
        for (int dz_ = 0; dz_ < 2; ++dz_)
#pragma unroll
            for (int dx_ = 0; dx_ < 2; ++dx_) {
                const int o = dx_ + 4 * dz_;
                Dy[o] = v[o + 2] - qc<VT>(ym + dx_ * QW, dz_);
                Dy[o + 2] = qc<VT>(yp + dx_ * QW, 2 + dz_) - v[o];
            }
#pragma unroll
        for (int dy_ = 0; dy_ < 2; ++dy_)
#pragma unroll
            for (int dx_ = 0; dx_ < 2; ++dx_) {
                const int o = dx_ + 2 * dy_;
                Dz[o] = v[o + 4] - qc<VT>(zm + dx_ * QW, 2 * dy_);
                Dz[o + 4] = qc<VT>(zp + dx_ * QW, 2 * dy_ + 1) - v[o];
            }
    }
    grad_filter<PACKED>(Dx, Dy, Dz, ax, ay, az, gx, gy, gz);
}

#ifndef VR_GRAD_ZPACK
#define VR_GRAD_ZPACK 1  // A/B: 0 = (Dx, Dy)-packed tri8x2 + scalar Dz
#endif
// The difference field's words one shaded sample reads.  f32 (H = false): rows y and y + 1 of
// the cell, elements x and x + 1, 3 x 16 B each.  binary16 (H = true): element e holds per
// axis {D(y,z), D(y,z+1), D(y+1,z), D(y+1,z+1)}, so elements x and x + 1 are 48 contiguous
// bytes: 3 x 16 B.
template <bool H>
struct FieldRowsT {
    f4a a0, a1, a2, b0, b1, b2;
};
template <>
struct FieldRowsT<true> {
    u4a a0, a1, a2;
};
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2v h2f(uint32_t w)  // two binary16 -> two f32 (exact)
{
    return __builtin_convertvector(__builtin_bit_cast(h2v, w), f2v);
}
__device__ __forceinline__ void field_rows_load(const char *__restrict__ gbase, size_t e,
                                                FieldRowsT<true> &r)
{
    const char *p = gbase + e * kGradElemBytes;
    r.a0 = *reinterpret_cast<const u4a *>(p);
    r.a1 = *reinterpret_cast<const u4a *>(p + 16);
    r.a2 = *reinterpret_cast<const u4a *>(p + 32);
}
// The f32 path's filter (below) on the converted pairs: per axis a, words 2a / 2a + 1 of
// element x are the y / y + 1 pairs {D(z), D(z+1)}, words 6 + 2a / 7 + 2a those of x + 1.
// VR_FIELD_MIX = 1 (default): the x lerps of the binary16 pairs as v_fma_mix_f32 (binary16
// operands read in place: b * 1 - a, then w * d + a, each rounded once as lerpf's subtraction
// and fma), instead of converting every half first: 12 fewer VALU per shaded sample, C3 +2-3%
// (profiles/r03/field_mix/; bit-identical frames)
#ifndef VR_FIELD_MIX
#define VR_FIELD_MIX 1
#endif
template <bool HI>
__device__ __forceinline__ float mix_lerp(uint32_t a, uint32_t b, float w)
{
    float d, r;
    if constexpr (HI) {
        asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(b), "v"(a));
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r) : "v"(w), "v"(d), "v"(a));
    } else {
        asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[1,0,1]" : "=v"(d) : "v"(b), "v"(a));
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,0,1]" : "=v"(r) : "v"(w), "v"(d), "v"(a));
    }
    return r;
}
__device__ __forceinline__ void field_rows_filter(const FieldRowsT<true> &r, float ax, float ay,
                                                  float az, float &gx, float &gy, float &gz)
{
    const uint32_t w[12] = {r.a0.x, r.a0.y, r.a0.z, r.a0.w, r.a1.x, r.a1.y,
                            r.a1.z, r.a1.w, r.a2.x, r.a2.y, r.a2.z, r.a2.w};
    auto axis = [&](int a) {
#if VR_FIELD_MIX
        const f2v c0 = {mix_lerp<false>(w[2 * a], w[6 + 2 * a], ax),
                        mix_lerp<true>(w[2 * a], w[6 + 2 * a], ax)};
        const f2v c1 = {mix_lerp<false>(w[2 * a + 1], w[7 + 2 * a], ax),
                        mix_lerp<true>(w[2 * a + 1], w[7 + 2 * a], ax)};
        const f2v q = lerp2(c0, c1, ay);
#else
        const f2v q = lerp2(lerp2(h2f(w[2 * a]), h2f(w[6 + 2 * a]), ax),
                            lerp2(h2f(w[2 * a + 1]), h2f(w[7 + 2 * a]), ax), ay);
#endif
        return lerpf(q.x, q.y, az);
    };
    gx = axis(0);
    gy = axis(1);
    gz = axis(2);
}
__device__ __forceinline__ void field_rows_load(const char *__restrict__ gbase, size_t e,
                                                FieldRowsT<false> &r)
{
    const char *row0 = gbase + e * kGradElemBytes;
    const char *row1 = row0 + (size_t)GeomWide::Row * kGradElemBytes;
    r.a0 = *reinterpret_cast<const f4a *>(row0);       // Dx(x) z,z+1  Dy(x) z,z+1
    r.a1 = *reinterpret_cast<const f4a *>(row0 + 16);  // Dz(x) z,z+1  Dx(x+1) z,z+1
    r.a2 = *reinterpret_cast<const f4a *>(row0 + 32);  // Dy(x+1) ...  Dz(x+1) ...
    r.b0 = *reinterpret_cast<const f4a *>(row1);
    r.b1 = *reinterpret_cast<const f4a *>(row1 + 16);
    r.b2 = *reinterpret_cast<const f4a *>(row1 + 32);
}
// Each axis filtered with its z = 0 / z = 1 halves as packed pairs, which the field's element
// layout already holds adjacent ({D(z), D(z+1)}): lerp2 over x of rows y and y + 1 gives
// {c00, c01} and {c10, c11}, lerp2 over y {c0, c1}, then the z lerp -- tri8's IEEE operations
// per element, without repacking (Dx, Dy) pairs.
__device__ __forceinline__ void field_rows_filter(const FieldRowsT<false> &r, float ax, float ay,
                                                  float az, float &gx, float &gy, float &gz)
{
    auto axis = [&](f2v y0x0, f2v y0x1, f2v y1x0, f2v y1x1) {
        const f2v q = lerp2(lerp2(y0x0, y0x1, ax), lerp2(y1x0, y1x1, ax), ay);
        return lerpf(q.x, q.y, az);
    };
    gx = axis(f2v{r.a0.x, r.a0.y}, f2v{r.a1.z, r.a1.w}, f2v{r.b0.x, r.b0.y}, f2v{r.b1.z, r.b1.w});
    gy = axis(f2v{r.a0.z, r.a0.w}, f2v{r.a2.x, r.a2.y}, f2v{r.b0.z, r.b0.w}, f2v{r.b2.x, r.b2.y});
    gz = axis(f2v{r.a1.x, r.a1.y}, f2v{r.a2.z, r.a2.w}, f2v{r.b1.x, r.b1.y}, f2v{r.b2.z, r.b2.w});
}
// Gradient from the precomputed f32 field: the cell's 8 corners of {Dx, Dy, Dz}, rows y and
// y + 1 of elements x, x + 1 (48 B each: 3 x 16-B loads), filtered as grad_filter.
template <bool PACKED, bool H = false>
__device__ __forceinline__ void grad_field(const char *__restrict__ gbase, size_t e, float ax,
                                           float ay, float az, float &gx, float &gy, float &gz)
{
    if constexpr (H) {
        FieldRowsT<true> r;
        field_rows_load(gbase, e, r);
        field_rows_filter(r, ax, ay, az, gx, gy, gz);
        return;
    }
#if VR_GRAD_ZPACK
    if constexpr (PACKED) {
        FieldRowsT<false> r;
        field_rows_load(gbase, e, r);
        field_rows_filter(r, ax, ay, az, gx, gy, gz);
        return;
    }
#endif
    float Dx[8], Dy[8], Dz[8];
#pragma unroll
    for (int dy_ = 0; dy_ < 2; ++dy_) {
        const char *row = gbase + (e + (size_t)dy_ * GeomWide::Row) * kGradElemBytes;
        const f4a r0 = *reinterpret_cast<const f4a *>(row);       // Dx(x) z,z+1  Dy(x) z,z+1
        const f4a r1 = *reinterpret_cast<const f4a *>(row + 16);  // Dz(x) z,z+1  Dx(x+1) z,z+1
        const f4a r2 = *reinterpret_cast<const f4a *>(row + 32);  // Dy(x+1) ...  Dz(x+1) ...
        const int o = 2 * dy_;  // corner dx + 2 dy + 4 dz
        Dx[o] = r0.x; Dx[o + 4] = r0.y; Dy[o] = r0.z; Dy[o + 4] = r0.w;
        Dz[o] = r1.x; Dz[o + 4] = r1.y; Dx[o + 1] = r1.z; Dx[o + 5] = r1.w;
        Dy[o + 1] = r2.x; Dy[o + 5] = r2.y; Dz[o + 1] = r2.z; Dz[o + 5] = r2.w;
    }
    grad_filter<PACKED>(Dx, Dy, Dz, ax, ay, az, gx, gy, gz);
}

// Steps k in [1, K] of a ray whose positions provably stay strictly inside (0, 1)^3, where the
// reference's bounds test (volume.frag:34-37) never breaks and, with the default slicing, the
// strict slab test (:39-40) always passes: the loop skips both there.  p_k is p_0 plus k float
// additions of s = fl(d * step); while |p| < 1 each addition rounds by at most 2^-25, so with
// delta = 2^-24 per step, p_k lies within p_0 + k s +- k delta.  Each bound is linear in k:
// f(k) = A + B k > 0 holds on [1, K] iff it holds at both ends.
__device__ __forceinline__ int interior_steps(const float *p, const float *d, float step,
                                              int nsteps)
{
    constexpr double delta = 0x1p-24;
    double K = (double)(nsteps - 1);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double s = (double)(d[a] * step), q = (double)p[a];
        const double A[2] = {q, 1.0 - q}, B[2] = {s - delta, -(s + delta)};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (!(A[c] + B[c] > 0.0)) return 0;
            if (B[c] < 0.0) K = fmin(K, floor(A[c] / -B[c]) - 1.0);
        }
    }
    return K > 0.0 ? (int)K : 0;
}

__device__ __forceinline__ void texel_coord(float p, float n, int &i, float &a)
{
    const float u = p * n - 0.5f;
    const float f = floorf(u);
    a = u - f;
    i = (int)f;
}

// Pixel-centre ray -> cube entry (front face inside the clip volume), as the oracle's
// pixel_ray: unproject ndc z = 0 and z = 1 through inverse(proj*view) in double.
__device__ __forceinline__ bool pixel_ray(const MarchParams &P, uint32_t px, uint32_t py,
                                          float tex[3], float dir[3])
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
    // the entry face's coordinate is constant over the face (volume.vert:20, cube :55-90)
    frag[axis] = d[axis] > 0.0 ? -0.5f : 0.5f;
    tex[axis] = d[axis] > 0.0 ? 0.0f : 1.0f;
    // volume.frag:23
    const float vx = frag[0] - P.cam[0];
    const float vy = frag[1] - P.cam[1];
    const float vz = frag[2] - P.cam[2];
    const float len = sqrtf(vx * vx + vy * vy + vz * vz);
    dir[0] = vx / len;
    dir[1] = vy / len;
    dir[2] = vz / len;
    return true;
}

// (x / range) correctly rounded.  P.div_fast (host: 2^-40 <= range < 2^100, |min|, |max| <
// 2^100): q = x * RN(1/range), then one fma residual correction.  Markstein's theorem gives
// the IEEE quotient when the residual is exact (|x| >= 2^-100 here); checked against x86
// IEEE division on 3.8e9 (x, range) pairs of that domain, 0 mismatches.  Smaller |x| give
// |t| < 2^-60, where t * n - 0.5 rounds to -0.5 whatever t's last bit: the frame is the
// same.  Otherwise the full IEEE division sequence.
template <typename PT>
__device__ __forceinline__ float div_by_range(float x, const PT &P)
{
    if (P.div_fast) {
        const float q = x * P.inv_range;
        const float e = fmaf(-q, P.range, x);
        return fmaf(e, P.inv_range, q);
    }
    return x / P.range;
}

// 1D TF, linear filter, clamp-to-edge (offscreen_pass.cpp:1125-1150).  lut holds n + 2
// entries {c, d} (float4 pairs): entry i + 1 is texel i as {c_i, c_(i+1) - c_i} (difference 0
// for the last texel, computed on the host with the same IEEE subtraction), entry 0 = {c_0, 0}
// and entry n + 1 = {c_(n-1), 0} are the clamp-to-edge sentinels.  With u clamped to [-1, n],
// floor(u) = i0 lies in [-1, n] and lerp(c_i0, c_i1, w) = fma(w, d, c) is one fma per channel
// with no index clamp: below the first texel centre (i0 = -1) and at u = n the sentinel's
// difference 0 returns the edge texel for any w.  NaN t clamps to u = -1 (texel 0).
// The LUT is read through an LDS-typed pointer (LdsF4) when staged, a global one otherwise:
// never through a generic pointer chosen between the two.  (With one generic pointer the
// compiler merged both lookups into FLAT loads and folded the +1 texel offset into the
// instruction offset; for u < 0 (texel -1, the low sentinel) the base then sat 32 B below the
// LDS aperture, the access was routed as a global one to the aperture's base address, and the
// launch faulted with MEMORY_APERTURE_VIOLATION.)
typedef float F4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const F4v LdsF4;
template <typename Lut>
__device__ __forceinline__ float4 tf_lookup(Lut *lut, int n, float nf, float t)
{
    (void)n;
    float u = t * nf - 0.5f;
    u = fminf(fmaxf(u, -1.0f), nf);
    const float f = floorf(u);
    const float w = u - f;
    int e = (int)f + 1;
    if (VR_OOB(1, (unsigned long long)(long long)e, (unsigned long long)(n + 2))) e = 0;
    const auto a = lut[2 * e], d = lut[2 * e + 1];
    return make_float4(fmaf(w, d.x, a.x), fmaf(w, d.y, a.y), fmaf(w, d.z, a.z),
                       fmaf(w, d.w, a.w));
}

__device__ __forceinline__ uint32_t unorm8(float x)
{
    const float v = fminf(fmaxf(x, 0.0f), 1.0f);
    return (uint32_t)(v * 255.0f + 0.5f);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// skip_empty: longest leap in steps (bounds the float drift the leap margin must cover)
constexpr int kMaxLeap = 256;

// Minimum of k in [0, kMaxLeap] over the ACTIVE lanes (binary search on ballots: a ballot
// sees only active lanes, where a DPP reduction would read stale values of inactive ones).
__device__ __forceinline__ int wave_min_leap(int k)
{
    int lo = 0, hi = kMaxLeap;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (__ballot(k <= mid) != 0ull)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

#ifdef VR_WG_TIMES
// Experiment builds: per workgroup of the march launches since the last reset, 4 words: start
// and end wall clock (100 MHz), the tile id, and (XCC_ID << 32 | HW_ID) from the hardware
// registers (which XCD / SE / CU ran it); read by vr_debug_wg_times (tools/wg_timeline.py).
constexpr uint32_t kWgTimesMax = 1u << 17;
__device__ unsigned long long g_wg_times[4 * kWgTimesMax];
__device__ unsigned int g_wg_count;
__device__ __forceinline__ void wg_times_record(unsigned long long t0, uint32_t tile)
{
    const unsigned int slot = atomicAdd(&g_wg_count, 1u);
    if (slot < kWgTimesMax) {
        const unsigned long long hw = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
        const unsigned long long xcc = (unsigned)__builtin_amdgcn_s_getreg((3 << 11) | 20);
        g_wg_times[4 * slot] = t0;
        g_wg_times[4 * slot + 1] = (unsigned long long)wall_clock64();
        g_wg_times[4 * slot + 2] = ((unsigned long long)blockIdx.x << 32) | tile;
        g_wg_times[4 * slot + 3] = (xcc << 32) | hw;
    }
}
#endif

// Occupancy floor (waves per SIMD): the shaded f32 kernel holds 2 x 16-B centre loads plus
// 10 gradient loads in flight and would take 102 VGPRs (4 waves) unconstrained; 6 waves
// measured best (A/B: 0.79 vs 0.91 ms for C3).  The skip-empty kernel (scalar gradient) is
// left unconstrained (96 VGPRs, 5 waves: a floor of 5 yields the same occupancy but measured
// 12% slower), the counting kernels (not timed) get 4: no spills.
#ifndef VR_MARCH_MIN_WAVES
#define VR_MARCH_MIN_WAVES 6
#endif
#ifndef VR_SKIP_MIN_WAVES
#define VR_SKIP_MIN_WAVES 1
#endif
#ifndef VR_DEFER_SHADE
#define VR_DEFER_SHADE 1  // pipelined + difference field: shade a sample one sample later
#endif
#ifndef VR_PIPE_MIN_WAVES
#define VR_PIPE_MIN_WAVES 1
#endif
// The pipelined shaded kernel with the difference field (the C3 headline kernel).  Round 2,
// without deferred shading: 6 waves (78 VGPRs, no spills) against 5 unconstrained (84): C3
// +1.1% (profiles/r02/pipeline/min_waves6_*).  Deferred shading holds 24 more VGPRs of field
// rows: 94 VGPRs at 5 waves (at 6 it spills); C3 +1.2% against the round-2 kernel, shaded
// fill/oblique/top views 1-2% faster (profiles/r03/deferred_shading/).
#ifndef VR_PIPE_GF_MIN_WAVES
#define VR_PIPE_GF_MIN_WAVES (VR_DEFER_SHADE ? 5 : 6)
#endif
template <bool COUNT, bool SKIP, bool GF, bool PIPE>
constexpr int kMarchMinWaves =
    PIPE ? (GF ? VR_PIPE_GF_MIN_WAVES : VR_PIPE_MIN_WAVES)
         : (GF ? 1 : (COUNT ? 4 : (SKIP ? VR_SKIP_MIN_WAVES : VR_MARCH_MIN_WAVES)));

#ifndef VR_SKIP_PACKED_GRADIENT
#define VR_SKIP_PACKED_GRADIENT 0
#endif
template <bool SKIP>
constexpr bool kPackedGradient = !SKIP || VR_SKIP_PACKED_GRADIENT;

// GF: shaded f32 with the precomputed difference field (P.grad); without it the kernel forms
// the differences from the stencil (60 vs 80 VGPRs: 8 vs 6 waves per SIMD).
// Block -> tile.  Workgroups b and b+8 run on the same XCD (round-robin dispatch; speed
// only, never correctness).  Orders: 1 raster; 2 each XCD a contiguous band of tiles
// (bijective remap); 3 each XCD every 8th 4x4-tile super-tile in raster order, its tiles
// consecutive on that XCD: L2 locality inside a super-tile, every XCD sampling the whole
// frame (load balance when the volume covers part of it).  false: no tile (grid padding).
__device__ __forceinline__ bool block_tile(const MarchParams &P, uint32_t &tile_x,
                                           uint32_t &tile_y)
{
    const uint32_t nwg = gridDim.x, b = blockIdx.x;
    if (P.tile_perm) {  // adaptive order (launch_order_tiles)
        if (VR_OOB(5, b, P.nperm)) return false;
        const uint32_t t = P.tile_perm[b];
        if (t != 0xFFFFFFFFu && VR_OOB(6, t, P.tiles_x * P.tiles_y)) return false;
        tile_x = t % P.tiles_x;
        tile_y = t / P.tiles_x;
        return t != 0xFFFFFFFFu;
    }
    if (P.tile_order >= 3) {  // 3, and 4 before its first permutation
        const uint32_t k = b >> 3, w = k & (kSuper * kSuper - 1);
        const uint32_t s = (b & 7u) + 8u * (k >> (2 * kSuperShift));
        tile_x = (s % P.supers_x) * kSuper + (w & (kSuper - 1));
        tile_y = (s / P.supers_x) * kSuper + (w >> kSuperShift);
        return s < P.supers_total && tile_x < P.tiles_x && tile_y < P.tiles_y;
    }
    if (P.tile_order == 2) {
        const uint32_t xcd = b & 7u, q = nwg >> 3, r = nwg & 7u;
        const uint32_t t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
        tile_x = t % P.tiles_x;
        tile_y = t / P.tiles_x;
        return true;
    }
    tile_x = b % P.tiles_x;
    tile_y = b / P.tiles_x;
    return true;
}

// Headlight Phong of one sample from its filtered central differences (gx, gy, gz): gradient
// scaled to normalised coordinates, ndl = |n . dir|, rgb' = rgb (ka + kd ndl) + ks ndl^p; a
// zero gradient leaves the colour unshaded.  The oracle's march_pixel, same operation order.
__device__ __forceinline__ void phong(const MarchParams &P, float gx, float gy_, float gz,
                                      float d0, float d1, float d2, float4 &s)
{
    const float wx = gx * P.fnx, wy = gy_ * P.fny, wz = gz * P.fnz;
    const float g2 = wx * wx + wy * wy + wz * wz;
    if (g2 > 0.0f) {
        const float inv = inv_sqrt_ieee(g2);  // 1.0f / sqrtf(g2), vr_exact_math.h
        const float ndl = fabsf((wx * d0 + wy * d1 + wz * d2) * inv);
        const float kdiff = P.ka + P.kd * ndl;
        // ndl^p by binary exponentiation (the oracle's powi): p uniform.  The default p = 16
        // unrolled: powi squares four times and multiplies 1 by the result (exact), so
        // ((ndl^2)^2)^2)^2 is its value bit for bit, without the loop's scalar branches.
        float sp = 1.0f, b = ndl;
        if (P.spec_power == 16) {
            b = b * b;
            b = b * b;
            b = b * b;
            sp = b * b;
        } else {
            for (int e = P.spec_power; e;) {
                if (e & 1) sp = sp * b;
                e >>= 1;
                if (e) b = b * b;
            }
        }
        const float spec = P.ks * sp;
        s.x = s.x * kdiff + spec;
        s.y = s.y * kdiff + spec;
        s.z = s.z * kdiff + spec;
    }
}

// Gradient Phong extension for one sample with alpha > 0 (s: TF colour in/out): gradient from
// the difference field (GF) or the stencil, scaled to normalised coordinates, headlight
// ndl = |n . dir|, rgb' = rgb (ka + kd ndl) + ks ndl^p.  The oracle's march_pixel, same order.
template <typename VT, bool GF, bool PACKED>
__device__ __forceinline__ void shade_sample(const MarchParams &P, const char *__restrict__ vol,
                                             size_t ce, const Cell8<VT> &c, int pi, int pj,
                                             int pk, long by_stride, long bz_stride, float ax,
                                             float ay, float az, float d0, float d1, float d2,
                                             float4 &s)
{
    float gx, gy_, gz;
    if constexpr (GF) {  // f32: precomputed difference field
        grad_field<PACKED, kHalfField<VT>>(reinterpret_cast<const char *>(P.grad), ce, ax, ay, az,
                                           gx, gy_, gz);
    } else {
        gradient<VT, PACKED>(vol, ce, c, pi, pj, pk, P.nbx, P.nby, by_stride, bz_stride, ax, ay,
                             az, gx, gy_, gz);
    }
    phong(P, gx, gy_, gz, d0, d1, d2, s);
}

// ---- what the frame kernels share: a lane's pixel, the pixel's epilogue, the tile's frame ------
// (The ray walk itself -- position update, bounds break, slab test -- stays spelled out in each
// of march_strip, proj_strip, iso_strip and march_pair_kernel: every shared form of it tried
// moved the composite kernels' machine code or the range kernels' registers; CHANGELOG.)
// div_by_range, flush_counters, blend_over_clear and store_pixel are templates on the parameter
// struct: MarchParams for the frame kernels, MprArgs (same field names) for mpr_strip.

// Row ly of this rank's share of the frame -> the frame's row gy (vr_internal.h RowShare);
// false: below the frame.
__device__ __forceinline__ bool share_row(const MarchParams &P, uint32_t ly, uint32_t &gy)
{
    const uint32_t blk = ly / P.row_block;
    gy = share_global_block(blk, P.rank, P.nranks, RowShare{P.share_w0, P.share_w}) * P.row_block +
         (ly - blk * P.row_block);
    return gy < P.H;
}

// The pixel of a lane: column px, row ly of the share (the output's row), gy of the frame.
struct LanePixel {
    uint32_t px, ly, gy;
    bool active;  // inside the share and the frame
};
// Strip kernels: wavefront `wave` of the 16 x kMarchRows tile (tile_x, tile_y) covers ww x wh
// pixels, ww = 2^wave_w_shift; the wavefronts together tile the tile.
__device__ __forceinline__ LanePixel strip_pixel(const MarchParams &P, uint32_t tile_x,
                                                 uint32_t tile_y, uint32_t wave, uint32_t lane)
{
    const uint32_t ws = P.wave_w_shift, ww = 1u << ws, wh = 64u >> ws;
    const uint32_t wpr = kTile >> ws;  // wavefronts per tile row
    const uint32_t lx_ = lane & (ww - 1), ly_ = lane >> ws;
    LanePixel pix;
    pix.px = tile_x * kTile + (wave % wpr) * ww + lx_;
    pix.ly = tile_y * kMarchRows + (wave / wpr) * wh + ly_;
    pix.active = pix.px < P.W && pix.ly < P.local_rows;
    const bool in_frame = share_row(P, pix.ly, pix.gy);
    pix.active = pix.active && in_frame;
    return pix;
}

// The counting kernels' totals into vr_stats: rays, samples, shaded, steps, skipped.
template <typename PT>
__device__ __forceinline__ void flush_counters(const PT &P, uint32_t lane, bool covered,
                                               unsigned long long n_samples,
                                               unsigned long long n_shaded,
                                               unsigned long long n_steps,
                                               unsigned long long n_skipped)
{
    const unsigned long long rays = wave_sum(covered ? 1ull : 0ull);
    const unsigned long long sm = wave_sum(n_samples);
    const unsigned long long sh = wave_sum(n_shaded);
    const unsigned long long st = wave_sum(n_steps);
    const unsigned long long sk = wave_sum(n_skipped);
    if (lane == 0) {
        atomicAdd(&P.counters[0], rays);
        atomicAdd(&P.counters[1], sm);
        atomicAdd(&P.counters[2], sh);
        atomicAdd(&P.counters[3], st);
        atomicAdd(&P.counters[4], sk);
    }
}

// volume.frag:50 + blend (offscreen_pass.cpp:715-725) of a ray's colour C and transmittance T
// over the clear colour; an uncovered pixel has T = 1, C = 0 -> clear.
template <typename PT>
__device__ __forceinline__ float4 blend_over_clear(const PT &P, float cr, float cg,
                                                   float cb, float T)
{
    const float A = 1.0f - T;
    const float omA = 1.0f - A;
    return make_float4(cr * A + P.clear[0] * omA, cg * A + P.clear[1] * omA,
                       cb * A + P.clear[2] * omA, A * A + P.clear[3] * omA);
}

// The pixel's colour into the rank's output: RGBA8 (UNORM8 store :293) or RGBA32F.
template <typename PT>
__device__ __forceinline__ void store_pixel(const PT &P, uint32_t px, uint32_t ly,
                                            float4 o)
{
    const size_t idx = (size_t)ly * P.W + px;
    if (VR_OOB(4, idx * (P.out_format == 0 ? 4 : 16), P.out_bytes)) return;
    if (P.out_format == 0) {
        static_cast<uint32_t *>(P.out)[idx] =
            unorm8(o.x) | (unorm8(o.y) << 8) | (unorm8(o.z) << 16) | (unorm8(o.w) << 24);
    } else {
        static_cast<float4 *>(P.out)[idx] = o;
    }
}

// The TF into LDS ({texel, difference to the next} pairs + sentinels) by the workgroup's
// `threads` threads.
__device__ __forceinline__ void stage_tf(const MarchParams &P, float4 *s_tf, int threads)
{
    for (int i = threadIdx.x; i < 2 * (P.tf_n + 2); i += threads) s_tf[i] = P.tf[i];
}

// Adaptive order: this tile's duration for the next launch (the workgroup's last step).
__device__ __forceinline__ void write_tile_cost(const MarchParams &P, uint32_t tile_x,
                                                uint32_t tile_y, long long wg_start)
{
    if (P.tile_cost) {
        __syncthreads();
        if (threadIdx.x == 0)
            P.tile_cost[tile_y * P.tiles_x + tile_x] =
                (uint32_t)min(wall_clock64() - wg_start, 0x7FFFFFFFLL);
    }
}

// PIPE: the loads of sample k + 1 are issued before sample k is filtered, shaded and
// composited (two samples of the ray in flight).  For launches with few waves per CU (one
// rank's share of a multi-GPU frame), where every wave's serial chain of memory round trips,
// not the chip's throughput, sets the time.  Reference-semantics results are identical.
// One wavefront's strip of a tile (wave index `wave` of the 16 x kMarchRows tile (tile_x,
// tile_y)): every ray of it marched and its pixels written.  s_tf: the TF staged in LDS (when
// tf_in_lds).  march_kernel runs one tile per workgroup.
template <typename VT, bool SHADE, bool COUNT, bool SKIP, bool GF, bool PIPE>
__device__ __forceinline__ void march_strip(const MarchParams &P, LdsF4 *s_tf,
                                            bool tf_in_lds, uint32_t tile_x, uint32_t tile_y,
                                            uint32_t wave, uint32_t lane)
{
    using G = GeomOf<VT>;
    const long by_stride = (long)P.nbx * G::Elems;  // elements between brick rows/slabs
    const long bz_stride = (long)P.nbx * P.nby * G::Elems;

    const LanePixel pix = strip_pixel(P, tile_x, tile_y, wave, lane);

    float tex[3] = {0.f, 0.f, 0.f}, dir[3] = {0.f, 0.f, 0.f};
    const bool covered = pix.active && pixel_ray(P, pix.px, pix.gy, tex, dir);

    float T = 1.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
    unsigned long long n_samples = 0, n_shaded = 0, n_steps = 0, n_skipped = 0;
    uint32_t cur_brick = 0xFFFFFFFFu, cur_dist = 0;
    const char *__restrict__ vol = static_cast<const char *>(P.vol);
    const int nsteps = covered ? P.nsteps : 0;
    float p0 = tex[0], p1 = tex[1], p2 = tex[2];
    const float d0 = dir[0], d1 = dir[1], d2 = dir[2];
    // steps 1..kin need neither the bounds nor (default slicing) the slab test
    const int kin = (covered && P.slab_default) ? interior_steps(tex, dir, P.step, nsteps) : 0;
    // skip_empty leap constants: steps per cell along each axis, and a margin (cells) covering
    // the leap's float-accumulation drift (<= kMaxLeap half-ulps of p < 2, times N) + rounding
    float inv_du[3] = {0.f, 0.f, 0.f}, leap_margin[3] = {0.f, 0.f, 0.f};
    if (!COUNT && SKIP) {
        const float dd[3] = {d0, d1, d2}, fn[3] = {P.fnx, P.fny, P.fnz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            inv_du[a] = 1.0f / (fabsf(dd[a]) * P.step * fn[a]);
            leap_margin[a] = 0.5f + (float)kMaxLeap * 1.2e-7f * fn[a];
        }
    }
    if constexpr (PIPE) {
        // Positions, predicates and operations exactly as the loop below.  Loads are
        // unconditional (a cell of the first brick off-slab) and alpha is 0 off-slab, which
        // composites +0 and leaves T: no load sits under a data-dependent branch, so the
        // compiler waits with counted vmcnt(N) and the next sample's loads stay in flight.
        // The TF is LDS-resident (host guarantees tf_n <= kTfLds for PIPE).
        struct Stage {
            CellRaw<VT> w;  // loaded words, decoded at consume
            // the cell's element (kYMajor: the field's, in either order; 32-bit)
            std::conditional_t<kYMajor<VT>, uint32_t, size_t> ce;
            float ax, ay, az;
            int pi, pj, pk;
            bool ok, slab;
        };
        // live = false: a lane whose ray has ended; its stage is not ok and loads the first
        // brick's first cell (one cached line per wave), so the wave's loads stay unconditional
        auto prep = [&](Stage &S, int k, bool live = true) {
            const bool interior = (unsigned)(k - 1) < (unsigned)kin;
            S.ok = live && k < nsteps &&
                   (interior || !(p0 > 1.0f || p1 > 1.0f || p2 > 1.0f || p0 < 0.0f ||
                                  p1 < 0.0f || p2 < 0.0f));
            S.slab = S.ok && (interior || (p0 < P.smax[0] && p1 < P.smax[1] && p2 < P.smax[2] &&
                                           p0 > P.smin[0] && p1 > P.smin[1] && p2 > P.smin[2]));
            int i, j, kk;
            texel_coord(p0, P.fnx, i, S.ax);
            texel_coord(p1, P.fny, j, S.ay);
            texel_coord(p2, P.fnz, kk, S.az);
            if (!S.slab) i = j = kk = 0;
            S.pi = i + kPad;
            S.pj = j + kPad;
            S.pk = kk + kPad;
            if constexpr (kYMajor<VT>) {
                // the stage keeps the field's element of this cell: with the y-major field
                // (P.grad_ymajor, wave-uniform) the copy's own; with the shared z-major field
                // that one, and the copy's element -- another brick slot (ymajor_slot against
                // brick_slot), another in-brick order -- only issues the loads.  32-bit indices
                // (the host sends no volume of 2^32 elements here): the second index costs
                // one register, which a 64-bit one would not leave this kernel
                uint32_t e = (uint32_t)cell_offset<VT>(S.pi, S.pj, S.pk, P.nbx, P.nbz);
                S.ce = (!SHADE || P.grad_ymajor)
                           ? e
                           : (uint32_t)cell_offset<float>(S.pi, S.pj, S.pk, P.nbx, P.nby);
                if (VR_OOB(3, (size_t)e * kElemBytes<VT>, P.vol_bytes)) e = S.ce = 0;
                Cell8<VT>::issue(S.w, vol, e);
            } else {
                S.ce = cell_offset<VT>(S.pi, S.pj, S.pk, P.nbx, P.nby);
                if (VR_OOB(3, S.ce * kElemBytes<VT>, P.vol_bytes)) S.ce = 0;
                Cell8<VT>::issue(S.w, vol, S.ce);
            }
        };
        auto composite = [&](const float4 &sm) -> bool {  // volume.frag:44-45
            cr = cr + (sm.x * sm.w) * T;
            cg = cg + (sm.y * sm.w) * T;
            cb = cb + (sm.z * sm.w) * T;
            T = T * (1.0f - sm.w);
            return T == 0.0f || T < P.ert_eps;
        };
        // Deferred shading (shaded frames with the difference field): a sample with alpha > 0
        // issues its 6 field loads and is shaded and composited one sample later, when the next
        // sample is consumed (its loads landed under the same wait as that sample's density
        // loads, with the sample after it in flight).  Composites keep the sample order, an
        // alpha-0 sample composites exactly nothing (C += (rgb 0) T = +0, T *= 1) and is not
        // held back, and the ray still ends at the first T == 0 / T < eps: the same bits.
        constexpr bool kDefer = VR_DEFER_SHADE && SHADE && GF;
        struct Pend {
            FieldRowsT<kHalfField<VT>> g;
            float4 sm;
            float ax, ay, az;
            bool on;
        } X;
        X.on = false;
        auto finish = [&]() -> bool {  // shade + composite the held sample; true: the ray ends
            if (!kDefer || !X.on) return false;
            X.on = false;
            float gx, gy_, gz;
            field_rows_filter(X.g, X.ax, X.ay, X.az, gx, gy_, gz);
            phong(P, gx, gy_, gz, d0, d1, d2, X.sm);
            return composite(X.sm);
        };
        auto consume_cell = [&](const Stage &S, const Cell8<VT> &c) -> bool {  // true: the ray ends
            if (kDefer && finish()) return true;
            const float d = c.tri(S.ax, S.ay, S.az);
            const float tt = div_by_range(d - P.vmin, P);
            float4 sm = tf_lookup(s_tf, P.tf_n, P.tf_nf, tt);
            if (!S.slab) sm.w = 0.0f;
            if constexpr (kDefer) {
                if (sm.w > 0.0f) {
                    field_rows_load(reinterpret_cast<const char *>(P.grad), S.ce, X.g);
                    X.sm = sm;
                    X.ax = S.ax;
                    X.ay = S.ay;
                    X.az = S.az;
                    X.on = true;
                }
                return false;
            }
            if (SHADE && sm.w > 0.0f)
                shade_sample<VT, GF, true>(P, vol, S.ce, c, S.pi, S.pj, S.pk, by_stride,
                                           bz_stride, S.ax, S.ay, S.az, d0, d1, d2, sm);
            return composite(sm);
        };
        auto consume = [&](const Stage &S) -> bool {
            Cell8<VT> c;
            c.decode(S.w);
            return consume_cell(S, c);
        };
        auto advance = [&]() {
            p0 = p0 + d0 * P.step;
            p1 = p1 + d1 * P.step;
            p2 = p2 + d2 * P.step;
        };
        Stage A, B;
        int k = 0;
        {
            prep(A, k);
            while (A.ok) {  // ping-pong: no register copies between the two stages
                advance();
                prep(B, ++k);
                if (consume(A) || !B.ok) break;
                advance();
                prep(A, ++k);
                if (consume(B)) break;
            }
        }
        finish();  // deferred shading: the sample still held when the ray left the volume
    } else
    for (int it = 0; it < nsteps; ++it) {
        const bool interior = (unsigned)(it - 1) < (unsigned)kin;  // it in [1, kin]
        // volume.frag:34-37
        if (!interior &&
            (p0 > 1.0f || p1 > 1.0f || p2 > 1.0f || p0 < 0.0f || p1 < 0.0f || p2 < 0.0f))
            break;
        if (COUNT) ++n_steps;
        // volume.frag:39-40 (strict)
        if (interior || (p0 < P.smax[0] && p1 < P.smax[1] && p2 < P.smax[2] && p0 > P.smin[0] &&
                         p1 > P.smin[1] && p2 > P.smin[2])) {
            int i, j, k;
            float ax, ay, az;
            texel_coord(p0, P.fnx, i, ax);
            texel_coord(p1, P.fny, j, ay);
            texel_coord(p2, P.fnz, k, az);
            const int pi = i + kPad, pj = j + kPad, pk = k + kPad;
            uint32_t dist = 0;
            if (SKIP) {
                // skip_empty: distance (in bricks) from the cell's brick to the nearest brick
                // that can produce a visible sample (classify_kernel); cached per brick
                const uint32_t bb = ((uint32_t)pk / G::BZ * P.nby + (uint32_t)pj / G::BY) * P.nbx +
                                    (uint32_t)pi / G::BX;
                if (bb != cur_brick) {
                    cur_brick = bb;
                    cur_dist = P.skip_dist[bb];
                }
                dist = cur_dist;
            }
            // the wavefront leaps only when every lane sampling here is in empty space, and
            // by the smallest safe leap of its lanes: lanes stay in lock-step (a lane-private
            // leap desynchronises the wave and multiplies its fetch instructions)
            const bool wave_empty = SKIP && !COUNT && __all(dist != 0);
            if (dist != 0) {
                if (COUNT) {
                    ++n_skipped;  // the counting kernel walks every step (exact counters)
                } else if (wave_empty) {
                    // Leap: every brick within Chebyshev radius dist - 1 of this one is empty.
                    // Take the steps whose cells provably stay inside that box (cell
                    // coordinate u = p N - 0.5, brick of u: (floor(u) + 2) >> 3), advancing p
                    // with the same float additions as the reference loop, so the first
                    // non-empty sample is reached at the bit-identical position.
                    float kf = (float)min(nsteps - 1 - it, kMaxLeap);
                    const int bi[3] = {pi / G::BX, pj / G::BY, pk / G::BZ};
                    const float pp[3] = {p0, p1, p2}, dd[3] = {d0, d1, d2};
                    const float fn[3] = {P.fnx, P.fny, P.fnz};
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const float u = pp[a] * fn[a] - 0.5f;
                        const int bc = G::cells(a);
                        const float reach = (float)((int)(dist - 1) * bc);
                        const float room = dd[a] > 0.0f
                                               ? (float)((bi[a] + 1) * bc - kPad) + reach - u
                                               : u - (float)(bi[a] * bc - kPad) + reach;
                        // NaN (axis not moving) is ignored by fminf
                        kf = fminf(kf, (room - leap_margin[a]) * inv_du[a]);
                    }
                    const int k = wave_min_leap(kf >= 1.0f ? (int)kf : 0);
                    for (int j = 0; j < k; ++j) {
                        p0 = p0 + d0 * P.step;
                        p1 = p1 + d1 * P.step;
                        p2 = p2 + d2 * P.step;
                    }
                    it += k;
                }
            } else {
                size_t ce = cell_offset<VT>(pi, pj, pk, P.nbx, P.nby);
                if (VR_OOB(2, ce * kElemBytes<VT>, P.vol_bytes)) ce = 0;
                Cell8<VT> c;
                c.load(vol, ce);
                const float d = c.tri(ax, ay, az);
                // volume.frag:42 (d - min) / (max - min), correctly rounded; for a normal
                // range the reciprocal + one fma correction gives the IEEE quotient (see
                // div_by_range)
                const float tt = div_by_range(d - P.vmin, P);
                float4 s = tf_in_lds ? tf_lookup(s_tf, P.tf_n, P.tf_nf, tt)
                                     : tf_lookup(P.tf, P.tf_n, P.tf_nf, tt);
                if (COUNT) ++n_samples;
                if (SHADE && s.w > 0.0f) {
                    shade_sample<VT, GF, kPackedGradient<SKIP>>(P, vol, ce, c, pi, pj, pk, by_stride,
                                                                bz_stride, ax, ay, az, d0, d1, d2, s);
                    if (COUNT) ++n_shaded;
                }
                // volume.frag:44-45
                cr = cr + (s.x * s.w) * T;
                cg = cg + (s.y * s.w) * T;
                cb = cb + (s.z * s.w) * T;
                T = T * (1.0f - s.w);
                if (T == 0.0f) break;
                if (T < P.ert_eps) break;
            }
        }
        // volume.frag:47
        p0 = p0 + d0 * P.step;
        p1 = p1 + d1 * P.step;
        p2 = p2 + d2 * P.step;
    }

    if (COUNT) flush_counters(P, lane, covered, n_samples, n_shaded, n_steps, n_skipped);
    if (!pix.active) return;

    store_pixel(P, pix.px, pix.ly, blend_over_clear(P, cr, cg, cb, T));
}

// One workgroup's tile of a composite frame, the body of march_kernel and march_y_kernel: the
// TF staged in LDS (when it fits), each wavefront its strip, the tile's duration written back.
template <typename VT, bool SHADE, bool COUNT, bool SKIP, bool GF, bool PIPE>
__device__ __forceinline__ void march_tile(const MarchParams &P, float4 *s_tf, uint32_t tile_x,
                                           uint32_t tile_y, long long wg_start)
{
    const int tid = threadIdx.x;
    const bool tf_in_lds = P.tf_n <= kTfLds;  // (always with PIPE: the host grants it no other TF)
    if (tf_in_lds) stage_tf(P, s_tf, (int)kThreadsPerTile);
    __syncthreads();
    march_strip<VT, SHADE, COUNT, SKIP, GF, PIPE>(P, (LdsF4 *)s_tf, tf_in_lds, tile_x, tile_y,
                                                  (uint32_t)tid >> 6, (uint32_t)tid & 63u);
    write_tile_cost(P, tile_x, tile_y, wg_start);
}

template <typename VT, bool SHADE, bool COUNT, bool SKIP, bool GF, bool PIPE>
__global__ __launch_bounds__(kThreadsPerTile, (kMarchMinWaves<COUNT, SKIP, GF, PIPE>)) void march_kernel(const MarchParams P)
{
    __shared__ float4 s_tf[kTfLut];  // {texel, difference to the next} pairs + sentinels
    uint32_t tile_x, tile_y;
    if (!block_tile(P, tile_x, tile_y)) return;
    const long long wg_start = wall_clock64();
    march_tile<VT, SHADE, COUNT, SKIP, GF, PIPE>(P, s_tf, tile_x, tile_y, wg_start);
#ifdef VR_WG_TIMES
    __syncthreads();
    if (threadIdx.x == 0)
        wg_times_record((unsigned long long)wg_start, tile_y * P.tiles_x + tile_x);
#endif
}


// The y-major copy's kernels (VT = F32Y unshaded, F32HY shaded with the binary16 field): the
// pipelined single-lane march_strip over y-pair bricks.  A family of its own, so that
// march_kernel's instantiations stay those of its own layout list (vr_variant.h).
// The shaded one at a floor of 6 waves per SIMD: 80 VGPRs without scratch, as the F32H kernel
// takes unconstrained (unconstrained, this one takes 84 and drops to 5 waves).
template <typename VT, bool SHADE>
__global__ __launch_bounds__(kThreadsPerTile, (SHADE ? 6 : kMarchMinWaves<false, false, false, true>)) void march_y_kernel(const MarchParams P)
{
    static_assert(kYMajor<VT> && kHalfField<VT> == SHADE, "F32Y unshaded, F32HY shaded");
    __shared__ float4 s_tf[kTfLut];  // as march_kernel's
    uint32_t tile_x, tile_y;
    if (!block_tile(P, tile_x, tile_y)) return;
    march_tile<VT, SHADE, false, false, SHADE, true>(P, s_tf, tile_x, tile_y, wall_clock64());
}

// ---- maximum-, minimum- and mean-intensity projection (include/vr/vr_modes.h) ----------------
// The same ray as march_strip (pixel_ray, nsteps, the f32 position update, the bounds break and
// the strict slab test), but a pixel keeps one quantity v of its ray's trilinear samples and
// reads the TF once, at v: one composite step from T = 1 over the clear colour.  There is no
// dependent chain between samples: K steps' loads are issued before any of them is filtered
// (lanes whose ray has ended, or whose sample is off-slab or skipped, load element 0 of the
// volume, one cached line, so the loads stay unconditional; with SKIP a step no lane of the
// wave fetches issues no load).  mip_kernel runs OP = kProjMax, proj_kernel the other two.
//
// OP = kProjMax: v is the largest sample, m = fmaxf(m, d) from -INFINITY.  fmaxf is exact and
// commutative and ignores a NaN operand, so the order the samples are taken in, K, and which
// samples are proven not to exceed the running maximum and left out, never show in the frame.
//   SKIP: a sample whose brick's stored maximum hi (brick_range_kernel: every value a sample in
//   the brick can read, apron and zero border included) is not above the ray's running maximum
//   is not fetched.  Exact: a sample is three levels of fmaf(w, b - a, a) with w in [0, 1].  For
//   8/16-bit voxels b - a is exact, so each level is the correctly rounded value of a point
//   between a and b and cannot pass max(a, b): tri <= hi.  For f32 voxels b - a rounds, and with
//   w = 1 (u - floor(u) rounds up to 1 just below a voxel centre) a level can pass max(a, b) by
//   an ulp of the larger operand, so hi is widened by the classifier's margin (classify_kernel,
//   4e-6 (|lo| + |hi|), three orders above the three roundings; infinite when b - a can
//   overflow).  !(hi <= m) keeps NaN bricks.  The test reads m as it stood before the batch of
//   K steps: any earlier value of the maximum proves the same.  A ray of an 8/16-bit volume
//   ends once m reaches the largest hi of the volume (the entry after the last brick).
// OP = kProjMin: the mirror image, m = fminf(m, d) from +INFINITY.  The bound is the brick's
//   stored minimum lo, lowered for f32 by the same margin (-INFINITY when b - a can overflow):
//   tri >= lo by the argument above with min(a, b) for max(a, b).  !(lo >= m) keeps NaN bricks,
//   and the ray ends once m reaches the smallest lo of the volume (then a sample was taken: m
//   is finite only after one).
// OP = kProjMean: v = sum / (float)n, sum one f32 addition per in-slab sample from +0.  The
// order of the additions is part of the result: the consume half of a batch adds its K samples
// in step order into the one running sum, so every K gives the reference's bits.
//   SKIP: a sample whose brick has lo == hi, finite, is not fetched and adds lo at its step's
//   place (it counts in n).  Exact: every voxel the sample can read is c = lo, each lerp level
//   is fmaf(w, c - c, c) = fmaf(w, 0, c) = c for finite c.  An infinite c gives inf - inf =
//   NaN, so such a brick is fetched; a NaN brick stores (NaN, NaN) and lo == hi is false.  A
//   brick of mixed +0 / -0 also has lo == hi and adds a zero of either sign where the filter
//   gives one of either sign: x + (+-0) = x for x != 0, +0 + (+-0) = +0, and a sum that
//   started at +0 is never -0 (two operands sum to -0 only when both are -0), so the sign
//   never shows.  There is no early end.
// COUNT: walks every step, fetches and skips per lane, and fills vr_stats (shaded 0); samples +
// skipped is the number of in-slab steps.
template <typename VT>
constexpr bool kMipQuadRaw = !kZPair<VT> && !kPlainByte<VT>;
template <typename VT, typename = void>
struct MipRaw {
    CellRaw<VT> w;
    __device__ __forceinline__ void issue(const char *__restrict__ base, size_t e)
    {
        Cell8<VT>::issue(w, base, e);
    }
    __device__ __forceinline__ void decode(Cell8<VT> &c) const { c.decode(w); }
};
// yz-quad elements: the loaded words, decoded at consume (as CellRaw's z-pair and byte forms)
template <typename VT>
struct MipRaw<VT, std::enable_if_t<kMipQuadRaw<VT>>> {
    uint32_t w[2 * kQuadWords<VT>];
    __device__ __forceinline__ void issue(const char *__restrict__ base, size_t e)
    {
        quad_load2<VT>(base, e, w);
    }
    __device__ __forceinline__ void decode(Cell8<VT> &c) const
    {
        constexpr int QW = kQuadWords<VT>;
        c.v[0] = qc<VT>(w, 0);
        c.v[4] = qc<VT>(w, 1);
        c.v[2] = qc<VT>(w, 2);
        c.v[6] = qc<VT>(w, 3);
        c.v[1] = qc<VT>(w + QW, 0);
        c.v[5] = qc<VT>(w + QW, 1);
        c.v[3] = qc<VT>(w + QW, 2);
        c.v[7] = qc<VT>(w + QW, 3);
    }
};

template <typename VT, int OP, bool COUNT, bool SKIP, int K>
__device__ __forceinline__ void proj_strip(const MarchParams &P, const ProjArgs &M, uint32_t tile_x,
                                           uint32_t tile_y, uint32_t wave, uint32_t lane)
{
    static_assert(OP == kProjMin || OP == kProjMean || OP == kProjMax, "minimum, mean or maximum");
    static_assert(!COUNT || K == 1, "the counting kernels walk one step at a time");
    constexpr bool MEAN = OP == kProjMean, MAX = OP == kProjMax;
    using G = GeomOf<VT>;
    const LanePixel pix = strip_pixel(P, tile_x, tile_y, wave, lane);

    float tex[3] = {0.f, 0.f, 0.f}, dir[3] = {0.f, 0.f, 0.f};
    const bool covered = pix.active && pixel_ray(P, pix.px, pix.gy, tex, dir);

    float m = MEAN ? 0.0f : MAX ? -INFINITY : INFINITY;  // the running sum, maximum or minimum
    int n = 0;                                           // mean: in-slab samples so far
    bool any = false;
    unsigned long long n_samples = 0, n_steps = 0, n_skipped = 0;
    uint32_t cur_brick = 0xFFFFFFFFu;
    // max / min: the brick's (widened) hi / (lowered) lo; mean: its constant or NaN
    float cur_bound = MEAN ? NAN : MAX ? INFINITY : -INFINITY;
    const char *__restrict__ vol = static_cast<const char *>(P.vol);
    const int nsteps = covered ? P.nsteps : 0;
    float p0 = tex[0], p1 = tex[1], p2 = tex[2];
    const float d0 = dir[0], d1 = dir[1], d2 = dir[2];
    const int kin = (covered && P.slab_default) ? interior_steps(tex, dir, P.step, nsteps) : 0;
    // 8/16-bit volumes: no sample is above the largest brick maximum / below the smallest minimum
    float end_at = MAX ? INFINITY : -INFINITY;
    if constexpr (!MEAN && SKIP && !COUNT && !kZPair<VT>)
        end_at = MAX ? M.brick_range[M.nbricks].y : M.brick_range[M.nbricks].x;

    // The maximum keeps its own Stage and takes its sample inside the issued branch, as
    // mip_kernel did before it ran this strip: with the minimum's forms 42 of the 56 mip_kernel
    // come out in another instruction order and the skipping ones run 1-3 % slower
    // (profiles/r12/proj_max/); so they are the same machine code as before.
    struct StageMax {
        MipRaw<VT> r;
        float ax, ay, az;
        bool fetch, issued;
    };
    struct StageSlab : StageMax {
        float c;  // mean with SKIP: what a sample that is not fetched adds
        bool slab;
    };
    using Stage = std::conditional_t<MAX, StageMax, StageSlab>;
    bool live = nsteps > 0;
    for (int it = 0; live; it += K) {
        Stage S[K];
        const float m_in = m;
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const int k = it + s;
            const bool interior = (unsigned)(k - 1) < (unsigned)kin;
            // volume.frag:34-37: the first position outside ends the ray
            live = live && k < nsteps &&
                   (interior || !(p0 > 1.0f || p1 > 1.0f || p2 > 1.0f || p0 < 0.0f || p1 < 0.0f ||
                                  p2 < 0.0f));
            if (COUNT && live) ++n_steps;
            // volume.frag:39-40 (strict)
            const bool slab = live && (interior || (p0 < P.smax[0] && p1 < P.smax[1] &&
                                                    p2 < P.smax[2] && p0 > P.smin[0] &&
                                                    p1 > P.smin[1] && p2 > P.smin[2]));
            int i, j, kk;
            texel_coord(p0, P.fnx, i, S[s].ax);
            texel_coord(p1, P.fny, j, S[s].ay);
            texel_coord(p2, P.fnz, kk, S[s].az);
            const int pi = i + kPad, pj = j + kPad, pk = kk + kPad;
            bool fetch = slab;
            if constexpr (SKIP) {
                if (slab) {
                    const uint32_t bb = ((uint32_t)pk / G::BZ * P.nby + (uint32_t)pj / G::BY) * P.nbx +
                                        (uint32_t)pi / G::BX;
                    if (bb != cur_brick) {
                        cur_brick = bb;
                        const float2 r = VR_OOB(7, bb, M.nbricks) ? make_float2(NAN, NAN)
                                                                   : M.brick_range[bb];
                        if constexpr (MEAN)
                            cur_bound = (r.x == r.y && fabsf(r.x) < INFINITY) ? r.x : NAN;
                        else if constexpr (MAX)
                            cur_bound = kZPair<VT> ? r.y + (fabsf(r.x) + fabsf(r.y)) * 4.0e-6f : r.y;
                        else
                            cur_bound = kZPair<VT> ? r.x - (fabsf(r.x) + fabsf(r.y)) * 4.0e-6f : r.x;
                    }
                    fetch = MEAN  ? cur_bound != cur_bound
                            : MAX ? !(cur_bound <= m_in)
                                  : !(cur_bound >= m_in);
                }
                if constexpr (!MAX) S[s].c = cur_bound;
            }
            if (COUNT && slab) {
                if (fetch)
                    ++n_samples;
                else
                    ++n_skipped;
            }
            any = any || slab;
            if constexpr (!MAX) S[s].slab = slab;
            S[s].fetch = fetch;
            size_t ce = fetch ? cell_offset<VT>(pi, pj, pk, P.nbx, P.nby) : (size_t)0;
            if (VR_OOB(2, ce * kElemBytes<VT>, P.vol_bytes)) ce = 0;
            // without SKIP every step loads; with it a step no lane of the wave fetches does not
            S[s].issued = !SKIP || __any(fetch);
            if (S[s].issued) S[s].r.issue(vol, ce);
            // volume.frag:47
            p0 = p0 + d0 * P.step;
            p1 = p1 + d1 * P.step;
            p2 = p2 + d2 * P.step;
        }
#pragma unroll
        for (int s = 0; s < K; ++s) {  // in step order: the mean's additions are ordered
            float d = 0.0f;
            if (S[s].issued) {
                Cell8<VT> c;
                S[s].r.decode(c);
                d = c.tri(S[s].ax, S[s].ay, S[s].az);
                if constexpr (MAX)
                    if (S[s].fetch) m = fmaxf(m, d);  // a NaN sample leaves m
            }
            if constexpr (MEAN) {
                if constexpr (SKIP) d = S[s].fetch ? d : S[s].c;
                if (S[s].slab) {
                    m = m + d;
                    ++n;
                }
            } else if constexpr (!MAX) {
                if (S[s].fetch) m = fminf(m, d);  // a NaN sample leaves m
            }
        }
        if (!MEAN && !COUNT && (MAX ? m >= end_at : m <= end_at)) live = false;
    }

    if (COUNT) flush_counters(P, lane, covered, n_samples, 0, n_steps, n_skipped);
    if (!pix.active) return;

    // one composite step from T = 1 (volume.frag:42-45), then the blend over the clear colour
    float T = 1.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
    if (any) {
        const float v = MEAN ? m / (float)n : m;  // (the correctly rounded quotient: Makefile)
        const float tt = div_by_range(v - P.vmin, P);
        const float4 s = tf_lookup(P.tf, P.tf_n, P.tf_nf, tt);
        cr = (s.x * s.w) * 1.0f;
        cg = (s.y * s.w) * 1.0f;
        cb = (s.z * s.w) * 1.0f;
        T = 1.0f * (1.0f - s.w);
    }
    store_pixel(P, pix.px, pix.ly, blend_over_clear(P, cr, cg, cb, T));
}

template <typename VT, bool COUNT, bool SKIP, int K>
__global__ __launch_bounds__(kThreadsPerTile) void mip_kernel(const MarchParams P, const MipArgs M)
{
    const int tid = threadIdx.x;
    uint32_t tile_x, tile_y;
    if (!block_tile(P, tile_x, tile_y)) return;
    const long long wg_start = wall_clock64();
    proj_strip<VT, kProjMax, COUNT, SKIP, K>(P, ProjArgs{M.brick_range, M.nbricks}, tile_x, tile_y,
                                             (uint32_t)tid >> 6, (uint32_t)tid & 63u);
    write_tile_cost(P, tile_x, tile_y, wg_start);
}

template <typename VT, int OP, bool COUNT, bool SKIP, int K>
__global__ __launch_bounds__(kThreadsPerTile) void proj_kernel(const MarchParams P, const ProjArgs M)
{
    const int tid = threadIdx.x;
    uint32_t tile_x, tile_y;
    if (!block_tile(P, tile_x, tile_y)) return;
    const long long wg_start = wall_clock64();
    proj_strip<VT, OP, COUNT, SKIP, K>(P, M, tile_x, tile_y, (uint32_t)tid >> 6, (uint32_t)tid & 63u);
    write_tile_cost(P, tile_x, tile_y, wg_start);
}

// ---- multi-planar reformat (include/vr/vr_mpr.h) -----------------------------------------------
// A plane through the volume, thin or thickened into a slab of nsamples positions along its
// normal: a parallel, short ray set that starts on the plane instead of at the camera.  One pixel
// per lane, 16 x 16-pixel tiles (thin slices in raster order, slabs in the frames' XCD-interleaved
// super-tiles: kMprTileOrder), a wavefront the 16 x 4 strip of strip_pixel.
// Sample s of pixel (px, py) is at
//     q = (float)(origin + cx du + cy dv + t dn),   cx = px + 0.5 - W / 2, cy = py + 0.5 - H / 2,
//                                                   t = s - (nsamples - 1) / 2
// left to right in double, rounded once (contraction is off, and each product is exact anyway):
// the prefix origin + cx du + cy dv is the pixel's own, and no position depends on the one
// before it, so the loads of up to K = 4 samples are issued before any is filtered, as
// proj_strip's, with its MipRaw and the composite's Cell8::tri.  The trip count is uniform, so a
// step no lane of the wavefront samples (an overhanging image, the slice box) loads nothing.
// Unlike a march a position outside the cube is passed over, not the end of the ray.
// OP = kMprMax / kMprMin / kMprMean: proj_strip's operators (NaN rules included); the mean adds
// in s order into the one running sum whatever K is.  kMprThin: nsamples == 1, no loop; the
// three operators then differ for a NaN sample only, so one instantiation per storage tag reads
// A.op at run time and performs that operator's own single operation.
// COUNT: walks the positions and fills vr_stats (rays = pixels with a step; shaded and skipped
// 0); it fetches nothing and writes no pixel, so one instantiation serves every layout.
template <typename VT, int OP, bool COUNT>
__device__ __forceinline__ void mpr_strip(const MprArgs &A, uint32_t tile_x, uint32_t tile_y,
                                          uint32_t wave, uint32_t lane)
{
    static_assert(OP == kMprMax || OP == kMprMin || OP == kMprMean || OP == kMprThin, "vr_mpr_op or thin");
    constexpr bool MEAN = OP == kMprMean, MAX = OP == kMprMax, THIN = OP == kMprThin;
    constexpr int K = THIN ? 1 : 4;
    const uint32_t px = tile_x * kTile + (lane & 15u);
    const uint32_t py = tile_y * kTile + wave * 4u + (lane >> 4);
    const bool active = px < A.W && py < A.H;

    const double cx = (double)px + 0.5 - A.half_w, cy = (double)py + 0.5 - A.half_h;
    double b[3];  // the pixel's prefix of the position sum
#pragma unroll
    for (int a = 0; a < 3; ++a) b[a] = A.origin[a] + cx * A.du[a] + cy * A.dv[a];

    // slab kernels: the running maximum, minimum or sum; thin: the one sample
    float m = MEAN ? 0.0f : MAX ? -INFINITY : INFINITY;
    int n = 0;  // in-slab samples so far
    unsigned long long n_steps = 0;
    const char *__restrict__ vol = static_cast<const char *>(A.vol);
    const uint32_t ns = THIN ? 1u : A.nsamples;

    struct Stage {
        MipRaw<VT> r;
        float ax, ay, az;
        bool slab, issued;
    };
    for (uint32_t it = 0; it < ns; it += K) {
        Stage S[K];
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const double t = (double)(it + (uint32_t)s) - A.half_n;
            const float q0 = (float)(b[0] + t * A.dn[0]);
            const float q1 = (float)(b[1] + t * A.dn[1]);
            const float q2 = (float)(b[2] + t * A.dn[2]);
            // the march's bounds test: a position outside is no step
            const bool step = active && it + (uint32_t)s < ns &&
                              !(q0 > 1.0f || q1 > 1.0f || q2 > 1.0f || q0 < 0.0f || q1 < 0.0f ||
                                q2 < 0.0f);
            if (COUNT && step) ++n_steps;
            // the march's strict slab test
            const bool slab = step && q0 < A.smax[0] && q1 < A.smax[1] && q2 < A.smax[2] &&
                              q0 > A.smin[0] && q1 > A.smin[1] && q2 > A.smin[2];
            S[s].slab = slab;
            if constexpr (COUNT) {
                S[s].issued = false;
            } else {
                int i, j, kk;
                texel_coord(q0, A.fnx, i, S[s].ax);
                texel_coord(q1, A.fny, j, S[s].ay);
                texel_coord(q2, A.fnz, kk, S[s].az);
                // in the cube: i in [-1, n - 1], padded index in [1, n + 1] (vr_internal.h bricks_for)
                size_t ce = slab ? cell_offset<VT>(i + kPad, j + kPad, kk + kPad, A.nbx, A.nby)
                                 : (size_t)0;
                if (VR_OOB(2, ce * kElemBytes<VT>, A.vol_bytes)) ce = 0;
                S[s].issued = __any(slab);
                if (S[s].issued) S[s].r.issue(vol, ce);
            }
        }
#pragma unroll
        for (int s = 0; s < K; ++s) {  // in s order: the mean's additions are ordered
            if constexpr (COUNT) {
                if (S[s].slab) ++n;
            } else if (S[s].issued) {
                Cell8<VT> c;
                S[s].r.decode(c);
                const float d = c.tri(S[s].ax, S[s].ay, S[s].az);
                if (S[s].slab) {
                    ++n;
                    if constexpr (THIN)
                        m = A.op == kMprMax   ? fmaxf(-INFINITY, d)
                            : A.op == kMprMin ? fminf(INFINITY, d)
                                              : (0.0f + d) / 1.0f;
                    else if constexpr (MEAN)
                        m = m + d;
                    else if constexpr (MAX)
                        m = fmaxf(m, d);  // a NaN sample leaves m
                    else
                        m = fminf(m, d);
                }
            }
        }
    }

    if constexpr (COUNT) {
        flush_counters(A, lane, n_steps > 0, (unsigned long long)n, 0, n_steps, 0);
        return;
    }
    if (!active) return;
    // one composite step from T = 1 (volume.frag:42-45), then the blend over the clear colour
    float T = 1.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
    if (n > 0) {
        const float v = MEAN ? m / (float)n : m;  // (the correctly rounded quotient: Makefile)
        // A pixel whose samples are all NaN keeps the operator's start, -+INFINITY, and x is then
        // infinite: the IEEE quotient by the (positive, div_fast) range is x itself, where
        // div_by_range's residual correction would give inf - inf = NaN (texel 0 for +inf too).
        const float x = v - A.vmin;
        const float tt = A.div_fast && fabsf(x) == INFINITY ? x : div_by_range(x, A);
        const float4 s = tf_lookup(A.tf, A.tf_n, A.tf_nf, tt);
        cr = (s.x * s.w) * 1.0f;
        cg = (s.y * s.w) * 1.0f;
        cb = (s.z * s.w) * 1.0f;
        T = 1.0f * (1.0f - s.w);
    }
    store_pixel(A, px, py, blend_over_clear(A, cr, cg, cb, T));
}

template <typename VT, int OP, bool COUNT>
__global__ __launch_bounds__(kTile * kTile) void mpr_kernel(const MprArgs A)
{
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    uint32_t tile_x = b % A.tiles_x, tile_y = b / A.tiles_x;
    if (A.tile_order == 3) {  // block_tile's order 3: workgroups b and b + 8 share an XCD
        const uint32_t k = b >> 3, w = k & (kSuper * kSuper - 1);
        const uint32_t s = (b & 7u) + 8u * (k >> (2 * kSuperShift));
        tile_x = (s % A.supers_x) * kSuper + (w & (kSuper - 1));
        tile_y = (s / A.supers_x) * kSuper + (w >> kSuperShift);
        if (!(s < A.supers_total && tile_x < A.tiles_x && tile_y < A.tiles_y)) return;  // grid padding
    }
    mpr_strip<VT, OP, COUNT>(A, tile_x, tile_y, tid >> 6, tid & 63u);
}

// ---- first-hit isosurface (include/vr/vr_iso.h) ----------------------------------------------
// The same ray as march_strip and proj_strip, but the pixel shows the first in-slab sample whose
// density reaches the isovalue: a search with an ordered early exit, then -- once the whole
// wavefront has left the search loop -- four bisection fetches between the last sample below
// (q) and the hit, one gradient from the base bricks (the exact f32 central differences of
// gradient<VT>, never the binary16 field) and the composite's Phong; the pixel is opaque.
// The search loop is proj_strip's: K steps' loads are issued before any is filtered, lanes
// whose ray has ended or whose sample is off-slab or skipped load element 0.  Unlike the
// maximum the result depends on the order: the samples of a batch are examined in step order
// behind a position cursor that repeats the ray's own additions, the hit is the lowest step
// that passes, q the in-slab step before it (possibly of the previous batch), and what the
// batch loaded beyond the hit is dropped.  So the frame is the same for every K.
//
// SKIP: a sample whose brick's stored maximum hi (widened for f32 as proj_strip's, by the same
// argument: every sample in the brick is <= hi) is below the isovalue cannot hit and is not
// fetched; it still counts as a sample below (prev, q).  !(hi < iso) keeps NaN bricks, and a
// NaN sample never hits (d >= iso is false).
// COUNT (K = 1, so a hit ends the lane before its next step is counted): rays, steps, search
// samples fetched and skipped; shaded = rays whose surface point was shaded.  The bisection
// fetches are not counted.
template <typename VT, bool COUNT, bool SKIP, int K>
__device__ __forceinline__ void iso_strip(const MarchParams &P, const IsoArgs &I, uint32_t tile_x,
                                          uint32_t tile_y, uint32_t wave, uint32_t lane)
{
    static_assert(!COUNT || K == 1, "the counting kernels walk one step at a time");
    using G = GeomOf<VT>;
    const long by_stride = (long)P.nbx * G::Elems;  // elements between brick rows/slabs
    const long bz_stride = (long)P.nbx * P.nby * G::Elems;
    const LanePixel pix = strip_pixel(P, tile_x, tile_y, wave, lane);

    float tex[3] = {0.f, 0.f, 0.f}, dir[3] = {0.f, 0.f, 0.f};
    const bool covered = pix.active && pixel_ray(P, pix.px, pix.gy, tex, dir);

    const float iso = I.iso;
    bool hit = false, prev = false;
    float q0 = 0.f, q1 = 0.f, q2 = 0.f;  // the last in-slab position below the isovalue
    float h0 = 0.f, h1 = 0.f, h2 = 0.f;  // the hit
    unsigned long long n_samples = 0, n_steps = 0, n_skipped = 0;
    uint32_t cur_brick = 0xFFFFFFFFu;
    float cur_hi = INFINITY;
    const char *__restrict__ vol = static_cast<const char *>(P.vol);
    const int nsteps = covered ? P.nsteps : 0;
    float p0 = tex[0], p1 = tex[1], p2 = tex[2];
    const float d0 = dir[0], d1 = dir[1], d2 = dir[2];
    const int kin = (covered && P.slab_default) ? interior_steps(tex, dir, P.step, nsteps) : 0;

    struct Stage {
        MipRaw<VT> r;
        float ax, ay, az;
        bool live, slab, fetch, issued;
    };
    bool live = nsteps > 0;
    for (int it = 0; live; it += K) {
        Stage S[K];
        float c0 = p0, c1 = p1, c2 = p2;  // the position of the step being examined
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const int k = it + s;
            const bool interior = (unsigned)(k - 1) < (unsigned)kin;
            // volume.frag:34-37: the first position outside ends the ray
            live = live && k < nsteps &&
                   (interior || !(p0 > 1.0f || p1 > 1.0f || p2 > 1.0f || p0 < 0.0f || p1 < 0.0f ||
                                  p2 < 0.0f));
            if (COUNT && live) ++n_steps;
            // volume.frag:39-40 (strict)
            const bool slab = live && (interior || (p0 < P.smax[0] && p1 < P.smax[1] &&
                                                    p2 < P.smax[2] && p0 > P.smin[0] &&
                                                    p1 > P.smin[1] && p2 > P.smin[2]));
            int i, j, kk;
            texel_coord(p0, P.fnx, i, S[s].ax);
            texel_coord(p1, P.fny, j, S[s].ay);
            texel_coord(p2, P.fnz, kk, S[s].az);
            const int pi = i + kPad, pj = j + kPad, pk = kk + kPad;
            bool fetch = slab;
            if constexpr (SKIP) {
                if (slab) {
                    const uint32_t bb = ((uint32_t)pk / G::BZ * P.nby + (uint32_t)pj / G::BY) * P.nbx +
                                        (uint32_t)pi / G::BX;
                    if (bb != cur_brick) {
                        cur_brick = bb;
                        const float2 r = VR_OOB(7, bb, I.nbricks) ? make_float2(NAN, NAN)
                                                                   : I.brick_range[bb];
                        cur_hi = kZPair<VT> ? r.y + (fabsf(r.x) + fabsf(r.y)) * 4.0e-6f : r.y;
                    }
                    fetch = !(cur_hi < iso);
                }
            }
            if (COUNT && slab) {
                if (fetch)
                    ++n_samples;
                else
                    ++n_skipped;
            }
            S[s].live = live;
            S[s].slab = slab;
            S[s].fetch = fetch;
            size_t ce = fetch ? cell_offset<VT>(pi, pj, pk, P.nbx, P.nby) : (size_t)0;
            if (VR_OOB(2, ce * kElemBytes<VT>, P.vol_bytes)) ce = 0;
            // without SKIP every step loads; with it a step no lane of the wave fetches does not
            S[s].issued = !SKIP || __any(fetch);
            if (S[s].issued) S[s].r.issue(vol, ce);
            // volume.frag:47
            p0 = p0 + d0 * P.step;
            p1 = p1 + d1 * P.step;
            p2 = p2 + d2 * P.step;
        }
#pragma unroll
        for (int s = 0; s < K; ++s) {
            float d = 0.0f;
            if (S[s].issued) {
                Cell8<VT> c;
                S[s].r.decode(c);
                d = c.tri(S[s].ax, S[s].ay, S[s].az);
            }
            if (!hit && S[s].live) {
                if (S[s].slab) {
                    if (S[s].fetch && d >= iso) {
                        hit = true;
                        h0 = c0;
                        h1 = c1;
                        h2 = c2;
                    } else {
                        prev = true;
                        q0 = c0;
                        q1 = c1;
                        q2 = c2;
                    }
                } else {
                    prev = false;
                }
            }
            c0 = c0 + d0 * P.step;
            c1 = c1 + d1 * P.step;
            c2 = c2 + d2 * P.step;
        }
        live = live && !hit;
    }

    const bool shade = hit && I.shading != 0;
    if (COUNT)
        flush_counters(P, lane, covered, n_samples, shade ? 1ull : 0ull, n_steps, n_skipped);
    if (!pix.active) return;

    // no hit: the clear colour, with an uncovered pixel's arithmetic (T = 1, C = 0)
    float o0 = 0.0f * 0.0f + P.clear[0] * 1.0f, o1 = 0.0f * 0.0f + P.clear[1] * 1.0f,
          o2 = 0.0f * 0.0f + P.clear[2] * 1.0f, o3 = 0.0f * 0.0f + P.clear[3] * 1.0f;
    if (hit) {
        if (prev) {  // bisection between q (below) and the hit (at or above): in-slab by convexity
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                const float m0 = (q0 + h0) * 0.5f, m1 = (q1 + h1) * 0.5f, m2 = (q2 + h2) * 0.5f;
                int i, j, kk;
                float ax, ay, az;
                texel_coord(m0, P.fnx, i, ax);
                texel_coord(m1, P.fny, j, ay);
                texel_coord(m2, P.fnz, kk, az);
                size_t ce = cell_offset<VT>(i + kPad, j + kPad, kk + kPad, P.nbx, P.nby);
                if (VR_OOB(2, ce * kElemBytes<VT>, P.vol_bytes)) ce = 0;
                Cell8<VT> c;
                c.load(vol, ce);
                const bool above = c.tri(ax, ay, az) >= iso;
                h0 = above ? m0 : h0;
                h1 = above ? m1 : h1;
                h2 = above ? m2 : h2;
                q0 = above ? q0 : m0;
                q1 = above ? q1 : m1;
                q2 = above ? q2 : m2;
            }
        }
        // the surface colour: the TF at the isovalue (alpha ignored), read through the global
        // pointer once per ray
        const float tt = div_by_range(iso - P.vmin, P);
        float4 s = tf_lookup(P.tf, P.tf_n, P.tf_nf, tt);
        if (shade) {
            int i, j, kk;
            float ax, ay, az;
            texel_coord(h0, P.fnx, i, ax);
            texel_coord(h1, P.fny, j, ay);
            texel_coord(h2, P.fnz, kk, az);
            const int pi = i + kPad, pj = j + kPad, pk = kk + kPad;
            size_t ce = cell_offset<VT>(pi, pj, pk, P.nbx, P.nby);
            if (VR_OOB(2, ce * kElemBytes<VT>, P.vol_bytes)) ce = 0;
            Cell8<VT> c;
            c.load(vol, ce);
            float gx, gy_, gz;
            gradient<VT, false>(vol, ce, c, pi, pj, pk, P.nbx, P.nby, by_stride, bz_stride, ax, ay,
                                az, gx, gy_, gz);
            phong(P, gx, gy_, gz, d0, d1, d2, s);
        }
        o0 = s.x;
        o1 = s.y;
        o2 = s.z;
        o3 = 1.0f;
    }
    store_pixel(P, pix.px, pix.ly, make_float4(o0, o1, o2, o3));
}

template <typename VT, bool COUNT, bool SKIP, int K>
__global__ __launch_bounds__(kThreadsPerTile) void iso_kernel(const MarchParams P, const IsoArgs I)
{
    const int tid = threadIdx.x;
    uint32_t tile_x, tile_y;
    if (!block_tile(P, tile_x, tile_y)) return;
    const long long wg_start = wall_clock64();
    iso_strip<VT, COUNT, SKIP, K>(P, I, tile_x, tile_y, (uint32_t)tid >> 6, (uint32_t)tid & 63u);
    write_tile_cost(P, tile_x, tile_y, wg_start);
}

// ---- hit records and picking (include/vr/vr_hit.h) --------------------------------------------
// The same ray as march_strip, proj_strip and iso_strip, but the lane writes where its pixel
// comes from instead of a colour: one 24-byte record {pos[3], depth, value, step}.  P describes
// the request's rectangle (W, H, local_rows and the tile counts; vr_internal.h HitArgs) and the
// ray is the one of framebuffer pixel (A.x0 + px, A.y0 + gy).  The walk is iso_strip's search
// loop without range skipping: K steps' loads are issued before any is filtered, lanes whose
// ray has ended or whose sample is off-slab load element 0, and the samples of a batch are
// examined in step order behind a position cursor that repeats the ray's own additions, so the
// record is the same for every K: OPACITY's product and "the first one wins" both need the
// order, and what a batch loaded beyond the hit is dropped.
//   kHitEntry    the first in-slab sample (its value may be NaN)
//   kHitOpacity  T = T * (1 - tf(t).a) per in-slab sample with the composite's division and
//                lookup (the TF staged in LDS and read through the LdsF4-typed pointer, or the
//                global one when it does not fit: never a generic pointer, see tf_lookup); the
//                first sample with (1 - T) >= threshold
//   kHitMax      the first sample equal to the ray's maximum: d > m from -INFINITY, so a NaN and
//   kHitMin      a -inf sample never update; the mirror image from +INFINITY.  The whole ray.
//   kHitIso      iso_strip's search and four bisection fetches, then one fetch of the value at
//                the refined point (a cap: the sample's own cell again, the same bits)
// depth: once per pixel in f64, left to right, rounded to f32 once.  The record goes out as three
// 8-byte vector stores.
// COUNT (K = 1, so the hit ends the lane before its next step is counted): rays, steps and
// samples up to and including the ones that ended the walk; shaded = pixels with a hit; the
// bisection and value fetches are not counted; no record is written.
template <typename VT, int KIND, bool COUNT, int K>
__device__ __forceinline__ void hit_strip(const MarchParams &P, const HitArgs &A, LdsF4 *s_tf,
                                          bool tf_in_lds, uint32_t tile_x, uint32_t tile_y,
                                          uint32_t wave, uint32_t lane)
{
    static_assert(KIND >= kHitEntry && KIND <= kHitIso, "vr_hit_kind");
    static_assert(K == 1 || K == 2, "one or two samples in flight");
    static_assert(!COUNT || K == 1, "the counting kernels walk one step at a time");
    constexpr bool ENTRY = KIND == kHitEntry, OPAC = KIND == kHitOpacity, MAX = KIND == kHitMax,
                   MIN = KIND == kHitMin, ISO = KIND == kHitIso;
    constexpr bool EXTREME = MAX || MIN;  // no early end: the whole ray
    const LanePixel pix = strip_pixel(P, tile_x, tile_y, wave, lane);

    float tex[3] = {0.f, 0.f, 0.f}, dir[3] = {0.f, 0.f, 0.f};
    const bool covered = pix.active && pixel_ray(P, A.x0 + pix.px, A.y0 + pix.gy, tex, dir);

    bool hit = false, prev = false;
    float q0 = 0.f, q1 = 0.f, q2 = 0.f;  // ISO: the last in-slab position below the isovalue
    float h0 = 0.f, h1 = 0.f, h2 = 0.f;  // the hit
    float hv = 0.f;                      // its value
    int hk = -1;                         // and its step
    float m = MAX ? -INFINITY : INFINITY;
    float T = 1.0f;
    unsigned long long n_samples = 0, n_steps = 0;
    const char *__restrict__ vol = static_cast<const char *>(P.vol);
    const int nsteps = covered ? P.nsteps : 0;
    float p0 = tex[0], p1 = tex[1], p2 = tex[2];
    const float d0 = dir[0], d1 = dir[1], d2 = dir[2];
    const int kin = (covered && P.slab_default) ? interior_steps(tex, dir, P.step, nsteps) : 0;

    struct Stage {
        MipRaw<VT> r;
        float ax, ay, az;
        bool live, slab;
    };
    bool live = nsteps > 0;
    for (int it = 0; live; it += K) {
        Stage S[K];
        float c0 = p0, c1 = p1, c2 = p2;  // the position of the step being examined
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const int k = it + s;
            const bool interior = (unsigned)(k - 1) < (unsigned)kin;
            // volume.frag:34-37: the first position outside ends the ray
            live = live && k < nsteps &&
                   (interior || !(p0 > 1.0f || p1 > 1.0f || p2 > 1.0f || p0 < 0.0f || p1 < 0.0f ||
                                  p2 < 0.0f));
            if (COUNT && live) ++n_steps;
            // volume.frag:39-40 (strict)
            const bool slab = live && (interior || (p0 < P.smax[0] && p1 < P.smax[1] &&
                                                    p2 < P.smax[2] && p0 > P.smin[0] &&
                                                    p1 > P.smin[1] && p2 > P.smin[2]));
            if (COUNT && slab) ++n_samples;
            int i, j, kk;
            texel_coord(p0, P.fnx, i, S[s].ax);
            texel_coord(p1, P.fny, j, S[s].ay);
            texel_coord(p2, P.fnz, kk, S[s].az);
            S[s].live = live;
            S[s].slab = slab;
            // in the cube: i in [-1, n - 1], padded index in [1, n + 1] (vr_internal.h bricks_for)
            size_t ce = slab ? cell_offset<VT>(i + kPad, j + kPad, kk + kPad, P.nbx, P.nby) : (size_t)0;
            if (VR_OOB(2, ce * kElemBytes<VT>, P.vol_bytes)) ce = 0;
            S[s].r.issue(vol, ce);
            // volume.frag:47
            p0 = p0 + d0 * P.step;
            p1 = p1 + d1 * P.step;
            p2 = p2 + d2 * P.step;
        }
#pragma unroll
        for (int s = 0; s < K; ++s) {  // in step order: the first hit wins
            Cell8<VT> c;
            S[s].r.decode(c);
            const float d = c.tri(S[s].ax, S[s].ay, S[s].az);
            if ((EXTREME || !hit) && S[s].live) {
                if (S[s].slab) {
                    bool take;
                    if constexpr (ENTRY) {
                        take = true;
                    } else if constexpr (OPAC) {
                        // volume.frag:42 and :45 (the composite's division, lookup and product)
                        const float tt = div_by_range(d - P.vmin, P);
                        const float4 sm = tf_in_lds ? tf_lookup(s_tf, P.tf_n, P.tf_nf, tt)
                                                    : tf_lookup(P.tf, P.tf_n, P.tf_nf, tt);
                        T = T * (1.0f - sm.w);
                        take = (1.0f - T) >= A.threshold;
                    } else if constexpr (MAX) {
                        take = d > m;  // a NaN sample never updates
                    } else if constexpr (MIN) {
                        take = d < m;
                    } else {
                        take = d >= A.iso;  // a NaN sample never hits
                    }
                    if (take) {
                        hit = true;
                        m = d;
                        hv = d;
                        hk = it + s;
                        h0 = c0;
                        h1 = c1;
                        h2 = c2;
                    } else if (ISO) {
                        prev = true;
                        q0 = c0;
                        q1 = c1;
                        q2 = c2;
                    }
                } else if (ISO) {
                    prev = false;
                }
            }
            c0 = c0 + d0 * P.step;
            c1 = c1 + d1 * P.step;
            c2 = c2 + d2 * P.step;
        }
        if (!EXTREME) live = live && !hit;
    }

    if (COUNT) {
        flush_counters(P, lane, covered, n_samples, hit ? 1ull : 0ull, n_steps, 0);
        return;
    }
    if (!pix.active) return;

    if (ISO && hit) {
        if (prev) {  // bisection between q (below) and the hit (at or above): in-slab by convexity
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                const float m0 = (q0 + h0) * 0.5f, m1 = (q1 + h1) * 0.5f, m2 = (q2 + h2) * 0.5f;
                int i, j, kk;
                float ax, ay, az;
                texel_coord(m0, P.fnx, i, ax);
                texel_coord(m1, P.fny, j, ay);
                texel_coord(m2, P.fnz, kk, az);
                size_t ce = cell_offset<VT>(i + kPad, j + kPad, kk + kPad, P.nbx, P.nby);
                if (VR_OOB(2, ce * kElemBytes<VT>, P.vol_bytes)) ce = 0;
                Cell8<VT> c;
                c.load(vol, ce);
                const bool above = c.tri(ax, ay, az) >= A.iso;
                h0 = above ? m0 : h0;
                h1 = above ? m1 : h1;
                h2 = above ? m2 : h2;
                q0 = above ? q0 : m0;
                q1 = above ? q1 : m1;
                q2 = above ? q2 : m2;
            }
        }
        int i, j, kk;
        float ax, ay, az;
        texel_coord(h0, P.fnx, i, ax);
        texel_coord(h1, P.fny, j, ay);
        texel_coord(h2, P.fnz, kk, az);
        size_t ce = cell_offset<VT>(i + kPad, j + kPad, kk + kPad, P.nbx, P.nby);
        if (VR_OOB(2, ce * kElemBytes<VT>, P.vol_bytes)) ce = 0;
        Cell8<VT> c;
        c.load(vol, ce);
        hv = c.tri(ax, ay, az);
    }

    // the miss record: {0, 0, 0, +INFINITY, 0, 0xFFFFFFFF}
    float depth = INFINITY;
    if (hit) {
        const double dx = ((double)h0 - 0.5) - (double)P.cam[0];
        const double dy = ((double)h1 - 0.5) - (double)P.cam[1];
        const double dz = ((double)h2 - 0.5) - (double)P.cam[2];
        depth = (float)sqrt(dx * dx + dy * dy + dz * dz);
    } else {
        h0 = h1 = h2 = hv = 0.0f;
    }
    const size_t idx = (size_t)pix.ly * P.W + pix.px;
    if (VR_OOB(4, idx * kHitRecordBytes + (kHitRecordBytes - 1), A.out_bytes)) return;
    float2 *o = reinterpret_cast<float2 *>(static_cast<char *>(A.out) + idx * kHitRecordBytes);
    o[0] = make_float2(h0, h1);
    o[1] = make_float2(h2, depth);
    o[2] = make_float2(hv, __uint_as_float((uint32_t)hk));
}

template <typename VT, int KIND, bool COUNT, int K>
__global__ __launch_bounds__(kThreadsPerTile) void hit_kernel(const MarchParams P, const HitArgs A)
{
    const int tid = threadIdx.x;
    uint32_t tile_x, tile_y;
    if (!block_tile(P, tile_x, tile_y)) return;
    if constexpr (KIND == kHitOpacity) {
        __shared__ float4 s_tf[kTfLut];  // as march_kernel's
        const bool tf_in_lds = P.tf_n <= kTfLds;
        if (tf_in_lds) stage_tf(P, s_tf, (int)kThreadsPerTile);
        __syncthreads();
        hit_strip<VT, KIND, COUNT, K>(P, A, (LdsF4 *)s_tf, tf_in_lds, tile_x, tile_y,
                                      (uint32_t)tid >> 6, (uint32_t)tid & 63u);
    } else {
        hit_strip<VT, KIND, COUNT, K>(P, A, (LdsF4 *)nullptr, false, tile_x, tile_y,
                                      (uint32_t)tid >> 6, (uint32_t)tid & 63u);
    }
}

// ---- lane-pair march (small launches) ----------------------------------------------------------
// Two lanes per ray: lane 0 of the pair fetches, filters and shades the even samples, lane 1 the
// odd ones; both keep the ray position with the same float additions (p_(k+1) = p_k + d step,
// every step), exchange their sample through a lane shuffle, and composite the pair in sample
// order with identical operations, so C and T are the single-lane march's bit for bit (an
// off-slab sample composites alpha 0: +0, T unchanged).  Halves each ray's serial chain and
// doubles the wavefronts of a launch: for a rank's share of a multi-GPU frame.  A workgroup is
// a 16x8-pixel tile (wavefront: 16x2 pixels); the TF is LDS-resident (host: tf_n <= kTfLds).
template <typename VT, bool SHADE, bool GF, int L>
__global__ __launch_bounds__(kThreads) void march_pair_kernel(const MarchParams P)
{
    __shared__ float4 s_tf[kTfLut];
    const int tid = threadIdx.x;
    uint32_t tile_x, tile_y;
    if (!block_tile(P, tile_x, tile_y)) return;
    stage_tf(P, s_tf, kThreads);  // (no tf_in_lds test: the host grants these kernels no other TF)
    __syncthreads();
    const long long wg_start = wall_clock64();
#ifdef VR_WG_TIMES
    const unsigned long long wg_t0 = wg_start;
#endif
    using G = GeomOf<VT>;
    const long by_stride = (long)P.nbx * G::Elems;
    const long bz_stride = (long)P.nbx * P.nby * G::Elems;

    // L lanes per ray; wavefront = 16 x (4 / L) pixels; workgroup tile 16 x (16 / L).  The row
    // mapping is share_row's, spelled out: calling it here moves this kernel's machine code, which
    // keys the committed traffic figures (vr_amd.kernel_code_hash; CHANGELOG, "Share the pixel")
    const uint32_t wave = tid >> 6, lane = tid & 63, q = lane / L, half = lane % L;
    const uint32_t px = tile_x * kTile + (q & 15);
    const uint32_t ly = tile_y * (kTile / L) + wave * (4 / L) + (q >> 4);
    bool active = px < P.W && ly < P.local_rows;
    const uint32_t blk = ly / P.row_block;
    const uint32_t gy = share_global_block(blk, P.rank, P.nranks, RowShare{P.share_w0, P.share_w}) *
                            P.row_block + (ly - blk * P.row_block);
    active = active && gy < P.H;

    float tex[3] = {0.f, 0.f, 0.f}, dir[3] = {0.f, 0.f, 0.f};
    const bool covered = active && pixel_ray(P, px, gy, tex, dir);
    const char *__restrict__ vol = static_cast<const char *>(P.vol);
    const int nsteps = covered ? P.nsteps : 0;
    float p0 = tex[0], p1 = tex[1], p2 = tex[2];
    const float d0 = dir[0], d1 = dir[1], d2 = dir[2];
    const int kin = (covered && P.slab_default) ? interior_steps(tex, dir, P.step, nsteps) : 0;
    auto advance = [&]() {
        p0 = p0 + d0 * P.step;
        p1 = p1 + d1 * P.step;
        p2 = p2 + d2 * P.step;
    };
    float T = 1.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
    // Each lane also runs its own samples software-pipelined (its next sample's loads in
    // flight while the current one is filtered): unconditional loads (a first-brick cell
    // off-slab, alpha 0 there), ping-pong stages, as march_kernel's PIPE path.
    struct Stage {
        Cell8<VT> c;
        size_t ce;
        float ax, ay, az;
        int pi, pj, pk;
        bool ok, slab;
    };
    auto prep = [&](Stage &S, int k) {
        const bool interior = (unsigned)(k - 1) < (unsigned)kin;
        S.ok = k < nsteps && (interior || !(p0 > 1.0f || p1 > 1.0f || p2 > 1.0f || p0 < 0.0f ||
                                            p1 < 0.0f || p2 < 0.0f));
        S.slab = S.ok && (interior || (p0 < P.smax[0] && p1 < P.smax[1] && p2 < P.smax[2] &&
                                       p0 > P.smin[0] && p1 > P.smin[1] && p2 > P.smin[2]));
        int i, j, kk;
        texel_coord(p0, P.fnx, i, S.ax);
        texel_coord(p1, P.fny, j, S.ay);
        texel_coord(p2, P.fnz, kk, S.az);
        if (!S.slab) i = j = kk = 0;
        S.pi = i + kPad;
        S.pj = j + kPad;
        S.pk = kk + kPad;
        S.ce = cell_offset<VT>(S.pi, S.pj, S.pk, P.nbx, P.nby);
        S.c.load(vol, S.ce);
    };
    // this lane's sample -> exchange -> the pair's two samples composited in order; true: the
    // ray ends (bounds, nsteps, T == 0 or ERT), identically in both lanes
    auto consume = [&](const Stage &S) -> bool {
        float4 sm = tf_lookup((LdsF4 *)s_tf, P.tf_n, P.tf_nf,
                              div_by_range(S.c.tri(S.ax, S.ay, S.az) - P.vmin, P));
        if (!S.slab) sm.w = 0.0f;
        if (SHADE && sm.w > 0.0f)
            shade_sample<VT, GF, true>(P, vol, S.ce, S.c, S.pi, S.pj, S.pk, by_stride, bz_stride,
                                       S.ax, S.ay, S.az, d0, d1, d2, sm);
        // the group's L samples, in sample order (lane j of the group holds sample k0 + j)
        const int base = (int)(lane - half);
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const float sx = __shfl(sm.x, base + j, 64), sy = __shfl(sm.y, base + j, 64);
            const float sz = __shfl(sm.z, base + j, 64), sw = __shfl(sm.w, base + j, 64);
            const int sok = __shfl((int)S.ok, base + j, 64);
            if (!sok) return true;
            cr = cr + (sx * sw) * T;  // volume.frag:44-45
            cg = cg + (sy * sw) * T;
            cb = cb + (sz * sw) * T;
            T = T * (1.0f - sw);
            if (T == 0.0f || T < P.ert_eps) return true;
        }
        return false;
    };
    for (uint32_t j = 0; j < half; ++j) advance();  // lane j of the group starts at sample j
    Stage S0, S1;
    int k = (int)half;
    prep(S0, k);
    for (;;) {  // the lanes of a group leave together (same ok flags and T)
#pragma unroll
        for (int j = 0; j < L; ++j) advance();
        k += L;
        prep(S1, k);
        if (consume(S0)) break;
#pragma unroll
        for (int j = 0; j < L; ++j) advance();
        k += L;
        prep(S0, k);
        if (consume(S1)) break;
    }
    write_tile_cost(P, tile_x, tile_y, wg_start);
#ifdef VR_WG_TIMES
    __syncthreads();
    if (tid == 0) wg_times_record((unsigned long long)wg_t0, tile_y * P.tiles_x + tile_x);
#endif
    if (!active || half) return;
    store_pixel(P, px, ly, blend_over_clear(P, cr, cg, cb, T));
}

// ---- adaptive tile order --------------------------------------------------------------------

// One workgroup per XCD x over its tile list (the tiles of the super-tiles s = x (mod 8), as
// tile_order 3 assigns them; built on the host once per geometry: lists[x * per_xcd + j],
// ~0 = none): counting-sorted by their last duration into 64 log-scale buckets, longest
// first, written to perm[x + 8 j] (j = rank), the XCD's remaining slots ~0.  Workgroups are
// dispatched in index order round-robin over the XCDs, so each XCD starts its longest tiles
// first and the frame no longer ends on a few long rays.
// Each XCD's tiles, longest first by the last launch's durations: a stable counting sort
// over one bucket per octave of duration (bucket 31 = longest).  Thread t owns list entries
// [t chunk, (t + 1) chunk); counts per (bucket, thread), offsets bucket-major (longest
// first) and thread-minor, so the tiles of one bucket keep their list order (the XCD's
// super-tiles in raster order) and tiles running together on an XCD stay neighbours.
// Against 4 buckets per octave in arbitrary order: C3 +1.8%, shaded views 1-4% faster
// (profiles/r01/tile_order/stable_octave_ab.txt).
#ifndef VR_ORDER_OCTAVES
#define VR_ORDER_OCTAVES 1
#endif
__global__ __launch_bounds__(256) void order_tiles_kernel(const uint32_t *__restrict__ cost,
                                                          const uint32_t *__restrict__ lists,
                                                          uint32_t *__restrict__ perm,
                                                          uint32_t per_xcd)
{
    constexpr int NB = 32;
    __shared__ uint32_t cnt[NB][257];  // [b][t]: offset within bucket b; [b][256]: bucket base
    __shared__ uint32_t n_tiles;
    const uint32_t x = blockIdx.x, tid = threadIdx.x;
    const uint32_t *list = lists + (size_t)x * per_xcd;
    // experiment builds: VR_ORDER_OCTAVES octaves per bucket
    auto bucket = [](uint32_t c) -> uint32_t { return c < 2 ? 0u : (31u - __clz(c)) / VR_ORDER_OCTAVES; };
    const uint32_t chunk = (per_xcd + 255) / 256;
    const uint32_t j0 = min(per_xcd, tid * chunk), j1 = min(per_xcd, j0 + chunk);
    for (int b = 0; b < NB; ++b) cnt[b][tid] = 0;
    __syncthreads();
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t t = list[j];
        if (t != 0xFFFFFFFFu) ++cnt[bucket(cost[t])][tid];
    }
    __syncthreads();
    if (tid < NB) {  // exclusive prefix over the threads of bucket tid; its total in [256]
        uint32_t acc = 0;
        for (int k = 0; k < 256; ++k) {
            const uint32_t v = cnt[tid][k];
            cnt[tid][k] = acc;
            acc += v;
        }
        cnt[tid][256] = acc;
    }
    __syncthreads();
    if (tid == 0) {  // bucket bases, longest first
        uint32_t acc = 0;
        for (int b = NB - 1; b >= 0; --b) {
            const uint32_t v = cnt[b][256];
            cnt[b][256] = acc;
            acc += v;
        }
        n_tiles = acc;
    }
    __syncthreads();
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t t = list[j];
        if (t != 0xFFFFFFFFu) {
            const uint32_t b = bucket(cost[t]);
            perm[x + 8 * (cnt[b][256] + cnt[b][tid]++)] = t;
        }
    }
    for (uint32_t j = n_tiles + tid; j < per_xcd; j += blockDim.x) perm[x + 8 * j] = 0xFFFFFFFFu;
}

// ---- volume ingest: linear (any NRRD element type) -> bricked paired elements -------------

// One thread per stored element: padded element coordinates -> the voxels it holds (2 z-pair,
// 4 yz-quad), 0 outside the logical volume (border).
template <typename SrcT, typename DstT>
__global__ __launch_bounds__(256) void brick_kernel(const SrcT *__restrict__ src,
                                                    Vox<DstT> *__restrict__ dst, uint32_t nx,
                                                    uint32_t ny, uint32_t nz, uint32_t nbx,
                                                    uint32_t nby, size_t nbricks)
{
    constexpr bool zpair = kZPair<DstT>;
    using G = GeomOf<DstT>;
    using V = Vox<DstT>;
    // a workgroup per brick (grid-stride over bricks), its threads over the brick's elements:
    // brick coordinates once per brick, element coordinates by constant divisors, and each
    // brick's elements written contiguously
    for (size_t bidx = blockIdx.x; bidx < nbricks; bidx += gridDim.x)
    for (uint32_t l = threadIdx.x; l < (uint32_t)G::Elems; l += blockDim.x) {
        const size_t g = bidx * G::Elems + l;
        const uint32_t lx = l % G::EX, lyz = l / G::EX, lyy = lyz % G::EY, lz = lyz / G::EY;
        uint32_t bx, by, bz;
        brick_coords((uint32_t)bidx, nbx, nby, bx, by, bz);
        const long x = (long)bx * G::BX + lx - G::Lo - kPad;
        const long y = (long)by * G::BY + lyy - G::Lo - kPad;
        const long z = (long)bz * G::BZ + lz - G::Lo - kPad;
        auto at = [&](long xx, long yy, long zz) -> V {
            if (xx < 0 || yy < 0 || zz < 0 || xx >= (long)nx || yy >= (long)ny || zz >= (long)nz)
                return (V)0;
            return (V)src[(size_t)xx + (size_t)nx * ((size_t)yy + (size_t)ny * (size_t)zz)];
        };
        // one store per element (a u8 quad is one dword, not four byte stores)
        if constexpr (kPlainF32<DstT> || kPlainByte<DstT>) {
            dst[g] = at(x, y, z);
        } else if constexpr (zpair) {
            reinterpret_cast<float2 *>(dst)[g] = make_float2(at(x, y, z), at(x, y, z + 1));
        } else {
            struct alignas(4 * sizeof(V)) Quad {
                V v[4];
            };
            Quad q;
            q.v[0] = at(x, y, z);
            q.v[1] = at(x, y, z + 1);
            q.v[2] = at(x, y + 1, z);
            q.v[3] = at(x, y + 1, z + 1);
            reinterpret_cast<Quad *>(dst)[g] = q;
        }
    }
}

// ---- synthetic volumes (multi-GiB configs): generated linear, then bricked --------------------

__device__ __forceinline__ float hash01(uint32_t x, uint32_t y, uint32_t z)
{
    uint32_t h = (x * 73856093u) ^ (y * 19349663u) ^ (z * 83492791u);
    h ^= h >> 13;
    h *= 0x5bd1e995u;
    h ^= h >> 15;
    return (float)(h & 0xFFFFFFu) * (1.0f / 16777216.0f);
}

template <typename DstT>
__device__ __forceinline__ DstT to_storage(float v)
{
    if constexpr (sizeof(DstT) == 4) {
        return v;
    } else {
        constexpr float lo = (DstT)(-1) < (DstT)0 ? (sizeof(DstT) == 1 ? -128.f : -32768.f) : 0.f;
        constexpr float hi = (DstT)(-1) < (DstT)0 ? (sizeof(DstT) == 1 ? 127.f : 32767.f)
                                                  : (sizeof(DstT) == 1 ? 255.f : 65535.f);
        return (DstT)fminf(fmaxf(rintf(v), lo), hi);
    }
}

// params: [ng, noise_amp, out_scale, ng * (cx, cy, cz, k, amp)] in voxel units;
// value = out_scale * (sum_g amp exp(-k |x - c|^2) + noise_amp * hash01(x,y,z)).
template <typename DstT>
__global__ __launch_bounds__(256) void generate_kernel(DstT *__restrict__ dst, uint32_t nx,
                                                       uint32_t ny, size_t total,
                                                       const float *__restrict__ prm)
{
    const int ng = (int)prm[0];
    const float noise = prm[1], scale = prm[2];
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
         g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t x = (uint32_t)(g % nx);
        const size_t yz = g / nx;
        const uint32_t y = (uint32_t)(yz % ny), z = (uint32_t)(yz / ny);
        const float fx = (float)x, fy = (float)y, fz = (float)z;
        float acc = 0.0f;
        for (int q = 0; q < ng; ++q) {
            const float *c = prm + 3 + 5 * q;
            const float dx = fx - c[0], dy = fy - c[1], dz = fz - c[2];
            acc += c[4] * __expf(-c[3] * (dx * dx + dy * dy + dz * dz));
        }
        acc += noise * hash01(x, y, z);
        dst[g] = to_storage<DstT>(acc * scale);
    }
}

// ---- min/max over a linear buffer -------------------------------------------------------------

__device__ __forceinline__ uint32_t ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <typename VT>
__global__ __launch_bounds__(256) void minmax_kernel(const VT *__restrict__ vol, size_t total,
                                                     uint32_t *out)
{
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
         g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t o = ordered((float)vol[g]);
        lo = o < lo ? o : lo;
        hi = o > hi ? o : hi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    // one atomic pair per workgroup: the waves' results meet in LDS first (a pair per wave on
    // one address serialised the kernel: 1.55 ms for 512^3 f32)
    __shared__ uint32_t s_lo[4], s_hi[4];
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_lo[w] = lo;
        s_hi[w] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t i = 1; i < (blockDim.x >> 6); ++i) {
            lo = s_lo[i] < lo ? s_lo[i] : lo;
            hi = s_hi[i] > hi ? s_hi[i] : hi;
        }
        atomicMin(&out[0], lo);
        atomicMax(&out[1], hi);
    }
}

// ---- narrowest exact storage of 32/64-bit input ---------------------------------------------
// The reference converts every NRRD element type to float (nrrd_file_parser.cpp:49-77), so an
// 8-bit CT volume reaches volume_dataset_changed as floats.  out[0] / out[1]: the minimum and
// maximum voxel (as int) when every voxel is an integer in [kIntRangeLo, kIntRangeHi]; out[2]
// != 0 otherwise (a fraction, NaN, infinity, -0.0, or a value outside that range).  A float
// voxel counts as an integer only if v == rint(v) and it is not -0.0, so storing it in an
// 8/16-bit type and converting back (float(int) is exact) gives the same bits.
constexpr int kIntRangeLo = -32768, kIntRangeHi = 65535;
template <typename SrcT>
__global__ __launch_bounds__(256) void int_range_kernel(const SrcT *__restrict__ src, size_t total,
                                                        int *out)
{
    int lo = kIntRangeHi, hi = kIntRangeLo, bad = 0;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
         g += (size_t)gridDim.x * blockDim.x) {
        const SrcT v = src[g];
        int iv;
        if constexpr (std::is_floating_point<SrcT>::value) {
            const float f = (float)v;
            const bool ok = f >= (float)kIntRangeLo && f <= (float)kIntRangeHi && f == rintf(f) &&
                            !(f == 0.0f && signbit(f));
            bad |= ok ? 0 : 1;
            iv = ok ? (int)f : 0;
        } else {
            const bool ok = (long long)v >= kIntRangeLo && (long long)v <= kIntRangeHi &&
                            !(std::is_unsigned<SrcT>::value && (unsigned long long)v > (unsigned long long)kIntRangeHi);
            bad |= ok ? 0 : 1;
            iv = ok ? (int)v : 0;
        }
        lo = iv < lo ? iv : lo;
        hi = iv > hi ? iv : hi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64), b2 = __shfl_xor(bad, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
        bad |= b2;
    }
    __shared__ int s_lo[4], s_hi[4], s_bad[4];  // one atomic set per workgroup (minmax_kernel)
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_lo[w] = lo;
        s_hi[w] = hi;
        s_bad[w] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t i = 1; i < (blockDim.x >> 6); ++i) {
            lo = s_lo[i] < lo ? s_lo[i] : lo;
            hi = s_hi[i] > hi ? s_hi[i] : hi;
            bad |= s_bad[i];
        }
        atomicMin(&out[0], lo);
        atomicMax(&out[1], hi);
        if (bad) atomicOr(&out[2], 1);
    }
}

// ---- f32 gradient field (shading) ------------------------------------------------------------

// Voxel at padded coordinates (p = logical + kPad) from the bricked z-pair density: component
// 0 of the element at p (cell_offset); 0 outside the logical volume.
__device__ __forceinline__ float padded_voxel(const float *__restrict__ bricks, int px, int py,
                                              int pz, uint32_t nx, uint32_t ny, uint32_t nz,
                                              uint32_t nbx, uint32_t nby)
{
    if (px < kPad || py < kPad || pz < kPad || px >= (int)nx + kPad || py >= (int)ny + kPad ||
        pz >= (int)nz + kPad)
        return 0.0f;
    return bricks[kF32VoxelsPerElement * cell_offset<float>(px, py, pz, nbx, nby)];
}

// The f32 alternative-geometry copies straight from the 8^3 z-pair bricks (round 6; before: an
// unbrick to a linear f32 temporary, then brick_kernel from it): one thread per stored element
// of the copy, its voxels read as padded_voxel (0 outside the volume) -- the same values
// brick_kernel stores, so the same bytes, without the volume-sized temporary and one pass less.
template <typename DstT>
__global__ __launch_bounds__(256) void rebrick_f32_kernel(const float *__restrict__ src,
                                                          float *__restrict__ dst, uint32_t nx,
                                                          uint32_t ny, uint32_t nz, uint32_t snbx,
                                                          uint32_t snby, uint32_t snbz, uint32_t nbx,
                                                          uint32_t nby, size_t nbricks)
{
    using G = GeomOf<DstT>;
    for (size_t bidx = blockIdx.x; bidx < nbricks; bidx += gridDim.x) {
        uint32_t bx, by, bz;
        brick_coords((uint32_t)bidx, nbx, nby, bx, by, bz);
        for (uint32_t l = threadIdx.x; l < (uint32_t)G::Elems; l += blockDim.x) {
            const size_t g = bidx * G::Elems + l;
            const uint32_t lx = l % G::EX, lyz = l / G::EX, lyy = lyz % G::EY, lz = lyz / G::EY;
            // padded coordinates of the element (brick_kernel's logical ones + kPad)
            const int x = (int)(bx * G::BX + lx) - G::Lo, y = (int)(by * G::BY + lyy) - G::Lo,
                      z = (int)(bz * G::BZ + lz) - G::Lo;
            if constexpr (kPlainF32<DstT>) {
                dst[g] = padded_voxel(src, x, y, z, nx, ny, nz, snbx, snby);
            } else if (kF32VoxelsPerElement == 2 && x >= 0 && y >= 0 && z >= 0 &&
                       x < (int)(snbx * GeomWide::BX) && y < (int)(snby * GeomWide::BY) &&
                       z < (int)(snbz * GeomWide::BZ)) {
                // a source z-pair element holds {v(z), v(z + 1)} with the border stored as 0
                reinterpret_cast<float2 *>(dst)[g] =
                    reinterpret_cast<const float2 *>(src)[cell_offset<float>(x, y, z, snbx, snby)];
            } else {
                reinterpret_cast<float2 *>(dst)[g] =
                    make_float2(padded_voxel(src, x, y, z, nx, ny, nz, snbx, snby),
                                padded_voxel(src, x, y, z + 1, nx, ny, nz, snbx, snby));
            }
        }
    }
}

// The y-major copy (vr_internal.h F32Y) from the 8^3 z-pair bricks: the same brick grid, one
// thread per stored element, {v(x, y, z), v(x, y + 1, z)} read as padded_voxel -- the y + 1 voxel
// of a brick's top layer from the neighbour brick, 0 outside the volume.
__global__ __launch_bounds__(256) void rebrick_ymajor_kernel(const float *__restrict__ src,
                                                             float2 *__restrict__ dst, uint32_t nx,
                                                             uint32_t ny, uint32_t nz, uint32_t nbx,
                                                             uint32_t nby, size_t nbricks)
{
    using G = GeomWide;
    const uint32_t nbz = (uint32_t)(nbricks / ((size_t)nbx * nby));
    for (size_t bidx = blockIdx.x; bidx < nbricks; bidx += gridDim.x) {  // bidx: the ymajor_slot
        uint32_t bx, by, bz;
        ymajor_coords((uint32_t)bidx, nbx, nbz, bx, by, bz);
        for (uint32_t l = threadIdx.x; l < (uint32_t)G::Elems; l += blockDim.x) {
            const uint32_t lx = l % G::EX, lzy = l / G::EX, lz = lzy % G::EZ, ly = lzy / G::EZ;
            float2 v = make_float2(0.0f, 0.0f);  // (and the brick's alignment padding)
            if (ly < (uint32_t)G::EY) {
                const int x = (int)(bx * G::BX + lx), y = (int)(by * G::BY + ly),
                          z = (int)(bz * G::BZ + lz);
                v = make_float2(padded_voxel(src, x, y, z, nx, ny, nz, nbx, nby),
                                padded_voxel(src, x, y + 1, z, nx, ny, nz, nbx, nby));
            }
            dst[bidx * G::Elems + l] = v;
        }
    }
}

// binary16 of d * 2^k (scale = 2^k): clamped to +-65504 first (NaN passes), rounded to nearest
// even (v_cvt_f16_f32; f16 denormals kept).  The oracle's round_f16 restates it.
__device__ __forceinline__ _Float16 field_half(float d, float scale)
{
    float x = d * scale;
    x = x > 65504.0f ? 65504.0f : (x < -65504.0f ? -65504.0f : x);
    return (_Float16)x;
}

// One thread per stored element: D_e(p) = v(p + e) - v(p - e) (the oracle's dvox).  f32 (H =
// false): the element's two voxels p = (x, y, z) and (x, y, z + 1), written as {Dx, Dx', Dy,
// Dy', Dz, Dz'}.  binary16 (H = true): the four voxels (x, y + dy, z + dz), per axis
// {D(y,z), D(y,z+1), D(y+1,z), D(y+1,z+1)}, each field_half(D, scale).
// A workgroup per brick (grid-stride over bricks): the brick's voxel neighbourhood -- padded
// coordinates [B b - 1, B b + E] in x, [B b - 1, B b + E + H] in y, [B b - 1, B b + E + 1] in z
// (E = elements per axis) -- is staged in LDS once, with one gather per voxel, and every
// element's differences read from there (the same subtractions, so the same bits): one global
// load per staged voxel instead of 12 (f32) or 24 (binary16) per element.  Each brick's
// elements are written contiguously.
// ymajor (binary16 only): the y-major field -- the same 24-B elements in the y-major copy's
// order (vr_internal.h: bricks in ymajor_slot order, a brick's elements at ymajor_local), read
// from the same z-pair bricks; only the place of an element in the staged brick and the brick's
// place in memory differ.
template <bool H>
__global__ __launch_bounds__(256) void grad_field_kernel(const float *__restrict__ bricks,
                                                         float *__restrict__ grad, uint32_t nx,
                                                         uint32_t ny, uint32_t nz, uint32_t nbx,
                                                         uint32_t nby, size_t nbricks, float scale,
                                                         uint32_t ymajor)
{
    using G = GeomWide;
    constexpr int LX = G::EX + 2, LY = G::EY + 2 + (H ? 1 : 0), LZ = G::EZ + 3;
    __shared__ float box[LX * LY * LZ];
    // the brick's 24-B elements, assembled here and stored as consecutive 8-B words per lane
    __shared__ uint2 ostage[3 * G::Elems];
    uint2 *__restrict__ out = reinterpret_cast<uint2 *>(grad);
    const uint32_t nbz = (uint32_t)(nbricks / ((size_t)nbx * nby));
    for (size_t bidx = blockIdx.x; bidx < nbricks; bidx += gridDim.x) {
        uint32_t bx, by, bz;
        if (H && ymajor)
            ymajor_coords((uint32_t)bidx, nbx, nbz, bx, by, bz);
        else
            brick_coords((uint32_t)bidx, nbx, nby, bx, by, bz);
        const int x0 = (int)(bx * G::BX) - 1, y0 = (int)(by * G::BY) - 1, z0 = (int)(bz * G::BZ) - 1;
        __syncthreads();  // the previous brick's elements have read the box and left ostage
        // two z-slices per load: the z-pair element at (x, y, z) holds {v(z), v(z + 1)}, the
        // border stored as 0 (padded_voxel where the element is outside the stored grid)
        static_assert(LZ % 2 == 0, "the box is loaded in z-pairs");
        for (int i = (int)threadIdx.x; i < LX * LY * (LZ / 2); i += (int)blockDim.x) {
            const int ix = i % LX, iyz = i / LX, iy = iyz % LY, iz = 2 * (iyz / LY);
            const int px = x0 + ix, py = y0 + iy, pz = z0 + iz;
            float2 v;
            if (kF32VoxelsPerElement == 2 && px >= 0 && py >= 0 && pz >= 0 &&
                px < (int)(nbx * G::BX) && py < (int)(nby * G::BY) && pz < (int)(nbz * G::BZ))
                v = reinterpret_cast<const float2 *>(bricks)[cell_offset<float>(px, py, pz, nbx, nby)];
            else
                v = make_float2(padded_voxel(bricks, px, py, pz, nx, ny, nz, nbx, nby),
                                padded_voxel(bricks, px, py, pz + 1, nx, ny, nz, nbx, nby));
            box[(iz * LY + iy) * LX + ix] = v.x;
            box[((iz + 1) * LY + iy) * LX + ix] = v.y;
        }
        __syncthreads();
        for (uint32_t l = threadIdx.x; l < (uint32_t)G::Elems; l += blockDim.x) {
            const uint32_t lx = l % G::EX, lyz = l / G::EX, lyy = lyz % G::EY, lz = lyz / G::EY;
            uint2 *o = ostage + 3 * l;
            if (lz >= (uint32_t)G::EZ) {  // alignment padding of the brick: never read
                o[0] = o[1] = o[2] = make_uint2(0u, 0u);
                continue;
            }
            if (H && ymajor) o = ostage + 3 * ymajor_local(lx, lyy, lz);
            // box index of padded voxel (x0 + 1 + lx + dx, y0 + 1 + lyy + dy, z0 + 1 + lz + dz)
            const int c = ((int)lz + 1) * (LX * LY) + ((int)lyy + 1) * LX + ((int)lx + 1);
            if constexpr (H) {
                _Float16 hv[12];
#pragma unroll
                for (int q = 0; q < 4; ++q) {  // q = dz + 2 dy
                    const int cq = c + (q >> 1) * LX + (q & 1) * (LX * LY);
                    auto V = [&](int dx, int dy, int dz) { return box[cq + dx + dy * LX + dz * (LX * LY)]; };
                    hv[0 + q] = field_half(V(1, 0, 0) - V(-1, 0, 0), scale);
                    hv[4 + q] = field_half(V(0, 1, 0) - V(0, -1, 0), scale);
                    hv[8 + q] = field_half(V(0, 0, 1) - V(0, 0, -1), scale);
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const h2v lo = {hv[4 * i], hv[4 * i + 1]}, hi = {hv[4 * i + 2], hv[4 * i + 3]};
                    o[i] = make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
                }
            } else {
                float d[6];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int ch = c + h * (LX * LY);
                    auto V = [&](int dx, int dy, int dz) { return box[ch + dx + dy * LX + dz * (LX * LY)]; };
                    d[0 + h] = V(1, 0, 0) - V(-1, 0, 0);
                    d[2 + h] = V(0, 1, 0) - V(0, -1, 0);
                    d[4 + h] = V(0, 0, 1) - V(0, 0, -1);
                }
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    o[i] = make_uint2(__float_as_uint(d[2 * i]), __float_as_uint(d[2 * i + 1]));
            }
        }
        __syncthreads();
        uint2 *__restrict__ ob = out + bidx * (3 * (size_t)G::Elems);
        for (uint32_t j = threadIdx.x; j < 3u * (uint32_t)G::Elems; j += blockDim.x) ob[j] = ostage[j];
    }
}

// ---- empty-space classification (skip_empty) --------------------------------------------------

// One wavefront per brick: min/max over every voxel its stored elements hold (apron and zero
// border included: exactly the values a sample whose cell lies in the brick can read).  A
// brick holding a NaN gets (NaN, NaN), which the classifier never calls empty.
template <typename VT>
__global__ __launch_bounds__(256) void brick_range_kernel(const VT *__restrict__ bricks,
                                                          uint32_t nbricks, uint32_t per_brick,
                                                          uint32_t nbx, uint32_t nby,
                                                          float2 *__restrict__ range)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= nbricks) return;  // wave-uniform
    const VT *src = bricks + (size_t)b * per_brick;
    float lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    for (uint32_t e = lane; e < per_brick; e += 64) {
        const float v = (float)src[e];
        nan = nan || v != v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    const bool any_nan = __ballot(nan) != 0;
    // range is indexed by the brick grid (x-fastest), whatever the memory order
    uint32_t bx, by, bz;
    brick_coords(b, nbx, nby, bx, by, bz);
    if (lane == 0) range[(bz * nby + by) * nbx + bx] = any_nan ? make_float2(NAN, NAN) : make_float2(lo, hi);
}

// One workgroup: range[nbricks] = {smallest lo, largest hi} over the bricks without a NaN (the
// MIP kernel ends a ray of an 8/16-bit volume at that maximum).
__global__ __launch_bounds__(256) void range_max_kernel(float2 *__restrict__ range, uint32_t nbricks)
{
    __shared__ float s_lo[4], s_hi[4];
    float lo = INFINITY, hi = -INFINITY;
    for (uint32_t b = threadIdx.x; b < nbricks; b += 256) {
        const float2 r = range[b];
        lo = fminf(lo, r.x);  // fminf / fmaxf drop a NaN operand
        hi = fmaxf(hi, r.y);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        range[nbricks] = make_float2(fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3])),
                                     fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3])));
}

// ---- value histogram (include/vr/vr_hist.h) ---------------------------------------------------

// One pass over the base bricks the box touches, a brick per workgroup iteration (grid-stride over
// the box's bricks; the others are never read).  Every voxel counts once, through its own element:
// the cells of the brick (no apron, so no neighbour's copy), component 0 of the element (what
// unbrick_kernel reads: never the z+1 / yz-quad neighbours), and only where the logical index lies
// in the box (never the two padding layers nor cells beyond nx, ny, nz).
// The bin of v is the largest b with e[b] <= v (vr_hist_host.h hist_bin, restated): a first guess
// in double (the f32 product misplaces a tenth of the edge values, and hi - lo may overflow f32),
// corrected against the edge table in LDS.  Counters are private to the workgroup, 32-bit in LDS
// (a workgroup counts nwork / gridDim bricks of at most 512 voxels: with launch_hist's grid that
// stays below 2^32 for every volume the device can hold), flushed with one 64-bit atomic per
// non-zero bin.  below / above / nan and the extremes (the integer ordered() form: nothing depends
// on the float min/max NaN and denormal modes) reduce per wave, then per workgroup, before their
// atomics, as minmax_kernel's do.  The minimum is kept inverted (~ordered, reduced with max), so
// an all-zero output block is the identity of every reduction.
// AGG: lanes whose bin equals the wave's first active lane's add once, by its popcount (the hot
// bin of a CT-like volume, where all 64 lanes would meet in one LDS word); the others add singly.
// Plain 8-bit bricks with 8-B rows (the 7 x 8 x 8 geometry of C4 / C5) take the code path: a bin
// is a function of the code, so the workgroup histograms the 256 raw codes -- a wave per brick, a
// lane per brick row, one 8-B load for the row's 7 cells, no binning per voxel -- and folds the
// codes into bins, below / above and the extremes once, at its end, by the same rule.
template <typename VT>
constexpr bool kHistCodes = kPlainByte<VT> && GeomOf<VT>::EX == 8 && GeomOf<VT>::BY * GeomOf<VT>::BZ == 64;

template <typename VT, bool AGG>
__global__ __launch_bounds__(256) void hist_kernel(const HistArgs A)
{
    using G = GeomOf<VT>;
    using V = Vox<VT>;
    constexpr uint32_t vpe = std::is_same<VT, float>::value ? (uint32_t)kF32VoxelsPerElement
                                                            : (kPlainByte<VT> ? 1u : 4u);
    constexpr uint32_t kCells = (uint32_t)(G::BX * G::BY * G::BZ);
    __shared__ uint32_t s_bins[kHistMaxBins];  // (the code path: its first 256 words, per code)
    __shared__ float s_edges[kHistMaxBins];
    __shared__ uint32_t s_red[4][5];
    const uint32_t tid = threadIdx.x, nbins = A.nbins;
    for (uint32_t i = tid; i < (kHistCodes<VT> && nbins < 256u ? 256u : nbins); i += 256) {
        s_bins[i] = 0;
        if (i < nbins) s_edges[i] = A.edges[i];
    }
    __syncthreads();
    const V *__restrict__ vol = static_cast<const V *>(A.vol);
    unsigned long long *__restrict__ out = A.out;
    const float lo = A.lo, hi = A.hi;
    const double dlo = (double)lo, scale = A.scale;
    uint32_t below = 0, above = 0, nan = 0, inv_mn = 0, mx = 0;
    // the bin of v, lo <= v <= hi: the guess, then the edges.  Both neighbours are read at once, so
    // the common case (the guess, or one off) costs one LDS round trip
    auto bin_of = [&](float v) __attribute__((always_inline)) {
        const double g = ((double)v - dlo) * scale;
        uint32_t b = g >= (double)(nbins - 1) ? nbins - 1 : (g > 0.0 ? (uint32_t)g : 0u);
        const bool last = b + 1 >= nbins;
        const float e0 = s_edges[b], e1 = s_edges[last ? b : b + 1];
        if (!last && e1 <= v) {
            ++b;
            while (b + 1 < nbins && s_edges[b + 1] <= v) ++b;
        } else if (e0 > v) {  // (b > 0: e[0] == lo <= v)
            --b;
            while (b > 0 && s_edges[b] > v) --b;
        }
        return b;
    };
    // one count for word b of s_bins from every lane with `counts`
    auto add = [&](bool counts, uint32_t b) __attribute__((always_inline)) {
        if constexpr (AGG) {
            const unsigned long long active = __ballot(counts);
            if (active) {  // wave-uniform
                const int leader = __ffsll((long long)active) - 1;
                const uint32_t lb = (uint32_t)__shfl((int)b, leader, 64);
                const unsigned long long same = __ballot(counts && b == lb);
                if ((int)(tid & 63u) == leader)
                    atomicAdd(&s_bins[lb], (uint32_t)__popcll(same));
                else if (counts && b != lb)
                    atomicAdd(&s_bins[b], 1u);
            }
        } else {
            if (counts) atomicAdd(&s_bins[b], 1u);
        }
    };
    // v (not a NaN), n times: the extremes, and below / above / its bin (false: it has a bin)
    auto classify = [&](float v, uint32_t n) __attribute__((always_inline)) {
        const uint32_t o = ordered(v == 0.0f ? 0.0f : v);  // -0.0 orders as 0
        inv_mn = ~o > inv_mn ? ~o : inv_mn;
        mx = o > mx ? o : mx;
        const bool lt = v < lo, gt = v > hi;
        below += lt ? n : 0u;  // (unconditional adds: a choice between the two counters' addresses
        above += gt ? n : 0u;  //  would keep them in scratch)
        return lt || gt;
    };
    if constexpr (kHistCodes<VT>) {
        const uint32_t wave = tid >> 6, lane = tid & 63u;
        const uint32_t yl = lane % (uint32_t)G::BY, zl = lane / (uint32_t)G::BY;
        for (uint32_t w0 = blockIdx.x * 4u; w0 < A.nwork; w0 += gridDim.x * 4u) {
            const uint32_t w = w0 + wave;
            if (w >= A.nwork) continue;  // wave-uniform
            const uint32_t bx = A.b0[0] + w % A.nb[0], by = A.b0[1] + (w / A.nb[0]) % A.nb[1],
                           bz = A.b0[2] + w / (A.nb[0] * A.nb[1]);
            const uint32_t y = by * (uint32_t)G::BY + yl - (uint32_t)kPad,
                           z = bz * (uint32_t)G::BZ + zl - (uint32_t)kPad;
            const bool row_in = y >= A.box_min[1] && y < A.box_max[1] && z >= A.box_min[2] && z < A.box_max[2];
            const V *__restrict__ row = vol + (size_t)brick_slot(bx, by, bz, A.nbx, A.nby) * (size_t)G::Elems +
                                        (zl * (uint32_t)G::EY + yl) * (uint32_t)G::EX;
            // (bricks are 648 B and rows 8 B: the row is 8-aligned)
            const uint2 d = row_in ? *reinterpret_cast<const uint2 *>(row) : make_uint2(0u, 0u);
#pragma unroll
            for (uint32_t xl = 0; xl < (uint32_t)G::BX; ++xl) {
                const uint32_t x = bx * (uint32_t)G::BX + xl - (uint32_t)kPad;
                const uint32_t code = ((xl < 4 ? d.x : d.y) >> (8u * (xl & 3u))) & 0xFFu;
                add(row_in && x >= A.box_min[0] && x < A.box_max[0], code);
            }
        }
        __syncthreads();
        // fold: thread c owns code c
        const uint32_t n = s_bins[tid];
        if (n) {
            const float v = (float)(V)tid;
            if (!classify(v, n)) atomicAdd(&out[bin_of(v)], (unsigned long long)n);
        }
    } else {
        for (uint32_t w = blockIdx.x; w < A.nwork; w += gridDim.x) {
            const uint32_t bx = A.b0[0] + w % A.nb[0], by = A.b0[1] + (w / A.nb[0]) % A.nb[1],
                           bz = A.b0[2] + w / (A.nb[0] * A.nb[1]);
            const V *__restrict__ src =
                vol + (size_t)brick_slot(bx, by, bz, A.nbx, A.nby) * (size_t)G::Elems * vpe;
#pragma unroll
            for (uint32_t c = tid; c < kCells; c += 256) {
                const uint32_t xl = c % (uint32_t)G::BX, yl = (c / (uint32_t)G::BX) % (uint32_t)G::BY,
                               zl = c / (uint32_t)(G::BX * G::BY);
                // logical index = padded - kPad; a padding cell wraps to a huge value and fails < max
                const uint32_t x = bx * (uint32_t)G::BX + xl - (uint32_t)kPad,
                               y = by * (uint32_t)G::BY + yl - (uint32_t)kPad,
                               z = bz * (uint32_t)G::BZ + zl - (uint32_t)kPad;
                const bool in = x >= A.box_min[0] && x < A.box_max[0] && y >= A.box_min[1] &&
                                y < A.box_max[1] && z >= A.box_min[2] && z < A.box_max[2];
                bool counts = false;
                uint32_t b = 0;
                if (in) {
                    const float v = (float)src[((zl * (uint32_t)G::EY + yl) * (uint32_t)G::EX + xl) * vpe];
                    if (v != v) {
                        ++nan;
                    } else if (!classify(v, 1u)) {
                        b = bin_of(v);
                        counts = true;
                    }
                }
                add(counts, b);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        below += __shfl_xor(below, off, 64);
        above += __shfl_xor(above, off, 64);
        nan += __shfl_xor(nan, off, 64);
        const uint32_t m2 = __shfl_xor(inv_mn, off, 64), h2 = __shfl_xor(mx, off, 64);
        inv_mn = m2 > inv_mn ? m2 : inv_mn;
        mx = h2 > mx ? h2 : mx;
    }
    if ((tid & 63u) == 0) {
        uint32_t *r = s_red[tid >> 6];
        r[0] = below;
        r[1] = above;
        r[2] = nan;
        r[3] = inv_mn;
        r[4] = mx;
    }
    __syncthreads();
    if constexpr (!kHistCodes<VT>) {
        for (uint32_t i = tid; i < nbins; i += 256) {
            const uint32_t n = s_bins[i];
            if (n) atomicAdd(&out[i], (unsigned long long)n);
        }
    }
    if (tid == 0) {
        for (uint32_t i = 1; i < 4; ++i) {
            below += s_red[i][0];
            above += s_red[i][1];
            nan += s_red[i][2];
            inv_mn = s_red[i][3] > inv_mn ? s_red[i][3] : inv_mn;
            mx = s_red[i][4] > mx ? s_red[i][4] : mx;
        }
        if (below) atomicAdd(&out[nbins + 0], (unsigned long long)below);
        if (above) atomicAdd(&out[nbins + 1], (unsigned long long)above);
        if (nan) atomicAdd(&out[nbins + 2], (unsigned long long)nan);
        uint32_t *__restrict__ ext = reinterpret_cast<uint32_t *>(out + nbins + 3);
        atomicMax(&ext[0], inv_mn);
        atomicMax(&ext[1], mx);
    }
}

// ---- isosurface mesh (include/vr/vr_mesh.h) ----------------------------------------------------
// Surface nets over the base bricks, four passes (vr_internal.h MeshArgs): classify, scan, vertex,
// quad.  Classify, vertex and quad grid-stride over the work bricks, a brick per workgroup
// iteration and a lane per cell, as hist_kernel walks a box's bricks.  A cell's eight corners are
// its own brick's elements (Cell8's loads, apron included), so no pass looks into a neighbour
// brick for values; the quad pass looks up neighbour cells' vertex ids, through the masks.
// Everything a result depends on is an integer or the f32 arithmetic of one lane: no result
// depends on an order of accumulation or on the grid.

// One cell after the box rule: corner i's value is the stored one where the node lies in N and
// +0.0f elsewhere (the closed mesh's ring; never what the bricks hold there).
struct MeshCell {
    float v[8];    // index dx + 2 dy + 4 dz
    int c[3];      // the cell's logical index (padded - kPad; -1: the ring cell below voxel 0)
    uint32_t m8;   // bit i: corner i is inside (v >= iso; a NaN never is)
    bool in_set;   // a cell of the cell set
};

template <typename VT>
__device__ __forceinline__ MeshCell mesh_cell(const MeshArgs &A, const char *__restrict__ vol,
                                              uint32_t bx, uint32_t by, uint32_t bz, uint32_t cell)
{
    using G = GeomOf<VT>;
    static_assert(G::Lo == 0, "the base layouts");
    const uint32_t xl = cell % (uint32_t)G::BX, yl = (cell / (uint32_t)G::BX) % (uint32_t)G::BY,
                   zl = cell / (uint32_t)(G::BX * G::BY);
    MeshCell m;
    m.c[0] = (int)(bx * (uint32_t)G::BX + xl) - kPad;
    m.c[1] = (int)(by * (uint32_t)G::BY + yl) - kPad;
    m.c[2] = (int)(bz * (uint32_t)G::BZ + zl) - kPad;
    const size_t e = (size_t)brick_slot(bx, by, bz, A.nbx, A.nby) * (size_t)G::Elems +
                     (zl * (uint32_t)G::EY + yl) * (uint32_t)G::EX + xl;
    Cell8<VT> c8;
    c8.load(vol, e);
    m.m8 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        // a node below 0 wraps to a huge value and fails < hi
        const uint32_t x = (uint32_t)(m.c[0] + (i & 1)), y = (uint32_t)(m.c[1] + ((i >> 1) & 1)),
                       z = (uint32_t)(m.c[2] + (i >> 2));
        const bool in = x >= A.lo[0] && x < A.hi[0] && y >= A.lo[1] && y < A.hi[1] && z >= A.lo[2] &&
                        z < A.hi[2];
        m.v[i] = in ? c8.v[i] : 0.0f;
        m.m8 |= m.v[i] >= A.iso ? 1u << i : 0u;
    }
    m.in_set = m.c[0] >= A.clo[0] && m.c[0] <= A.chi[0] && m.c[1] >= A.clo[1] && m.c[1] <= A.chi[1] &&
               m.c[2] >= A.clo[2] && m.c[2] <= A.chi[2];
    return m;
}
__device__ __forceinline__ bool mesh_active(const MeshCell &m)
{
    return m.in_set && m.m8 != 0u && m.m8 != 0xFFu;
}
// Bit a: the cell owns a qualifying edge along axis a -- the lattice edge from its corner 0 to
// corner 1 << a crosses the surface and the three other cells around it are cells of the set.
__device__ __forceinline__ uint32_t mesh_edges(const MeshArgs &A, const MeshCell &m)
{
    uint32_t q = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        const bool cross = ((m.m8 ^ (m.m8 >> (1 << a))) & 1u) != 0u;
        q |= m.in_set && cross && m.c[b] > A.clo[b] && m.c[c] > A.clo[c] ? 1u << a : 0u;
    }
    return q;
}
__device__ __forceinline__ void mesh_work_brick(const MeshArgs &A, uint32_t w, uint32_t &bx, uint32_t &by,
                                                uint32_t &bz)
{
    bx = A.b0[0] + w % A.nb[0];
    by = A.b0[1] + (w / A.nb[0]) % A.nb[1];
    bz = A.b0[2] + w / (A.nb[0] * A.nb[1]);
}
// Active cells of work brick w below `cell`.
__device__ __forceinline__ uint32_t mesh_prefix(const uint32_t *__restrict__ mask, uint32_t w, uint32_t cell)
{
    const uint32_t *__restrict__ m = mask + (size_t)w * kMeshMaskWords;
    const uint32_t wi = cell >> 5;
    uint32_t n = (uint32_t)__popc(m[wi] & ((1u << (cell & 31u)) - 1u));
    for (uint32_t i = 0; i < wi; ++i) n += (uint32_t)__popc(m[i]);
    return n;
}
// The vertex id of the active cell with logical index (cx, cy, cz), a cell of the cell set.
template <typename VT>
__device__ __forceinline__ uint32_t mesh_vertex_id(const MeshArgs &A, int cx, int cy, int cz)
{
    using G = GeomOf<VT>;
    const uint32_t px = (uint32_t)(cx + kPad), py = (uint32_t)(cy + kPad), pz = (uint32_t)(cz + kPad);
    const uint32_t bx = px / (uint32_t)G::BX, by = py / (uint32_t)G::BY, bz = pz / (uint32_t)G::BZ;
    const uint32_t cell = (px - bx * (uint32_t)G::BX) +
                          (uint32_t)G::BX * ((py - by * (uint32_t)G::BY) + (uint32_t)G::BY * (pz - bz * (uint32_t)G::BZ));
    const uint32_t w = (bx - A.b0[0]) + A.nb[0] * ((by - A.b0[1]) + A.nb[1] * (bz - A.b0[2]));
    return (uint32_t)A.chunk[2u * (w / kMeshChunk)] + A.pre[w].x + mesh_prefix(A.mask, w, cell);
}

// Pass 1.  Per brick: the mask of active cells (a ballot per wave of 64 cells), the counts of
// active cells and of owned qualifying edges (wave popcounts, summed through LDS: s_cnt is
// double-buffered by the iteration's parity, so a brick costs one barrier).  The inside voxels --
// corner 0 of every walked cell whose own index lies in N -- count per lane, then per wave and
// workgroup, before one 64-bit atomic.
template <typename VT>
__global__ __launch_bounds__(256) void mesh_classify_kernel(const MeshArgs A)
{
    using G = GeomOf<VT>;
    constexpr uint32_t kCells = (uint32_t)(G::BX * G::BY * G::BZ);
    constexpr uint32_t kIters = (kCells + 255u) / 256u;
    static_assert(kCells <= kMeshMaskWords * 32u, "a brick's cells fit its mask");
    __shared__ uint32_t s_cnt[2][4][2];
    __shared__ uint32_t s_in[4];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const char *__restrict__ vol = static_cast<const char *>(A.vol);
    uint32_t inside = 0, par = 0;
    for (uint32_t w = blockIdx.x; w < A.nwork; w += gridDim.x, par ^= 1u) {
        uint32_t bx, by, bz;
        mesh_work_brick(A, w, bx, by, bz);
        uint32_t nv = 0, ne = 0;
#pragma unroll
        for (uint32_t it = 0; it < kIters; ++it) {
            const uint32_t cell = it * 256u + tid;
            bool act = false;
            uint32_t q = 0;
            if (cell < kCells) {
                const MeshCell m = mesh_cell<VT>(A, vol, bx, by, bz, cell);
                act = mesh_active(m);
                q = mesh_edges(A, m);
                const uint32_t x = (uint32_t)m.c[0], y = (uint32_t)m.c[1], z = (uint32_t)m.c[2];
                const bool in = x >= A.lo[0] && x < A.hi[0] && y >= A.lo[1] && y < A.hi[1] &&
                                z >= A.lo[2] && z < A.hi[2];
                inside += in && (m.m8 & 1u) ? 1u : 0u;
            }
            const unsigned long long ba = __ballot(act);
            nv += (uint32_t)__popcll(ba);
            ne += (uint32_t)(__popcll(__ballot((q & 1u) != 0u)) + __popcll(__ballot((q & 2u) != 0u)) +
                             __popcll(__ballot((q & 4u) != 0u)));
            if (lane == 0)  // cells 64 (4 it + wave) .. + 63: words 2 (4 it + wave), + 1
                *reinterpret_cast<uint2 *>(A.mask + (size_t)w * kMeshMaskWords + (it * 4u + wave) * 2u) =
                    make_uint2((uint32_t)ba, (uint32_t)(ba >> 32));
        }
        if (lane == 0) {
            s_cnt[par][wave][0] = nv;
            s_cnt[par][wave][1] = ne;
        }
        __syncthreads();
        if (tid == 0)
            A.cnt[w] = make_uint2(s_cnt[par][0][0] + s_cnt[par][1][0] + s_cnt[par][2][0] + s_cnt[par][3][0],
                                  s_cnt[par][0][1] + s_cnt[par][1][1] + s_cnt[par][2][1] + s_cnt[par][3][1]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) inside += __shfl_xor(inside, off, 64);
    if (lane == 0) s_in[wave] = inside;
    __syncthreads();
    if (tid == 0) {
        const uint32_t n = s_in[0] + s_in[1] + s_in[2] + s_in[3];
        if (n) atomicAdd(&A.out[2], (unsigned long long)n);
    }
}

// Pass 2a.  One workgroup per chunk of kMeshChunk bricks, four bricks per lane: the exclusive
// prefix of cnt inside the chunk into pre (32-bit: a chunk holds at most 1024 x 1536 edges), the
// chunk's two sums into chunk.
__global__ __launch_bounds__(256) void mesh_scan_bricks_kernel(const MeshArgs A)
{
    static_assert(kMeshChunk == 1024, "256 lanes x 4 bricks");
    __shared__ uint32_t s_tot[4][2];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t i0 = blockIdx.x * kMeshChunk + tid * 4u;
    uint2 n[4];
    uint32_t tv = 0, te = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        n[k] = i0 + k < A.nwork ? A.cnt[i0 + k] : make_uint2(0u, 0u);
        tv += n[k].x;
        te += n[k].y;
    }
    uint32_t sv = tv, se = te;  // inclusive over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t pv = __shfl_up(sv, off, 64), pe = __shfl_up(se, off, 64);
        sv += (int)lane >= off ? pv : 0u;
        se += (int)lane >= off ? pe : 0u;
    }
    if (lane == 63) {
        s_tot[wave][0] = sv;
        s_tot[wave][1] = se;
    }
    __syncthreads();
    uint32_t bv = sv - tv, be = se - te;  // exclusive
    for (uint32_t k = 0; k < wave; ++k) {
        bv += s_tot[k][0];
        be += s_tot[k][1];
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (i0 + k < A.nwork) A.pre[i0 + k] = make_uint2(bv, be);
        bv += n[k].x;
        be += n[k].y;
    }
    if (tid == 255) {  // (bv, be: the chunk's sums now)
        A.chunk[2u * blockIdx.x] = bv;
        A.chunk[2u * blockIdx.x + 1u] = be;
    }
}

// Pass 2b.  One workgroup: the chunk sums into their exclusive prefix, 256 chunks a round with a
// carry, in 64 bits; the totals into out[0] (vertices) and out[1] (quads).
__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int off)
{
    const uint32_t lo = __shfl_up((uint32_t)v, off, 64), hi = __shfl_up((uint32_t)(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__global__ __launch_bounds__(256) void mesh_scan_chunks_kernel(const MeshArgs A)
{
    __shared__ unsigned long long s_tot[2][4][2];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    unsigned long long cv = 0, ce = 0;  // the carry: the sums of the rounds before
    uint32_t par = 0;
    for (uint32_t g0 = 0; g0 < A.nchunks; g0 += 256u, par ^= 1u) {
        const uint32_t g = g0 + tid;
        const unsigned long long tv = g < A.nchunks ? A.chunk[2u * g] : 0ull,
                                 te = g < A.nchunks ? A.chunk[2u * g + 1u] : 0ull;
        unsigned long long sv = tv, se = te;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long pv = shfl_up_u64(sv, off), pe = shfl_up_u64(se, off);
            sv += (int)lane >= off ? pv : 0ull;
            se += (int)lane >= off ? pe : 0ull;
        }
        if (lane == 63) {
            s_tot[par][wave][0] = sv;
            s_tot[par][wave][1] = se;
        }
        __syncthreads();
        unsigned long long bv = cv + (sv - tv), be = ce + (se - te);
        for (uint32_t k = 0; k < wave; ++k) {
            bv += s_tot[par][k][0];
            be += s_tot[par][k][1];
        }
        if (g < A.nchunks) {
            A.chunk[2u * g] = bv;
            A.chunk[2u * g + 1u] = be;
        }
        cv += s_tot[par][0][0] + s_tot[par][1][0] + s_tot[par][2][0] + s_tot[par][3][0];
        ce += s_tot[par][0][1] + s_tot[par][1][1] + s_tot[par][2][1] + s_tot[par][3][1];
    }
    if (tid == 0) {
        A.out[0] = cv;
        A.out[1] = ce;
    }
}

// Voxel (x, y, z) through the sampler's border rule: component 0 of its own element (what
// unbrick_kernel reads), +0.0f outside the volume.
template <typename VT>
__device__ __forceinline__ float mesh_voxel(const MeshArgs &A, const char *__restrict__ vol, int x, int y,
                                            int z)
{
    constexpr size_t vpe = std::is_same<VT, float>::value ? kF32VoxelsPerElement
                                                          : (kPlainByte<VT> ? (size_t)1 : (size_t)4);
    if ((uint32_t)x >= A.dims[0] || (uint32_t)y >= A.dims[1] || (uint32_t)z >= A.dims[2]) return 0.0f;
    const size_t e = cell_offset<VT>(x + kPad, y + kPad, z + kPad, A.nbx, A.nby);
    return (float)reinterpret_cast<const Vox<VT> *>(vol)[e * vpe];
}

// Pass 3.  A lane per active cell: the vertex of vr_mesh.h, at id = the brick's base + the mask's
// prefix.  The normal's gradient is gradient<VT, false>, the device code iso_strip shades with, at
// the texel cell of pos; where rounding puts that cell outside [-1, n - 1] -- beyond what the
// stencil's taps may touch -- the same differences are formed voxel by voxel under the border rule.
template <typename VT, bool NORMALS>
__global__ __launch_bounds__(256) void mesh_vertex_kernel(const MeshArgs A)
{
    using G = GeomOf<VT>;
    constexpr uint32_t kCells = (uint32_t)(G::BX * G::BY * G::BZ);
    constexpr uint32_t kIters = (kCells + 255u) / 256u;
    const uint32_t tid = threadIdx.x;
    const char *__restrict__ vol = static_cast<const char *>(A.vol);
    const long by_stride = (long)A.nbx * G::Elems;
    const long bz_stride = (long)A.nbx * A.nby * G::Elems;
    const float iso = A.iso;
    for (uint32_t w = blockIdx.x; w < A.nwork; w += gridDim.x) {
        if (A.cnt[w].x == 0u) continue;  // (workgroup-uniform)
        uint32_t bx, by, bz;
        mesh_work_brick(A, w, bx, by, bz);
        const uint32_t base = (uint32_t)A.chunk[2u * (w / kMeshChunk)] + A.pre[w].x;
#pragma unroll 1
        for (uint32_t it = 0; it < kIters; ++it) {
            const uint32_t cell = it * 256u + tid;
            if (cell >= kCells) continue;
            if (((A.mask[(size_t)w * kMeshMaskWords + (cell >> 5)] >> (cell & 31u)) & 1u) == 0u) continue;
            const uint32_t id = base + mesh_prefix(A.mask, w, cell);
            const MeshCell m = mesh_cell<VT>(A, vol, bx, by, bz, cell);
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, n = 0.0f;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // the j-th corner with bit a clear, ascending; its partner along a
                    const int ca = a == 0 ? 2 * j : (a == 1 ? (j & 1) | ((j >> 1) << 2) : j);
                    const int cb = ca | (1 << a);
                    const bool cross = (((m.m8 >> ca) ^ (m.m8 >> cb)) & 1u) != 0u;
                    const float va = m.v[ca], vb = m.v[cb];
                    float t = (iso - va) / (vb - va);
                    if (!(t >= 0.0f)) t = 0.0f;
                    if (t > 1.0f) t = 1.0f;
                    const float p0 = a == 0 ? t : (float)(ca & 1), p1 = a == 1 ? t : (float)((ca >> 1) & 1),
                                p2 = a == 2 ? t : (float)(ca >> 2);
                    s0 = cross ? s0 + p0 : s0;
                    s1 = cross ? s1 + p1 : s1;
                    s2 = cross ? s2 + p2 : s2;
                    n = cross ? n + 1.0f : n;
                }
            const float pos0 = (((float)m.c[0] + 0.5f) + s0 / n) / A.fdims[0],
                        pos1 = (((float)m.c[1] + 0.5f) + s1 / n) / A.fdims[1],
                        pos2 = (((float)m.c[2] + 0.5f) + s2 / n) / A.fdims[2];
            float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
            if constexpr (NORMALS) {
                int i, j, k;
                float ax, ay, az, gx, gy, gz;
                texel_coord(pos0, A.fdims[0], i, ax);
                texel_coord(pos1, A.fdims[1], j, ay);
                texel_coord(pos2, A.fdims[2], k, az);
                if (i >= -1 && i < (int)A.dims[0] && j >= -1 && j < (int)A.dims[1] && k >= -1 &&
                    k < (int)A.dims[2]) {
                    const int pi = i + kPad, pj = j + kPad, pk = k + kPad;
                    const size_t ce = cell_offset<VT>(pi, pj, pk, A.nbx, A.nby);
                    Cell8<VT> c;
                    c.load(vol, ce);
                    gradient<VT, false>(vol, ce, c, pi, pj, pk, A.nbx, A.nby, by_stride, bz_stride, ax, ay,
                                        az, gx, gy, gz);
                } else {
                    float Dx[8], Dy[8], Dz[8];
#pragma unroll
                    for (int o = 0; o < 8; ++o) {
                        const int x = i + (o & 1), y = j + ((o >> 1) & 1), z = k + (o >> 2);
                        Dx[o] = mesh_voxel<VT>(A, vol, x + 1, y, z) - mesh_voxel<VT>(A, vol, x - 1, y, z);
                        Dy[o] = mesh_voxel<VT>(A, vol, x, y + 1, z) - mesh_voxel<VT>(A, vol, x, y - 1, z);
                        Dz[o] = mesh_voxel<VT>(A, vol, x, y, z + 1) - mesh_voxel<VT>(A, vol, x, y, z - 1);
                    }
                    grad_filter<false>(Dx, Dy, Dz, ax, ay, az, gx, gy, gz);
                }
                const float wx = gx * A.fdims[0], wy = gy * A.fdims[1], wz = gz * A.fdims[2];
                const float g2 = wx * wx + wy * wy + wz * wz;
                if (g2 > 0.0f) {
                    const float r = inv_sqrt_ieee(g2);
                    n0 = -(wx * r);
                    n1 = -(wy * r);
                    n2 = -(wz * r);
                }
            }
            // (f2a, u2a below: a caller's device buffer need only be 4-aligned)
            f2a *o = reinterpret_cast<f2a *>(static_cast<char *>(A.verts) + (size_t)id * kMeshVertexBytes);
            o[0] = f2a{pos0, pos1};
            o[1] = f2a{pos2, n0};
            o[2] = f2a{n1, n2};
        }
    }
}

// Pass 4.  A lane per cell again; the cell re-reads its corners, so its owned qualifying edges and
// their directions are mesh_edges' once more.  A brick's quads are numbered cell by cell, x, y, z
// within a cell: ballots give a lane its place in the wave, LDS the waves' sums (double-buffered
// by parity: one barrier a brick).  Six indices leave as three 8-byte stores.
template <typename VT>
__global__ __launch_bounds__(256) void mesh_quad_kernel(const MeshArgs A)
{
    using G = GeomOf<VT>;
    constexpr uint32_t kCells = (uint32_t)(G::BX * G::BY * G::BZ);
    constexpr uint32_t kIters = (kCells + 255u) / 256u;
    __shared__ uint32_t s_seg[2][kIters * 4u];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const char *__restrict__ vol = static_cast<const char *>(A.vol);
    uint32_t par = 0;
    for (uint32_t w = blockIdx.x; w < A.nwork; w += gridDim.x) {
        if (A.cnt[w].y == 0u) continue;  // (workgroup-uniform)
        uint32_t bx, by, bz;
        mesh_work_brick(A, w, bx, by, bz);
        const unsigned long long qbase = A.chunk[2u * (w / kMeshChunk) + 1u] + A.pre[w].y;
        uint32_t q[kIters], place[kIters];
#pragma unroll
        for (uint32_t it = 0; it < kIters; ++it) {
            const uint32_t cell = it * 256u + tid;
            q[it] = 0;
            if (cell < kCells) {
                const MeshCell m = mesh_cell<VT>(A, vol, bx, by, bz, cell);
                q[it] = mesh_edges(A, m) | ((m.m8 & 1u) << 3);
            }
            const unsigned long long e0 = __ballot((q[it] & 1u) != 0u), e1 = __ballot((q[it] & 2u) != 0u),
                                     e2 = __ballot((q[it] & 4u) != 0u);
            place[it] = (uint32_t)(__popcll(e0 & lt) + __popcll(e1 & lt) + __popcll(e2 & lt));
            if (lane == 0) s_seg[par][it * 4u + wave] = (uint32_t)(__popcll(e0) + __popcll(e1) + __popcll(e2));
        }
        __syncthreads();
#pragma unroll
        for (uint32_t it = 0; it < kIters; ++it) {
            if ((q[it] & 7u) == 0u) continue;
            uint32_t off = place[it];
            for (uint32_t s = 0; s < it * 4u + wave; ++s) off += s_seg[par][s];
            const uint32_t cell = it * 256u + tid;
            const uint32_t xl = cell % (uint32_t)G::BX, yl = (cell / (uint32_t)G::BX) % (uint32_t)G::BY,
                           zl = cell / (uint32_t)(G::BX * G::BY);
            const int c0 = (int)(bx * (uint32_t)G::BX + xl) - kPad, c1 = (int)(by * (uint32_t)G::BY + yl) - kPad,
                      c2 = (int)(bz * (uint32_t)G::BZ + zl) - kPad;
            const uint32_t v2 = mesh_vertex_id<VT>(A, c0, c1, c2);
            const bool p_in = (q[it] & 8u) != 0u;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (((q[it] >> a) & 1u) == 0u) continue;
                // b = (a + 1) % 3, c = (a + 2) % 3: C0 = P - e_b - e_c, C1 = P - e_c, C3 = P - e_b
                const int b0 = a == 2, b1 = a == 0, b2 = a == 1;  // e_b
                const int d0 = a == 1, d1 = a == 2, d2 = a == 0;  // e_c
                const uint32_t v0 = mesh_vertex_id<VT>(A, c0 - b0 - d0, c1 - b1 - d1, c2 - b2 - d2);
                const uint32_t v1 = mesh_vertex_id<VT>(A, c0 - d0, c1 - d1, c2 - d2);
                const uint32_t v3 = mesh_vertex_id<VT>(A, c0 - b0, c1 - b1, c2 - b2);
                u2a *o = reinterpret_cast<u2a *>(A.tris + (size_t)(qbase + off) * 6u);
                o[0] = u2a{v0, p_in ? v1 : v2};
                o[1] = u2a{p_in ? v2 : v1, v0};
                o[2] = u2a{p_in ? v2 : v3, p_in ? v3 : v2};
                ++off;
            }
        }
        par ^= 1u;
    }
}

// ---- connected components and region growing (include/vr/vr_label.h) ---------------------------
// A lock-free union-find over the voxels of the box N (vr_internal.h LabelArgs).  The label array P
// is the parent array: P[l] = 0 for a voxel that is not in, else 1 + the box-linear index of a
// voxel of the same component that is not larger than l -- l itself for a root.  The local pass
// unites inside a brick in LDS, the seam pass across bricks through P with atomicMin, the flatten
// pass replaces every parent by the root: the root is the component's smallest index, so P then
// holds vr_label.h's labels.  No workgroup ever waits for another: the order of the passes comes
// from the kernel boundaries.  Every loop is bounded: a find strictly descends (a parent is smaller
// than its child; `p >= x` also ends it on anything else), a unite retries only with one of its two
// roots strictly lowered, the wave rounds of the table pass are counted.

// parent + 1 of voxel x, as an agent-scope relaxed atomic load: it skips this CU's L1 but is served
// by the XCD's L2, which is not coherent with the other XCDs', so the value may be stale.  Nothing
// rests on its freshness: correctness is the stale-parent argument below and the atomicMin, which
// executes on the word itself and returns what it really held.
__device__ __forceinline__ uint32_t label_load(const uint32_t *P, uint32_t x)
{
    return __hip_atomic_load(P + (size_t)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The root above in-voxel x as far as this thread can see.  A stale parent is an older ancestor:
// still a voxel of x's component, and not below the true root.
__device__ __forceinline__ uint32_t label_find(const uint32_t *P, uint32_t x)
{
    for (;;) {
        const uint32_t p = label_load(P, x) - 1u;
        if (p >= x) return x;  // (p == x: a root)
        x = p;
    }
}
// Unite the components of in-voxels a and b.  atomicMin hangs the larger root under the smaller;
// where the larger one was no root any more (old != hi + 1), the link to old - 1 that the minimum
// kept or replaced must not be lost: go on uniting old - 1 with lo.  hi falls on every retry.
__device__ __forceinline__ void label_unite(uint32_t *P, uint32_t a, uint32_t b)
{
    for (;;) {
        a = label_find(P, a);
        b = label_find(P, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicMin(P + (size_t)hi, lo + 1u);
        if (old == hi + 1u) return;
        a = old - 1u;
        b = lo;
    }
}
// The same inside a brick, on the workgroup's LDS array of cell + 1.
__device__ __forceinline__ uint32_t label_find_lds(const uint32_t *s, uint32_t x)
{
    for (;;) {
        const uint32_t p = __hip_atomic_load(s + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - 1u;
        if (p >= x) return x;
        x = p;
    }
}
__device__ __forceinline__ void label_unite_lds(uint32_t *s, uint32_t a, uint32_t b)
{
    for (;;) {
        a = label_find_lds(s, a);
        b = label_find_lds(s, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicMin(s + hi, lo + 1u);
        if (old == hi + 1u) return;
        a = old - 1u;
        b = lo;
    }
}
// The 13 neighbour offsets that come before a voxel in (z, y, x) order; the first three are the
// 6-connected ones.
__device__ constexpr int kLabelNb[13][3] = {{-1, 0, 0},  {0, -1, 0},  {0, 0, -1}, {-1, -1, 0}, {1, -1, 0},
                                            {-1, 0, -1}, {1, 0, -1},  {0, -1, -1}, {0, 1, -1}, {-1, -1, -1},
                                            {1, -1, -1}, {-1, 1, -1}, {1, 1, -1}};

// 26-connectivity needs few of its diagonal pairs.  Let u and v = u + d differ along two or three
// axes, and let some other voxel w of the square or cube they span (every coordinate u's or v's) be
// in.  w differs from each of u and v along fewer axes than they differ from each other, so by
// induction on that number -- face pairs are always united -- u ~ w and w ~ v hold without the pair
// (u, v).  The rule reads in flags alone, which no pass changes, so both passes may apply it, each to
// its own pairs.  in(ax, ay, az): the voxel at u + (ax, ay, az) is in.
template <typename F>
__device__ __forceinline__ bool label_diagonal_redundant(const int d[3], F in)
{
    const int n = (d[0] != 0) + (d[1] != 0) + (d[2] != 0);
    if (n == 2) {
        if (d[0] == 0) return in(0, d[1], 0) || in(0, 0, d[2]);
        if (d[1] == 0) return in(d[0], 0, 0) || in(0, 0, d[2]);
        return in(d[0], 0, 0) || in(0, d[1], 0);
    }
    if (n == 3)
        return in(d[0], 0, 0) || in(0, d[1], 0) || in(0, 0, d[2]) || in(d[0], d[1], 0) || in(d[0], 0, d[2]) ||
               in(0, d[1], d[2]);
    return false;
}

// Pass 1.  A workgroup per work brick (grid-stride), a lane per cell: the box rule and the window
// give the in flags; the in cells unite with their in neighbours of the same brick in LDS (cell
// order is (z, y, x) order, as the box-linear index: the local root is the smallest l); every
// voxel of N in the brick then gets 1 + the box-linear index of its local root, or 0, in P.
template <typename VT, int CONN>
__global__ __launch_bounds__(256) void label_local_kernel(const LabelArgs A)
{
    using G = GeomOf<VT>;
    using V = Vox<VT>;
    static_assert(G::Lo == 0, "the base layouts");
    constexpr uint32_t vpe = std::is_same<VT, float>::value ? (uint32_t)kF32VoxelsPerElement
                                                            : (kPlainByte<VT> ? 1u : 4u);
    constexpr uint32_t BX = (uint32_t)G::BX, BY = (uint32_t)G::BY, BZ = (uint32_t)G::BZ;
    constexpr uint32_t kCells = BX * BY * BZ;
    constexpr uint32_t kIters = (kCells + 255u) / 256u;
    constexpr int kNb = CONN == 6 ? 3 : 13;
    __shared__ uint32_t s_par[kCells];
    const uint32_t tid = threadIdx.x;
    const V *__restrict__ vol = static_cast<const V *>(A.vol);
    uint32_t *__restrict__ P = A.P;
    const float lo = A.lo, hi = A.hi;
    for (uint32_t w = blockIdx.x; w < A.nwork; w += gridDim.x) {
        const uint32_t bx = A.b0[0] + w % A.nb[0], by = A.b0[1] + (w / A.nb[0]) % A.nb[1],
                       bz = A.b0[2] + w / (A.nb[0] * A.nb[1]);
        const V *__restrict__ src = vol + (size_t)brick_slot(bx, by, bz, A.nbx, A.nby) * (size_t)G::Elems * vpe;
        bool in_n[kIters], in[kIters];
        uint32_t lin[kIters];
#pragma unroll
        for (uint32_t it = 0; it < kIters; ++it) {
            const uint32_t cell = it * 256u + tid;
            in_n[it] = in[it] = false;
            lin[it] = 0;
            if (cell < kCells) {
                const uint32_t xl = cell % BX, yl = (cell / BX) % BY, zl = cell / (BX * BY);
                // logical index = padded - kPad; a padding cell wraps to a huge value and fails < max
                const uint32_t x = bx * BX + xl - (uint32_t)kPad, y = by * BY + yl - (uint32_t)kPad,
                               z = bz * BZ + zl - (uint32_t)kPad;
                in_n[it] = x >= A.blo[0] && x < A.bhi[0] && y >= A.blo[1] && y < A.bhi[1] && z >= A.blo[2] &&
                           z < A.bhi[2];
                if (in_n[it]) {
                    const float v = (float)src[((zl * (uint32_t)G::EY + yl) * (uint32_t)G::EX + xl) * vpe];
                    in[it] = lo <= v && v <= hi;
                    lin[it] = (x - A.blo[0]) + A.ext[0] * ((y - A.blo[1]) + A.ext[1] * (z - A.blo[2]));
                }
                s_par[cell] = in[it] ? cell + 1u : 0u;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t it = 0; it < kIters; ++it) {
            const uint32_t cell = it * 256u + tid;
            if (!in[it]) continue;
            const int xl = (int)(cell % BX), yl = (int)((cell / BX) % BY), zl = (int)(cell / (BX * BY));
#pragma unroll
            for (int k = 0; k < kNb; ++k) {
                const int nx = xl + kLabelNb[k][0], ny = yl + kLabelNb[k][1], nz = zl + kLabelNb[k][2];
                if (nx < 0 || nx >= (int)BX || ny < 0 || ny >= (int)BY || nz < 0) continue;
                const uint32_t ncell = (uint32_t)nx + BX * ((uint32_t)ny + BY * (uint32_t)nz);
                // (0 stays 0: a cell that is not in is never the target of a minimum)
                auto is_in = [&](int cx, int cy, int cz) __attribute__((always_inline)) {
                    return __hip_atomic_load(s_par + ((uint32_t)cx + BX * ((uint32_t)cy + BY * (uint32_t)cz)),
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u;
                };
                if (!is_in(nx, ny, nz)) continue;
                // A diagonal pair whose square or cube (inside the brick, as both ends are) holds
                // another in cell is joined through it by pairs that differ along fewer axes.
                if (label_diagonal_redundant(kLabelNb[k], [&](int ax, int ay, int az) __attribute__((always_inline)) {
                        return is_in(xl + ax, yl + ay, zl + az);
                    }))
                    continue;
                label_unite_lds(s_par, cell, ncell);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t it = 0; it < kIters; ++it) {
            const uint32_t cell = it * 256u + tid;
            if (!in_n[it]) continue;
            uint32_t out = 0;
            if (in[it]) {
                const uint32_t r = label_find_lds(s_par, cell);
                const uint32_t dx = r % BX - cell % BX, dy = (r / BX) % BY - (cell / BX) % BY,
                               dz = r / (BX * BY) - cell / (BX * BY);  // (differences modulo 2^32)
                out = lin[it] + dx + A.ext[0] * (dy + A.ext[1] * dz) + 1u;
            }
            P[(size_t)lin[it]] = out;
        }
        __syncthreads();  // (s_par is the next brick's)
    }
}

// Pass 2.  A wave per row of N (grid-stride), a lane per voxel: an in voxel unites with every in
// neighbour before it in (z, y, x) order that lies in N and in ANOTHER brick (the same brick's were
// united in pass 1).  It reads P alone: every load an agent-scope atomic load, every store an
// atomicMin.
template <int CONN, typename G>
__global__ __launch_bounds__(256) void label_seam_kernel(const LabelArgs A)
{
    constexpr int BX = G::BX, BY = G::BY, BZ = G::BZ;
    constexpr int kNb = CONN == 6 ? 3 : 13;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t ex = A.ext[0], ey = A.ext[1], ez = A.ext[2];
    const uint64_t nrows = (uint64_t)ey * ez;
    uint32_t *P = A.P;
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + wave; r < nrows; r += (uint64_t)gridDim.x * 4u) {
        const uint32_t yb = (uint32_t)(r % ey), zb = (uint32_t)(r / ey);
        const int yl = (int)((yb + A.blo[1] + (uint32_t)kPad) % (uint32_t)BY),
                  zl = (int)((zb + A.blo[2] + (uint32_t)kPad) % (uint32_t)BZ);
        // (A lane per voxel although on most rows only the voxels on an x face have work, one in BX:
        // walking those alone, 64 face voxels of a row at once, was measured and lost -- the seam
        // pass of C3 under 6 took 2.14 ms against this form's figure in DESIGN.md 4.12, C4's twice
        // as long -- 64 concurrent walks to one root instead of 8.)
        for (uint32_t xb = lane; xb < ex; xb += 64u) {
            const int xl = (int)((xb + A.blo[0] + (uint32_t)kPad) % (uint32_t)BX);
            if (xl != 0 && yl != 0 && zl != 0 && (CONN == 6 || (xl != BX - 1 && yl != BY - 1))) continue;
            const uint32_t l = xb + ex * (yb + ey * zb);
            if (label_load(P, l) == 0u) continue;
#pragma unroll
            for (int k = 0; k < kNb; ++k) {
                const int dx = kLabelNb[k][0], dy = kLabelNb[k][1], dz = kLabelNb[k][2];
                const bool crosses = (dx < 0 && xl == 0) || (dx > 0 && xl == BX - 1) || (dy < 0 && yl == 0) ||
                                     (dy > 0 && yl == BY - 1) || (dz < 0 && zl == 0);
                const bool in_n = (dx >= 0 || xb > 0u) && (dx <= 0 || xb + 1u < ex) && (dy >= 0 || yb > 0u) &&
                                  (dy <= 0 || yb + 1u < ey) && (dz >= 0 || zb > 0u);
                if (!crosses || !in_n) continue;
                // (index differences modulo 2^32; the voxels between two voxels of N are voxels of N)
                auto is_in = [&](int ax, int ay, int az) __attribute__((always_inline)) {
                    return label_load(P, l + (uint32_t)ax + ex * ((uint32_t)ay + ey * (uint32_t)az)) != 0u;
                };
                if (!is_in(dx, dy, dz) || label_diagonal_redundant(kLabelNb[k], is_in)) continue;
                label_unite(P, l, l + (uint32_t)dx + ex * ((uint32_t)dy + ey * (uint32_t)dz));
            }
        }
    }
}

// Pass 3.  A workgroup per chunk of kLabelChunk voxels: P[l] = 1 + the root above l (a root keeps
// its own; writing a root over a parent leaves every concurrent find a valid ancestor), so P holds
// the labels.  On the way the roots -- P[l] == l + 1, which this pass never changes -- become the
// root table: a bit per voxel in 64-bit words (a ballot each), the count of the chunk's roots
// before each word, and the chunk's count; the in voxels are counted into out[1].
__global__ __launch_bounds__(256) void label_flatten_kernel(const LabelArgs A)
{
    static_assert(kLabelChunk == 8192 && kLabelChunkWords == 128, "32 rounds of 256 lanes, 128 ballots");
    __shared__ unsigned long long s_m[kLabelChunkWords];
    __shared__ uint32_t s_tot[4], s_in[4];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * kLabelChunk;
    uint32_t *P = A.P;
    uint32_t nin = 0;
    for (uint32_t it = 0; it < 32u; ++it) {
        const uint64_t l64 = base + it * 256u + tid;
        bool root = false;
        if (l64 < (uint64_t)A.nvox) {
            const uint32_t l = (uint32_t)l64, p = label_load(P, l);
            if (p != 0u) {
                ++nin;
                root = p == l + 1u;
                if (!root) P[(size_t)l] = label_find(P, p - 1u) + 1u;
            }
        }
        const unsigned long long b = __ballot(root);
        if (lane == 0) s_m[it * 4u + wave] = b;
    }
    __syncthreads();
    const unsigned long long m = tid < kLabelChunkWords ? s_m[tid] : 0ull;
    const uint32_t cnt = (uint32_t)__popcll(m);
    uint32_t sc = cnt;  // inclusive over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t pv = __shfl_up(sc, off, 64);
        sc += (int)lane >= off ? pv : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nin += __shfl_xor(nin, off, 64);
    if (lane == 63) s_tot[wave] = sc;
    if (lane == 0) s_in[wave] = nin;
    __syncthreads();
    const uint32_t word = blockIdx.x * kLabelChunkWords + tid;
    if (tid < kLabelChunkWords && word < A.nwords) {
        A.mask[word] = m;
        A.wpre[word] = sc - cnt + (wave ? s_tot[0] : 0u);
    }
    if (tid == 0) {
        A.chunk[blockIdx.x] = s_tot[0] + s_tot[1];
        const uint32_t n = s_in[0] + s_in[1] + s_in[2] + s_in[3];
        if (n) atomicAdd(&A.out[1], (unsigned long long)n);
    }
}

// Pass 4a.  One workgroup: the chunks' root counts into their exclusive prefix, 256 chunks a round
// with a carry (at most 2^32 - 1 roots: 32 bits); the total into out[0], the components.
__global__ __launch_bounds__(256) void label_scan_chunks_kernel(const LabelArgs A)
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
    if (tid == 0) A.out[0] = carry;
}

// The record (vr_label_component, 64 bytes) as the table passes address it.
struct LabelRecord {
    uint32_t label, reserved;
    unsigned long long voxels;
    uint32_t bmin[3], bmax[3];
    unsigned long long sum[3];
};
static_assert(sizeof(LabelRecord) == kLabelComponentBytes, "vr_label_component");
// What a lane, a wave or a workgroup has gathered for one label.
struct LabelAcc {
    uint32_t cnt, mn[3], mx[3];
    unsigned long long sum[3];
};
__device__ __forceinline__ void label_acc_reset(LabelAcc &a)
{
    a.cnt = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.mn[k] = 0xFFFFFFFFu;
        a.mx[k] = 0u;
        a.sum[k] = 0ull;
    }
}
__device__ __forceinline__ void label_acc_merge(LabelAcc &a, const LabelAcc &b)
{
    a.cnt += b.cnt;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.mn[k] = b.mn[k] < a.mn[k] ? b.mn[k] : a.mn[k];
        a.mx[k] = b.mx[k] > a.mx[k] ? b.mx[k] : a.mx[k];
        a.sum[k] += b.sum[k];
    }
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off)
{
    const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}
// a over the lanes with `member` (the others give the identity); every lane of the wave calls it
__device__ __forceinline__ LabelAcc label_acc_wave(const LabelAcc &a, bool member)
{
    LabelAcc r;
    label_acc_reset(r);
    if (member) r = a;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        LabelAcc o;
        o.cnt = __shfl_xor(r.cnt, off, 64);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o.mn[k] = __shfl_xor(r.mn[k], off, 64);
            o.mx[k] = __shfl_xor(r.mx[k], off, 64);
            o.sum[k] = shfl_xor_u64(r.sum[k], off);
        }
        label_acc_merge(r, o);
    }
    return r;
}
// a into a record: integer atomics, mx already half open (index + 1).  (rec is null for a record
// index beyond the table, which no label of a flattened array has: nothing is written then.)
__device__ __forceinline__ void label_acc_flush(LabelRecord *rec, const LabelAcc &a)
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
__device__ __forceinline__ uint32_t label_rank(const LabelArgs &A, uint32_t lab)
{
    const uint32_t r = lab - 1u, w = r >> 6;
    return A.chunk[r / kLabelChunk] + A.wpre[w] + (uint32_t)__popcll(A.mask[w] & ((1ull << (r & 63u)) - 1ull));
}
__device__ __forceinline__ LabelRecord *label_record(const LabelArgs &A, uint32_t lab)
{
    const uint32_t i = label_rank(A, lab);
    return i < A.ncomps ? static_cast<LabelRecord *>(A.comps) + i : nullptr;
}
// Volume voxel index of box-linear index l.
__device__ __forceinline__ void label_coords(const LabelArgs &A, uint32_t l, uint32_t c[3])
{
    const uint32_t row = l / A.ext[0];
    c[0] = l - row * A.ext[0] + A.blo[0];
    const uint32_t zb = row / A.ext[1];
    c[1] = row - zb * A.ext[1] + A.blo[1];
    c[2] = zb + A.blo[2];
}

// Pass 4b.  The records before the sums: the identities of the reductions.
__global__ __launch_bounds__(256) void label_table_init_kernel(const LabelArgs A)
{
    LabelRecord *rec = static_cast<LabelRecord *>(A.comps);
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < (uint64_t)A.ncomps;
         i += (uint64_t)gridDim.x * 256u) {
        LabelRecord r;
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

// Pass 4c.  Count, bounding box and index sums per component.  A workgroup walks chunks
// (grid-stride), a lane keeps the sums of its current label in registers for as long as its voxels
// carry that label -- through a 15-million-voxel component, to the end -- and hands them on when
// the label changes: at most kLabelWaveRounds times the wave's first pending lane's label is
// combined over the lanes that share it and handed on by one lane, what is left goes singly.
// Handing on is an add into the workgroup's LDS slot of that label (kLabelSlots slots, claimed by a
// compare-and-swap on the slot's key; the label that finds its slot taken by another adds to its
// record in memory instead), and the slots go to the records once, at the workgroup's end: a large
// component, which every lane returns to after each speck it crosses, costs a workgroup one set
// of memory atomics instead of one per return.  Every sum is an integer, so no order shows in the
// result.  A root also stores its record's label.
constexpr int kLabelWaveRounds = 2;
constexpr uint32_t kLabelSlots = 64;
__global__ __launch_bounds__(256) void label_accum_kernel(const LabelArgs A)
{
    __shared__ LabelAcc s_acc[kLabelSlots];
    __shared__ uint32_t s_key[kLabelSlots];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t *__restrict__ P = A.P;
    if (tid < kLabelSlots) {
        s_key[tid] = 0u;
        label_acc_reset(s_acc[tid]);
    }
    __syncthreads();
    uint32_t key = 0;  // the label the lane gathers for; 0: none
    LabelAcc acc;
    label_acc_reset(acc);
    // r, gathered for label lab, into the label's slot or its record
    auto add = [&](uint32_t lab, const LabelAcc &r) __attribute__((always_inline)) {
        const uint32_t slot = (lab * 0x9E3779B1u) >> 26;
        static_assert(kLabelSlots == 64, "the hash keeps 6 bits");
        const uint32_t old = atomicCAS(&s_key[slot], 0u, lab);
        if (old == 0u || old == lab) {
            LabelAcc &t = s_acc[slot];
            atomicAdd(&t.cnt, r.cnt);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                atomicMin(&t.mn[k], r.mn[k]);
                atomicMax(&t.mx[k], r.mx[k]);
                atomicAdd(&t.sum[k], r.sum[k]);
            }
        } else {
            label_acc_flush(label_record(A, lab), r);
        }
    };
    // the lanes with `pend` hand their sums on; every lane of the wave calls it
    auto hand_on = [&](bool pend) __attribute__((always_inline)) {
#pragma unroll
        for (int round = 0; round < kLabelWaveRounds; ++round) {
            const unsigned long long todo = __ballot(pend);
            if (!todo) break;  // wave-uniform
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t lk = (uint32_t)__shfl((int)key, leader, 64);
            const bool same = pend && key == lk;
            const LabelAcc r = label_acc_wave(acc, same);
            if ((int)lane == leader) add(lk, r);
            if (same) {
                key = 0;
                label_acc_reset(acc);
            }
            pend = pend && !same;
        }
        if (pend) {
            add(key, acc);
            key = 0;
            label_acc_reset(acc);
        }
    };
    for (uint32_t ch = blockIdx.x; ch < A.nchunks; ch += gridDim.x) {
        const uint64_t base = (uint64_t)ch * kLabelChunk;
        for (uint32_t it = 0; it < 32u; ++it) {
            const uint64_t l64 = base + it * 256u + tid;
            const uint32_t l = (uint32_t)l64;
            const uint32_t lab = l64 < (uint64_t)A.nvox ? P[(size_t)l] : 0u;
            const bool change = lab != 0u && key != 0u && lab != key;
            if (__any(change)) hand_on(change);
            if (lab != 0u) {
                if (lab == l + 1u)
                    if (LabelRecord *own = label_record(A, lab)) own->label = lab;
                uint32_t c[3];
                label_coords(A, l, c);
                key = lab;
                ++acc.cnt;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    acc.mn[k] = c[k] < acc.mn[k] ? c[k] : acc.mn[k];
                    acc.mx[k] = c[k] + 1u > acc.mx[k] ? c[k] + 1u : acc.mx[k];
                    acc.sum[k] += c[k];
                }
            }
        }
    }
    hand_on(key != 0u);
    __syncthreads();
    if (tid < kLabelSlots && s_key[tid] != 0u) label_acc_flush(label_record(A, s_key[tid]), s_acc[tid]);
}

// Pass 4d.  The largest component: the maximum of voxels : ~label in 64 bits (most voxels, ties to
// the smallest label; a component has at most 2^32 - 1 voxels), into out[2].
__global__ __launch_bounds__(256) void label_largest_kernel(const LabelArgs A)
{
    const LabelRecord *rec = static_cast<const LabelRecord *>(A.comps);
    unsigned long long best = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < (uint64_t)A.ncomps;
         i += (uint64_t)gridDim.x * 256u) {
        const unsigned long long k = (rec[i].voxels << 32) | (unsigned long long)(~rec[i].label);
        best = k > best ? k : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = shfl_xor_u64(best, off);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63u) == 0 && best) atomicMax(&A.out[2], best);
}

// Region growing: the mask byte of every voxel of N (1 where the label is the seed's), and the
// seed's component's sums into record 0 -- per lane, per wave, per workgroup through LDS, then one
// lane's atomics.
__global__ __launch_bounds__(256) void label_grow_kernel(const LabelArgs A)
{
    __shared__ LabelAcc s_acc[4];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t *__restrict__ P = A.P;
    uint8_t *__restrict__ out = A.grow;
    LabelAcc acc;
    label_acc_reset(acc);
    for (uint64_t l64 = (uint64_t)blockIdx.x * 256u + tid; l64 < (uint64_t)A.nvox; l64 += (uint64_t)gridDim.x * 256u) {
        const uint32_t l = (uint32_t)l64;
        const bool hit = P[(size_t)l] == A.seed_label;
        out[(size_t)l] = hit ? (uint8_t)1 : (uint8_t)0;
        if (hit) {
            uint32_t c[3];
            label_coords(A, l, c);
            ++acc.cnt;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                acc.mn[k] = c[k] < acc.mn[k] ? c[k] : acc.mn[k];
                acc.mx[k] = c[k] + 1u > acc.mx[k] ? c[k] + 1u : acc.mx[k];
                acc.sum[k] += c[k];
            }
        }
    }
    const LabelAcc r = label_acc_wave(acc, true);
    if (lane == 0) s_acc[wave] = r;
    __syncthreads();
    if (tid == 0) {
        LabelAcc t = s_acc[0];
        for (uint32_t i = 1; i < 4u; ++i) label_acc_merge(t, s_acc[i]);
        label_acc_flush(static_cast<LabelRecord *>(A.comps), t);
    }
}

// One thread per brick: 0 if the brick can produce a visible sample, kSkipCap if EMPTY.
// Brick b is empty when every density d the trilinear filter can produce from its values maps
// to TF texels of alpha 0.  d lies in [lo, hi] up to the filter's rounding (3 levels of fmaf
// lerps: well under 1e-6 |d|), so the bounds are widened by kRangeMargin; t = (d - vmin) /
// range, u = t * n - 0.5 and floor are monotone, so the texels tf_lookup can touch are
// [floor(u(lo)), floor(u(hi)) + 1] clamped to [0, n - 1].  tf_nz is the prefix count of
// nonzero-alpha texels (n + 1 entries).  A sample whose alpha is lerp(0, 0, w) = 0 adds
// (rgb * 0) * T = +0 to C and leaves T unchanged: skipping it is exact.
__global__ __launch_bounds__(256) void classify_kernel(const float2 *__restrict__ range,
                                                       uint32_t nbricks,
                                                       const uint32_t *__restrict__ tf_nz,
                                                       int tf_n, float tf_nf, float vmin,
                                                       float vrange, uint8_t *__restrict__ dist)
{
    constexpr float kRangeMargin = 4.0e-6f;
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbricks) return;
    bool empty = false;
    if (vrange > 0.0f) {
        const float2 r = range[b];
        if (r.x == r.x && r.y == r.y) {  // no NaN in the brick
            const float m = (fabsf(r.x) + fabsf(r.y)) * kRangeMargin;
            const float t0 = ((r.x - m) - vmin) / vrange;
            const float t1 = ((r.y + m) - vmin) / vrange;
            float u0 = t0 * tf_nf - 0.5f, u1 = t1 * tf_nf - 0.5f;
            u0 = fminf(fmaxf(u0, -1.0f), tf_nf);
            u1 = fminf(fmaxf(u1, -1.0f), tf_nf);
            int i0 = (int)floorf(u0), i1 = (int)floorf(u1) + 1;
            i0 = i0 < 0 ? 0 : (i0 > tf_n - 1 ? tf_n - 1 : i0);
            i1 = i1 < 0 ? 0 : (i1 > tf_n - 1 ? tf_n - 1 : i1);
            empty = tf_nz[i1 + 1] == tf_nz[i0];
        }
    }
    dist[b] = empty ? (uint8_t)kSkipCap : (uint8_t)0;
}

// One separable pass of the Chebyshev (L-inf) distance transform of the non-empty bricks,
// along axis `axis`: out(b) = min over |o| <= kSkipCap of max(|o|, in(b + o e_axis)), capped.
// Three passes (x, y, z) from the classification give min(kSkipCap, distance in bricks to
// the nearest non-empty brick); bricks past the grid count as empty (a ray there has left
// the volume, and the march's bounds test ends it).
__global__ __launch_bounds__(256) void dist_pass_kernel(const uint8_t *__restrict__ in,
                                                        uint8_t *__restrict__ out, uint32_t nbx,
                                                        uint32_t nby, uint32_t nbz, int axis)
{
    const uint32_t nb = nbx * nby * nbz;
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const uint32_t bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
    const int pos = axis == 0 ? (int)bx : (axis == 1 ? (int)by : (int)bz);
    const int len = axis == 0 ? (int)nbx : (axis == 1 ? (int)nby : (int)nbz);
    const long stride = axis == 0 ? 1 : (axis == 1 ? (long)nbx : (long)nbx * nby);
    int best = in[b];
    for (int o = 1; o < kSkipCap && o < best; ++o) {
        if (pos - o >= 0) {
            const int v = in[b - o * stride];
            best = min(best, max(o, v));
        }
        if (pos + o < len) {
            const int v = in[b + o * stride];
            best = min(best, max(o, v));
        }
    }
    out[b] = (uint8_t)best;
}

// ---- rank-0 framebuffer assembly after the RCCL gather ---------------------------------------

template <typename PixT>
__global__ __launch_bounds__(256) void assemble_kernel(const PixT *__restrict__ gathered,
                                                       PixT *__restrict__ out, uint32_t W,
                                                       uint32_t H, uint32_t rb, uint32_t nranks,
                                                       uint32_t shard_rows, RowShare share)
{
    const size_t total = (size_t)W * H;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
         g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t y = (uint32_t)(g / W), x = (uint32_t)(g - (size_t)y * W);
        const uint32_t blk = y / rb;
        uint32_t rank, lb;
        share_owner(blk, nranks, share, rank, lb);
        const uint32_t ly = lb * rb + (y - blk * rb);
        out[g] = gathered[((size_t)rank * shard_rows + ly) * W + x];
    }
}

#ifdef VR_EXPERIMENTS
// Experiment builds only: dynamic LDS reserved per march workgroup (VR_MARCH_LDS_PAD bytes),
// which caps the workgroups resident on a CU -- fewer waves sharing its L1.
static uint32_t march_lds_pad()
{
    static const uint32_t v = [] {
        const char *e = std::getenv("VR_MARCH_LDS_PAD");
        return e ? (uint32_t)std::strtoul(e, nullptr, 10) : 0u;
    }();
    return v;
}
#else
constexpr uint32_t march_lds_pad() { return 0; }
#endif

// launch_frame: the kernels' storage type tags in VariantTag order (vr_variant.h), and one
// launcher per variant slot -- null where the library carries no such kernel (variant_built),
// so exactly the instantiations listed there exist.
using VariantTypes = std::tuple<uint8_t, int8_t, uint16_t, int16_t, float, Quad8<uint8_t>,
                                Quad8<int8_t>, F32Alt, F32H, F32P, F32S, F32Y, F32HY>;
static_assert(std::tuple_size<VariantTypes>::value == kVariantTags, "one type per VariantTag");
using FrameLauncher = void (*)(uint32_t nblocks, const MarchParams &, const MipArgs &, const IsoArgs &,
                               hipStream_t);

template <int I>
void launch_slot(uint32_t nblocks, const MarchParams &p, const MipArgs &m, const IsoArgs &iso,
                 hipStream_t stream)
{
    constexpr FrameVariant v = variant_at(I);
    using VT = std::tuple_element_t<v.tag, VariantTypes>;
    if constexpr (v.family == VF_MARCH)
        hipLaunchKernelGGL((march_kernel<VT, v.shade, v.count, v.skip, v.gf, v.pipe>), dim3(nblocks),
                           dim3(kThreadsPerTile), march_lds_pad(), stream, p);
    else if constexpr (v.family == VF_MARCH_Y)
        hipLaunchKernelGGL((march_y_kernel<VT, v.shade>), dim3(nblocks), dim3(kThreadsPerTile),
                           march_lds_pad(), stream, p);
    else if constexpr (v.family == VF_PAIR)
        hipLaunchKernelGGL((march_pair_kernel<VT, v.shade, v.gf, v.lanes>), dim3(nblocks),
                           dim3(kThreads), 0, stream, p);
    else if constexpr (v.family == VF_MIP)
        hipLaunchKernelGGL((mip_kernel<VT, v.count, v.skip, v.inflight>), dim3(nblocks),
                           dim3(kThreadsPerTile), 0, stream, p, m);
    else if constexpr (v.family == VF_PROJ)
        hipLaunchKernelGGL((proj_kernel<VT, v.op, v.count, v.skip, v.inflight>), dim3(nblocks),
                           dim3(kThreadsPerTile), 0, stream, p, ProjArgs{m.brick_range, m.nbricks});
    else
        hipLaunchKernelGGL((iso_kernel<VT, v.count, v.skip, v.inflight>), dim3(nblocks),
                           dim3(kThreadsPerTile), 0, stream, p, iso);
}

template <int I>
constexpr FrameLauncher slot_launcher()
{
    if constexpr (variant_built(variant_at(I)) && variant_index(variant_at(I)) == I)
        return &launch_slot<I>;
    else
        return nullptr;
}
template <int... I>
constexpr std::array<FrameLauncher, sizeof...(I)> slot_launchers(std::integer_sequence<int, I...>)
{
    return {{slot_launcher<I>()...}};
}

// workgroups for the per-brick kernels (brick_kernel, grad_field_kernel): one per brick
inline unsigned grid_bricks(size_t nb)
{
    return (unsigned)(nb > 65536 ? 65536 : (nb == 0 ? 1 : nb));
}

inline unsigned grid_for(size_t total)
{
    size_t g = (total + 255) / 256;
    return (unsigned)(g > 2048 * 8 ? 2048 * 8 : (g == 0 ? 1 : g));
}

// Readback (vr_debug_read_volume*): voxel v(x, y, z) is component 0 of element (x, y, z) of the
// bricked layout; slices [z0, z0 + cz) into a linear x-fastest buffer of the storage type.
template <typename T>
__global__ __launch_bounds__(256) void unbrick_kernel(const Vox<T> *__restrict__ bricks,
                                                     Vox<T> *__restrict__ dst, uint32_t nx,
                                                     uint32_t ny, uint32_t nbx, uint32_t nby,
                                                     uint32_t z0, size_t count)
{
    constexpr size_t vpe = std::is_same<T, float>::value ? kF32VoxelsPerElement
                                                         : (kPlainByte<T> ? 1 : 4);
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < count;
         g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t x = (uint32_t)(g % nx);
        const size_t yz = g / nx;
        const uint32_t y = (uint32_t)(yz % ny), z = z0 + (uint32_t)(yz / ny);
        const uint32_t pi = x + kPad, pj = y + kPad, pk = z + kPad;
        dst[g] = bricks[cell_offset<T>((int)pi, (int)pj, (int)pk, nbx, nby) * vpe];
    }
}

template <typename SrcT>
hipError_t brick_from(const void *src, void *dst, uint32_t nx, uint32_t ny, uint32_t nz,
                      int storage, hipStream_t s)
{
    const uint32_t nbx = bricks_for(nx, 0, storage), nby = bricks_for(ny, 1, storage),
                   nbz = bricks_for(nz, 2, storage);
    const size_t total = (size_t)nbx * nby * nbz;  // bricks
    const SrcT *sp = static_cast<const SrcT *>(src);
    switch (storage) {
        case ST_U8: hipLaunchKernelGGL((brick_kernel<SrcT, uint8_t>), dim3(grid_bricks(total)), dim3(256), 0, s, sp, (uint8_t *)dst, nx, ny, nz, nbx, nby, total); break;
        case ST_I8: hipLaunchKernelGGL((brick_kernel<SrcT, int8_t>), dim3(grid_bricks(total)), dim3(256), 0, s, sp, (int8_t *)dst, nx, ny, nz, nbx, nby, total); break;
        case ST_U8 | kQuadFlag: hipLaunchKernelGGL((brick_kernel<SrcT, Quad8<uint8_t>>), dim3(grid_bricks(total)), dim3(256), 0, s, sp, (uint8_t *)dst, nx, ny, nz, nbx, nby, total); break;
        case ST_I8 | kQuadFlag: hipLaunchKernelGGL((brick_kernel<SrcT, Quad8<int8_t>>), dim3(grid_bricks(total)), dim3(256), 0, s, sp, (int8_t *)dst, nx, ny, nz, nbx, nby, total); break;
        case ST_U16: hipLaunchKernelGGL((brick_kernel<SrcT, uint16_t>), dim3(grid_bricks(total)), dim3(256), 0, s, sp, (uint16_t *)dst, nx, ny, nz, nbx, nby, total); break;
        case ST_I16: hipLaunchKernelGGL((brick_kernel<SrcT, int16_t>), dim3(grid_bricks(total)), dim3(256), 0, s, sp, (int16_t *)dst, nx, ny, nz, nbx, nby, total); break;
        case ST_F32 | kAltFlag: hipLaunchKernelGGL((brick_kernel<SrcT, F32Alt>), dim3(grid_bricks(total)), dim3(256), 0, s, sp, (float *)dst, nx, ny, nz, nbx, nby, total); break;
        case ST_F32 | kPlainF32Flag: hipLaunchKernelGGL((brick_kernel<SrcT, F32P>), dim3(grid_bricks(total)), dim3(256), 0, s, sp, (float *)dst, nx, ny, nz, nbx, nby, total); break;
        case ST_F32 | kStencilF32Flag: hipLaunchKernelGGL((brick_kernel<SrcT, F32S>), dim3(grid_bricks(total)), dim3(256), 0, s, sp, (float *)dst, nx, ny, nz, nbx, nby, total); break;
        default: hipLaunchKernelGGL((brick_kernel<SrcT, float>), dim3(grid_bricks(total)), dim3(256), 0, s, sp, (float *)dst, nx, ny, nz, nbx, nby, total); break;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_frame(const FrameVariant &v, const MarchParams &p, const MipArgs &m,
                        const IsoArgs &iso, hipStream_t stream)
{
    static constexpr auto launchers = slot_launchers(std::make_integer_sequence<int, kVariantSlots>{});
    const int i = variant_index(v);
    const FrameLauncher fn = i >= 0 && i < kVariantSlots ? launchers[(size_t)i] : nullptr;
    if (!fn || ((v.family == VF_MIP || v.family == VF_PROJ) && v.skip && !m.brick_range) ||
        (v.family == VF_ISO && v.skip && !iso.brick_range))
        return hipErrorInvalidValue;
    if (p.tiles_x * p.tiles_y == 0) return hipSuccess;
    const uint32_t nblocks = p.tile_perm ? p.nperm
                             : p.tile_order >= 3 ? ((p.supers_total + 7) / 8) * 8 * kSuper * kSuper
                                                 : p.tiles_x * p.tiles_y;
    fn(nblocks, p, m, iso, stream);
    return hipGetLastError();
}

namespace {
template <typename VT>
void launch_mpr_tag(const MprArgs &a, uint32_t nblocks, hipStream_t stream)
{
    const dim3 grid(nblocks), block(kTile * kTile);
    if (a.nsamples == 1)
        hipLaunchKernelGGL((mpr_kernel<VT, kMprThin, false>), grid, block, 0, stream, a);
    else if (a.op == kMprMax)
        hipLaunchKernelGGL((mpr_kernel<VT, kMprMax, false>), grid, block, 0, stream, a);
    else if (a.op == kMprMin)
        hipLaunchKernelGGL((mpr_kernel<VT, kMprMin, false>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((mpr_kernel<VT, kMprMean, false>), grid, block, 0, stream, a);
}
}  // namespace

hipError_t launch_mpr(int layout, bool count, const MprArgs &a, hipStream_t stream, std::string *name)
{
    const int tag = layout >= ST_U8 && layout <= ST_F32 ? layout
                    : layout == (ST_U8 | kQuadFlag)     ? (int)TAG_QUAD_U8
                    : layout == (ST_I8 | kQuadFlag)     ? (int)TAG_QUAD_I8
                                                        : -1;
    if (tag < 0 || a.op < kMprMax || a.op > kMprMean || a.nsamples == 0) return hipErrorInvalidValue;
    if (name)
        *name = std::string("void vr::(anonymous namespace)::mpr_kernel<") + kTagNames[count ? (int)TAG_F32 : tag] +
                ", " + std::to_string(count ? kMprMax : a.nsamples == 1 ? kMprThin : a.op) +
                (count ? ", true" : ", false") + ">(vr::MprArgs)";
    const unsigned long long tiles = (unsigned long long)a.tiles_x * a.tiles_y;
    if (tiles == 0) return hipSuccess;
    if (tiles >= 1ull << 31) return hipErrorInvalidValue;
    // order 3: whole super-tiles, dealt over the 8 XCDs (launch_frame's grid)
    const unsigned long long padded = ((a.supers_total + 7ull) / 8) * 8 * kSuper * kSuper;
    if (a.tile_order == 3 && padded >= 1ull << 31) return hipErrorInvalidValue;
    const uint32_t nblocks = a.tile_order == 3 ? (uint32_t)padded : (uint32_t)tiles;
    if (count) {
        hipLaunchKernelGGL((mpr_kernel<float, kMprMax, true>), dim3(nblocks), dim3(kTile * kTile), 0,
                           stream, a);
        return hipGetLastError();
    }
    switch (tag) {
        case TAG_U8: launch_mpr_tag<uint8_t>(a, nblocks, stream); break;
        case TAG_I8: launch_mpr_tag<int8_t>(a, nblocks, stream); break;
        case TAG_U16: launch_mpr_tag<uint16_t>(a, nblocks, stream); break;
        case TAG_I16: launch_mpr_tag<int16_t>(a, nblocks, stream); break;
        case TAG_F32: launch_mpr_tag<float>(a, nblocks, stream); break;
        case TAG_QUAD_U8: launch_mpr_tag<Quad8<uint8_t>>(a, nblocks, stream); break;
        default: launch_mpr_tag<Quad8<int8_t>>(a, nblocks, stream); break;
    }
    return hipGetLastError();
}

namespace {
template <typename VT>
void launch_hist_tag(bool agg, const HistArgs &a, uint32_t nblocks, hipStream_t stream)
{
    if (agg)
        hipLaunchKernelGGL((hist_kernel<VT, true>), dim3(nblocks), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((hist_kernel<VT, false>), dim3(nblocks), dim3(256), 0, stream, a);
}
}  // namespace

hipError_t launch_hist(int layout, bool agg, const HistArgs &a, hipStream_t stream, std::string *name)
{
    const int tag = layout >= ST_U8 && layout <= ST_F32 ? layout
                    : layout == (ST_U8 | kQuadFlag)     ? (int)TAG_QUAD_U8
                    : layout == (ST_I8 | kQuadFlag)     ? (int)TAG_QUAD_I8
                                                        : -1;
    if (tag < 0 || a.nwork == 0 || a.nbins == 0 || a.nbins > kHistMaxBins) return hipErrorInvalidValue;
    if (name)
        *name = std::string("void vr::(anonymous namespace)::hist_kernel<") + kTagNames[tag] +
                (agg ? ", true" : ", false") + ">(vr::HistArgs)";
    // (the code path of plain 8-bit bricks walks a brick per wave: four per workgroup)
    const uint32_t groups = (tag == TAG_U8 && kHistCodes<uint8_t>) || (tag == TAG_I8 && kHistCodes<int8_t>)
                                ? (a.nwork + 3) / 4 : a.nwork;
    const uint32_t nblocks = groups < kHistMaxGrid ? groups : kHistMaxGrid;
    switch (tag) {
        case TAG_U8: launch_hist_tag<uint8_t>(agg, a, nblocks, stream); break;
        case TAG_I8: launch_hist_tag<int8_t>(agg, a, nblocks, stream); break;
        case TAG_U16: launch_hist_tag<uint16_t>(agg, a, nblocks, stream); break;
        case TAG_I16: launch_hist_tag<int16_t>(agg, a, nblocks, stream); break;
        case TAG_F32: launch_hist_tag<float>(agg, a, nblocks, stream); break;
        case TAG_QUAD_U8: launch_hist_tag<Quad8<uint8_t>>(agg, a, nblocks, stream); break;
        default: launch_hist_tag<Quad8<int8_t>>(agg, a, nblocks, stream); break;
    }
    return hipGetLastError();
}

namespace {
int mesh_tag(int layout)
{
    return layout >= ST_U8 && layout <= ST_F32     ? layout
           : layout == (ST_U8 | kQuadFlag)         ? (int)TAG_QUAD_U8
           : layout == (ST_I8 | kQuadFlag)         ? (int)TAG_QUAD_I8
                                                   : -1;
}
// pass: 0 classify, 1 vertices, 2 vertices with normals, 3 quads
template <typename VT>
void launch_mesh_tag(int pass, const MeshArgs &a, uint32_t nblocks, hipStream_t stream)
{
    const dim3 grid(nblocks), block(256);
    if (pass == 0)
        hipLaunchKernelGGL((mesh_classify_kernel<VT>), grid, block, 0, stream, a);
    else if (pass == 1)
        hipLaunchKernelGGL((mesh_vertex_kernel<VT, false>), grid, block, 0, stream, a);
    else if (pass == 2)
        hipLaunchKernelGGL((mesh_vertex_kernel<VT, true>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((mesh_quad_kernel<VT>), grid, block, 0, stream, a);
}
hipError_t launch_mesh_pass(int layout, int pass, const MeshArgs &a, hipStream_t stream)
{
    const int tag = mesh_tag(layout);
    if (tag < 0 || a.nwork == 0) return hipErrorInvalidValue;
    const uint32_t nblocks = a.nwork < kMeshMaxGrid ? a.nwork : kMeshMaxGrid;
    switch (tag) {
        case TAG_U8: launch_mesh_tag<uint8_t>(pass, a, nblocks, stream); break;
        case TAG_I8: launch_mesh_tag<int8_t>(pass, a, nblocks, stream); break;
        case TAG_U16: launch_mesh_tag<uint16_t>(pass, a, nblocks, stream); break;
        case TAG_I16: launch_mesh_tag<int16_t>(pass, a, nblocks, stream); break;
        case TAG_F32: launch_mesh_tag<float>(pass, a, nblocks, stream); break;
        case TAG_QUAD_U8: launch_mesh_tag<Quad8<uint8_t>>(pass, a, nblocks, stream); break;
        default: launch_mesh_tag<Quad8<int8_t>>(pass, a, nblocks, stream); break;
    }
    return hipGetLastError();
}
}  // namespace

hipError_t launch_mesh_classify(int layout, const MeshArgs &a, hipStream_t stream, std::string *name)
{
    const int tag = mesh_tag(layout);
    if (tag < 0 || a.nwork == 0 || a.nchunks != (a.nwork + kMeshChunk - 1) / kMeshChunk)
        return hipErrorInvalidValue;
    if (name)
        *name = std::string("void vr::(anonymous namespace)::mesh_classify_kernel<") + kTagNames[tag] +
                ">(vr::MeshArgs)";
    if (hipError_t e = launch_mesh_pass(layout, 0, a, stream)) return e;
    hipLaunchKernelGGL(mesh_scan_bricks_kernel, dim3(a.nchunks), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(mesh_scan_chunks_kernel, dim3(1), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_mesh_vertices(int layout, bool normals, const MeshArgs &a, hipStream_t stream)
{
    return launch_mesh_pass(layout, normals ? 2 : 1, a, stream);
}

hipError_t launch_mesh_quads(int layout, const MeshArgs &a, hipStream_t stream)
{
    return launch_mesh_pass(layout, 3, a, stream);
}

namespace {
template <typename VT>
void launch_label_tag(int connectivity, int pass, const LabelArgs &a, uint32_t nlocal, uint32_t nseam,
                      hipStream_t stream)
{
    using G = GeomOf<VT>;
    if (connectivity == 6) {
        if (pass == 0) hipLaunchKernelGGL((label_local_kernel<VT, 6>), dim3(nlocal), dim3(256), 0, stream, a);
        if (pass == 1) hipLaunchKernelGGL((label_seam_kernel<6, G>), dim3(nseam), dim3(256), 0, stream, a);
    } else {
        if (pass == 0) hipLaunchKernelGGL((label_local_kernel<VT, 26>), dim3(nlocal), dim3(256), 0, stream, a);
        if (pass == 1) hipLaunchKernelGGL((label_seam_kernel<26, G>), dim3(nseam), dim3(256), 0, stream, a);
    }
}
}  // namespace

hipError_t launch_label(int layout, int connectivity, int pass, const LabelArgs &a, hipStream_t stream,
                        std::string *name)
{
    const int tag = mesh_tag(layout);
    if (pass < 0 || pass >= kLabelPasses || tag < 0 || a.nwork == 0 || a.nvox == 0 || (connectivity != 6 && connectivity != 26) ||
        a.nchunks != (uint32_t)(((uint64_t)a.nvox + kLabelChunk - 1) / kLabelChunk))
        return hipErrorInvalidValue;
    if (name)
        *name = std::string("void vr::(anonymous namespace)::label_local_kernel<") + kTagNames[tag] + ", " +
                std::to_string(connectivity) + ">(vr::LabelArgs)";
    const uint32_t nlocal = a.nwork < kLabelMaxGrid ? a.nwork : kLabelMaxGrid;
    const uint64_t rowgroups = ((uint64_t)a.ext[1] * a.ext[2] + 3) / 4;
    const uint32_t nseam = rowgroups < kLabelMaxGrid ? (uint32_t)rowgroups : kLabelMaxGrid;
    if (pass == 2) hipLaunchKernelGGL(label_flatten_kernel, dim3(a.nchunks), dim3(256), 0, stream, a);
    if (pass == 3) hipLaunchKernelGGL(label_scan_chunks_kernel, dim3(1), dim3(256), 0, stream, a);
    if (pass >= 2) return hipGetLastError();
    switch (tag) {
        case TAG_U8: launch_label_tag<uint8_t>(connectivity, pass, a, nlocal, nseam, stream); break;
        case TAG_I8: launch_label_tag<int8_t>(connectivity, pass, a, nlocal, nseam, stream); break;
        case TAG_U16: launch_label_tag<uint16_t>(connectivity, pass, a, nlocal, nseam, stream); break;
        case TAG_I16: launch_label_tag<int16_t>(connectivity, pass, a, nlocal, nseam, stream); break;
        case TAG_F32: launch_label_tag<float>(connectivity, pass, a, nlocal, nseam, stream); break;
        case TAG_QUAD_U8: launch_label_tag<Quad8<uint8_t>>(connectivity, pass, a, nlocal, nseam, stream); break;
        default: launch_label_tag<Quad8<int8_t>>(connectivity, pass, a, nlocal, nseam, stream); break;
    }
    return hipGetLastError();
}

hipError_t launch_label_table(int pass, const LabelArgs &a, hipStream_t stream)
{
    if (pass < 0 || pass > 2 || a.ncomps == 0 || !a.comps) return hipErrorInvalidValue;
    const uint32_t per = (a.ncomps + 255u) / 256u;
    const uint32_t ninit = per < kLabelMaxGrid ? per : kLabelMaxGrid;
    const uint32_t nacc = a.nchunks < kLabelMaxGrid ? a.nchunks : kLabelMaxGrid;
    if (pass == 0) hipLaunchKernelGGL(label_table_init_kernel, dim3(ninit), dim3(256), 0, stream, a);
    if (pass == 1) hipLaunchKernelGGL(label_accum_kernel, dim3(nacc), dim3(256), 0, stream, a);
    if (pass == 2) hipLaunchKernelGGL(label_largest_kernel, dim3(ninit), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_label_grow(const LabelArgs &a, hipStream_t stream)
{
    if (a.nvox == 0 || !a.grow || !a.comps || a.seed_label == 0) return hipErrorInvalidValue;
    const uint64_t per = ((uint64_t)a.nvox + 255u) / 256u;
    const uint32_t n = per < kLabelMaxGrid ? (uint32_t)per : kLabelMaxGrid;
    hipLaunchKernelGGL(label_grow_kernel, dim3(n), dim3(256), 0, stream, a);
    return hipGetLastError();
}

namespace {
template <typename VT, int KIND>
void launch_hit_kind(bool count, int inflight, const MarchParams &p, const HitArgs &a, uint32_t nblocks,
                     hipStream_t stream)
{
    const dim3 grid(nblocks), block(kThreadsPerTile);
    if (count)
        hipLaunchKernelGGL((hit_kernel<VT, KIND, true, 1>), grid, block, 0, stream, p, a);
    else if (inflight == 2)
        hipLaunchKernelGGL((hit_kernel<VT, KIND, false, 2>), grid, block, 0, stream, p, a);
    else
        hipLaunchKernelGGL((hit_kernel<VT, KIND, false, 1>), grid, block, 0, stream, p, a);
}
template <typename VT>
void launch_hit_tag(int kind, bool count, int inflight, const MarchParams &p, const HitArgs &a,
                    uint32_t nblocks, hipStream_t stream)
{
    switch (kind) {
        case kHitEntry: launch_hit_kind<VT, kHitEntry>(count, inflight, p, a, nblocks, stream); break;
        case kHitOpacity: launch_hit_kind<VT, kHitOpacity>(count, inflight, p, a, nblocks, stream); break;
        case kHitMax: launch_hit_kind<VT, kHitMax>(count, inflight, p, a, nblocks, stream); break;
        case kHitMin: launch_hit_kind<VT, kHitMin>(count, inflight, p, a, nblocks, stream); break;
        default: launch_hit_kind<VT, kHitIso>(count, inflight, p, a, nblocks, stream); break;
    }
}
}  // namespace

hipError_t launch_hit(int layout, int kind, bool count, int inflight, const MarchParams &p,
                      const HitArgs &a, hipStream_t stream, std::string *name)
{
    const int tag = layout >= ST_U8 && layout <= ST_F32 ? layout
                    : layout == (ST_U8 | kQuadFlag)     ? (int)TAG_QUAD_U8
                    : layout == (ST_I8 | kQuadFlag)     ? (int)TAG_QUAD_I8
                                                        : -1;
    if (count) inflight = 1;
    if (tag < 0 || kind < 0 || kind >= kHitKinds || (inflight != 1 && inflight != 2) ||
        p.tile_order != 3 || p.tile_perm)
        return hipErrorInvalidValue;
    if (name)
        *name = std::string("void vr::(anonymous namespace)::hit_kernel<") + kTagNames[tag] + ", " +
                std::to_string(kind) + (count ? ", true, " : ", false, ") + std::to_string(inflight) +
                ">(vr::MarchParams, vr::HitArgs)";
    if (p.tiles_x * p.tiles_y == 0) return hipSuccess;
    // order 3: whole super-tiles, dealt over the 8 XCDs (launch_frame's grid)
    const unsigned long long padded = ((p.supers_total + 7ull) / 8) * 8 * kSuper * kSuper;
    if (padded >= 1ull << 31) return hipErrorInvalidValue;
    const uint32_t nblocks = (uint32_t)padded;
    switch (tag) {
        case TAG_U8: launch_hit_tag<uint8_t>(kind, count, inflight, p, a, nblocks, stream); break;
        case TAG_I8: launch_hit_tag<int8_t>(kind, count, inflight, p, a, nblocks, stream); break;
        case TAG_U16: launch_hit_tag<uint16_t>(kind, count, inflight, p, a, nblocks, stream); break;
        case TAG_I16: launch_hit_tag<int16_t>(kind, count, inflight, p, a, nblocks, stream); break;
        case TAG_F32: launch_hit_tag<float>(kind, count, inflight, p, a, nblocks, stream); break;
        case TAG_QUAD_U8: launch_hit_tag<Quad8<uint8_t>>(kind, count, inflight, p, a, nblocks, stream); break;
        default: launch_hit_tag<Quad8<int8_t>>(kind, count, inflight, p, a, nblocks, stream); break;
    }
    return hipGetLastError();
}

hipError_t launch_range_max(float2 *range_dev, uint32_t nbricks, hipStream_t s)
{
    hipLaunchKernelGGL(range_max_kernel, dim3(1), dim3(256), 0, s, range_dev, nbricks);
    return hipGetLastError();
}

hipError_t launch_unbrick(int storage, const void *bricks, void *dst, uint32_t nx, uint32_t ny,
                          uint32_t z0, uint32_t cz, hipStream_t s)
{
    const size_t n = (size_t)nx * ny * cz;
    const unsigned g = grid_for(n);
    const uint32_t bx = bricks_for(nx, 0, storage), by = bricks_for(ny, 1, storage);
    switch (storage) {
        case ST_U8: case ST_I8: hipLaunchKernelGGL((unbrick_kernel<uint8_t>), dim3(g), dim3(256), 0, s, (const uint8_t *)bricks, (uint8_t *)dst, nx, ny, bx, by, z0, n); break;
        case ST_U8 | kQuadFlag: case ST_I8 | kQuadFlag: hipLaunchKernelGGL((unbrick_kernel<Quad8<uint8_t>>), dim3(g), dim3(256), 0, s, (const uint8_t *)bricks, (uint8_t *)dst, nx, ny, bx, by, z0, n); break;
        case ST_U16: case ST_I16: hipLaunchKernelGGL((unbrick_kernel<uint16_t>), dim3(g), dim3(256), 0, s, (const uint16_t *)bricks, (uint16_t *)dst, nx, ny, bx, by, z0, n); break;
        default: hipLaunchKernelGGL((unbrick_kernel<float>), dim3(g), dim3(256), 0, s, (const float *)bricks, (float *)dst, nx, ny, bx, by, z0, n); break;
    }
    return hipGetLastError();
}

hipError_t launch_brick_from_linear(int src_dtype, const void *src, void *dst, uint32_t nx,
                                    uint32_t ny, uint32_t nz, int storage, hipStream_t s)
{
    switch (src_dtype) {  // enum vr_dtype
        case 1: return brick_from<int8_t>(src, dst, nx, ny, nz, storage, s);
        case 2: return brick_from<uint8_t>(src, dst, nx, ny, nz, storage, s);
        case 3: return brick_from<int16_t>(src, dst, nx, ny, nz, storage, s);
        case 4: return brick_from<uint16_t>(src, dst, nx, ny, nz, storage, s);
        case 5: return brick_from<int32_t>(src, dst, nx, ny, nz, storage, s);
        case 6: return brick_from<uint32_t>(src, dst, nx, ny, nz, storage, s);
        case 7: return brick_from<int64_t>(src, dst, nx, ny, nz, storage, s);
        case 8: return brick_from<uint64_t>(src, dst, nx, ny, nz, storage, s);
        case 9: return brick_from<float>(src, dst, nx, ny, nz, storage, s);
        case 10: return brick_from<double>(src, dst, nx, ny, nz, storage, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_generate(int kind, int storage, void *dst, uint32_t nx, uint32_t ny,
                           uint32_t nz, const float *params_dev, int nparams, hipStream_t s)
{
    (void)nparams;
    if (kind != 0) return hipErrorInvalidValue;
    const size_t total = (size_t)nx * ny * nz;
    switch (storage) {
        case ST_U8: hipLaunchKernelGGL((generate_kernel<uint8_t>), dim3(grid_for(total)), dim3(256), 0, s, (uint8_t *)dst, nx, ny, total, params_dev); break;
        case ST_U16: hipLaunchKernelGGL((generate_kernel<uint16_t>), dim3(grid_for(total)), dim3(256), 0, s, (uint16_t *)dst, nx, ny, total, params_dev); break;
        case ST_F32: hipLaunchKernelGGL((generate_kernel<float>), dim3(grid_for(total)), dim3(256), 0, s, (float *)dst, nx, ny, total, params_dev); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_minmax(int storage, const void *linear, size_t count, float *minmax_dev,
                         hipStream_t s)
{
    uint32_t *o = reinterpret_cast<uint32_t *>(minmax_dev);
    const unsigned g = std::min(grid_for(count), 2048u);  // 8 workgroups per CU, grid-stride
    switch (storage) {
        case ST_U8: hipLaunchKernelGGL((minmax_kernel<uint8_t>), dim3(g), dim3(256), 0, s, (const uint8_t *)linear, count, o); break;
        case ST_I8: hipLaunchKernelGGL((minmax_kernel<int8_t>), dim3(g), dim3(256), 0, s, (const int8_t *)linear, count, o); break;
        case ST_U16: hipLaunchKernelGGL((minmax_kernel<uint16_t>), dim3(g), dim3(256), 0, s, (const uint16_t *)linear, count, o); break;
        case ST_I16: hipLaunchKernelGGL((minmax_kernel<int16_t>), dim3(g), dim3(256), 0, s, (const int16_t *)linear, count, o); break;
        default: hipLaunchKernelGGL((minmax_kernel<float>), dim3(g), dim3(256), 0, s, (const float *)linear, count, o); break;
    }
    return hipGetLastError();
}

hipError_t launch_int_range(int src_dtype, const void *src, size_t count, int *out3_dev,
                            hipStream_t s)
{
    const unsigned g = std::min(grid_for(count), 2048u);  // 8 workgroups per CU, grid-stride
    switch (src_dtype) {  // enum vr_dtype: the 32/64-bit types NrrdFileParser makes float
        case 5: hipLaunchKernelGGL((int_range_kernel<int32_t>), dim3(g), dim3(256), 0, s, (const int32_t *)src, count, out3_dev); break;
        case 6: hipLaunchKernelGGL((int_range_kernel<uint32_t>), dim3(g), dim3(256), 0, s, (const uint32_t *)src, count, out3_dev); break;
        case 7: hipLaunchKernelGGL((int_range_kernel<int64_t>), dim3(g), dim3(256), 0, s, (const int64_t *)src, count, out3_dev); break;
        case 8: hipLaunchKernelGGL((int_range_kernel<uint64_t>), dim3(g), dim3(256), 0, s, (const uint64_t *)src, count, out3_dev); break;
        case 9: hipLaunchKernelGGL((int_range_kernel<float>), dim3(g), dim3(256), 0, s, (const float *)src, count, out3_dev); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_assemble(const void *gathered, void *out, int out_format, uint32_t W,
                           uint32_t H, uint32_t row_block, uint32_t nranks,
                           uint32_t shard_rows, RowShare share, hipStream_t s)
{
    const unsigned g = grid_for((size_t)W * H);
    if (out_format == 0)
        hipLaunchKernelGGL((assemble_kernel<uint32_t>), dim3(g), dim3(256), 0, s,
                           (const uint32_t *)gathered, (uint32_t *)out, W, H, row_block, nranks,
                           shard_rows, share);
    else
        hipLaunchKernelGGL((assemble_kernel<float4>), dim3(g), dim3(256), 0, s,
                           (const float4 *)gathered, (float4 *)out, W, H, row_block, nranks,
                           shard_rows, share);
    return hipGetLastError();
}

hipError_t launch_brick_range(int storage, const void *bricks, uint32_t nbx, uint32_t nby,
                              uint32_t nbz, float2 *range_dev, hipStream_t s)
{
    const uint32_t nbricks = nbx * nby * nbz;
    const unsigned g = (nbricks + 3) / 4;
    const uint32_t per = (uint32_t)(brick_elems(storage) * voxels_per_element(storage));
    switch (storage & 0xF) {  // the voxels of every element, whatever the layout
        case ST_U8: hipLaunchKernelGGL((brick_range_kernel<uint8_t>), dim3(g), dim3(256), 0, s, (const uint8_t *)bricks, nbricks, per, nbx, nby, range_dev); break;
        case ST_I8: hipLaunchKernelGGL((brick_range_kernel<int8_t>), dim3(g), dim3(256), 0, s, (const int8_t *)bricks, nbricks, per, nbx, nby, range_dev); break;
        case ST_U16: hipLaunchKernelGGL((brick_range_kernel<uint16_t>), dim3(g), dim3(256), 0, s, (const uint16_t *)bricks, nbricks, per, nbx, nby, range_dev); break;
        case ST_I16: hipLaunchKernelGGL((brick_range_kernel<int16_t>), dim3(g), dim3(256), 0, s, (const int16_t *)bricks, nbricks, per, nbx, nby, range_dev); break;
        default: hipLaunchKernelGGL((brick_range_kernel<float>), dim3(g), dim3(256), 0, s, (const float *)bricks, nbricks, per, nbx, nby, range_dev); break;
    }
    return hipGetLastError();
}

hipError_t launch_grad_field(const float *bricks, float *grad, uint32_t nx, uint32_t ny,
                             uint32_t nz, bool half, int scale_log2, bool ymajor, hipStream_t s)
{
    if (ymajor && !half) return hipErrorInvalidValue;  // the y-major field is binary16 only
    const uint32_t nbx = bricks_for(nx, 0, ST_F32), nby = bricks_for(ny, 1, ST_F32),
                   nbz = bricks_for(nz, 2, ST_F32);
    const size_t total = (size_t)nbx * nby * nbz;  // bricks
    const float scale = std::ldexp(1.0f, scale_log2);
    if (half)
        hipLaunchKernelGGL(grad_field_kernel<true>, dim3(grid_bricks(total)), dim3(256), 0, s,
                           bricks, grad, nx, ny, nz, nbx, nby, total, scale, ymajor ? 1u : 0u);
    else
        hipLaunchKernelGGL(grad_field_kernel<false>, dim3(grid_bricks(total)), dim3(256), 0, s,
                           bricks, grad, nx, ny, nz, nbx, nby, total, scale, 0u);
    return hipGetLastError();
}

hipError_t launch_rebrick_f32(const float *src_bricks, void *dst, uint32_t nx, uint32_t ny,
                              uint32_t nz, int storage, hipStream_t s)
{
    const uint32_t snbx = bricks_for(nx, 0, ST_F32), snby = bricks_for(ny, 1, ST_F32),
                   snbz = bricks_for(nz, 2, ST_F32);
    const uint32_t nbx = bricks_for(nx, 0, storage), nby = bricks_for(ny, 1, storage),
                   nbz = bricks_for(nz, 2, storage);
    const size_t total = (size_t)nbx * nby * nbz;
    float *d = static_cast<float *>(dst);
    switch (storage) {
        case ST_F32 | kAltFlag: hipLaunchKernelGGL((rebrick_f32_kernel<F32Alt>), dim3(grid_bricks(total)), dim3(256), 0, s, src_bricks, d, nx, ny, nz, snbx, snby, snbz, nbx, nby, total); break;
        case ST_F32 | kPlainF32Flag: hipLaunchKernelGGL((rebrick_f32_kernel<F32P>), dim3(grid_bricks(total)), dim3(256), 0, s, src_bricks, d, nx, ny, nz, snbx, snby, snbz, nbx, nby, total); break;
        case ST_F32 | kStencilF32Flag: hipLaunchKernelGGL((rebrick_f32_kernel<F32S>), dim3(grid_bricks(total)), dim3(256), 0, s, src_bricks, d, nx, ny, nz, snbx, snby, snbz, nbx, nby, total); break;
        case ST_F32 | kYMajorFlag: hipLaunchKernelGGL(rebrick_ymajor_kernel, dim3(grid_bricks(total)), dim3(256), 0, s, src_bricks, reinterpret_cast<float2 *>(d), nx, ny, nz, snbx, snby, total); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_skip_dist(const float2 *range_dev, uint32_t nbx, uint32_t nby, uint32_t nbz,
                            const uint32_t *tf_nz_dev, int tf_n, float vmin, float vrange,
                            uint8_t *dist_dev, uint8_t *scratch_dev, hipStream_t s)
{
    const uint32_t nb = nbx * nby * nbz;
    const unsigned g = (nb + 255) / 256;
    hipLaunchKernelGGL(classify_kernel, dim3(g), dim3(256), 0, s, range_dev, nb, tf_nz_dev, tf_n,
                       (float)tf_n, vmin, vrange, dist_dev);
    hipLaunchKernelGGL(dist_pass_kernel, dim3(g), dim3(256), 0, s, (const uint8_t *)dist_dev,
                       scratch_dev, nbx, nby, nbz, 0);
    hipLaunchKernelGGL(dist_pass_kernel, dim3(g), dim3(256), 0, s, (const uint8_t *)scratch_dev,
                       dist_dev, nbx, nby, nbz, 1);
    hipLaunchKernelGGL(dist_pass_kernel, dim3(g), dim3(256), 0, s, (const uint8_t *)dist_dev,
                       scratch_dev, nbx, nby, nbz, 2);
    return hipMemcpyAsync(dist_dev, scratch_dev, nb, hipMemcpyDeviceToDevice, s);
}

#ifdef VR_WG_TIMES
hipError_t debug_wg_times_reset()
{
    const unsigned int z = 0;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_wg_count), &z, sizeof(z));
}
hipError_t debug_wg_times_read(unsigned long long *out, unsigned int max, unsigned int *count)
{
    unsigned int n = 0;
    hipError_t e = hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_wg_count), sizeof(n));
    if (e != hipSuccess) return e;
    n = n < kWgTimesMax ? n : kWgTimesMax;
    n = n < max ? n : max;
    *count = n;
    return n ? hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_times), 4 * n * sizeof(unsigned long long))
             : hipSuccess;
}
#endif

hipError_t launch_order_tiles(const uint32_t *cost, const uint32_t *lists, uint32_t *perm,
                              uint32_t per_xcd, hipStream_t s)
{
    hipLaunchKernelGGL(order_tiles_kernel, dim3(8), dim3(256), 0, s, cost, lists, perm, per_xcd);
    return hipGetLastError();
}

}  // namespace vr
