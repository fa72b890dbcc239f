// vr_internal.h — shared definitions between the C-ABI layer (vr_api.hip) and the
// gfx950 kernels (vr_kernels.hip).  Not installed; the public boundary is include/vr/vr.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <type_traits>

#include "vr_hist_host.h"
#include "vr_hit_host.h"
#include "vr_label_host.h"
#include "vr_mesh_host.h"
#include "vr_variant.h"

namespace vr {

// ---- Bricked volume layout in HBM ----------------------------------------------------------
// The logical volume (nx, ny, nz) is shifted by kPad = 2 zero voxels on the low side of each
// axis ("padded index" p = logical + 2) and cut into bricks of BX x BY x BZ cells (BrickGeom
// below).  A brick stores ELEMENTS for padded indices [B b, B b + B] on each axis (B + 1: a
// 1-element apron), bricks in brick_slot order, elements x-fastest in a brick, so every
// trilinear footprint lies in one brick.  Per storage type:
//   f32 (and 32/64-bit inputs, converted): "z-pair" element = {v(x,y,z), v(x,y,z+1)}, 8 B, in
//         8^3-cell bricks; a sample = 2 x 16-B loads (elements x, x+1 of rows y and y+1).
//         2 x (9/8)^3 = 2.85x the f32 voxels.
//   16-bit: "yz-quad" element = {v(y,z), v(y,z+1), v(y+1,z), v(y+1,z+1)} at x, 8 B, in 8^3
//         bricks; a sample = 1 x 16-B load of elements x, x+1.  4 x (9/8)^3 = 5.7x.
//   8-bit: plain voxels in 7 x 8 x 8-cell bricks (8-B rows, 648-B bricks); a sample = 2 x
//         16-B loads (rows y, y+1 of slices z and z+1, from the 4-aligned address at or below
//         the cell).  8 x 9 x 9 / (7 x 8 x 8) = 1.45x the voxels (VR_U8_PLAIN=0: yz-quads).
// Voxels outside [0, N) are stored as 0: CLAMP_TO_BORDER/TRANSPARENT_BLACK without a bounds
// test.
// Brick geometry (compile-time): BX x BY x BZ cells per brick, each axis storing cells + 1
// elements (the apron); element (x, y, z) of a brick at x + EX (y + EY z), the brick padded to
// Elems.  f32 and 16-bit volumes use GeomWide (default 8^3 cells, 9^3 = 729 elements), 8-bit
// volumes GeomByte.  Experiment builds may set VR_BRICK_CELLS="bx,by,bz" (e.g. 15,7,8: 16-element
// rows = one 128-B line of f32 z-pairs) and VR_BRICK_ALIGN (elements a brick is rounded up to).
#ifndef VR_BRICK_CELLS
#define VR_BRICK_CELLS 8, 8, 8
#endif
#ifndef VR_BRICK_ALIGN
#define VR_BRICK_ALIGN 1
#endif
// LO = 1 (the stencil copy below): every axis also stores one element below the brick's first
// cell and one more above, so a cell's gradient taps (x - 1 .. x + 2, per axis) never leave it.
template <int X, int Y, int Z, int LO = 0>
struct BrickGeom {
    static constexpr int BX = X, BY = Y, BZ = Z;
    static constexpr int Lo = LO;  // apron elements below the first cell
    static constexpr int EX = X + 1 + 2 * LO, EY = Y + 1 + 2 * LO, EZ = Z + 1 + 2 * LO;  // elements per axis
    static constexpr int Row = EX, Slice = EX * EY;           // element strides of y, z
    static constexpr int Elems = (EX * EY * EZ + VR_BRICK_ALIGN - 1) / VR_BRICK_ALIGN * VR_BRICK_ALIGN;
    __host__ __device__ static constexpr int cells(int a) { return a == 0 ? X : (a == 1 ? Y : Z); }
};
using GeomWide = BrickGeom<VR_BRICK_CELLS>;
// 8-bit volumes (VR_U8_PLAIN = 1): one voxel per element, bricks of 7 x 8 x 8 cells, so a brick
// row is 8 bytes and a 648-B brick keeps every row 4-aligned: one dwordx4 from the 4-aligned
// address at or below the cell's element holds elements x, x + 1 of rows y and y + 1 (byte
// offsets s, s+1, s+8, s+9 with s = x mod 4 <= 3), a second one the same at z + 1.
// VR_U8_BRICK_CELLS="3,8,8" (experiment builds): 4-byte rows, one dwordx2 per slice (half the
// bytes per sample), 1.69x the voxels: C4 +1.5%, C5 +-0, views -2..+4%
// (profiles/r02/u8_geometry/).
// VR_U8_PLAIN = 0: yz-quad elements in GeomWide bricks (one 8-B load, 5.7x the voxels).
#ifndef VR_U8_PLAIN
#define VR_U8_PLAIN 1
#endif
#ifndef VR_U8_BRICK_CELLS
#define VR_U8_BRICK_CELLS 7, 8, 8
#endif
using GeomByte = std::conditional_t<VR_U8_PLAIN != 0, BrickGeom<VR_U8_BRICK_CELLS>, GeomWide>;
// wide loads of the last brick read up to this many bytes past its end
constexpr size_t kBrickSlackBytes = 64;
// VR_F32_PLAIN=1 (experiment builds): f32 elements hold one voxel (no z-pair duplication);
// a sample is then 4 x 8-B loads (elements x, x+1 of the rows (y|y+1, z|z+1)).
#ifndef VR_F32_PLAIN
#define VR_F32_PLAIN 0
#endif
constexpr size_t kF32VoxelsPerElement = VR_F32_PLAIN ? 1 : 2;
constexpr int kPad = 2;

// Brick memory order (north_star: "Z-ordered bricks").  kGroupShift = 0: bricks x-fastest over
// the brick grid.  kGroupShift = g > 0: the grid is cut into groups of 2^g bricks per axis,
// groups x-fastest, and the 2^3g bricks of a group in Morton (Z) order, so bricks near in 3-D
// are near in memory (fewer distinct pages per wave-level load on oblique views).
#ifndef VR_BRICK_GROUP_SHIFT
#define VR_BRICK_GROUP_SHIFT 0
#endif
constexpr int kGroupShift = VR_BRICK_GROUP_SHIFT;
constexpr uint32_t kGroupMask = (1u << kGroupShift) - 1;

// Bits 0..g-1 of v moved to bits 0, 3, 6, ... (one axis of a Morton code).
__host__ __device__ __forceinline__ constexpr uint32_t morton_spread(uint32_t v)
{
    uint32_t r = 0;
#pragma unroll
    for (int t = 0; t < kGroupShift; ++t) r |= ((v >> t) & 1u) << (3 * t);
    return r;
}

// Memory slot of brick (bx, by, bz) of an nbx x nby x * grid (whole groups per axis).
__host__ __device__ __forceinline__ constexpr uint32_t brick_slot(uint32_t bx, uint32_t by,
                                                                  uint32_t bz, uint32_t nbx,
                                                                  uint32_t nby)
{
    if constexpr (kGroupShift == 0) {
        return (bz * nby + by) * nbx + bx;
    } else {
        constexpr uint32_t G = kGroupShift;
        const uint32_t grp = ((bz >> G) * (nby >> G) + (by >> G)) * (nbx >> G) + (bx >> G);
        return (grp << (3 * G)) | morton_spread(bx & kGroupMask) |
               (morton_spread(by & kGroupMask) << 1) | (morton_spread(bz & kGroupMask) << 2);
    }
}

// Inverse of brick_slot.
__host__ __device__ __forceinline__ void brick_coords(uint32_t slot, uint32_t nbx, uint32_t nby,
                                                      uint32_t &bx, uint32_t &by, uint32_t &bz)
{
    if constexpr (kGroupShift == 0) {
        bx = slot % nbx;
        by = (slot / nbx) % nby;
        bz = slot / (nbx * nby);
    } else {
        constexpr uint32_t G = kGroupShift;
        const uint32_t grp = slot >> (3 * G), m = slot & ((1u << (3 * G)) - 1);
        const uint32_t gx = nbx >> G, gy = nby >> G;
        uint32_t lx = 0, ly = 0, lz = 0;
#pragma unroll
        for (int t = 0; t < (int)G; ++t) {
            lx |= ((m >> (3 * t)) & 1u) << t;
            ly |= ((m >> (3 * t + 1)) & 1u) << t;
            lz |= ((m >> (3 * t + 2)) & 1u) << t;
        }
        bx = ((grp % gx) << G) | lx;
        by = (((grp / gx) % gy) << G) | ly;
        bz = ((grp / (gx * gy)) << G) | lz;
    }
}

// (enum StorageType and the layout flags named below: vr_variant.h)
// Brick layout code = storage type | kQuadFlag: 8-bit voxels kept in yz-quad elements (GeomWide
// bricks, one 8-B load per sample) instead of plain 7x8x8-cell bricks.  Volumes of at most
// kQuadMaxVoxels voxels use it (the quads, 5.7x the voxels, stay cache-resident: C2 256^3
// 459 against 420 Gsamples/s plain); larger ones the plain bricks (C4 HBM 5.70 -> 1.89 GB per
// frame).  The layout code is what the brick helpers below and the march launchers take.
constexpr size_t kQuadMaxVoxels = 1ull << 25;
// kernel-side tag type of 8-bit voxels T in yz-quad elements
template <typename T>
struct Quad8 {
    T v;
};
// Alternative f32 geometry: a further resident copy of an f32 volume in bricks whose z-pair
// rows never straddle a 128-B line, for the views where a wavefront's lanes sit on different
// brick rows and every straddled line is another L1 miss:
//   kAltFlag  (F32Alt):  7 x 15 x 8 cells (8-element, 64-B rows; 8704-B bricks, 68 lines), for
//                        oblique views (diagonal: 0.81 -> 0.68 ms per C3 frame).
// The frame-filling, side and top views stay in 8^3 bricks (2-4% faster there).  (A 15 x 15 x 8
// z-pair copy for sparse views, superseded by the plain and stencil copies below, is kept as a
// patch: tools/experiments/r04_pruned/.)
#ifndef VR_ALT_BRICK_CELLS
#define VR_ALT_BRICK_CELLS 7, 15, 8
#endif
using GeomAlt = BrickGeom<VR_ALT_BRICK_CELLS>;
// kernel-side tag type of f32 voxels in the kAltFlag layout
struct F32Alt {
    float v;
};
// A plain f32 copy (kPlainF32Flag, kernel tag F32P): one voxel per 4-B element, no z-pair
// duplication (1.2x the voxels against 2.6x), in GeomPlainRows bricks; a sample is 4 x 8-B
// loads (elements x, x + 1 of the rows (y | y+1, z | z+1)).  For sparse views, which read their
// whole copy from HBM every frame.
#ifndef VR_PLAIN_BRICK_CELLS
#define VR_PLAIN_BRICK_CELLS 15, 15, 15
#endif
using GeomPlainRows = BrickGeom<VR_PLAIN_BRICK_CELLS>;
struct F32P {
    float v;
};
// The stencil copy (kStencilF32Flag, kernel tag F32S): plain f32 voxels in GeomStencil bricks,
// which store one element below and two above every cell on each axis (32^3 elements for 29^3
// cells: 128-B rows, 1.34x the voxels, 0.76 GB for 512^3), so a shaded
// sample's central-difference taps are constant element offsets inside the brick: its density
// loads are rows x - 1 .. x + 2 (16 B each) and carry the x differences, y / z taps are 8-B
// loads, no neighbour-brick selection.  For shaded sparse views: the
// reference's default camera 0.260 (15x15x8 z-pairs) -> 0.231 ms (profiles/r03/stencil2/ ..
// stencil4/: 13^3 cells 0.240, 29x13x13 0.236, 29x13x29 / 29x13x61 / 29^3 0.231).
#ifndef VR_STENCIL_BRICK_CELLS
#define VR_STENCIL_BRICK_CELLS 29, 29, 29
#endif
using GeomStencil = BrickGeom<VR_STENCIL_BRICK_CELLS, 1>;
struct F32S {
    float v;
};
// kernel-side tag type of the f32 8^3-brick volume read with the difference field in binary16
// (MarchParams::grad_half): a variant of its own (vr_variant.h TAG_F32H) over the ST_F32 bricks
struct F32H {
    float v;
};
// The y-major copy (kYMajorFlag, kernel tags F32Y and, read with the binary16 field, F32HY): the
// GeomWide brick grid with the bricks in ymajor_slot order (x, then z, then y: the bricks along a
// ray that runs along y are nbx * nbz slots apart, those under an image tile adjacent, as the
// z-pair bricks are for a ray along z), every element a y-pair {v(x,y,z), v(x,y+1,z)} and the
// elements of a brick ordered x + EX (z + EZ y) -- y slowest.  A sample is 2 x 16-B loads at
// e and e + EX (elements x, x + 1 of rows z and z + 1).  For dense-row views whose ray runs along
// y: a step of 2.56 voxels then passes whole 648-B y-layers by, where in the z-pair bricks it
// reads rows y and y + 1 of every z-layer, i.e. nearly every line.  The
// difference field exists in both orders: the y-major one (kernel flag MarchParams::grad_ymajor)
// has a cell's 24-B element at the copy's element index; the z-major one, shared with the 8^3
// bricks, has it at cell_offset<float> in brick_slot order.
struct F32Y {
    float v;
};
struct F32HY {
    float v;
};
// Local element indices of padded cell (pi, pj, pk) inside its GeomWide brick: z-major (the
// ST_F32 bricks, the field) and y-major (the copy).
__host__ __device__ constexpr uint32_t zmajor_local(uint32_t xl, uint32_t yl, uint32_t zl)
{
    return xl + (uint32_t)GeomWide::EX * (yl + (uint32_t)GeomWide::EY * zl);
}
__host__ __device__ constexpr uint32_t ymajor_local(uint32_t xl, uint32_t yl, uint32_t zl)
{
    return xl + (uint32_t)GeomWide::EX * (zl + (uint32_t)GeomWide::EZ * yl);
}
// zmajor_local - ymajor_local (8^3 cells: 72 (zl - yl))
__host__ __device__ constexpr int ymajor_field_delta(uint32_t yl, uint32_t zl)
{
    return GeomWide::EX * (GeomWide::BY * (int)zl - GeomWide::BZ * (int)yl);
}
// Memory slot of brick (bx, by, bz) in the y-major structures: x fastest, then z, then y (the
// mirror image of brick_slot's x, y, z; no brick groups).
__host__ __device__ constexpr uint32_t ymajor_slot(uint32_t bx, uint32_t by, uint32_t bz,
                                                   uint32_t nbx, uint32_t nbz)
{
    return bx + nbx * (bz + nbz * by);
}
// Inverse of ymajor_slot.
__host__ __device__ constexpr void ymajor_coords(uint32_t slot, uint32_t nbx, uint32_t nbz,
                                                 uint32_t &bx, uint32_t &by, uint32_t &bz)
{
    bx = slot % nbx;
    bz = (slot / nbx) % nbz;
    by = slot / (nbx * nbz);
}
// Element index of padded cell (pi, pj, pk) in the y-major copy (and the y-major field);
// *field_delta (when not null): the in-brick part of the way to the same cell's element in the
// z-major layout (the bricks' slots differ as well: ymajor_slot against brick_slot).
__host__ __device__ constexpr size_t ymajor_cell_offset(uint32_t pi, uint32_t pj, uint32_t pk,
                                                        uint32_t nbx, uint32_t nbz,
                                                        int *field_delta = nullptr)
{
    using G = GeomWide;
    const uint32_t bx = pi / G::BX, by = pj / G::BY, bz = pk / G::BZ;
    const uint32_t xl = pi - bx * G::BX, yl = pj - by * G::BY, zl = pk - bz * G::BZ;
    if (field_delta) *field_delta = ymajor_field_delta(yl, zl);
    return (size_t)ymajor_slot(bx, by, bz, nbx, nbz) * (size_t)G::Elems + ymajor_local(xl, yl, zl);
}
namespace ymajor_check {
// Over an NBX x NBY x NBZ-brick grid: ymajor_slot is a bijection onto [0, bricks) with
// ymajor_coords its inverse; every element (cells and apron) of every brick maps into its own
// brick's [0, 729) exactly once, and the z-major index is the y-major one + the field delta.
template <uint32_t NBX, uint32_t NBY, uint32_t NBZ>
constexpr bool map_ok()
{
    using G = GeomWide;
    constexpr uint32_t nbx = NBX, nby = NBY, nbz = NBZ;
    bool slot_seen[nbx * nby * nbz] = {};
    for (uint32_t bz = 0; bz < nbz; ++bz)
        for (uint32_t by = 0; by < nby; ++by)
            for (uint32_t bx = 0; bx < nbx; ++bx) {
                const uint32_t slot = ymajor_slot(bx, by, bz, nbx, nbz);
                if (slot >= nbx * nby * nbz || slot_seen[slot]) return false;
                slot_seen[slot] = true;
                uint32_t cx = 0, cy = 0, cz = 0;
                ymajor_coords(slot, nbx, nbz, cx, cy, cz);
                if (cx != bx || cy != by || cz != bz) return false;
                bool seen[G::EX * G::EY * G::EZ] = {};
                const size_t base = (size_t)slot * (size_t)G::Elems;
                for (uint32_t zl = 0; zl < (uint32_t)G::EZ; ++zl)
                    for (uint32_t yl = 0; yl < (uint32_t)G::EY; ++yl)
                        for (uint32_t xl = 0; xl < (uint32_t)G::EX; ++xl) {
                            const uint32_t l = ymajor_local(xl, yl, zl);
                            if (l >= (uint32_t)(G::EX * G::EY * G::EZ) || seen[l]) return false;
                            seen[l] = true;
                            if ((int)zmajor_local(xl, yl, zl) - (int)l != ymajor_field_delta(yl, zl))
                                return false;
                            // cells (not the apron) through the kernels' addressing
                            if (xl < (uint32_t)G::BX && yl < (uint32_t)G::BY && zl < (uint32_t)G::BZ) {
                                int fd = 0;
                                const size_t e = ymajor_cell_offset(bx * G::BX + xl, by * G::BY + yl,
                                                                    bz * G::BZ + zl, nbx, nbz, &fd);
                                if (e != base + l || fd != ymajor_field_delta(yl, zl)) return false;
                            }
                        }
            }
    return true;
}
static_assert(map_ok<3, 2, 2>(), "the y-major maps are bijections, 72 (zl - yl) from z-major");
static_assert(map_ok<2, 1, 3>() && map_ok<1, 3, 2>(), "... also where nby != nbz");
static_assert(GeomWide::BX != 8 || GeomWide::BY != 8 || GeomWide::BZ != 8 ||
                  ymajor_field_delta(3, 5) == 72 * (5 - 3),
              "8^3 cells: l_zmajor - l_ymajor == 72 (zl - yl)");
}  // namespace ymajor_check

// Bytes of one voxel of storage type (or layout code) st.
inline size_t storage_size(int st)
{
    switch (st & 0xF) {
        case ST_U8:
        case ST_I8: return 1;
        case ST_U16:
        case ST_I16: return 2;
        default: return 4;
    }
}
// layout code st holds plain 8-bit voxels (one per element, GeomByte bricks)
inline bool byte_storage(int st)
{
    return VR_U8_PLAIN && !(st & kQuadFlag) && (st == ST_U8 || st == ST_I8);
}
inline size_t voxels_per_element(int st)
{
    if (st & (kPlainF32Flag | kStencilF32Flag)) return 1;
    return (st & 0xF) == ST_F32 ? kF32VoxelsPerElement : (byte_storage(st) ? 1 : 4);
}
inline size_t element_size(int st) { return storage_size(st) * voxels_per_element(st); }
// Brick geometry of layout code st: cells along axis a (0 x, 1 y, 2 z), elements per brick.
inline int brick_cells(int st, int a)
{
    if (st & kAltFlag) return GeomAlt::cells(a);
    if (st & kPlainF32Flag) return GeomPlainRows::cells(a);
    if (st & kStencilF32Flag) return GeomStencil::cells(a);
    return byte_storage(st) ? GeomByte::cells(a) : GeomWide::cells(a);
}
inline size_t brick_elems(int st)
{
    if (st & kAltFlag) return GeomAlt::Elems;
    if (st & kPlainF32Flag) return GeomPlainRows::Elems;
    if (st & kStencilF32Flag) return GeomStencil::Elems;
    return byte_storage(st) ? GeomByte::Elems : GeomWide::Elems;
}

// Bricks along axis a of an n-voxel axis: fetch base indices lie in [1, N + 1] (march) and
// gradient taps reach one element below and (in z-pair x/y) two above, i.e. padded [0, N + 3];
// rounded up to whole brick groups.
inline uint32_t bricks_for(uint32_t n, int a, int st)
{
    return ((n + 3) / (uint32_t)brick_cells(st, a) + 1 + kGroupMask) & ~kGroupMask;
}

// ---- Frame rows over ranks (sort-first tiling) ------------------------------
// The frame's rows are cut into blocks of row_block rows and dealt in periods of
// w0 + (n - 1) w blocks: rank 0 takes the first w0 blocks of each period, rank r > 0 the w
// blocks after w0 + (r - 1) w.  w0 = w = 1 (the default) is block b -> rank b mod n.  A smaller
// w0 / w lightens rank 0, which also receives the other shards and assembles the frame
// (vr_set_row_share).  Every rank sends the same number of rows (ncclGather
// counts are equal): the largest share, padded.
struct RowShare {
    uint32_t w0, w;
};
__host__ __device__ inline uint32_t share_period(uint32_t n, RowShare s) { return s.w0 + (n - 1) * s.w; }
__host__ __device__ inline uint32_t share_offset(uint32_t r, RowShare s)
{
    return r == 0 ? 0u : s.w0 + (r - 1) * s.w;
}
// global block of rank r's local block lb
__host__ __device__ inline uint32_t share_global_block(uint32_t lb, uint32_t r, uint32_t n, RowShare s)
{
    const uint32_t w = r == 0 ? s.w0 : s.w;
    return (lb / w) * share_period(n, s) + share_offset(r, s) + lb % w;
}
// owner rank and local block of global block gb
__host__ __device__ inline void share_owner(uint32_t gb, uint32_t n, RowShare s, uint32_t &r,
                                            uint32_t &lb)
{
    const uint32_t P = share_period(n, s), q = gb / P, o = gb - q * P;
    if (o < s.w0) {
        r = 0;
        lb = q * s.w0 + o;
    } else {
        const uint32_t t = o - s.w0;
        r = 1 + t / s.w;
        lb = q * s.w + t % s.w;
    }
}
// blocks rank r owns among the nb blocks of a frame
inline uint32_t share_blocks(uint32_t nb, uint32_t r, uint32_t n, RowShare s)
{
    const uint32_t P = share_period(n, s), q = nb / P, o = nb - q * P;
    const uint32_t w = r == 0 ? s.w0 : s.w, off = share_offset(r, s);
    const uint32_t tail = o > off ? (o - off < w ? o - off : w) : 0u;
    return q * w + tail;
}
// rows of every rank's shard buffer: the largest share
inline uint32_t share_shard_rows(uint32_t height, uint32_t row_block, uint32_t n, RowShare s)
{
    if (row_block == 0 || n == 0 || s.w0 == 0 || s.w == 0) return 0;
    const uint32_t nb = (height + row_block - 1) / row_block;
    uint32_t m = share_blocks(nb, 0, n, s);
    if (n > 1) {
        const uint32_t b1 = share_blocks(nb, 1, n, s);  // rank 1 owns the most of ranks >= 1
        m = b1 > m ? b1 : m;
    }
    return m * row_block;
}

// ---- Kernel parameters (one frame) -------------------------------------------------------
struct MarchParams {
    const void *vol;        // bricked voxels, storage type per kernel instantiation
    const float4 *tf;       // decoded TF texels (linear RGB, linear A), device
    void *out;              // shard buffer (local_rows x W pixels)
    unsigned long long *counters;  // COUNT variant: rays, samples, shaded, steps

    double inv[16];         // inverse of float (proj * view), column-major
    double fw, fh;          // framebuffer W, H as double

    uint32_t nx, ny, nz;
    uint32_t nbx, nby;      // bricks per axis (x, y)
    float fnx, fny, fnz;    // float(nx) ...
    float vmin, range;      // Dataset.min, max - min
    int32_t tf_n;
    float tf_nf;

    float smin[3], smax[3];
    float cam[3];
    float step;
    int32_t nsteps;
    float ert_eps;
    float clear[4];
    float ka, kd, ks;
    int32_t spec_power;

    uint32_t W, H;
    uint32_t row_block, rank, nranks, local_rows;
    uint32_t tiles_x, tiles_y;
    uint32_t tile_order;    // 1 raster, 2 XCD bands, 3 XCD-interleaved super-tiles
    uint32_t supers_x, supers_total;  // super-tile grid (tile_order 3)
    uint32_t wave_w_shift;  // wavefront pixel footprint: 2^shift x (64 >> shift) (8x8: 3)
    int32_t out_format;
    int32_t slab_default;   // slicing is the whole volume (0,0,0)-(1,1,1)
    int32_t pipelined;      // two samples in flight per ray (few waves per CU: see PIPE)
    int32_t pair;           // lane-pair march (march_pair_kernel), 16x8-pixel tiles
    // adaptive tile order (tile_order 4): workgroup b renders tile tile_perm[b] (tile id =
    // ty * tiles_x + tx, ~0 = none; nperm workgroups) and records its duration in
    // tile_cost[tile id]; null: order by tile_order
    const uint32_t *tile_perm;
    uint32_t *tile_cost;
    uint32_t nperm;
    // skip_empty: per brick (index as in cell_offset) the Chebyshev distance in bricks to the
    // nearest brick that can produce a visible sample, capped at kSkipCap; 0 = not empty
    const uint8_t *skip_dist;
    int32_t skip_empty;
    int32_t div_fast;       // density normalisation by reciprocal + fma correction
    // f32 shading: precomputed central differences, element e = {Dx, Dy, Dz} x {z, z + 1}
    // (24 B, same element index as the density); null -> formed from the stencil
    const float *grad;
    // the field holds {Dx, Dy, Dz} x {(y,z), (y,z+1), (y+1,z), (y+1,z+1)} as binary16, scaled by
    // 2^k (field_scale_log2; the shading normalises the gradient, so the scale cancels)
    int32_t grad_half;
    float inv_range;        // RN(1 / range) (div_fast)
    uint32_t share_w0, share_w;  // RowShare of the row blocks over nranks
    // bytes of the volume copy P.vol points at and of the output buffer (bounds-checking
    // debug builds, -DVR_BOUNDS_CHECK: an out-of-range access is printed and skipped)
    unsigned long long vol_bytes, out_bytes;
    // the y-major structures (F32Y): bricks per axis z (ymajor_slot), and whether `grad` is the
    // y-major binary16 field (a cell's element at the copy's element index) or the z-major one
    uint32_t nbz;
    int32_t grad_ymajor;
};

// Launchers (vr_kernels.hip).  All asynchronous on `stream`.
// ---- Maximum-intensity projection (include/vr/vr_modes.h, mip_kernel) ----
// What the MIP kernel reads beside MarchParams (a kernel argument of its own: MarchParams'
// size is part of the composite kernels' descriptors, which the committed roofline data is
// keyed on).  brick_range: per brick (index as skip_dist) {lo, hi} of every value a sample in
// the brick can read, NaN bricks {NaN, NaN}, and one more entry after the last brick whose .y
// is the largest hi of all (launch_range_max); null without range skipping.
struct MipArgs {
    const float2 *brick_range;
    uint32_t nbricks;
};
// ---- First-hit isosurface (include/vr/vr_iso.h, iso_kernel) ----
// What the ISO kernel reads beside MarchParams (its own argument, as MipArgs): the brick ranges
// of MipArgs (null without range skipping), the isovalue in density units and vr_params.shading
// (read once per ray: a run-time flag, not a template argument).
struct IsoArgs {
    const float2 *brick_range;
    uint32_t nbricks;
    float iso;
    int32_t shading;
};
// ---- Minimum- and mean-intensity projection (include/vr/vr_modes.h, proj_kernel) ----
// What proj_kernel reads beside MarchParams (its own argument, as MipArgs): the brick ranges of
// MipArgs, null without range skipping.  MinIP reads .x of the entry after the last brick, the
// smallest lo of all.  Also what proj_strip takes: mip_kernel runs it with the maximum as its
// operator (kProjMax, vr_variant.h) and hands its MipArgs on as these.
struct ProjArgs {
    const float2 *brick_range;
    uint32_t nbricks;
};
// The kernel `v` names (resolve_variant) over p's tiles; m is read by mip_kernel and (as its
// ProjArgs) proj_kernel, i by iso_kernel alone.  hipErrorInvalidValue: no such kernel
// (variant_built), or MIP / ISO / MinIP / mean skipping without the brick ranges.
hipError_t launch_frame(const FrameVariant &v, const MarchParams &p, const MipArgs &m,
                        const IsoArgs &i, hipStream_t stream);
// ---- Multi-planar reformat (include/vr/vr_mpr.h, mpr_kernel) ----
// MPR is no frame: it has no camera, an image size of its own and a parallel ray set, so its
// kernel takes this argument alone (MarchParams does not grow) and is launched outside
// launch_frame and FrameVariant.  The fields the shared pixel epilogue reads (vmin .. out_bytes)
// carry MarchParams' names.
struct MprArgs {
    const void *vol;        // the base bricks (layout code `layout` of launch_mpr)
    const float4 *tf;       // decoded TF texels, device (read through this global pointer)
    void *out;              // H x W pixels
    unsigned long long *counters;  // the counting kernel: rays, samples, shaded, steps, skipped
    double origin[3], du[3], dv[3], dn[3];  // the plane's f32 vectors, widened (exact)
    double half_w, half_h, half_n;  // 0.5 W, 0.5 H, 0.5 (nsamples - 1)
    uint32_t nbx, nby;      // bricks per axis (x, y)
    float fnx, fny, fnz;
    float vmin, range, inv_range;
    int32_t div_fast;
    int32_t tf_n;
    float tf_nf;
    float smin[3], smax[3];
    float clear[4];
    uint32_t W, H, nsamples;
    uint32_t tiles_x, tiles_y;  // 16 x 16-pixel tiles, one per workgroup
    // workgroup -> tile: 1 raster, 3 the frames' XCD-interleaved 4 x 4-tile super-tiles
    // (block_tile's order 3; supers_x, supers_total as MarchParams')
    uint32_t tile_order, supers_x, supers_total;
    int32_t out_format;
    int32_t op;             // vr_mpr_op (the thin-slice kernel reads it; the slab kernels' is a template argument)
    unsigned long long vol_bytes, out_bytes;  // bounds-checking debug builds
};
// mpr_kernel's OP: vr_mpr_op's three values over a slab, and the thin slice (nsamples == 1: one
// instantiation per storage tag, the operator read at run time for its NaN rule alone)
constexpr int kMprMax = 0, kMprMin = 1, kMprMean = 2, kMprThin = 3;
// The tile order of an MPR launch unless VR_KNOB_TILE_ORDER asks for one (1 or 3).  Measured on
// 1024^2 images of the 512^3 f32 volume at a pitch of one voxel (profiles/r13/mpr/c3.json, both
// orders alternated in one process): 64-sample slabs run 9.4 % faster in super-tiles on the
// sagittal plane (0.127 -> 0.115 ms), 1-2.4 % faster on the axial and oblique ones and 1.1-1.6 %
// slower on the coronal one; thin slices (6-7 us a launch) are 0.3-0.9 us faster in raster order
// on all four planes.
constexpr uint32_t kMprTileOrder(uint32_t nsamples) { return nsamples == 1 ? 1u : 3u; }
// The MPR kernel of a base layout (a storage type, or an 8-bit one | kQuadFlag) over a's tiles:
// the slab kernel of a.op, the thin-slice kernel when a.nsamples == 1, or (count) the counting
// kernel, which walks the positions, fetches nothing and writes no pixel.  *name (when not null):
// the demangled kernel name.  hipErrorInvalidValue: no such layout or operator.
hipError_t launch_mpr(int layout, bool count, const MprArgs &a, hipStream_t stream,
                      std::string *name);
// ---- Value histogram (include/vr/vr_hist.h, hist_kernel) ----
// out: nbins 64-bit counts, then below, above, nan, then one 64-bit slot holding two 32-bit words:
// ~ordered(minimum) and ordered(maximum) over the non-NaN voxels (minmax_kernel's encoding; the
// minimum inverted so that both reduce with atomicMax).  The caller zeroes all of it: zero is the
// identity of every one of these reductions.
struct HistArgs {
    const void *vol;        // the base bricks (layout code `layout` of launch_hist)
    const float *edges;     // nbins lower edges (vr_hist_host.h hist_edges), device
    unsigned long long *out;
    double scale;           // hist_scale: the first guess of a bin is (v - lo) * scale
    float lo, hi;
    uint32_t nbins;
    uint32_t nbx, nby;      // bricks per axis (x, y) of the volume
    uint32_t box_min[3], box_max[3];  // logical voxel indices, half open
    uint32_t b0[3], nb[3];  // the bricks that hold the box's voxels: first and count per axis
    uint32_t nwork;         // nb[0] * nb[1] * nb[2]
};
constexpr size_t kHistOutWords = (size_t)kHistMaxBins + 4;  // 64-bit words of HistArgs::out
// workgroups of a histogram launch at most (8 per CU; hist_kernel's 32-bit private counters)
constexpr uint32_t kHistMaxGrid = 2048;
// The histogram kernel of a base layout (a storage type, or an 8-bit one | kQuadFlag) over the
// bricks a.b0 .. a.b0 + a.nb.  agg: the wave-aggregated form (hist_kernel AGG).  *name (when not
// null): the demangled kernel name.  hipErrorInvalidValue: no such layout, or no work.
hipError_t launch_hist(int layout, bool agg, const HistArgs &a, hipStream_t stream,
                       std::string *name);
// ---- Hit records and picking (include/vr/vr_hit.h, hit_kernel) ----
// What hit_kernel reads beside MarchParams (its own argument, as MipArgs and IsoArgs: MarchParams
// keeps its size).  The MarchParams of a hit launch describes the request's rectangle -- W, H,
// local_rows and the tile counts are the rectangle's, so strip_pixel and block_tile walk its
// pixels -- while fw / fh stay the framebuffer's: pixel (px, py) of the rectangle casts the ray of
// framebuffer pixel (x0 + px, y0 + py).  out: W * H records of kHitRecordBytes, row-major.
struct HitArgs {
    void *out;
    unsigned long long out_bytes;  // bounds-checking debug builds
    float threshold;               // kHitOpacity
    float iso;                     // kHitIso: the context's isovalue
    uint32_t x0, y0;               // the rectangle's origin in the framebuffer
};
// Samples of a ray the hit kernels keep in flight unless VR_KNOB_HIT_INFLIGHT says otherwise: two
// for every kind.  Whole-frame hit images, K = 1 -> K = 2, ms (profiles/r16/hit/c3.json, c4.json;
// tools/hit_bench.py): OPACITY 0.387 -> 0.293 and 0.898 -> 0.724, MAX 0.421 -> 0.381 and 1.130 ->
// 1.017, MIN the same, ISO 0.374 -> 0.314 and 0.838 -> 0.735; ENTRY ends at its first sample and
// is a tie within its round-to-round spread (0.0364 / 0.0359 and 0.0736 / 0.0736).
constexpr int kHitDefaultInFlight(int /* kind: the same side won for each */) { return 2; }
// The hit kernel of a base layout (a storage type, or an 8-bit one | kQuadFlag) over p's tiles in
// tile order 3: kind a vr_hit_kind, inflight 1 or 2; count: the counting kernel (one sample in
// flight, no record written).  *name (when not null): the demangled kernel name.
// hipErrorInvalidValue: no such layout, kind or inflight.
hipError_t launch_hit(int layout, int kind, bool count, int inflight, const MarchParams &p,
                      const HitArgs &a, hipStream_t stream, std::string *name);
// ---- Isosurface mesh (include/vr/vr_mesh.h; mesh_classify_kernel, mesh_scan_*, mesh_vertex_kernel,
// mesh_quad_kernel) ----
// A launch walks the "work bricks" b0 .. b0 + nb of the base layout (vr_mesh_host.h
// mesh_brick_range), work index w = x-fastest over them; a brick's cells are numbered
// xl + BX (yl + BY zl), at most kMeshMaskWords * 32 of them.  Per work brick the scratch holds
//   mask  kMeshMaskWords words: bit c = cell c is an active cell of the cell set (classify)
//   cnt   {active cells, owned qualifying edges}                                  (classify)
//   pre   the exclusive prefix of cnt inside its chunk of kMeshChunk bricks       (scan)
// and per chunk `chunk` holds the two chunk sums, which mesh_scan_chunks_kernel turns into their
// exclusive prefix (64-bit: 16.8 M bricks x 1536 edges pass 2^32).  So a cell's vertex id is
// chunk[2 (w / kMeshChunk)] + pre[w].x + popcount(mask below the cell), and a brick's first quad
// chunk[2 (w / kMeshChunk) + 1] + pre[w].y.  out: {vertices, quads, inside voxels}, zeroed by the
// caller (inside voxels is an atomic sum; the other two are stored by the chunk scan).
// The emit pass re-reads the cell's corners and re-applies the box rule instead of keeping three
// edge and three direction bits per cell: 80 B of scratch per brick instead of 464 B.
struct MeshArgs {
    const void *vol;        // the base bricks (layout code `layout` of the launchers)
    uint32_t *mask;
    uint2 *cnt, *pre;
    unsigned long long *chunk;
    unsigned long long *out;
    void *verts;            // vr_mesh_vertex records (mesh_vertex_kernel)
    uint32_t *tris;         // three indices per triangle (mesh_quad_kernel)
    float iso;
    float fdims[3];         // float(nx) ...
    uint32_t dims[3];
    uint32_t nbx, nby;      // bricks per axis (x, y) of the volume
    uint32_t lo[3], hi[3];  // the node box N, logical voxel indices, half open
    int32_t clo[3], chi[3]; // the cell set, logical cell indices, both ends included
    uint32_t b0[3], nb[3];  // the work bricks: first and count per axis
    uint32_t nwork;         // nb[0] * nb[1] * nb[2]
    uint32_t nchunks;       // ceil(nwork / kMeshChunk)
};
constexpr uint32_t kMeshMaskWords = 16;
constexpr uint32_t kMeshChunk = 1024;  // bricks one workgroup of mesh_scan_bricks_kernel scans
// workgroups of a classify / vertex / quad launch at most, as the histogram's
constexpr uint32_t kMeshMaxGrid = 2048;
// Bytes of the scratch of nwork work bricks, and the sub-buffers' offsets in it (all 16-aligned).
struct MeshScratch {
    size_t mask, cnt, pre, chunk, out, bytes;
};
inline MeshScratch mesh_scratch(uint64_t nwork)
{
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t nchunks = (size_t)((nwork + kMeshChunk - 1) / kMeshChunk);
    MeshScratch s;
    s.mask = 0;
    s.cnt = up(s.mask + (size_t)nwork * kMeshMaskWords * 4);
    s.pre = up(s.cnt + (size_t)nwork * 8);
    s.chunk = up(s.pre + (size_t)nwork * 8);
    s.out = up(s.chunk + nchunks * 16);
    s.bytes = s.out + 32;
    return s;
}
// The passes of a base layout (a storage type, or an 8-bit one | kQuadFlag), each asynchronous on
// `stream`.  launch_mesh_classify: classify, then the two scans, so a.out then holds the counts;
// *name (when not null): the classify kernel's demangled name.  hipErrorInvalidValue: no such
// layout, or no work.
hipError_t launch_mesh_classify(int layout, const MeshArgs &a, hipStream_t stream, std::string *name);
hipError_t launch_mesh_vertices(int layout, bool normals, const MeshArgs &a, hipStream_t stream);
hipError_t launch_mesh_quads(int layout, const MeshArgs &a, hipStream_t stream);
// ---- Connected components and region growing (include/vr/vr_label.h; label_local_kernel,
// label_seam_kernel, label_flatten_kernel, label_scan_chunks_kernel, label_table_init_kernel,
// label_accum_kernel, label_largest_kernel, label_grow_kernel) ----
// P: one word per voxel of the box N in box-linear order, parent + 1 during the passes (0: not in)
// and the label after label_flatten_kernel.  The root table over N, cut into words of 64 voxels and
// chunks of kLabelChunk voxels: mask (bit i of word w: voxel 64 w + i is a root), wpre (the roots of
// the word's chunk before the word), chunk (the chunk's roots, then -- label_scan_chunks_kernel --
// the roots before the chunk), so the record index of the component with root r is
// chunk[r / kLabelChunk] + wpre[r / 64] + popcount(mask[r / 64] below bit r % 64): the records come
// out sorted by label.  out: {components, in voxels, largest (voxels << 32 | ~label), 0}, zeroed by
// the caller.
struct LabelArgs {
    const void *vol;        // the base bricks (layout code `layout` of launch_label)
    uint32_t *P;
    unsigned long long *mask;
    uint32_t *wpre;
    uint32_t *chunk;
    unsigned long long *out;
    void *comps;            // ncomps vr_label_component records (8-aligned)
    uint8_t *grow;          // label_grow_kernel's mask, a byte per voxel of N
    float lo, hi;           // the window
    uint32_t nbx, nby;      // bricks per axis (x, y) of the volume
    uint32_t blo[3], bhi[3], ext[3];  // the box N, logical voxel indices, half open; its extents
    uint32_t b0[3], nb[3];  // the work bricks: first and count per axis
    uint32_t nwork;         // nb[0] * nb[1] * nb[2]
    uint32_t nvox;          // voxels of N, at most 2^32 - 1
    uint32_t nwords;        // ceil(nvox / 64)
    uint32_t nchunks;       // ceil(nvox / kLabelChunk)
    uint32_t ncomps;        // records (the table passes)
    uint32_t seed_label;    // label_grow_kernel
};
constexpr uint32_t kLabelChunk = 8192;  // voxels one workgroup of label_flatten_kernel walks
constexpr uint32_t kLabelChunkWords = kLabelChunk / 64;
// workgroups of a local / seam / table / grow launch at most, as the histogram's
constexpr uint32_t kLabelMaxGrid = 2048;
// Bytes of the root table of nvox voxels, and the sub-buffers' offsets in it (all 16-aligned).
struct LabelScratch {
    size_t mask, wpre, chunk, out, bytes;
};
inline LabelScratch label_scratch(uint64_t nvox)
{
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t nwords = (size_t)((nvox + 63) / 64), nchunks = (size_t)((nvox + kLabelChunk - 1) / kLabelChunk);
    LabelScratch s;
    s.mask = 0;
    s.wpre = up(s.mask + nwords * 8);
    s.chunk = up(s.wpre + nwords * 4);
    s.out = up(s.chunk + nchunks * 4);
    s.bytes = s.out + 32;
    return s;
}
// The passes of a base layout (a storage type, or an 8-bit one | kQuadFlag), one kernel a call (the
// host may record an event between two), each asynchronous on `stream`.  launch_label, pass 0 ..
// kLabelPasses - 1: local, seam, flatten, scan; after the last a.P holds the labels and a.out the
// components and the in voxels; *name (when not null): the local kernel's demangled name.
// launch_label_table, pass 0 .. 2: init, accumulate and largest over a.ncomps records at a.comps (a
// region grow runs init alone, on its single record).  launch_label_grow: the mask and record 0.
// hipErrorInvalidValue: no such layout, connectivity or pass, or no work.
constexpr int kLabelPasses = 4;
// vr_debug_label_pass_ms's slots: the kernels in launch order
enum LabelPassSlot { kLabelLocal, kLabelSeam, kLabelFlatten, kLabelScan, kLabelTableInit, kLabelAccum,
                     kLabelLargest, kLabelGrow, kLabelPassSlots };
hipError_t launch_label(int layout, int connectivity, int pass, const LabelArgs &a, hipStream_t stream,
                        std::string *name);
hipError_t launch_label_table(int pass, const LabelArgs &a, hipStream_t stream);
hipError_t launch_label_grow(const LabelArgs &a, hipStream_t stream);
constexpr int kMipDefaultInFlight = 2;
// range[nbricks] = {min lo, max hi} over the non-NaN bricks of range[0 .. nbricks)
hipError_t launch_range_max(float2 *range_dev, uint32_t nbricks, hipStream_t stream);
// Wavefront count below which a launch uses the pipelined kernel (see build_params).
constexpr uint32_t kPipelineMaxWaves = 24576;  // between N = 2 (16 K) and N = 1 (33 K) at 1080p
constexpr size_t kPipelineMinBytes = 4ull << 30;  // large volumes: always pipelined
constexpr size_t kPipelineMinVoxels = 1ull << 29;
// march_kernel tiles: 16 pixels wide, kMarchRows tall, one lane per pixel (experiment
// builds may set VR_MARCH_ROWS=32: 512-thread workgroups whose 8 wavefronts share one CU's L1)
#ifndef VR_MARCH_ROWS
#define VR_MARCH_ROWS 16
#endif
constexpr uint32_t kMarchRows = VR_MARCH_ROWS;
// super-tiles (tile orders 3 and 4): 2^kSuperShift tiles per side, dealt round-robin over the
// 8 XCDs; experiment builds may change the size (VR_SUPER_SHIFT) and the order an XCD's tile
// list is kept in for the adaptive sort (VR_LIST_ORDER 0: frame raster, 1: super-tile major)
#ifndef VR_SUPER_SHIFT
#define VR_SUPER_SHIFT 2
#endif
#ifndef VR_LIST_ORDER
#define VR_LIST_ORDER 0
#endif
constexpr uint32_t kSuperShift = VR_SUPER_SHIFT;
constexpr uint32_t kSuper = 1u << kSuperShift;
constexpr uint32_t kThreadsPerTile = 16 * kMarchRows;
// vr_render (host output): row bands per frame, each copied to the host while later bands render
constexpr int kHostBands = 4;
constexpr uint32_t kHostBandMinRows = 256;  // shorter frames: one band
// Adaptive tile order: from the per-tile durations of the last launch with the same tile
// geometry, the next launch's workgroup -> tile permutation, longest first within each XCD's
// super-tiles (as tile_order 3 assigns them).
hipError_t launch_order_tiles(const uint32_t *cost, const uint32_t *lists, uint32_t *perm,
                              uint32_t per_xcd, hipStream_t stream);
// launches of one geometry per re-ordering (the order kernel runs on every 4th)
#ifndef VR_REORDER_EVERY
#define VR_REORDER_EVERY 4
#endif
constexpr uint32_t kReorderEvery = VR_REORDER_EVERY;
// schedules kept (one per geometry, stream and march variant; oldest dropped first)
constexpr size_t kMaxTileScheds = 64;
// Wavefront count (single-lane tiling) below which a launch uses the lane-pair kernel.
constexpr uint32_t kPairMaxWaves = 24576;
constexpr uint32_t kPairQuadMaxWaves = 6144;  // below: 4 lanes per ray
hipError_t launch_brick_from_linear(int src_dtype, const void *src, void *dst, uint32_t nx,
                                    uint32_t ny, uint32_t nz, int storage, hipStream_t stream);
// Bricked volume -> linear x-fastest voxels of the storage type, slices [z0, z0 + cz).
hipError_t launch_unbrick(int storage, const void *bricks, void *dst, uint32_t nx, uint32_t ny,
                          uint32_t z0, uint32_t cz, hipStream_t stream);
// Synthetic volume into a LINEAR buffer of the storage type (then bricked).
hipError_t launch_generate(int kind, int storage, void *dst_linear, uint32_t nx, uint32_t ny,
                           uint32_t nz, const float *params_dev, int nparams,
                           hipStream_t stream);
hipError_t launch_assemble(const void *gathered, void *out, int out_format, uint32_t W,
                           uint32_t H, uint32_t row_block, uint32_t nranks,
                           uint32_t shard_rows, RowShare share, hipStream_t stream);
// Integer range of a LINEAR buffer of 32-bit or 64-bit voxels (vr_dtype 5..9): out3_dev = {min,
// max, not-all-integers flag}, pre-set by the caller to {INT_MAX, INT_MIN, 0}.  Integers are
// counted only in [-32768, 65535]; -0.0, NaN, infinities and fractions set the flag.
hipError_t launch_int_range(int src_dtype, const void *src, size_t count, int *out3_dev,
                            hipStream_t stream);
// min/max over a LINEAR buffer of the storage type (ordered-uint encoding in minmax_dev).
hipError_t launch_minmax(int storage, const void *linear, size_t count, float *minmax_dev,
                         hipStream_t stream);

// Empty-space skipping (skip_empty): per-brick value range of the stored elements, then per
// (volume, TF) the capped Chebyshev distance field over the brick grid (1 byte per brick;
// scratch_dev: the same size, for the separable passes).
constexpr int kSkipCap = 16;
// f32 gradient field (see MarchParams::grad) from the bricked density: same brick grid.
constexpr size_t kGradElemBytes = 24;
// half: the binary16 field of MarchParams::grad_half, each difference times 2^scale_log2 and
// clamped to +-65504 (NaN kept) before rounding to nearest even.  ymajor (half only): the same
// elements in the y-major copy's brick and element order (MarchParams::grad_ymajor)
hipError_t launch_grad_field(const float *bricks, float *grad, uint32_t nx, uint32_t ny,
                             uint32_t nz, bool half, int scale_log2, bool ymajor,
                             hipStream_t stream);
// The f32 copy in layout `storage` (kAltFlag / kPlainF32Flag / kStencilF32Flag) straight from the
// 8^3 z-pair bricks: the same bytes as launch_unbrick + launch_brick_from_linear.  kYMajorFlag:
// the y-major copy (F32Y above), one pass of its own over the same bricks.
hipError_t launch_rebrick_f32(const float *src_bricks, void *dst, uint32_t nx, uint32_t ny,
                              uint32_t nz, int storage, hipStream_t stream);
// The binary16 field's scale: the largest k in [-120, 120] with B 2^k <= 65504, where
// B = max(vmax, 0) - min(vmin, 0) bounds every central difference of voxels in [vmin, vmax]
// (and of the zero border); 0 when B is 0 or not finite.  oracle/oracle.c restates it.
inline int field_scale_log2(float vmin, float vmax)
{
    const double B = (double)(vmax > 0.0f ? vmax : 0.0f) - (double)(vmin < 0.0f ? vmin : 0.0f);
    if (!(B > 0.0) || B > 1e300) return 0;
    int k = 0;
    while (k > -120 && B * std::ldexp(1.0, k) > 65504.0) --k;
    while (k < 120 && B * std::ldexp(1.0, k + 1) <= 65504.0) ++k;
    return k;
}
hipError_t launch_brick_range(int storage, const void *bricks, uint32_t nbx, uint32_t nby,
                              uint32_t nbz, float2 *range_dev, hipStream_t stream);
hipError_t launch_skip_dist(const float2 *range_dev, uint32_t nbx, uint32_t nby, uint32_t nbz,
                            const uint32_t *tf_nz_dev, int tf_n, float vmin, float vrange,
                            uint8_t *dist_dev, uint8_t *scratch_dev, hipStream_t stream);

#ifdef VR_WG_TIMES
hipError_t debug_wg_times_reset();
hipError_t debug_wg_times_read(unsigned long long *out, unsigned int max, unsigned int *count);
#endif

}  // namespace vr
