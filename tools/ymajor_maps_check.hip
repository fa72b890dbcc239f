// Host check of the y-major index maps (csrc/vr_internal.h) over given volume sizes: no device
// is touched.  For every brick slot and in-brick element as the builders place them
// (rebrick_ymajor_kernel, grad_field_kernel with ymajor), the march's addressing
// (ymajor_cell_offset, the element of both the copy and the y-major field) must name the same
// element, inside the allocation; and the z-major field element the fallback form reads
// (brick_slot order, zmajor_local) must lie inside its allocation too and be hit exactly once.
// Usage: ymajor_maps_check NX NY NZ [NX NY NZ ...]; prints "ok" per volume, exit 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../volumetric-renderer_amd/csrc/vr_internal.h"

using namespace vr;

static bool check(uint32_t nx, uint32_t ny, uint32_t nz)
{
    using G = GeomWide;
    const uint32_t nbx = bricks_for(nx, 0, ST_F32), nby = bricks_for(ny, 1, ST_F32),
                   nbz = bricks_for(nz, 2, ST_F32);
    const size_t nbricks = (size_t)nbx * nby * nbz, total = nbricks * (size_t)G::Elems;
    std::vector<unsigned char> ycopy(total, 0), zfield(total, 0);
    size_t bad = 0;
    for (size_t slot = 0; slot < nbricks; ++slot) {
        uint32_t bx, by, bz;
        ymajor_coords((uint32_t)slot, nbx, nbz, bx, by, bz);  // the builders' brick of this slot
        if (bx >= nbx || by >= nby || bz >= nbz) return false;
        for (uint32_t l = 0; l < (uint32_t)(G::EX * G::EY * G::EZ); ++l) {
            // rebrick_ymajor_kernel's decomposition of l; grad_field_kernel stores the element
            // of (lx, ly, lz) at ymajor_local(lx, ly, lz), which must be the same l
            const uint32_t lx = l % G::EX, lzy = l / G::EX, lz = lzy % G::EZ, ly = lzy / G::EZ;
            if (ymajor_local(lx, ly, lz) != l) ++bad;
            if (lx >= (uint32_t)G::BX || ly >= (uint32_t)G::BY || lz >= (uint32_t)G::BZ) continue;
            // a cell: what the march computes for its padded coordinates
            const uint32_t pi = bx * G::BX + lx, pj = by * G::BY + ly, pk = bz * G::BZ + lz;
            const size_t e = ymajor_cell_offset(pi, pj, pk, nbx, nbz);
            if (e != slot * (size_t)G::Elems + l || e >= total) ++bad;
            if (e < total && ycopy[e]++) ++bad;
            const size_t z = (size_t)brick_slot(bx, by, bz, nbx, nby) * (size_t)G::Elems +
                             zmajor_local(lx, ly, lz);
            if (z >= total || zfield[z]++) ++bad;
        }
    }
    // every padded cell the march can address, [kPad - 1, n + kPad] per axis, is inside
    for (uint32_t pk = 1; pk <= nz + kPad; ++pk)
        for (uint32_t pj = 1; pj <= ny + kPad; ++pj)
            for (uint32_t pi = 1; pi <= nx + kPad; ++pi)
                if (ymajor_cell_offset(pi, pj, pk, nbx, nbz) + G::EX + 1 >= total) ++bad;
    std::printf("%u x %u x %u: bricks %u x %u x %u, %s\n", nx, ny, nz, nbx, nby, nbz,
                bad ? "MISMATCH" : "ok");
    return bad == 0;
}

int main(int argc, char **argv)
{
    bool ok = argc >= 4 && (argc - 1) % 3 == 0;
    for (int i = 1; ok && i + 2 < argc; i += 3)
        ok = check((uint32_t)std::atoi(argv[i]), (uint32_t)std::atoi(argv[i + 1]),
                   (uint32_t)std::atoi(argv[i + 2]));
    return ok ? 0 : 1;
}
