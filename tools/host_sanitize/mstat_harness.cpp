// mstat_harness.cpp — the host side of include/vr/vr_mstat.h (csrc/vr_mstat_host.h: what a request is
// refused for, the grid it resolves to, the overlap and capacity rules, the launch geometry and
// scratch layout of the passes, and the voxel-to-element addressing the kernels share) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_mstat_cpu.py.  It checks
// every rule itself (exit status 1 on a mismatch) and prints the resolved grids and geometries, which
// the test compares with its own statement of the rule.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/vr/vr_mstat.h"
#include "../../volumetric-renderer_amd/csrc/vr_mstat_host.h"
#include "harness_check.h"

using namespace vr;

static_assert(sizeof(vr_mstat_region) == 64 && sizeof(vr_mstat_info) == 32, "vr_mstat.h structs");
static_assert(sizeof(vr_mstat_region) == kMstatRecordBytes && sizeof(vr_label_component) == kMstatRecordBytes, "records");
static_assert(VR_MSTAT_MAX_EXTENT == kMaskMaxExtent && VR_MSTAT_NONE == kMstatNone, "vr_mstat.h constants");
static_assert(VR_EINVAL == kMaskEinval && VR_ENOSPC == kMaskEnospc && VR_OK == kMaskOk, "codes");
static_assert(VR_HIST_MAX_BINS == kHistMaxBins, "vr_hist.h");

static void grid_case(uint32_t bx, uint32_t by, uint32_t bz, uint64_t nrec)
{
    // the array sits at the very end of a heap block: a read past [2] is an ASan report
    std::vector<uint32_t> ext{bx, by, bz};
    MaskGrid g;
    std::memset(&g, 0x77, sizeof g);
    const MaskGrid before = g;
    const char *m = kMstatTexts[mask_grid_resolve(ext.data(), &g)];
    bool want = true;
    unsigned long long vox = 1;
    for (uint32_t e : ext) {
        want = want && e >= 1 && e <= 32768;
        vox *= want ? e : 1;
    }
    want = want && vox <= 0xFFFFFFFFull;
    CHECK((m == nullptr) == want);
    if (m) CHECK(std::memcmp(&g, &before, sizeof g) == 0);  // untouched
    MstatGeom G;
    std::memset(&G, 0, sizeof G);
    if (!m) {
        CHECK(g.voxels == vox && g.ext[0] == bx && g.ext[1] == by && g.ext[2] == bz);
        G = mstat_geometry(g, nrec);
        CHECK((unsigned long long)G.tiles_x * kMstatTileX >= bx && (G.tiles_x - 1ull) * kMstatTileX < bx);
        CHECK((unsigned long long)G.tiles_y * kMstatTileY >= by && (G.tiles_y - 1ull) * kMstatTileY < by);
        CHECK(G.tiles == (unsigned long long)G.tiles_x * G.tiles_y * bz && G.tiles >= 1 && G.tiles <= vox);
        CHECK(G.grid >= 1 && G.grid <= kMstatMaxGrid && G.grid <= G.tiles);
        CHECK(G.rec_grid >= 1 && G.rec_grid <= kMstatMaxGrid);
        // the scratch: the parts in order, none overlapping, the 64-bit ones 8-byte aligned
        CHECK(G.cnt == 0 && G.bins == 64 && G.edges == G.bins + 8 * 4096 && G.acc == G.edges + 4 * 4096);
        CHECK(G.acc % 8 == 0 && G.rec == G.acc + nrec * 48 && G.rec % 8 == 0 && G.lab == G.rec + nrec * 64);
        CHECK(G.bytes == G.lab + nrec * 4);
    }
    std::printf("grid %u %u %u %llu: %d %llu  %u %u %llu %u %u %zu\n", bx, by, bz, (unsigned long long)nrec,
                (int)(m == nullptr), m ? 0ull : vox, G.tiles_x, G.tiles_y, (unsigned long long)G.tiles, G.grid,
                G.rec_grid, G.bytes);
}

// hist_kernel's addressing, restated with the bricks' numbers spelled out
static unsigned long long element_restated(int kind, uint32_t nbx, uint32_t nby, uint32_t x, uint32_t y, uint32_t z)
{
    const unsigned long long BX = kind == kMstatPlain8 ? 7 : 8, BY = 8, BZ = 8;
    const unsigned long long EX = BX + 1, EY = BY + 1, EZ = BZ + 1;
    const unsigned long long elems = EX * EY * EZ;
    const unsigned long long px = x + 2ull, py = y + 2ull, pz = z + 2ull;
    const unsigned long long bx = px / BX, by = py / BY, bz = pz / BZ;
    const unsigned long long slot = (bz * nby + by) * nbx + bx;
    return slot * elems + ((pz % BZ) * EY + py % BY) * EX + px % BX;
}

static void addressing()
{
    unsigned long long total = 0;
    for (int kind = 0; kind < kMstatKinds; ++kind) {
        const MstatLayout L = mstat_layout(kind);
        CHECK(L.elems == L.ex * L.ey * (L.bz + 1) && L.ex == L.bx + 1 && L.ey == L.by + 1);
        CHECK(L.vpe == (kind == kMstatF32 ? 2u : kind == kMstatPlain8 ? 1u : 4u));
        CHECK(L.bx == (kind == kMstatPlain8 ? 7u : 8u) && L.by == 8 && L.bz == 8);
        std::vector<uint32_t> stamp;
        uint32_t round = 0;
        for (uint32_t nz = 1; nz <= 15; ++nz)
            for (uint32_t ny = 1; ny <= 15; ++ny)
                for (uint32_t nx = 1; nx <= 15; ++nx) {
                    const uint32_t nbx = mstat_bricks(nx, L.bx), nby = mstat_bricks(ny, L.by), nbz = mstat_bricks(nz, L.bz);
                    CHECK(nbx == (nx + 3) / L.bx + 1);
                    const size_t buffer = (size_t)nbx * nby * nbz * L.elems;  // the brick buffer, in elements
                    if (stamp.size() < buffer) stamp.resize(buffer, 0);
                    ++round;
                    bool ok = true;
                    for (uint32_t z = 0; z < nz; ++z)
                        for (uint32_t y = 0; y < ny; ++y)
                            for (uint32_t x = 0; x < nx; ++x) {
                                const uint64_t e = mstat_element(L, nbx, nby, x, y, z);
                                ok = ok && e < buffer && e == element_restated(kind, nbx, nby, x, y, z);
                                if (e < buffer) {
                                    ok = ok && stamp[e] != round;  // distinct
                                    stamp[e] = round;
                                }
                                ++total;
                            }
                    CHECK(ok);
                }
    }
    // a 2048^3 volume's last voxel: the element index passes 32 bits and stays exact
    const MstatLayout W = mstat_layout(kMstatF32);
    const uint32_t nb = mstat_bricks(2048, 8);
    CHECK(mstat_element(W, nb, nb, 2047, 2047, 2047) == element_restated(kMstatF32, nb, nb, 2047, 2047, 2047));
    CHECK(mstat_element(W, nb, nb, 2047, 2047, 2047) > 0xFFFFFFFFull);
    std::printf("addressing %llu voxels\n", total);
}

int main()
{
    const uint32_t M = 0xFFFFFFFFu;
    const uint32_t grids[][3] = {{1, 1, 1}, {70, 33, 19}, {129, 5, 3}, {257, 1, 1}, {1, 300, 1}, {1, 1, 257},
                                 {64, 64, 64}, {130, 70, 33}, {128, 96, 80}, {2, 2, 2}, {17, 9, 5}, {65, 65, 1},
                                 {130, 33, 4}, {512, 512, 512}, {1024, 1024, 1024}, {32768, 1, 1}, {1, 32768, 1},
                                 {1, 1, 32768}, {8192, 1, 1}, {8193, 1, 1}, {63, 4, 2}, {64, 4, 2}, {65, 4, 2},
                                 {64, 5, 2}, {32768, 32768, 3}, {32768, 32768, 4}, {2048, 2048, 1024},
                                 {2048, 2048, 1023}, {1, 32768, 32768}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}, {32769, 1, 1},
                                 {1, 32769, 1}, {1, 1, 32769}, {M, 1, 1}, {M, M, M}, {32768, 32768, 32768}};
    const uint64_t nrecs[] = {0, 1, 255, 256, 257, 690123, 0xFFFFFFFFull};
    int i = 0;
    for (const auto &g : grids) grid_case(g[0], g[1], g[2], nrecs[i++ % 7]);

    addressing();

    {  // alignment and overlap
        alignas(8) static unsigned char buf[64] = {0};
        CHECK(mask_aligned4(buf) && mask_aligned4(buf + 4) && !mask_aligned4(buf + 1) && !mask_aligned4(buf + 2) &&
              !mask_aligned4(buf + 3));
        CHECK(mask_overlap(buf, 8, buf, 8) && mask_overlap(buf, 8, buf + 7, 1) && mask_overlap(buf + 7, 1, buf, 8));
        CHECK(!mask_overlap(buf, 8, buf + 8, 8) && !mask_overlap(buf + 8, 8, buf, 8));
        CHECK(mask_overlap(buf, 64, buf + 20, 4) && mask_overlap(buf + 20, 4, buf, 64));
    }
    {  // the grid against the volume
        MaskGrid g;
        const uint32_t ext[3] = {4, 3, 2}, dims[3] = {10, 9, 8};
        CHECK(!mask_grid_resolve(ext, &g));
        const uint32_t ok[][3] = {{0, 0, 0}, {6, 6, 6}, {6, 0, 0}, {0, 6, 0}, {0, 0, 6}};
        const uint32_t bad[][3] = {{7, 0, 0}, {0, 7, 0}, {0, 0, 7}, {M, 0, 0}, {0, M - 1, 0}, {0, 0, M - 2}, {M, M, M}, {10, 9, 8}};
        for (const auto &o : ok) {
            std::memcpy(g.origin, o, sizeof g.origin);
            CHECK(mstat_origin_error(g, dims) == nullptr);
        }
        for (const auto &o : bad) {
            std::memcpy(g.origin, o, sizeof g.origin);
            CHECK(mstat_origin_error(g, dims) != nullptr);
        }
    }
    {  // the request checks: every refusal leaves the grid untouched; ENOSPC resolves it
        alignas(8) static unsigned char mask[4 * 24 + 8], out[64 * 24 + 8], tab[64 * 5 + 8];
        const uint32_t ext[3] = {4, 3, 2}, bad[3] = {4, 0, 2}, org[3] = {5, 6, 7};
        const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
        vr_mstat_region reg;
        vr_mstat_info mi;
        vr_morph_info wi;
        vr_hist_info hi;
        uint64_t bins[8];
        const char *msg = nullptr;
        MaskGrid g;
        auto fresh = [&] { std::memset(&g, 0x77, sizeof g); };
        auto untouched = [&] {
            MaskGrid f;
            std::memset(&f, 0x77, sizeof f);
            return std::memcmp(&g, &f, sizeof g) == 0;
        };
        // vr_mask_stats*
        auto stats = [&](const uint32_t *e, const uint32_t *o, const void *m, uint32_t eb, bool have, uint32_t use_box,
                         float lo, float hi_, uint32_t nbins, const void *b, const void *h, const void *r, bool dev) {
            return mstat_check_stats(e, o, m, eb, have, use_box, lo, hi_, nbins, b, h, r, dev, &g, &msg);
        };
        fresh();
        CHECK(stats(ext, org, mask, 1, false, 0, 0, 0, 0, nullptr, nullptr, &reg, true) == 0 && g.voxels == 24 && !msg);
        CHECK(g.origin[0] == 5 && g.origin[1] == 6 && g.origin[2] == 7 && g.ext[0] == 4 && g.ext[2] == 2);
        CHECK(stats(ext, org, mask + 1, 1, true, 0, 0.0f, 1.0f, 8, bins, &hi, &reg, true) == 0);
        CHECK(stats(ext, org, mask, 4, true, 0, -1.0f, 1.0f, 4096, bins, &hi, &reg, true) == 0);
        fresh();
        CHECK(stats(nullptr, org, mask, 1, false, 0, 0, 0, 0, nullptr, nullptr, &reg, true) == -22 && msg && untouched());
        CHECK(stats(ext, nullptr, mask, 1, false, 0, 0, 0, 0, nullptr, nullptr, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, nullptr, 1, false, 0, 0, 0, 0, nullptr, nullptr, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, false, 0, 0, 0, 0, nullptr, nullptr, nullptr, true) == -22 && untouched());
        // hist, bins and hinfo: NULL together or not at all
        CHECK(stats(ext, org, mask, 1, false, 0, 0, 0, 0, bins, nullptr, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, false, 0, 0, 0, 0, nullptr, &hi, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, false, 0, 0, 0, 0, bins, &hi, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, true, 0, 0.0f, 1.0f, 8, nullptr, &hi, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, true, 0, 0.0f, 1.0f, 8, bins, nullptr, &reg, true) == -22 && untouched());
        CHECK(stats(bad, org, mask, 1, false, 0, 0, 0, 0, nullptr, nullptr, &reg, true) == -22 && untouched());
        for (uint32_t eb : {0u, 2u, 3u, 5u, 8u, M})
            CHECK(stats(ext, org, mask, eb, false, 0, 0, 0, 0, nullptr, nullptr, &reg, true) == -22 && untouched());
        for (int off = 1; off < 4; ++off) {
            CHECK(stats(ext, org, mask + off, 4, false, 0, 0, 0, 0, nullptr, nullptr, &reg, true) == -22 && untouched());
            CHECK(stats(ext, org, mask + off, 4, false, 0, 0, 0, 0, nullptr, nullptr, &reg, false) == 0);  // a host array
            fresh();
        }
        for (uint32_t ub : {1u, 2u, M})
            CHECK(stats(ext, org, mask, 1, true, ub, 0.0f, 1.0f, 8, bins, &hi, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, true, 0, 1.0f, 1.0f, 8, bins, &hi, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, true, 0, 2.0f, 1.0f, 8, bins, &hi, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, true, 0, nan, 1.0f, 8, bins, &hi, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, true, 0, 0.0f, inf, 8, bins, &hi, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, true, 0, -inf, 0.0f, 8, bins, &hi, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, true, 0, 0.0f, 1.0f, 0, bins, &hi, &reg, true) == -22 && untouched());
        CHECK(stats(ext, org, mask, 1, true, 0, 0.0f, 1.0f, 4097, bins, &hi, &reg, true) == -22 && untouched());

        // vr_label_stats*
        auto labels = [&](const uint32_t *e, const uint32_t *o, const void *l, const void *t, uint64_t nt, const void *r,
                          uint64_t rcap, const void *info, bool dev) {
            return mstat_check_labels(e, o, l, t, nt, r, rcap, info, dev, &g, &msg);
        };
        fresh();
        CHECK(labels(ext, org, mask, tab, 5, out, 5, &mi, true) == 0 && g.voxels == 24 && !msg);
        CHECK(labels(ext, org, mask, tab + 1, 5, out + 3, 24, &mi, true) == 0);  // the table and the records anywhere
        CHECK(labels(ext, org, mask, tab, 0, out, 0, &mi, true) == 0);           // an empty table
        CHECK(labels(ext, org, mask, tab, 0xFFFFFFFFull, out, 0, &mi, true) == -28);  // the largest table is a table
        fresh();
        CHECK(labels(nullptr, org, mask, tab, 5, out, 5, &mi, true) == -22 && msg && untouched());
        CHECK(labels(ext, nullptr, mask, tab, 5, out, 5, &mi, true) == -22 && untouched());
        CHECK(labels(ext, org, nullptr, tab, 5, out, 5, &mi, true) == -22 && untouched());
        CHECK(labels(ext, org, mask, nullptr, 5, out, 5, &mi, true) == -22 && untouched());
        CHECK(labels(ext, org, mask, tab, 5, nullptr, 5, &mi, true) == -22 && untouched());
        CHECK(labels(ext, org, mask, tab, 5, out, 5, nullptr, true) == -22 && untouched());
        CHECK(labels(bad, org, mask, tab, 5, out, 5, &mi, true) == -22 && untouched());
        CHECK(labels(ext, org, mask, tab, 0x100000000ull, out, 0x100000000ull, &mi, true) == -22 && untouched());
        CHECK(labels(ext, org, mask, tab, 0x100000000ull, out, 0, &mi, true) == -22 && untouched());  // EINVAL before ENOSPC
        for (int off = 1; off < 4; ++off) {
            CHECK(labels(ext, org, mask + off, tab, 5, out, 5, &mi, true) == -22 && untouched());
            CHECK(labels(ext, org, mask + off, tab, 5, out, 5, &mi, false) == 0);
            fresh();
        }
        CHECK(labels(ext, org, mask, tab, 1, mask + 95, 1, &mi, true) == -22 && untouched());  // the records on the labels
        CHECK(labels(ext, org, mask, tab, 5, tab + 319, 5, &mi, true) == -22 && untouched());  // ... on the table
        CHECK(labels(ext, org, mask, out, 5, out + 64, 5, &mi, true) == -22 && untouched());
        CHECK(labels(ext, org, mask, tab, 5, mask + 95, 0, &mi, true) == -28 && g.voxels == 24);  // no record is written
        fresh();
        CHECK(labels(ext, org, mask, tab, 5, out, 4, &mi, true) == -28 && g.voxels == 24 && msg);
        CHECK(labels(ext, org, mask, tab, 1, out, 0, &mi, true) == -28 && g.voxels == 24);

        // vr_mask_window*
        auto window = [&](const uint32_t *e, const uint32_t *o, const void *m, uint32_t eb, float lo, float hi_,
                          const void *ob, uint64_t mcap, const void *info, bool dev) {
            return mstat_check_window(e, o, m, eb, lo, hi_, ob, mcap, info, dev, &g, &msg);
        };
        fresh();
        CHECK(window(ext, org, mask, 1, 0.0f, 1.0f, out, 24, &wi, true) == 0 && g.voxels == 24 && !msg);
        CHECK(window(ext, org, nullptr, 1, -inf, inf, out + 1, 1000, &wi, true) == 0);  // no mask; infinite bounds
        CHECK(window(ext, org, nullptr, 4, 1.0f, 1.0f, out + 1, 24, &wi, true) == 0);   // lo == hi
        CHECK(window(ext, org, mask, 4, 0.0f, 1.0f, out + 3, 24, &wi, true) == 0);
        fresh();
        CHECK(window(nullptr, org, mask, 1, 0.0f, 1.0f, out, 24, &wi, true) == -22 && msg && untouched());
        CHECK(window(ext, nullptr, mask, 1, 0.0f, 1.0f, out, 24, &wi, true) == -22 && untouched());
        CHECK(window(ext, org, mask, 1, 0.0f, 1.0f, nullptr, 24, &wi, true) == -22 && untouched());
        CHECK(window(ext, org, mask, 1, 0.0f, 1.0f, out, 24, nullptr, true) == -22 && untouched());
        CHECK(window(bad, org, mask, 1, 0.0f, 1.0f, out, 24, &wi, true) == -22 && untouched());
        for (uint32_t eb : {0u, 2u, 3u, 5u, M}) {
            CHECK(window(ext, org, mask, eb, 0.0f, 1.0f, out, 24, &wi, true) == -22 && untouched());
            CHECK(window(ext, org, nullptr, eb, 0.0f, 1.0f, out, 24, &wi, true) == -22 && untouched());
        }
        CHECK(window(ext, org, mask + 2, 4, 0.0f, 1.0f, out, 24, &wi, true) == -22 && untouched());
        CHECK(window(ext, org, mask, 1, nan, 1.0f, out, 24, &wi, true) == -22 && untouched());
        CHECK(window(ext, org, mask, 1, 0.0f, nan, out, 24, &wi, true) == -22 && untouched());
        CHECK(window(ext, org, mask, 1, 1.0f, 0.0f, out, 24, &wi, true) == -22 && untouched());
        CHECK(window(ext, org, mask, 1, inf, -inf, out, 0, &wi, true) == -22 && untouched());  // EINVAL before ENOSPC
        CHECK(window(ext, org, mask, 1, 0.0f, 1.0f, mask + 23, 24, &wi, true) == -22 && untouched());
        CHECK(window(ext, org, mask, 4, 0.0f, 1.0f, mask + 95, 24, &wi, true) == -22 && untouched());
        CHECK(window(ext, org, mask, 1, 0.0f, 1.0f, mask + 24, 24, &wi, true) == 0);
        fresh();
        CHECK(window(ext, org, mask, 1, 0.0f, 1.0f, out, 23, &wi, true) == -28 && g.voxels == 24 && msg);
        CHECK(window(ext, org, nullptr, 1, 0.0f, 1.0f, out, 0, &wi, true) == -28 && g.voxels == 24);
    }
    return harness_done("mstat");
}
