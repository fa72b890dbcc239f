// maskcc_harness.cpp — the host side of include/vr/vr_maskcc.h (csrc/vr_maskcc_host.h: what a
// labelling or selection request is refused for, the grid it resolves to, the overlap and capacity
// rules, and the launch geometry and scratch layout of the passes) as a stand-alone program, built
// with -fsanitize=address,undefined by tests/test_maskcc_cpu.py.  It checks every rule itself (exit
// status 1 on a mismatch) and prints the resolved grids and geometries, which the test compares
// with its own statement of the rule.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vr/vr_maskcc.h"
#include "../../volumetric-renderer_amd/csrc/vr_maskcc_host.h"
#include "harness_check.h"

using namespace vr;

static_assert(sizeof(vr_mask_select_request) == 32 && sizeof(vr_mask_select_info) == 40, "vr_maskcc.h structs");
static_assert(sizeof(vr_label_component) == kMccRecordBytes && sizeof(vr_label_info) == 40, "vr_label.h structs");
static_assert(VR_MASKCC_MAX_EXTENT == kMaskMaxExtent, "vr_maskcc.h constants");
static_assert(VR_EINVAL == kMaskEinval && VR_ENOSPC == kMaskEnospc && VR_OK == kMaskOk, "codes");
static_assert(VR_MASK_FILL_HOLES + 1 == kMccRules && VR_MASK_KEEP_SEED == kMccKeepSeed &&
                  VR_MASK_KEEP_LARGEST == kMccKeepLargest && VR_MASK_KEEP_MIN_VOXELS == kMccKeepMinVoxels &&
                  VR_MASK_FILL_HOLES == kMccFillHoles, "enum vr_mask_rule");

static void grid_case(uint32_t bx, uint32_t by, uint32_t bz)
{
    // the array sits at the very end of a heap block: a read past [2] is an ASan report
    std::vector<uint32_t> ext{bx, by, bz};
    MaskGrid g;
    std::memset(&g, 0x77, sizeof g);
    const MaskGrid before = g;
    const char *m = kMccTexts[mask_grid_resolve(ext.data(), &g)];
    bool want = true;
    unsigned long long vox = 1;
    for (uint32_t e : ext) {
        want = want && e >= 1 && e <= 32768;
        vox *= want ? e : 1;
    }
    want = want && vox <= 0xFFFFFFFFull;
    CHECK((m == nullptr) == want);
    if (m) CHECK(std::memcmp(&g, &before, sizeof g) == 0);  // untouched
    MccGeom G;
    std::memset(&G, 0, sizeof G);
    if (!m) {
        CHECK(g.voxels == vox && g.ext[0] == bx && g.ext[1] == by && g.ext[2] == bz);
        G = mcc_geometry(g);
        CHECK(G.rows * bx == vox && (unsigned long long)G.row_words * 64 >= bx && (G.row_words - 1ull) * 64 < bx);
        CHECK(G.row_grid >= 1 && G.row_grid <= kMccMaxGrid && G.sweep_grid >= 1 && G.sweep_grid <= kMccMaxGrid);
        CHECK((unsigned long long)G.nwords * 64 >= vox && (G.nwords - 1ull) * 64 < vox);
        CHECK((unsigned long long)G.nchunks * kMccChunk >= vox && (G.nchunks - 1ull) * kMccChunk < vox);
        CHECK((unsigned long long)G.nchunks * kMccChunkWords >= G.nwords);  // every word has its chunk
        // the scratch: the parts in order, none overlapping, the 64-bit ones 8-byte aligned
        CHECK(G.bits == 0 && G.wpre == (size_t)G.nwords * 8 && G.chunk == G.wpre + (size_t)G.nwords * 4);
        CHECK(G.cnt >= G.chunk + (size_t)G.nchunks * 4 && G.cnt % 8 == 0 && G.cnt < G.chunk + (size_t)G.nchunks * 4 + 8);
        CHECK(G.bytes == G.cnt + kMccCounters * 8);
    }
    std::printf("grid %u %u %u: %d %llu  %llu %u %u  %u %u %u %zu\n", bx, by, bz, (int)(m == nullptr), m ? 0ull : vox,
                (unsigned long long)G.rows, G.row_words, G.row_grid, G.nwords, G.nchunks, G.sweep_grid, G.bytes);
}

int main()
{
    const uint32_t M = 0xFFFFFFFFu;
    const uint32_t grids[][3] = {{1, 1, 1}, {70, 33, 19}, {129, 5, 3}, {257, 1, 1}, {1, 300, 1}, {1, 1, 257},
                                 {64, 64, 64}, {130, 9, 8}, {128, 96, 80}, {2, 2, 2}, {17, 9, 5}, {65, 65, 1},
                                 {130, 33, 4}, {512, 512, 512}, {1024, 1024, 1024}, {32768, 1, 1}, {1, 32768, 1},
                                 {1, 1, 32768}, {8192, 1, 1}, {8193, 1, 1}, {63, 4, 2}, {64, 4, 2}, {65, 4, 2},
                                 {32768, 32768, 3}, {32768, 32768, 4}, {2048, 2048, 1024}, {2048, 2048, 1023},
                                 {1, 32768, 32768}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}, {32769, 1, 1}, {1, 32769, 1},
                                 {1, 1, 32769}, {M, 1, 1}, {M, M, M}, {32768, 32768, 32768}};
    for (const auto &g : grids) grid_case(g[0], g[1], g[2]);

    {  // alignment and overlap
        alignas(8) static unsigned char buf[64] = {0};
        CHECK(mask_aligned4(buf) && mask_aligned4(buf + 4) && !mask_aligned4(buf + 1) && !mask_aligned4(buf + 2) &&
              !mask_aligned4(buf + 3));
        CHECK(mask_overlap(buf, 8, buf, 8) && mask_overlap(buf, 8, buf + 7, 1) && mask_overlap(buf + 7, 1, buf, 8));
        CHECK(!mask_overlap(buf, 8, buf + 8, 8) && !mask_overlap(buf + 8, 8, buf, 8));
        CHECK(mask_overlap(buf, 64, buf + 20, 4) && mask_overlap(buf + 20, 4, buf, 64));
    }
    {  // the request checks: every refusal leaves the grid untouched; ENOSPC resolves it
        alignas(8) static unsigned char mask[4 * 24 + 8], out[4 * 24 + 64 * 24 + 8];  // (labels, then records)
        const uint32_t ext[3] = {4, 3, 2}, bad[3] = {4, 0, 2};
        vr_label_info li;
        vr_mask_select_info si;
        const char *msg = nullptr;
        MaskGrid g;
        auto fresh = [&] { std::memset(&g, 0x77, sizeof g); };
        auto untouched = [&] {
            MaskGrid f;
            std::memset(&f, 0x77, sizeof f);
            return std::memcmp(&g, &f, sizeof g) == 0;
        };
        unsigned char *lab = out, *rec = out + 4 * 24;  // (4-byte aligned both)
        auto label = [&](const uint32_t *e, const void *m, uint32_t eb, uint32_t conn, const void *l, uint64_t lcap,
                         const void *r, uint64_t ccap, const void *info, bool dev) {
            return mcc_check_label(e, m, eb, conn, l, lcap, r, ccap, info, dev, &g, &msg);
        };
        fresh();
        CHECK(label(ext, mask, 1, 6, lab, 24, rec, 24, &li, true) == 0 && g.voxels == 24 && !msg);
        CHECK(label(ext, mask, 4, 26, lab, 1000, rec, 0, &li, true) == 0);
        CHECK(label(ext, mask + 1, 1, 6, lab, 24, rec + 1, 5, &li, true) == 0);  // a 1-byte mask and records anywhere
        fresh();
        CHECK(label(nullptr, mask, 1, 6, lab, 24, rec, 24, &li, true) == -22 && msg && untouched());
        CHECK(label(ext, nullptr, 1, 6, lab, 24, rec, 24, &li, true) == -22 && untouched());
        CHECK(label(ext, mask, 1, 6, nullptr, 24, rec, 24, &li, true) == -22 && untouched());
        CHECK(label(ext, mask, 1, 6, lab, 24, nullptr, 24, &li, true) == -22 && untouched());
        CHECK(label(ext, mask, 1, 6, lab, 24, rec, 24, nullptr, true) == -22 && untouched());
        CHECK(label(bad, mask, 1, 6, lab, 24, rec, 24, &li, true) == -22 && untouched());
        for (uint32_t eb : {0u, 2u, 3u, 5u, 8u, M})
            CHECK(label(ext, mask, eb, 6, lab, 24, rec, 24, &li, true) == -22 && untouched());
        for (uint32_t conn : {0u, 4u, 8u, 18u, 27u, M}) {
            CHECK(label(ext, mask, 1, conn, lab, 24, rec, 24, &li, true) == -22 && untouched());
            CHECK(label(ext, mask, 1, conn, lab, 0, rec, 24, &li, true) == -22 && untouched());  // EINVAL before ENOSPC
        }
        for (int off = 1; off < 4; ++off) {
            CHECK(label(ext, mask + off, 4, 6, lab, 24, rec, 24, &li, true) == -22 && untouched());
            CHECK(label(ext, mask, 1, 6, lab + off, 24, rec, 24, &li, true) == -22 && untouched());
            CHECK(label(ext, mask + off, 4, 6, lab + off, 24, rec, 24, &li, false) == 0);  // host arrays
            fresh();
        }
        CHECK(label(ext, mask, 4, 6, mask, 24, rec, 24, &li, true) == -22 && untouched());       // overlap
        CHECK(label(ext, mask, 4, 6, mask + 92, 24, rec, 24, &li, true) == -22 && untouched());
        CHECK(label(ext, mask + 96, 1, 6, mask, 24, rec, 24, &li, true) == 0);
        fresh();
        CHECK(label(ext, mask, 1, 6, lab, 24, mask + 23, 24, &li, true) == -22 && untouched());
        CHECK(label(ext, mask, 1, 6, lab, 24, mask + 23, 0, &li, true) == 0);  // no record is written
        fresh();
        CHECK(label(ext, mask, 1, 6, lab, 23, rec, 24, &li, true) == -28 && g.voxels == 24 && msg);
        CHECK(label(ext, mask, 1, 26, lab, 0, rec, 0, &li, true) == -28 && g.voxels == 24);

        auto select = [&](const uint32_t *e, bool have, uint32_t rule, uint32_t conn, const uint32_t *seed,
                          const void *m, uint32_t eb, const void *o, uint64_t mcap, const void *info, bool dev) {
            return mcc_check_select(e, have, rule, conn, seed, m, eb, o, mcap, info, dev, &g, &msg);
        };
        const uint32_t in[3] = {3, 2, 1}, outx[3] = {4, 0, 0}, outy[3] = {0, 3, 0}, outz[3] = {0, 0, 2}, far[3] = {M, M, M};
        fresh();
        for (uint32_t rule = 0; rule < 4; ++rule)
            for (uint32_t conn : {6u, 26u})
                CHECK(select(ext, true, rule, conn, in, mask, 1, out, 24, &si, true) == 0 && g.voxels == 24);
        CHECK(select(ext, true, 0, 6, far, mask, 4, out + 1, 24, &si, true) == 0);  // the seed is KEEP_SEED's alone
        CHECK(select(ext, true, 3, 6, far, mask, 4, out + 1, 24, &si, true) == 0);
        fresh();
        for (const uint32_t *s : {outx, outy, outz, far}) {
            CHECK(select(ext, true, 2, 6, s, mask, 1, out, 24, &si, true) == -22 && msg && untouched());
            CHECK(select(ext, true, 2, 6, s, mask, 1, out, 0, &si, true) == -22 && untouched());
        }
        for (uint32_t rule : {4u, 5u, M}) CHECK(select(ext, true, rule, 6, in, mask, 1, out, 24, &si, true) == -22 && untouched());
        for (uint32_t conn : {0u, 18u, M}) CHECK(select(ext, true, 0, conn, in, mask, 1, out, 24, &si, true) == -22 && untouched());
        CHECK(select(ext, false, 0, 6, nullptr, mask, 1, out, 24, &si, true) == -22 && untouched());
        CHECK(select(nullptr, true, 0, 6, in, mask, 1, out, 24, &si, true) == -22 && untouched());
        CHECK(select(ext, true, 0, 6, in, nullptr, 1, out, 24, &si, true) == -22 && untouched());
        CHECK(select(ext, true, 0, 6, in, mask, 1, nullptr, 24, &si, true) == -22 && untouched());
        CHECK(select(ext, true, 0, 6, in, mask, 1, out, 24, nullptr, true) == -22 && untouched());
        CHECK(select(bad, true, 0, 6, in, mask, 1, out, 24, &si, true) == -22 && untouched());
        CHECK(select(ext, true, 0, 6, in, mask, 3, out, 24, &si, true) == -22 && untouched());
        CHECK(select(ext, true, 0, 6, in, mask + 2, 4, out, 24, &si, true) == -22 && untouched());
        CHECK(select(ext, true, 0, 6, in, mask, 1, mask + 23, 24, &si, true) == -22 && untouched());
        CHECK(select(ext, true, 0, 6, in, mask, 4, mask + 95, 24, &si, true) == -22 && untouched());
        CHECK(select(ext, true, 0, 6, in, mask, 1, out, 23, &si, true) == -28 && g.voxels == 24);
        const uint32_t last[3] = {3, 2, 1};
        CHECK(mcc_linear(g, last) == 23);
    }
    return harness_done("maskcc");
}
