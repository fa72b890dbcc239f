// morph_harness.cpp — the host side of include/vr/vr_morph.h (csrc/vr_morph_host.h: what a request
// is refused for, the grid it resolves to, the overlap and capacity rules and the tiles of an axis
// pass) as a stand-alone program, built with -fsanitize=address,undefined by tests/
// test_morph_cpu.py.  It checks every rule itself (exit status 1 on a mismatch) and prints the
// resolved grids and tilings, which the test compares with its own statement of the rule.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vr/vr_morph.h"
#include "../../volumetric-renderer_amd/csrc/vr_morph_host.h"
#include "harness_check.h"

using namespace vr;

static_assert(sizeof(vr_edt_info) == 24 && sizeof(vr_morph_info) == 24, "vr_morph.h infos are 24 bytes");
static_assert(VR_EDT_NONE == kMorphNone && VR_MORPH_MAX_EXTENT == kMaskMaxExtent, "vr_morph.h constants");
static_assert(VR_EINVAL == kMaskEinval && VR_ENOSPC == kMaskEnospc && VR_OK == kMaskOk, "codes");
static_assert(VR_MORPH_CLOSE + 1 == kMorphOps && VR_EDT_TO_UNSET + 1 == kMorphTargets, "enums");
static_assert(3ull * 32767 * 32767 < VR_EDT_NONE, "the largest distance stays below the sentinel");

static void grid_case(uint32_t bx, uint32_t by, uint32_t bz)
{
    // the array sits at the very end of a heap block: a read past [2] is an ASan report
    std::vector<uint32_t> ext{bx, by, bz};
    MaskGrid g;
    std::memset(&g, 0x77, sizeof g);
    const MaskGrid before = g;
    const char *m = kMorphTexts[mask_grid_resolve(ext.data(), &g)];
    bool want = true;
    unsigned long long vox = 1;
    for (uint32_t e : ext) {
        want = want && e >= 1 && e <= 32768;
        vox *= want ? e : 1;
    }
    want = want && vox <= 0xFFFFFFFFull;
    CHECK((m == nullptr) == want);
    if (m) CHECK(std::memcmp(&g, &before, sizeof g) == 0);  // untouched
    unsigned long long tiles[3] = {0, 0, 0}, width[3] = {0, 0, 0};
    if (!m) {
        CHECK(g.voxels == vox && g.ext[0] == bx && g.ext[1] == by && g.ext[2] == bz);
        for (int axis = 1; axis <= 2; ++axis) {
            const MorphAxis A = morph_axis(g, axis);
            const unsigned long long w = 1ull << A.width_log2;
            CHECK(A.n == ext[axis] && A.width_log2 <= 6);
            CHECK(A.lds_words == (A.n > kMorphLdsWords ? kMorphLdsWordsLong : kMorphLdsWords));
            CHECK(w * A.n <= A.lds_words);                                     // the tile fits
            CHECK(A.width_log2 == 6 || 2 * w * A.n > A.lds_words);            // and is the widest that does
            CHECK(A.line == (axis == 1 ? bx : (unsigned long long)bx * by) && A.slabs == (axis == 1 ? bz : 1u));
            CHECK(A.tiles_line * w >= A.line && (A.tiles_line - 1) * w < A.line);  // the tiles cover a line, no more
            CHECK(A.tiles == A.slabs * A.tiles_line && A.slabs * A.line * A.n == g.voxels);
            tiles[axis] = A.tiles;
            width[axis] = w;
        }
    }
    std::printf("grid %u %u %u: %d %llu  %llu %llu  %llu %llu\n", bx, by, bz, (int)(m == nullptr), m ? 0ull : vox,
                width[1], tiles[1], width[2], tiles[2]);
}

int main()
{
    const uint32_t M = 0xFFFFFFFFu;
    const uint32_t grids[][3] = {{1, 1, 1}, {70, 33, 19}, {129, 5, 3}, {257, 1, 1}, {1, 300, 1}, {1, 1, 257},
                                 {64, 64, 64}, {200, 160, 96}, {3, 16400, 1}, {512, 512, 512}, {1024, 1024, 1024},
                                 {32768, 1, 1}, {1, 32768, 1}, {1, 1, 32768}, {5, 16384, 2}, {5, 16385, 2},
                                 {7, 257, 3}, {7, 256, 3}, {32768, 32768, 3}, {32768, 32768, 4}, {2048, 2048, 1024},
                                 {2048, 2048, 1023}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}, {32769, 1, 1}, {1, 32769, 1},
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
        alignas(8) static unsigned char mask[4 * 24 + 8], out[4 * 24 + 8];
        const uint32_t ext[3] = {4, 3, 2}, bad[3] = {4, 0, 2};
        vr_edt_info ei;
        vr_morph_info mi;
        const char *msg = nullptr;
        MaskGrid g;
        auto fresh = [&] { std::memset(&g, 0x77, sizeof g); };
        auto untouched = [&] {
            MaskGrid f;
            std::memset(&f, 0x77, sizeof f);
            return std::memcmp(&g, &f, sizeof g) == 0;
        };
        fresh();
        CHECK(morph_check_edt(ext, mask, 1, 0, out, 24, &ei, true, &g, &msg) == 0 && g.voxels == 24 && !msg);
        CHECK(morph_check_edt(ext, mask, 4, 1, out, 1000, &ei, true, &g, &msg) == 0);
        CHECK(morph_check_edt(ext, mask + 1, 1, 0, out, 24, &ei, true, &g, &msg) == 0);  // a 1-byte mask anywhere
        fresh();
        CHECK(morph_check_edt(nullptr, mask, 1, 0, out, 24, &ei, true, &g, &msg) == -22 && msg && untouched());
        CHECK(morph_check_edt(ext, nullptr, 1, 0, out, 24, &ei, true, &g, &msg) == -22 && untouched());
        CHECK(morph_check_edt(ext, mask, 1, 0, nullptr, 24, &ei, true, &g, &msg) == -22 && untouched());
        CHECK(morph_check_edt(ext, mask, 1, 0, out, 24, nullptr, true, &g, &msg) == -22 && untouched());
        CHECK(morph_check_edt(bad, mask, 1, 0, out, 24, &ei, true, &g, &msg) == -22 && untouched());
        for (uint32_t eb : {0u, 2u, 3u, 5u, 8u, M})
            CHECK(morph_check_edt(ext, mask, eb, 0, out, 24, &ei, true, &g, &msg) == -22 && untouched());
        for (int off = 1; off < 4; ++off) {
            CHECK(morph_check_edt(ext, mask + off, 4, 0, out, 24, &ei, true, &g, &msg) == -22 && untouched());
            CHECK(morph_check_edt(ext, mask, 1, 0, out + off, 24, &ei, true, &g, &msg) == -22 && untouched());
            CHECK(morph_check_edt(ext, mask + off, 4, 0, out + off, 24, &ei, false, &g, &msg) == 0);  // host arrays
            fresh();
        }
        CHECK(morph_check_edt(ext, mask, 1, 0, mask, 24, &ei, true, &g, &msg) == -22 && untouched());      // overlap
        CHECK(morph_check_edt(ext, mask, 1, 0, mask + 20, 24, &ei, true, &g, &msg) == -22 && untouched());
        CHECK(morph_check_edt(ext, mask + 92, 1, 0, mask, 24, &ei, true, &g, &msg) == -22 && untouched());
        CHECK(morph_check_edt(ext, mask + 96, 1, 0, mask, 24, &ei, true, &g, &msg) == 0);
        fresh();
        for (uint32_t t : {2u, 3u, M}) {
            CHECK(morph_check_edt(ext, mask, 1, t, out, 24, &ei, true, &g, &msg) == -22 && msg);
            CHECK(morph_check_edt(ext, mask, 1, t, out, 0, &ei, true, &g, &msg) == -22);  // EINVAL before ENOSPC
        }
        fresh();
        CHECK(morph_check_edt(ext, mask, 1, 0, out, 23, &ei, true, &g, &msg) == -28 && g.voxels == 24 && msg);
        CHECK(morph_check_edt(ext, mask, 1, 1, out, 0, &ei, true, &g, &msg) == -28 && g.voxels == 24);

        fresh();
        for (uint32_t op = 0; op < 4; ++op)
            for (uint32_t r2 : {0u, 1u, 100u, M - 1})
                CHECK(morph_check_morph(ext, op, r2, mask, 1, out, 24, &mi, true, &g, &msg) == 0 && g.voxels == 24);
        CHECK(morph_check_morph(ext, 0, 9, mask, 4, out + 1, 24, &mi, true, &g, &msg) == 0);  // a byte output anywhere
        fresh();
        for (uint32_t op : {4u, 5u, M}) {
            CHECK(morph_check_morph(ext, op, 1, mask, 1, out, 24, &mi, true, &g, &msg) == -22 && msg);
            CHECK(morph_check_morph(ext, op, 1, mask, 1, out, 2, &mi, true, &g, &msg) == -22);
        }
        CHECK(morph_check_morph(ext, 0, M, mask, 1, out, 24, &mi, true, &g, &msg) == -22);
        CHECK(morph_check_morph(ext, 3, M, mask, 1, out, 0, &mi, true, &g, &msg) == -22);
        fresh();
        CHECK(morph_check_morph(ext, 2, 1, mask, 1, mask + 23, 24, &mi, true, &g, &msg) == -22 && untouched());
        CHECK(morph_check_morph(ext, 2, 1, mask, 4, mask + 95, 24, &mi, true, &g, &msg) == -22 && untouched());
        CHECK(morph_check_morph(ext, 2, 1, nullptr, 1, out, 24, &mi, true, &g, &msg) == -22 && untouched());
        CHECK(morph_check_morph(ext, 2, 1, mask, 1, out, 24, nullptr, true, &g, &msg) == -22 && untouched());
        CHECK(morph_check_morph(bad, 2, 1, mask, 1, out, 24, &mi, true, &g, &msg) == -22 && untouched());
        CHECK(morph_check_morph(ext, 2, 1, mask, 1, out, 23, &mi, true, &g, &msg) == -28 && g.voxels == 24);
    }
    return harness_done("morph");
}
