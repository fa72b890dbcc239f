// mview_harness.cpp — the host side of include/vr/vr_mview.h (csrc/vr_mview_host.h: what a request is
// refused for, with the family's texts, the rectangle and the plane, the cell geometry of the
// occupancy words and vr_mview_occupancy_words) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_mview_cpu.py.  It checks every rule itself (exit status
// 1 on a mismatch) and prints the word counts and the geometry totals, which the test compares with
// its own statement of the rule.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/vr/vr_mview.h"
#include "../../volumetric-renderer_amd/csrc/vr_mview_host.h"
#include "harness_check.h"

using namespace vr;

static_assert(sizeof(vr_mask_hit) == 32 && sizeof(vr_mview_info) == 48 && sizeof(vr_mview_occ_info) == 32, "structs");
static_assert(sizeof(vr_mview_source) == sizeof(MviewSource) && offsetof(vr_mview_source, array) == offsetof(MviewSource, array) &&
                  offsetof(vr_mview_source, occupancy) == offsetof(MviewSource, occupancy) &&
                  offsetof(vr_mview_source, select) == offsetof(MviewSource, select),
              "vr_mview_source");
static_assert(sizeof(vr_mpr_plane) == sizeof(MviewPlane) && offsetof(vr_mpr_plane, op) == offsetof(MviewPlane, op), "plane");
static_assert(VR_MVIEW_MAX_EXTENT == kMaskMaxExtent && VR_MVIEW_CELL == kMviewCell && sizeof(vr_mask_hit) == kMviewHitBytes,
              "constants");
static_assert(VR_EINVAL == kMaskEinval && VR_ENOSPC == kMaskEnospc && VR_OK == kMaskOk, "codes");

// A source over `array` that every check accepts.
static MviewSource good(const void *array)
{
    MviewSource s;
    std::memset(&s, 0, sizeof s);
    s.ext[0] = 9;
    s.ext[1] = 8;
    s.ext[2] = 2;
    s.origin[0] = 1;
    s.elem_bytes = 1;
    s.array = array;
    return s;
}

// (msg by reference: it is read after the call that produced rc has written it)
static bool refused(int rc, const char *const &msg, const char *text) { return rc == kMaskEinval && msg == text; }

static void source_rules()
{
    alignas(8) static unsigned char arr[9 * 8 * 2 * 4 + 8];
    MaskGrid g;
    const char *msg = nullptr;
    MviewSource s = good(arr);
    CHECK(mview_check_source(&s, true, false, &g, &msg) == kMaskOk && g.voxels == 144 && g.origin[0] == 1);
    CHECK(refused(mview_check_source(nullptr, true, false, &g, &msg), msg, kMviewNull));
    s.array = nullptr;
    CHECK(refused(mview_check_source(&s, true, false, &g, &msg), msg, kMviewNull));
    // the extents at their bounds
    for (uint32_t e : {0u, 32769u}) {
        s = good(arr);
        s.ext[1] = e;
        CHECK(refused(mview_check_source(&s, true, false, &g, &msg), msg, kMviewTexts[kMaskExtent]));
    }
    s = good(arr);
    s.ext[0] = 32768;
    s.ext[1] = 32768;
    s.ext[2] = 4;  // 2^32 voxels: one too many
    CHECK(refused(mview_check_source(&s, true, false, &g, &msg), msg, kMviewTexts[kMaskVoxels]));
    s.ext[0] = 65535;
    s.ext[1] = 65537;
    s.ext[2] = 1;  // (refused for the extent first)
    CHECK(refused(mview_check_source(&s, true, false, &g, &msg), msg, kMviewTexts[kMaskExtent]));
    s.ext[0] = 32768;
    s.ext[1] = 32767;
    s.ext[2] = 4;  // 2^32 - 2^17: fine
    CHECK(mview_check_source(&s, true, false, &g, &msg) == kMaskOk && g.voxels == 0xFFFE0000ull);
    for (uint32_t eb : {0u, 2u, 3u, 5u, 8u}) {
        s = good(arr);
        s.elem_bytes = eb;
        CHECK(refused(mview_check_source(&s, true, false, &g, &msg), msg, kMviewTexts[kMaskElemBytes]));
    }
    s = good(arr + 1);  // a byte mask at an odd address is fine, a 4-byte array is not (device memory only)
    CHECK(mview_check_source(&s, true, false, &g, &msg) == kMaskOk);
    s.elem_bytes = 4;
    CHECK(refused(mview_check_source(&s, true, false, &g, &msg), msg, kMviewTexts[kMaskAlign]));
    CHECK(mview_check_source(&s, false, true, &g, &msg) == kMaskOk);
    s = good(arr);
    s.select = 2;
    CHECK(refused(mview_check_source(&s, true, false, &g, &msg), msg, kMviewSelect));
    s.select = kMviewLabel;
    CHECK(refused(mview_check_source(&s, true, false, &g, &msg), msg, kMviewLabelZero));
    s.label = 1;
    CHECK(mview_check_source(&s, true, false, &g, &msg) == kMaskOk);
    s.select = kMviewAny;  // ANY ignores the label
    s.label = 0;
    s.reserved = 1;
    CHECK(refused(mview_check_source(&s, true, false, &g, &msg), msg, kMviewReserved));
    s = good(arr);
    s.occupancy = arr + 8;
    CHECK(mview_check_source(&s, true, false, &g, &msg) == kMaskOk);
    CHECK(refused(mview_check_source(&s, false, true, &g, &msg), msg, kMviewHostOcc));
    s.occupancy = arr + 2;
    CHECK(refused(mview_check_source(&s, true, false, &g, &msg), msg, kMviewOccAlign));
    // the origin against the volume, at its boundary
    s = good(arr);
    CHECK(mview_check_source(&s, true, false, &g, &msg) == kMaskOk);
    const uint32_t fits[3] = {10, 8, 2}, cut[3] = {9, 8, 2};
    CHECK(mview_origin_error(g, fits) == nullptr && mview_origin_error(g, cut) == kMviewOrigin);
    g.origin[2] = 0xFFFFFFFFu;  // origin + ext passes 2^32
    CHECK(mview_origin_error(g, fits) == kMviewOrigin);
    std::printf("source rules checked\n");
}

static void call_rules()
{
    alignas(8) static unsigned char arr[144 + 16];
    alignas(8) static unsigned char out[32 * 64 + 64];
    alignas(8) static uint32_t words[4];
    vr_mview_info info;
    vr_mview_occ_info oinfo;
    const int cam = 0, par = 0;  // (only their addresses are looked at)
    MaskGrid g;
    HitRect q;
    const char *msg = nullptr;
    MviewSource s = good(arr);

    // ---- the hit image: a 5 x 3 rectangle of an 8 x 4 framebuffer, 15 records
    const uint32_t rect[4] = {3, 1, 5, 3};
    auto hit = [&](const MviewSource *src, const uint32_t *r, const void *o, uint64_t cap, bool device) {
        std::memset(&g, 0x77, sizeof g);
        return mview_check_hit(src, &cam, &par, r, 8, 4, o, cap, &info, sizeof info, device, &g, &q, &msg);
    };
    CHECK(hit(&s, rect, out, 15, true) == kMaskOk && g.voxels == 144 && q.x0 == 3 && q.y0 == 1 && q.w == 5 && q.h == 3);
    CHECK(hit(&s, rect, out, 14, true) == kMaskEnospc && msg == kMviewShortRecords && g.voxels == 144);
    CHECK(hit(&s, nullptr, out, 32, true) == kMaskOk && q.w == 8 && q.h == 4);
    CHECK(hit(&s, nullptr, out, 31, true) == kMaskEnospc);
    CHECK(refused(hit(nullptr, rect, out, 15, true), msg, kMviewNull) && refused(hit(&s, rect, nullptr, 15, true), msg, kMviewNull));
    CHECK(refused(mview_check_hit(&s, nullptr, &par, rect, 8, 4, out, 15, &info, 48, true, &g, &q, &msg), msg, kMviewNull));
    CHECK(refused(mview_check_hit(&s, &cam, nullptr, rect, 8, 4, out, 15, &info, 48, true, &g, &q, &msg), msg, kMviewNull));
    CHECK(refused(mview_check_hit(&s, &cam, &par, rect, 8, 4, out, 15, nullptr, 48, true, &g, &q, &msg), msg, kMviewNull));
    {
        MaskGrid before;
        std::memset(&before, 0x77, sizeof before);
        CHECK(std::memcmp(&g, &before, sizeof g) == 0);  // a refusal leaves the grid untouched
    }
    static const uint32_t bad_rects[5][4] = {{3, 1, 0, 3}, {3, 1, 5, 0}, {4, 1, 5, 3}, {3, 2, 5, 3}, {0xFFFFFFFFu, 0, 2, 1}};
    for (const auto &r : bad_rects) CHECK(refused(hit(&s, r, out, 64, true), msg, kMviewRect));
    CHECK(hit(&s, rect, out + 1, 15, false) == kMaskOk);  // host records: any alignment
    CHECK(refused(hit(&s, rect, out + 1, 15, true), msg, kMviewOutAlign));
    // the output against the array: one byte shared, and none
    s = good(out + 32 * 15 - 1);
    CHECK(refused(hit(&s, rect, out, 15, true), msg, kMviewOverArray));
    CHECK(refused(hit(&s, rect, out, 20, true), msg, kMviewOverArray));
    s = good(out + 32 * 15);
    CHECK(hit(&s, rect, out, 15, true) == kMaskOk);
    CHECK(hit(&s, rect, out, 14, true) == kMaskEnospc);
    // against the words (9 x 8 x 2 voxels: 2 cells, one word)
    s = good(arr);
    s.occupancy = out + 32 * 15 - 4;
    CHECK(refused(hit(&s, rect, out, 15, true), msg, kMviewOverOcc));
    s.occupancy = out + 32 * 15;
    CHECK(hit(&s, rect, out, 15, true) == kMaskOk);
    CHECK(refused(hit(&s, rect, out, 15, false), msg, kMviewHostOcc));
    // a host form's records against its info
    s = good(arr);
    CHECK(refused(mview_check_hit(&s, &cam, &par, rect, 8, 4, out, 15, out + 32 * 15 - 1, 48, false, &g, &q, &msg), msg,
                  kMviewOverInfo));
    CHECK(mview_check_hit(&s, &cam, &par, rect, 8, 4, out, 15, out + 32 * 15, 48, false, &g, &q, &msg) == kMaskOk);

    // ---- the pick
    CHECK(mview_check_pick(&s, &cam, &par, 7, 3, 8, 4, out, &g, &q, &msg) == kMaskOk && q.x0 == 7 && q.y0 == 3 && q.w == 1 &&
          q.h == 1);
    CHECK(refused(mview_check_pick(&s, &cam, &par, 8, 3, 8, 4, out, &g, &q, &msg), msg, kMviewPick));
    CHECK(refused(mview_check_pick(&s, &cam, &par, 7, 4, 8, 4, out, &g, &q, &msg), msg, kMviewPick));
    CHECK(refused(mview_check_pick(&s, &cam, &par, 0, 0, 8, 4, nullptr, &g, &q, &msg), msg, kMviewNull));
    s.occupancy = arr + 1;  // (not read)
    CHECK(mview_check_pick(&s, &cam, &par, 0, 0, 8, 4, out, &g, &q, &msg) == kMaskOk);

    // ---- the slice: a 6 x 5 image, 30 pixels
    MviewPlane pl;
    std::memset(&pl, 0, sizeof pl);
    pl.width = 6;
    pl.height = 5;
    pl.nsamples = 1;
    s = good(arr);
    auto slice = [&](const MviewPlane *p, const void *o, uint64_t cap, bool device) {
        return mview_check_slice(&s, p, o, cap, &info, sizeof info, device, &g, &msg);
    };
    CHECK(slice(&pl, out, 30, true) == kMaskOk && slice(&pl, out, 29, true) == kMaskEnospc && msg == kMviewShortPixels);
    CHECK(refused(slice(nullptr, out, 30, true), msg, kMviewNull));
    CHECK(refused(slice(&pl, out + 2, 30, true), msg, kMviewOutAlign) && slice(&pl, out + 2, 30, false) == kMaskOk);
    MviewPlane bad = pl;
    bad.dn[1] = std::numeric_limits<float>::infinity();
    CHECK(refused(slice(&bad, out, 30, true), msg, kMviewPlaneFinite));
    bad = pl;
    bad.origin[2] = std::nanf("");
    CHECK(refused(slice(&bad, out, 30, true), msg, kMviewPlaneFinite));
    bad = pl;
    bad.width = 0;
    CHECK(refused(slice(&bad, out, 30, true), msg, kMviewPlaneSize));
    bad = pl;
    bad.width = bad.height = 0xFFFFFFFFu;
    CHECK(refused(slice(&bad, out, 30, true), msg, kMviewPlaneLarge));
    for (uint32_t n : {0u, 4097u}) {
        bad = pl;
        bad.nsamples = n;
        CHECK(refused(slice(&bad, out, 30, true), msg, kMviewPlaneSamples));
    }
    bad = pl;
    bad.nsamples = 4096;
    CHECK(slice(&bad, out, 30, true) == kMaskOk);
    for (int op : {-1, 3}) {
        bad = pl;
        bad.op = op;
        CHECK(refused(slice(&bad, out, 30, true), msg, kMviewPlaneOp));
    }
    s = good(out + 4 * 30 - 1);
    CHECK(refused(slice(&pl, out, 30, true), msg, kMviewOverArray));
    s = good(out + 4 * 30);
    CHECK(slice(&pl, out, 30, true) == kMaskOk);

    // ---- the occupancy words: 9 x 8 x 2 voxels are one word; 37 x 19 x 17 are two
    s = good(arr);
    CHECK(mview_check_occupancy(&s, words, 1, &oinfo, &g, &msg) == kMaskOk);
    CHECK(mview_check_occupancy(&s, words, 0, &oinfo, &g, &msg) == kMaskEnospc && msg == kMviewShortWords && g.voxels == 144);
    CHECK(refused(mview_check_occupancy(&s, nullptr, 1, &oinfo, &g, &msg), msg, kMviewNull));
    CHECK(refused(mview_check_occupancy(&s, words, 1, nullptr, &g, &msg), msg, kMviewNull));
    CHECK(refused(mview_check_occupancy(&s, reinterpret_cast<unsigned char *>(words) + 2, 1, &oinfo, &g, &msg), msg, kMviewOutAlign));
    s = good(reinterpret_cast<unsigned char *>(words) + 3);
    CHECK(refused(mview_check_occupancy(&s, words, 1, &oinfo, &g, &msg), msg, kMviewOverArray));
    s = good(reinterpret_cast<unsigned char *>(words) + 4);
    CHECK(mview_check_occupancy(&s, words, 1, &oinfo, &g, &msg) == kMaskOk);
    s.occupancy = arr + 3;  // (the source's own field is not read)
    CHECK(mview_check_occupancy(&s, words, 1, &oinfo, &g, &msg) == kMaskOk);
    std::printf("call rules checked\n");
}

static void words_of(uint32_t bx, uint32_t by, uint32_t bz)
{
    std::vector<uint32_t> ext{bx, by, bz};  // at the very end of a heap block: a read past [2] is an ASan report
    std::printf("words %u %u %u: %llu\n", bx, by, bz, (unsigned long long)mview_occupancy_words(ext.data()));
}

// Every grid of 1 .. 20 voxels per axis: each voxel's cell lies inside the cells, each cell holds the
// voxels of its (cut) 8^3 block, and the words hold the cells.
static void geometry()
{
    unsigned long long voxels = 0, cells = 0, words = 0;
    std::vector<uint32_t> count;
    for (uint32_t bz = 1; bz <= 20; ++bz)
        for (uint32_t by = 1; by <= 20; ++by)
            for (uint32_t bx = 1; bx <= 20; ++bx) {
                const uint32_t ext[3] = {bx, by, bz};
                const MviewCells C = mview_cells(ext);
                CHECK(C.c[0] == (bx + 7) / 8 && C.c[1] == (by + 7) / 8 && C.c[2] == (bz + 7) / 8);
                CHECK(C.cells == (unsigned long long)C.c[0] * C.c[1] * C.c[2] && C.words == (C.cells + 31) / 32);
                CHECK(mview_occupancy_words(ext) == C.words);
                count.assign(C.cells, 0);  // (an index past the cells is an ASan report)
                for (uint32_t z = 0; z < bz; ++z)
                    for (uint32_t y = 0; y < by; ++y)
                        for (uint32_t x = 0; x < bx; ++x) ++count[mview_cell_index(x, y, z, C.c[0], C.c[1])];
                for (uint32_t ck = 0; ck < C.c[2]; ++ck)
                    for (uint32_t cj = 0; cj < C.c[1]; ++cj)
                        for (uint32_t ci = 0; ci < C.c[0]; ++ci) {
                            auto cut = [](uint32_t n, uint32_t c) { return n - 8 * c < 8 ? n - 8 * c : 8u; };
                            CHECK(count[ci + C.c[0] * (cj + C.c[1] * ck)] == cut(bx, ci) * cut(by, cj) * cut(bz, ck));
                        }
                voxels += (unsigned long long)bx * by * bz;
                cells += C.cells;
                words += C.words;
            }
    std::printf("geometry %llu voxels %llu cells %llu words\n", voxels, cells, words);
}

int main()
{
    source_rules();
    call_rules();
    for (uint32_t e : {1u, 8u, 9u, 32768u}) words_of(e, e <= 9 ? e : 1, 1);
    words_of(32768, 32768, 1);      // 2^30 voxels: 4096 x 4096 cells
    words_of(32768, 32767, 4);      // the last grid below the voxel bound on these axes
    words_of(65535, 65537, 1);      // 2^32 - 1 voxels, but an extent beyond 32768
    words_of(32768, 32768, 4);      // 2^32 voxels
    words_of(0, 8, 8);
    words_of(37, 19, 17);
    CHECK(mview_occupancy_words(nullptr) == 0);
    geometry();
    return harness_done("mview");
}
