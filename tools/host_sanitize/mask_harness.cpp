// mask_harness.cpp — the grid rule the mask families share (csrc/vr_mask_host.h: the grid a request
// resolves to, its two bounds, and what an array or an output is refused for) as a stand-alone
// program, built with -fsanitize=address,undefined by tests/test_mask_host_cpu.py.  It checks every
// reason code at its boundary itself (exit status 1 on a mismatch) and prints the resolved grids and,
// per family, the text each reason code maps to, which the test compares with its own copies.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../volumetric-renderer_amd/csrc/vr_maskcc_host.h"
#include "../../volumetric-renderer_amd/csrc/vr_morph_host.h"
#include "../../volumetric-renderer_amd/csrc/vr_mstat_host.h"
#include "harness_check.h"

using namespace vr;

static_assert(kMaskMaxExtent == 32768 && kMaskMaxVoxels == 0xFFFFFFFFull, "the two bounds");
static_assert(kMaskOk == 0 && kMaskEinval == -22 && kMaskEnospc == -28, "codes");
static_assert(kMaskFine == 0 && kMaskReasons == 7, "a text table is indexed by the reason");

static void grid_case(uint32_t bx, uint32_t by, uint32_t bz, MaskReason want)
{
    // the array sits at the very end of a heap block: a read past [2] is an ASan report
    std::vector<uint32_t> ext{bx, by, bz};
    MaskGrid g;
    std::memset(&g, 0x77, sizeof g);
    const MaskGrid before = g;
    const MaskReason why = mask_grid_resolve(ext.data(), &g);
    CHECK(why == want);
    if (why) {
        CHECK(std::memcmp(&g, &before, sizeof g) == 0);  // untouched
    } else {
        CHECK(g.ext[0] == bx && g.ext[1] == by && g.ext[2] == bz && g.voxels == (uint64_t)bx * by * bz);
        CHECK(g.origin[0] == 0 && g.origin[1] == 0 && g.origin[2] == 0);  // every field defined
    }
    std::printf("grid %u %u %u: %d %llu\n", bx, by, bz, (int)why, why ? 0ull : (unsigned long long)g.voxels);
}

int main()
{
    // the extent at its boundaries on each axis, then the voxel count at 2^32 - 1 against 2^32
    for (int a = 0; a < 3; ++a)
        for (uint32_t e : {0u, 1u, 32768u, 32769u}) {
            uint32_t ext[3] = {1, 1, 1};
            ext[a] = e;
            grid_case(ext[0], ext[1], ext[2], e >= 1 && e <= 32768 ? kMaskFine : kMaskExtent);
        }
    grid_case(32768, 32768, 3, kMaskFine);
    grid_case(32768, 32768, 4, kMaskVoxels);
    grid_case(2048, 2048, 1023, kMaskFine);
    grid_case(2048, 2048, 1024, kMaskVoxels);
    grid_case(65535, 65537, 1, kMaskExtent);  // 2^32 - 1 voxels, but no extent in range
    grid_case(0, 32769, 1, kMaskExtent);

    alignas(8) static unsigned char buf[64] = {0};
    {  // elem_bytes and alignment
        for (uint32_t eb : {0u, 2u, 3u, 5u, 8u, 0xFFFFFFFFu})
            for (bool dev : {false, true}) CHECK(mask_check_array(buf, eb, dev) == kMaskElemBytes);
        for (int off = 0; off < 4; ++off) {
            CHECK(mask_aligned4(buf + off) == (off == 0));
            CHECK(mask_check_array(buf + off, 1, true) == kMaskFine && mask_check_array(buf + off, 1, false) == kMaskFine);
            CHECK(mask_check_array(buf + off, 4, true) == (off ? kMaskAlign : kMaskFine));
            CHECK(mask_check_array(buf + off, 4, false) == kMaskFine);  // a host array is copied byte by byte
            CHECK(mask_check_array(buf + off, 2, true) == kMaskElemBytes);  // the width before the alignment
        }
        CHECK(mask_aligned4(buf + 4) && mask_check_array(nullptr, 4, true) == kMaskFine);  // no array: nothing to align
    }
    {  // overlap: touching but disjoint, one shared byte
        CHECK(!mask_overlap(buf, 8, buf + 8, 8) && !mask_overlap(buf + 8, 8, buf, 8));
        CHECK(mask_overlap(buf, 8, buf + 7, 1) && mask_overlap(buf + 7, 1, buf, 8) && mask_overlap(buf, 8, buf, 8));
        CHECK(mask_overlap(buf, 64, buf + 20, 4) && mask_overlap(buf + 20, 4, buf, 64));
    }
    {  // the output of a 24-voxel grid: the overlap of min(cap, full) elements, then the capacity
        CHECK(mask_check_output(buf, 24, buf + 24, 1, 24, 24) == kMaskFine);     // touching but disjoint
        CHECK(mask_check_output(buf + 24, 24, buf, 1, 24, 24) == kMaskFine);
        CHECK(mask_check_output(buf, 24, buf + 23, 1, 24, 24) == kMaskOverlap);  // one shared byte
        CHECK(mask_check_output(buf + 23, 24, buf, 1, 24, 24) == kMaskOverlap);
        CHECK(mask_check_output(buf + 24, 24, buf, 1, 1000, 24) == kMaskFine);   // no more than full is touched
        CHECK(mask_check_output(buf + 20, 24, buf, 4, 5, 24) == kMaskShort);     // 5 elements end where the input begins
        CHECK(mask_check_output(buf + 20, 24, buf, 4, 6, 24) == kMaskOverlap);   // the overlap outranks the capacity
        CHECK(mask_check_output(buf, 24, buf, 1, 0, 24) == kMaskShort);          // cap 0: nothing is touched
        CHECK(mask_check_output(buf, 24, buf, 1, 0, 0) == kMaskFine);            // and nothing is asked for
        CHECK(mask_check_output(buf, 24, buf + 24, 1, 23, 24) == kMaskShort);    // voxels - 1
        CHECK(mask_check_output(nullptr, 24, buf, 1, 24, 24) == kMaskFine);      // no input
        CHECK(mask_check_output(nullptr, 24, buf, 1, 23, 24) == kMaskShort);
    }
    {  // the end of a check: the grid resolved either way, the capacity's code and text
        const uint32_t ext[3] = {4, 3, 2};
        MaskGrid r, g;
        CHECK(mask_grid_resolve(ext, &r) == kMaskFine && r.voxels == 24);
        const char *msg = nullptr;
        std::memset(&g, 0x77, sizeof g);
        CHECK(mask_resolved(r, kMaskShort, "short", &g, &msg) == kMaskEnospc && msg && !std::strcmp(msg, "short"));
        CHECK(std::memcmp(&g, &r, sizeof g) == 0);
        msg = nullptr;
        std::memset(&g, 0x77, sizeof g);
        CHECK(mask_resolved(r, kMaskFine, "short", &g, &msg) == kMaskOk && !msg && std::memcmp(&g, &r, sizeof g) == 0);
        CHECK(mask_refuse(&msg, "text", -5) == -5 && !std::strcmp(msg, "text"));
    }
    // each family's texts for the shared rule
    const struct {
        const char *family;
        const char *const *texts;
    } tables[] = {{"morph", kMorphTexts}, {"maskcc", kMccTexts}, {"mstat", kMstatTexts}};
    for (const auto &t : tables) {
        CHECK(t.texts[kMaskFine] == nullptr);
        for (int why = kMaskExtent; why <= kMaskAlign; ++why) {
            CHECK(t.texts[why] && t.texts[why][0]);
            std::printf("text %s %d %s\n", t.family, why, t.texts[why] ? t.texts[why] : "");
        }
    }
    {  // and the texts each family's own check gives an output: on the mask, then one voxel short
        alignas(8) static unsigned char mask[64 * 24], out[64 * 24], tab[64 * 5];
        const uint32_t ext[3] = {4, 3, 2}, org[3] = {0, 0, 0}, seed[3] = {0, 0, 0};
        int info;
        for (int is_short = 0; is_short < 2; ++is_short) {
            void *o = is_short ? out : mask;
            const uint64_t cap = is_short ? 23 : 24, rcap = is_short ? 4 : 5;
            MaskGrid g;
            const char *msg[7];
            const int rc[7] = {morph_check_edt(ext, mask, 1, 0, o, cap, &info, true, &g, &msg[0]),
                               morph_check_morph(ext, 0, 1, mask, 1, o, cap, &info, true, &g, &msg[1]),
                               mcc_check_label(ext, mask, 1, 6, o, cap, tab, 5, &info, true, &g, &msg[2]),
                               mcc_check_label(ext, mask, 1, 6, out, 24, is_short ? tab : mask, 5, &info, true, &g, &msg[3]),
                               mcc_check_select(ext, true, 0, 6, seed, mask, 1, o, cap, &info, true, &g, &msg[4]),
                               mstat_check_labels(ext, org, mask, tab, 5, is_short ? out : tab, rcap, &info, true, &g, &msg[5]),
                               mstat_check_window(ext, org, mask, 1, 0.0f, 1.0f, o, cap, &info, true, &g, &msg[6])};
            const char *calls[7] = {"edt", "morph", "label", "label_records", "select", "label_stats", "window"};
            for (int i = 0; i < 7; ++i) {
                const bool records_fit = is_short && i == 3;  // the record capacity is held against the count, later
                CHECK(rc[i] == (records_fit ? kMaskOk : is_short ? kMaskEnospc : kMaskEinval) && (records_fit || msg[i]));
                std::printf("refusal %s %d %s\n", calls[i], rc[i], msg[i] ? msg[i] : "");
            }
        }
        const char *m = nullptr;
        MaskGrid g;
        CHECK(mstat_check_labels(ext, org, mask, tab, 5, mask + 8, 5, &info, true, &g, &m) == kMaskEinval && m);
        std::printf("refusal label_stats_labels -22 %s\n", m ? m : "");
    }
    return harness_done("mask");
}
