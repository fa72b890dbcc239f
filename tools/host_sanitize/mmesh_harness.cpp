// mmesh_harness.cpp — the host side of include/vr/vr_mmesh.h (csrc/vr_mmesh_host.h: what a request is
// refused for, with the family's texts, and the node, cell, word and scratch geometry) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_mmesh_cpu.py.  It checks
// every rule itself (exit status 1 on a mismatch) and prints the geometry of a few grids, the
// largest among them, which the test compares with its own statement of the rule.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../include/vr/vr_mmesh.h"
#include "../../volumetric-renderer_amd/csrc/vr_mmesh_host.h"
#include "harness_check.h"

using namespace vr;

static_assert(sizeof(vr_mmesh_request) == sizeof(MmeshRequest) && sizeof(vr_mmesh_request) == 64 &&
                  offsetof(vr_mmesh_request, relax) == offsetof(MmeshRequest, relax) &&
                  offsetof(vr_mmesh_request, array) == offsetof(MmeshRequest, array) &&
                  offsetof(vr_mmesh_request, closed) == offsetof(MmeshRequest, closed),
              "vr_mmesh_request");
static_assert(sizeof(vr_mmesh_info) == 32 && sizeof(vr_mesh_vertex) == kMmeshVertexBytes, "structs");
static_assert(VR_MMESH_MAX_EXTENT == kMaskMaxExtent && VR_MMESH_MAX_ITERS == kMmeshMaxIters && VR_MVIEW_ANY == kMmeshAny &&
                  VR_MVIEW_LABEL == kMmeshLabel,
              "constants");
static_assert(VR_EINVAL == kMaskEinval && VR_ENOSPC == kMaskEnospc && VR_OK == kMaskOk, "codes");

alignas(8) static unsigned char g_arr[9 * 8 * 2 * 4 + 8];
alignas(8) static unsigned char g_verts[9 * 10 * 4 * 24 + 8];  // more than the grid's most vertices hold
alignas(8) static unsigned char g_tris[9 * 10 * 4 * 6 * 12 + 8];
static vr_mmesh_info g_info;

// A request over g_arr that every check accepts.
static MmeshRequest good()
{
    MmeshRequest q;
    std::memset(&q, 0, sizeof q);
    q.ext[0] = 9;
    q.ext[1] = 8;
    q.ext[2] = 2;
    q.origin[0] = 1;
    q.elem_bytes = 1;
    q.closed = 1;
    q.normals = 1;
    q.smooth_iters = 3;
    q.relax = 0.5f;
    q.array = g_arr;
    return q;
}

static int count_rc(const MmeshRequest *q, const void *info, bool device, const char **msg, MaskGrid *g)
{
    return mmesh_check_request(q, info, device, g, msg);
}

static int extract_rc(const MmeshRequest *q, const void *v, uint64_t vcap, const void *t, uint64_t tcap, const void *info,
                      bool device, const char **msg, MaskGrid *g)
{
    return mmesh_check_extract(q, v, vcap, t, tcap, info, sizeof(vr_mmesh_info), device, g, msg);
}

// Both checks refuse q with `text` and leave the grid untouched.
static void both_refuse(const MmeshRequest &q, bool device, const char *text, int line)
{
    MaskGrid g;
    std::memset(&g, 0x5A, sizeof g);
    MaskGrid before = g;
    const char *msg = nullptr;
    int rc = count_rc(&q, &g_info, device, &msg, &g);
    bool ok = rc == kMaskEinval && msg == text;
    rc = extract_rc(&q, g_verts, 1000, g_tris, 1000, &g_info, device, &msg, &g);
    ok = ok && rc == kMaskEinval && msg == text && std::memcmp(&g, &before, sizeof g) == 0;
    if (!ok) {
        std::printf("FAILED line %d: expected \"%s\", got \"%s\"\n", line, text, msg ? msg : "(none)");
        ++g_bad;
    }
}
#define REFUSE(q, device, text) both_refuse(q, device, text, __LINE__)

static void request_rules()
{
    MaskGrid g;
    const char *msg = nullptr;
    MmeshRequest q = good();
    CHECK(count_rc(&q, &g_info, true, &msg, &g) == kMaskOk && msg == nullptr);
    CHECK(g.ext[0] == 9 && g.ext[1] == 8 && g.ext[2] == 2 && g.origin[0] == 1 && g.origin[1] == 0 && g.voxels == 144);
    CHECK(extract_rc(&q, g_verts, 7, g_tris, 7, &g_info, true, &msg, &g) == kMaskOk && msg == nullptr);
    CHECK(extract_rc(&q, g_verts, 0, g_tris, 0, &g_info, false, &msg, &g) == kMaskOk);  // a short capacity is no refusal here

    // NULLs
    CHECK(count_rc(nullptr, &g_info, true, &msg, &g) == kMaskEinval && msg == kMmeshNull);
    CHECK(count_rc(&q, nullptr, true, &msg, &g) == kMaskEinval && msg == kMmeshNull);
    CHECK(extract_rc(&q, nullptr, 7, g_tris, 7, &g_info, true, &msg, &g) == kMaskEinval && msg == kMmeshNull);
    CHECK(extract_rc(&q, g_verts, 7, nullptr, 7, &g_info, true, &msg, &g) == kMaskEinval && msg == kMmeshNull);
    CHECK(extract_rc(&q, g_verts, 7, g_tris, 7, nullptr, true, &msg, &g) == kMaskEinval && msg == kMmeshNull);
    q.array = nullptr;
    REFUSE(q, true, kMmeshNull);

    // the grid rule, at its boundaries
    q = good();
    q.ext[1] = 0;
    REFUSE(q, true, kMmeshTexts[kMaskExtent]);
    q.ext[1] = 32769;
    REFUSE(q, true, kMmeshTexts[kMaskExtent]);
    q.ext[0] = 32768, q.ext[1] = 32768, q.ext[2] = 4;  // 2^32 voxels
    REFUSE(q, true, kMmeshTexts[kMaskVoxels]);
    q.ext[0] = 32768, q.ext[1] = 32767, q.ext[2] = 4;      // 2^32 - 2^17: the rule admits it
    q.array = g_arr;
    CHECK(count_rc(&q, &g_info, false, &msg, &g) == kMaskOk && g.voxels == 4294836224ull);
    q = good();
    for (uint32_t eb : {0u, 2u, 3u, 8u}) {
        q.elem_bytes = eb;
        REFUSE(q, true, kMmeshTexts[kMaskElemBytes]);
    }
    q.elem_bytes = 4;
    CHECK(count_rc(&q, &g_info, true, &msg, &g) == kMaskOk);
    for (int off = 1; off < 4; ++off) {
        q.array = g_arr + off;
        REFUSE(q, true, kMmeshTexts[kMaskAlign]);
        CHECK(count_rc(&q, &g_info, false, &msg, &g) == kMaskOk);  // a host array is copied byte by byte
    }
    q.elem_bytes = 1;
    CHECK(count_rc(&q, &g_info, true, &msg, &g) == kMaskOk);  // a byte mask may have any address

    // the request's own fields
    q = good();
    q.select = 2;
    REFUSE(q, true, kMmeshSelect);
    q.select = kMmeshLabel;
    q.label = 0;
    REFUSE(q, true, kMmeshLabelZero);
    q.label = 0x80000000u;
    CHECK(count_rc(&q, &g_info, true, &msg, &g) == kMaskOk);
    q = good();
    q.label = 0;  // ANY ignores it
    CHECK(count_rc(&q, &g_info, true, &msg, &g) == kMaskOk);
    q.closed = 2;
    REFUSE(q, true, kMmeshClosed);
    q.closed = 0;
    q.normals = 2;
    REFUSE(q, true, kMmeshNormals);
    q.normals = 0;
    q.smooth_iters = kMmeshMaxIters;
    CHECK(count_rc(&q, &g_info, true, &msg, &g) == kMaskOk);
    q.smooth_iters = kMmeshMaxIters + 1;
    REFUSE(q, true, kMmeshIters);
    q.smooth_iters = 0;
    for (float r : {0.0f, -0.0f, 1.0f, 0.25f, std::numeric_limits<float>::denorm_min()}) {
        q.relax = r;
        CHECK(count_rc(&q, &g_info, true, &msg, &g) == kMaskOk);
    }
    for (float r : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                    -std::numeric_limits<float>::infinity(), std::nextafter(1.0f, 2.0f), -std::numeric_limits<float>::denorm_min()}) {
        q.relax = r;
        REFUSE(q, true, kMmeshRelax);
    }
    q.relax = 0.5f;
    q.reserved = 1;
    REFUSE(q, true, kMmeshReserved);
    std::printf("request rules checked\n");
}

static void output_rules()
{
    MaskGrid g;
    const char *msg = nullptr;
    MmeshRequest q = good();
    const MmeshGeom G = mmesh_geom(q.ext, q.closed);
    CHECK(G.cells == 10 * 9 * 3 && mmesh_max_vertices(G) == 270 && mmesh_max_triangles(G) == 1620);
    // alignment binds device outputs only
    for (int off = 1; off < 4; ++off) {
        CHECK(extract_rc(&q, g_verts + off, 7, g_tris, 7, &g_info, true, &msg, &g) == kMaskEinval && msg == kMmeshOutAlign);
        CHECK(extract_rc(&q, g_verts, 7, g_tris + off, 7, &g_info, true, &msg, &g) == kMaskEinval && msg == kMmeshOutAlign);
        CHECK(extract_rc(&q, g_verts + off, 7, g_tris + off, 7, &g_info, false, &msg, &g) == kMaskOk);
    }
    // an output over the array: one shared byte is enough, a touching one is none
    CHECK(extract_rc(&q, g_arr + 140, 1, g_tris, 7, &g_info, true, &msg, &g) == kMaskEinval && msg == kMmeshOverArray);
    CHECK(extract_rc(&q, g_arr + 144, 1, g_tris, 7, &g_info, true, &msg, &g) == kMaskOk);
    CHECK(extract_rc(&q, g_verts, 7, g_arr + 140, 1, &g_info, true, &msg, &g) == kMaskEinval && msg == kMmeshOverArray);
    CHECK(extract_rc(&q, g_verts, 7, g_arr + 144, 1, &g_info, true, &msg, &g) == kMaskOk);
    CHECK(extract_rc(&q, g_arr + 140, 0, g_tris, 7, &g_info, true, &msg, &g) == kMaskOk);  // a capacity of 0 touches nothing
    // the outputs against each other: what they could hold at most
    CHECK(extract_rc(&q, g_verts, 2, g_verts + 44, 1, &g_info, true, &msg, &g) == kMaskEinval && msg == kMmeshOverOutput);
    CHECK(extract_rc(&q, g_verts, 2, g_verts + 48, 1, &g_info, true, &msg, &g) == kMaskOk);
    CHECK(extract_rc(&q, g_verts + 12, 1, g_verts, 1, &g_info, true, &msg, &g) == kMaskOk);
    CHECK(extract_rc(&q, g_verts + 8, 1, g_verts, 1, &g_info, true, &msg, &g) == kMaskEinval && msg == kMmeshOverOutput);
    // a capacity beyond the grid's most counts as the most: 270 vertices of 24 bytes
    CHECK(extract_rc(&q, g_verts, ~0ull, g_verts + 270 * 24, 1, &g_info, true, &msg, &g) == kMaskOk);
    CHECK(extract_rc(&q, g_verts, ~0ull, g_verts + 270 * 24 - 4, 1, &g_info, true, &msg, &g) == kMaskEinval &&
          msg == kMmeshOverOutput);
    // the info: host forms only
    alignas(8) static unsigned char buf[64 + sizeof(vr_mmesh_info)];
    CHECK(extract_rc(&q, buf, 1, g_tris, 7, buf + 20, false, &msg, &g) == kMaskEinval && msg == kMmeshOverInfo);
    CHECK(extract_rc(&q, g_verts, 1, buf + 24, 1, buf + 32, false, &msg, &g) == kMaskEinval && msg == kMmeshOverInfo);
    CHECK(extract_rc(&q, buf, 1, g_tris, 7, buf + 24, false, &msg, &g) == kMaskOk);
    CHECK(extract_rc(&q, buf, 1, g_tris, 7, buf + 20, true, &msg, &g) == kMaskOk);  // (a device pointer is no host memory)

    // the volume, and the counts
    const uint32_t dims[3] = {10, 8, 2}, tight[3] = {9, 8, 2};
    CHECK(count_rc(&q, &g_info, true, &msg, &g) == kMaskOk);
    CHECK(mmesh_origin_error(g, dims) == nullptr && mmesh_origin_error(g, tight) == kMmeshOrigin);
    g.origin[2] = 0xFFFFFFFFu;
    CHECK(mmesh_origin_error(g, dims) == kMmeshOrigin);  // no wrap
    CHECK(mmesh_check_counts(kMmeshMaxVertices, 1ull << 40, false, 0, 0, &msg) == kMaskOk && msg == nullptr);
    CHECK(mmesh_check_counts(kMmeshMaxVertices + 1, 0, true, ~0ull, ~0ull, &msg) == kMaskEinval && msg == kMmeshTooMany);
    CHECK(mmesh_check_counts(5, 7, true, 5, 7, &msg) == kMaskOk);
    CHECK(mmesh_check_counts(5, 7, true, 4, 7, &msg) == kMaskEnospc && msg == kMmeshShort);
    CHECK(mmesh_check_counts(5, 7, true, 5, 6, &msg) == kMaskEnospc && msg == kMmeshShort);
    CHECK(mmesh_check_counts(5, 7, false, 0, 0, &msg) == kMaskOk);
    std::printf("output rules checked\n");
}

static void print_geom(const uint32_t ext[3], uint32_t closed)
{
    const MmeshGeom G = mmesh_geom(ext, closed);
    const MmeshScratch S = mmesh_scratch(G);
    std::printf("geom %u %u %u %u: nw %u cw %u node_words %llu cells %llu cell_words %llu groups %u span %u scratch %llu\n", ext[0],
                ext[1], ext[2], closed, G.nw, G.cw, (unsigned long long)G.node_words, (unsigned long long)G.cells,
                (unsigned long long)G.cell_words, G.groups, G.span, (unsigned long long)S.bytes);
    // the parts follow each other, 8-byte aligned, and the workgroups' spans cover the words
    CHECK(S.bits == 0 && S.active == G.node_words * 8 && S.pre_t == S.active + G.cell_words * 8 &&
          S.pre_v == S.pre_t + G.cell_words * 8 && S.gsum >= S.pre_v + G.cell_words * 4 && S.gsum % 8 == 0 &&
          S.matching == S.gsum + 16ull * kMmeshMaxGroups && S.bytes == S.matching + 8);
    CHECK(G.groups >= 1 && G.groups <= kMmeshMaxGroups && (uint64_t)G.groups * G.span >= G.cell_words);
    CHECK(G.span % (kMmeshScanTile * kMmeshSpanTiles) == 0 && G.span > 0);
    CHECK(G.node_words <= 0xFFFFFFFFull && G.cell_words <= 0xFFFFFFFFull);  // the kernels' word indices
    CHECK(G.cw <= G.nw && G.cell_words <= G.node_words);
}

static void geometry()
{
    const uint32_t grids[][3] = {{1, 1, 1},         {9, 8, 2},         {62, 5, 4},        {63, 5, 4},      {64, 5, 4},
                                 {65, 5, 4},        {66, 5, 4},        {3, 3, 7000},      {1024, 1024, 1024}, {32768, 1, 1},
                                 {1, 32768, 32768}, {3, 32768, 32768}, {32768, 32767, 4}, {62, 8322, 8323}, {1625, 1625, 1626}};
    for (const auto &e : grids)
        for (uint32_t closed = 0; closed < 2; ++closed) print_geom(e, closed);
    // every small grid: the totals
    unsigned long long node_words = 0, cell_words = 0, cells = 0;
    for (uint32_t a = 1; a <= 12; ++a)
        for (uint32_t b = 1; b <= 12; ++b)
            for (uint32_t c = 1; c <= 12; ++c)
                for (uint32_t closed = 0; closed < 2; ++closed) {
                    const uint32_t e[3] = {a * 11, b, c};
                    const MmeshGeom G = mmesh_geom(e, closed);
                    node_words += G.node_words;
                    cell_words += G.cell_words;
                    cells += G.cells;
                    CHECK(mmesh_local_stride(G.cells) % 8 == 0 && mmesh_local_stride(G.cells) >= G.cells * 12);
                }
    std::printf("totals %llu node words %llu cell words %llu cells\n", node_words, cell_words, cells);
}

int main()
{
    request_rules();
    output_rules();
    geometry();
    return harness_done("mmesh");
}
