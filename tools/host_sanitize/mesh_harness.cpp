// mesh_harness.cpp — the host side of include/vr/vr_mesh.h (csrc/vr_mesh_host.h: what a request
// is refused for, the node box and cell range it resolves to, the bricks a launch walks, and the
// PLY writer behind vr_host.h's vr_mesh_write_ply) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_mesh_cpu.py.  It checks every rule itself (exit
// status 1 on a mismatch) and prints the resolved boxes, which the test compares with its own
// statement of the rule.  argv[1]: a directory to write the PLY files into.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/vr/vr_mesh.h"
#include "../../volumetric-renderer_amd/csrc/vr_mesh_host.h"
#include "harness_check.h"

using namespace vr;

static_assert(sizeof(vr_mesh_request) == 40, "vr_mesh_request is 40 bytes");
static_assert(sizeof(vr_mesh_vertex) == kMeshVertexBytes && kMeshVertexBytes == 24, "vr_mesh_vertex is 24 bytes");
static_assert(sizeof(vr_mesh_info) == 32 && kMeshTriangleBytes == 12, "vr_mesh_info is four 64-bit counts");
static_assert(VR_ENOSPC == -28, "VR_ENOSPC");

// a request's box on a dims volume: what mesh_box_resolve says, printed for the test
static void box_case(uint32_t use_box, uint32_t closed, const uint32_t lo[3], const uint32_t hi[3],
                     const uint32_t dims[3])
{
    // the arrays sit at the very end of heap blocks: a read past [2] is an ASan report
    std::vector<uint32_t> mn(lo, lo + 3), mx(hi, hi + 3), dm(dims, dims + 3);
    MeshBox b;
    std::memset(&b, 0x77, sizeof b);
    const MeshBox before = b;
    const char *m = mesh_box_resolve(use_box, mn.data(), mx.data(), closed, dm.data(), &b);
    bool want = use_box <= 1 && closed <= 1;
    for (int a = 0; a < 3 && want; ++a) {
        const uint32_t l = use_box ? lo[a] : 0u, h = use_box ? hi[a] : dims[a];
        want = l < h && h <= dims[a];
    }
    CHECK((m == nullptr) == want);
    if (m) CHECK(std::memcmp(&b, &before, sizeof b) == 0);  // untouched
    uint32_t b0[3] = {0, 0, 0}, nb[3] = {0, 0, 0};
    unsigned long long nwork = 0;
    if (!m) {
        for (int a = 0; a < 3; ++a) {
            CHECK(b.lo[a] == (use_box ? lo[a] : 0u) && b.hi[a] == (use_box ? hi[a] : dims[a]));
            CHECK(b.clo[a] == (long long)b.lo[a] - (closed ? 1 : 0));
            CHECK(b.chi[a] == (long long)b.hi[a] - (closed ? 1 : 2));
        }
        const uint32_t cells[3] = {7, 8, 8};
        nwork = mesh_brick_range(b, cells, 2, b0, nb);
        for (int a = 0; a < 3; ++a) {
            // every padded cell index of the walk lies in the bricks b0 .. b0 + nb - 1
            const long long first = b.clo[a] + 2, last = (long long)b.hi[a] + 1;
            CHECK(first >= 1 && first / cells[a] == b0[a] && last / cells[a] == (long long)b0[a] + nb[a] - 1);
        }
        const unsigned __int128 prod = (unsigned __int128)nb[0] * nb[1] * nb[2];
        CHECK(nwork >= 1 && (prod >> 64 ? nwork == ~0ull : nwork == (unsigned long long)prod));
    }
    std::printf("box %u %u  %u %u %u  %u %u %u on %u %u %u: %d  %lld %lld %lld  %lld %lld %lld  %llu\n", use_box, closed,
                lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], dims[0], dims[1], dims[2], (int)(m == nullptr),
                m ? 0ll : (long long)b.clo[0], m ? 0ll : (long long)b.clo[1], m ? 0ll : (long long)b.clo[2],
                m ? 0ll : (long long)b.chi[0], m ? 0ll : (long long)b.chi[1], m ? 0ll : (long long)b.chi[2], nwork);
}

static std::vector<unsigned char> slurp(const std::string &p)
{
    std::vector<unsigned char> d;
    if (FILE *f = std::fopen(p.c_str(), "rb")) {
        unsigned char buf[4096];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
        std::fclose(f);
    }
    return d;
}

int main(int argc, char **argv)
{
    {  // iso and the three flags
        const float bad[] = {NAN, INFINITY, -INFINITY};
        for (float v : bad) CHECK(mesh_flags_error(v, 1, 1, 0) != nullptr);
        const float good[] = {0.0f, -0.0f, -3.5f, std::numeric_limits<float>::max(),
                              std::numeric_limits<float>::denorm_min()};
        for (float v : good) CHECK(mesh_flags_error(v, 0, 0, 0) == nullptr && mesh_flags_error(v, 1, 1, 1) == nullptr);
        const uint32_t M = 0xFFFFFFFFu;
        for (uint32_t v : {2u, 3u, M}) {
            CHECK(mesh_flags_error(0.5f, v, 0, 0) != nullptr);
            CHECK(mesh_flags_error(0.5f, 0, v, 0) != nullptr);
            CHECK(mesh_flags_error(0.5f, 0, 0, v) != nullptr);
        }
    }
    const uint32_t M = 0xFFFFFFFFu;
    const uint32_t dims[3] = {19, 17, 21}, big[3] = {M, M, M}, zero3[3] = {0, 0, 0};
    struct {
        uint32_t use, closed, lo[3], hi[3];
    } cases[] = {
        {0, 1, {0, 0, 0}, {0, 0, 0}},      // the whole volume: the box is not read for sense
        {0, 0, {9, 9, 9}, {1, 1, 1}},
        {1, 1, {0, 0, 0}, {19, 17, 21}},
        {1, 0, {0, 0, 0}, {19, 17, 21}},
        {1, 1, {3, 2, 5}, {15, 13, 18}},
        {1, 0, {3, 2, 5}, {4, 13, 18}},    // one node along x, open: no cell there
        {1, 1, {18, 16, 20}, {19, 17, 21}},
        {1, 1, {0, 0, 0}, {20, 17, 21}},   // beyond, by one
        {1, 1, {0, 0, 0}, {19, 18, 21}},
        {1, 0, {0, 0, 0}, {19, 17, 22}},
        {1, 1, {3, 3, 3}, {3, 4, 4}},      // empty
        {1, 1, {3, 5, 3}, {4, 4, 4}},      // min above max
        {1, 1, {0, 0, M}, {1, 1, 1}},
        {1, 1, {0, 0, 0}, {1, M, 1}},
        {2, 1, {0, 0, 0}, {1, 1, 1}},      // use_box
        {M, 0, {0, 0, 0}, {1, 1, 1}},
        {1, 2, {0, 0, 0}, {1, 1, 1}},      // closed
    };
    for (const auto &c : cases) box_case(c.use, c.closed, c.lo, c.hi, dims);
    box_case(0, 1, zero3, zero3, big);     // the largest there is
    box_case(1, 0, zero3, big, big);
    box_case(0, 1, zero3, zero3, zero3);   // no volume

    {  // the PLY writer
        const std::string dir = argc > 1 ? argv[1] : ".";
        const std::string path = dir + "/mesh_harness.ply";
        // the arrays at the very end of heap blocks
        std::vector<vr_mesh_vertex> v(4);
        for (int i = 0; i < 4; ++i) {
            v[i] = vr_mesh_vertex{{0.25f * i, 0.5f, 1.0f - 0.125f * i}, {0.0f, -1.0f, 0.0f}};
        }
        std::vector<uint32_t> t{0, 1, 2, 0, 2, 3};
        const float scale[3] = {19.0f, 17.0f, 21.0f}, offset[3] = {-0.5f, -0.5f, -0.5f};
        const char *m = nullptr;
        CHECK(mesh_write_ply(path.c_str(), v.data(), 4, t.data(), 2, scale, offset, &m) == 0 && m[0] == 0);
        std::vector<unsigned char> d = slurp(path);
        const char *end = "end_header\n";
        const std::string text(d.begin(), d.end());
        const size_t h = text.find(end);
        CHECK(h != std::string::npos && text.compare(0, 4, "ply\n") == 0);
        CHECK(text.find("format binary_little_endian 1.0\n") != std::string::npos);
        CHECK(text.find("element vertex 4\n") != std::string::npos && text.find("element face 2\n") != std::string::npos);
        if (h != std::string::npos) {
            const size_t body = h + std::strlen(end);
            CHECK(d.size() == body + 4 * 24 + 2 * 13);
            if (d.size() == body + 4 * 24 + 2 * 13) {
                float r[6];
                std::memcpy(r, d.data() + body + 24 * 3, sizeof r);  // (a little-endian host)
                CHECK(r[0] == v[3].pos[0] * 19.0f + -0.5f && r[1] == 0.5f * 17.0f + -0.5f && r[4] == -1.0f);
                const unsigned char *f1 = d.data() + body + 4 * 24 + 13;
                uint32_t idx[3];
                std::memcpy(idx, f1 + 1, sizeof idx);
                CHECK(f1[0] == 3 && idx[0] == 0 && idx[1] == 2 && idx[2] == 3);
            }
        }
        // NULL scale and offset: the positions as they are; an empty mesh: a header alone
        CHECK(mesh_write_ply(path.c_str(), v.data(), 4, t.data(), 2, nullptr, nullptr, nullptr) == 0);
        CHECK(mesh_write_ply(path.c_str(), nullptr, 0, nullptr, 0, scale, offset, &m) == 0);
        d = slurp(path);
        CHECK(!d.empty() && d.back() == '\n' && std::string(d.begin(), d.end()).find("element vertex 0\n") != std::string::npos);
        // refusals: nothing is written
        const std::string none = dir + "/mesh_harness_none.ply";
        CHECK(mesh_write_ply(nullptr, v.data(), 4, t.data(), 2, scale, offset, &m) == -22 && m[0] != 0);
        CHECK(mesh_write_ply(none.c_str(), nullptr, 4, t.data(), 2, scale, offset, &m) == -22);
        CHECK(mesh_write_ply(none.c_str(), v.data(), 4, nullptr, 2, scale, offset, &m) == -22);
        t[5] = 4;  // an index beyond the vertices
        CHECK(mesh_write_ply(none.c_str(), v.data(), 4, t.data(), 2, scale, offset, &m) == -22);
        CHECK(std::string(m).find("index") != std::string::npos);
        CHECK(slurp(none).empty());
        CHECK(mesh_write_ply((dir + "/no/such/dir/x.ply").c_str(), v.data(), 4, t.data(), 1, scale, offset, &m) == -1);
    }
    return harness_done("mesh");
}
