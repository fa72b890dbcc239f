// vr_cli — headless host for the MI355X ray-march, in C++ above the C ABI.
//
// Plays the role of the reference application's render loop (src/application.cpp:59-95)
// without SDL/ImGui/Vulkan: import a dataset (NrrdFileParser / CsvFileParser restatements),
// set up the orbit camera and the gradient transfer function as the UI would, render frames
// through Vol::Rendering::Hip::OffscreenPass (include/vr/offscreen_pass_hip.hpp) and write the
// RGBA8 image as a binary PPM (the presentation shim of SURVEY.md §8f-3, headless form).
//
//   vr_cli <file.nhdr|file.nrrd|synthetic:N> <out.ppm> [--size WxH] [--radius R]
//          [--rotate DX,DY] [--tf default|demo] [--shading] [--exact-gradient] [--ert EPS]
//          [--skip-empty] [--frames K] [--device-mask M]   (M: render every frame across these GPUs)
//          [--mode composite|mip|iso|minip|mean]   (mip / minip / mean: maximum-, minimum- and
//                                        mean-intensity projection, include/vr/vr_modes.h;
//                                        iso: first-hit isosurface, include/vr/vr_iso.h)
//          [--iso V]   (the isosurface's density, in the volume's units; default 0)
//          [--mpr AXIS:POSITION[:NSAMPLES:SPACING:OP]]   (AXIS axial|coronal|sagittal, OP
//                                        max|min|mean: write the multi-planar reformat image
//                                        of include/vr/vr_mpr.h at --size -- the plane at
//                                        POSITION in [0,1] along the axis, thin or a slab of
//                                        NSAMPLES samples SPACING apart -- instead of the 3D frame)
//          [--histogram N[:LO:HI]]   (write, in place of the image, the volume's value histogram of
//                                        include/vr/vr_hist.h as one JSON object: N bins over
//                                        [LO, HI], by default the dataset's value window)
//          [--window P_LO:P_HI]   (render with the value window set to the percentiles P_LO .. P_HI,
//                                        in [0,1], of a 4096-bin histogram over the data's exact range)
//          [--pick X,Y --hit KIND[:THRESHOLD]]   (in place of the image, print the hit record of
//                                        framebuffer pixel (X, Y) of this camera's frame,
//                                        include/vr/vr_hit.h, as one JSON line: pos, depth, value
//                                        and step, -1 for a miss.  KIND entry|opacity|max|min|iso;
//                                        THRESHOLD is opacity's, default 0.5; iso reads --iso)
//          [--mesh OUT.ply[:open]]   (in place of the image, extract the isosurface at --iso as a
//                                        triangle mesh, include/vr/vr_mesh.h, write it as a binary
//                                        PLY in voxel units and print its three counts as one
//                                        JSON line.  :open leaves the surface open where a face of
//                                        the volume cuts it)
//          [--label LO:HI[:26] [--seed X,Y,Z]]   (in place of the image, label the connected
//                                        components of the value window [LO, HI] -- either may be
//                                        inf or -inf -- under 6- or (:26) 26-connectivity,
//                                        include/vr/vr_label.h, and print the info as one JSON
//                                        line; with a seed, a volume voxel index, also the record
//                                        of the seed's component as "seed")
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vr/offscreen_pass_hip.hpp"
#include "../../include/vr/vr_host.h"

namespace {
std::vector<std::string> split_colons(const std::string &s)
{
    std::vector<std::string> f;
    for (size_t b = 0;;) {
        const size_t e = s.find(':', b);
        f.push_back(s.substr(b, e == std::string::npos ? e : e - b));
        if (e == std::string::npos) break;
        b = e + 1;
    }
    return f;
}

// the whole of s as a number
bool parse_double(const std::string &s, double *v)
{
    if (s.empty()) return false;
    char *end = nullptr;
    *v = std::strtod(s.c_str(), &end);
    return end && *end == '\0';
}

// %.9g, with the non-finite values spelt as JSON readers that accept them do
void print_float(FILE *fp, float v)
{
    if (v != v)
        std::fprintf(fp, "NaN");
    else if (std::isinf(v))
        std::fprintf(fp, v > 0 ? "Infinity" : "-Infinity");
    else
        std::fprintf(fp, "%.9g", (double)v);
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <file.nhdr|synthetic:N> <out.ppm> [--size WxH] [--radius R] "
                             "[--rotate DX,DY] [--tf default|demo] [--shading] [--exact-gradient] [--ert EPS] [--skip-empty] "
                             "[--frames K] [--device-mask M] [--mode composite|mip|iso|minip|mean] [--iso V] "
                             "[--mpr axial|coronal|sagittal:POSITION[:NSAMPLES:SPACING:max|min|mean]] "
                             "[--histogram N[:LO:HI]] [--window P_LO:P_HI] "
                             "[--pick X,Y --hit entry|opacity|max|min|iso[:THRESHOLD]] [--mesh OUT.ply[:open]] "
                             "[--label LO:HI[:26] [--seed X,Y,Z]]\n",
                     argv[0]);
        return 2;
    }
    std::string src = argv[1], out = argv[2];
    uint32_t W = 800, H = 600;
    float radius = 3.0f, rx = 0.0f, ry = 0.0f, ert = 0.0f, iso = 0.0f;
    int shading = 0, skip_empty = 0, frames = 1, exact_gradient = 0;
    uint32_t mask = 0;
    std::string tfname = "default", mode = "composite", mpr, hist, window, pick, hit, mesh, label, seed;
    for (int i = 3; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--size" && i + 1 < argc) std::sscanf(argv[++i], "%ux%u", &W, &H);
        else if (a == "--radius" && i + 1 < argc) radius = std::strtof(argv[++i], nullptr);
        else if (a == "--rotate" && i + 1 < argc) std::sscanf(argv[++i], "%f,%f", &rx, &ry);
        else if (a == "--tf" && i + 1 < argc) tfname = argv[++i];
        else if (a == "--shading") shading = 1;
        else if (a == "--exact-gradient") exact_gradient = 1;
        else if (a == "--skip-empty") skip_empty = 1;
        else if (a == "--ert" && i + 1 < argc) ert = std::strtof(argv[++i], nullptr);
        else if (a == "--mode" && i + 1 < argc) mode = argv[++i];
        else if (a == "--iso" && i + 1 < argc) iso = std::strtof(argv[++i], nullptr);
        else if (a == "--mpr" && i + 1 < argc) mpr = argv[++i];
        else if (a == "--histogram" && i + 1 < argc) hist = argv[++i];
        else if (a == "--window" && i + 1 < argc) window = argv[++i];
        else if (a == "--pick" && i + 1 < argc) pick = argv[++i];
        else if (a == "--hit" && i + 1 < argc) hit = argv[++i];
        else if (a == "--mesh" && i + 1 < argc) mesh = argv[++i];
        else if (a == "--label" && i + 1 < argc) label = argv[++i];
        else if (a == "--seed" && i + 1 < argc) seed = argv[++i];
        else if (a == "--frames" && i + 1 < argc) frames = std::atoi(argv[++i]);
        else if (a == "--device-mask" && i + 1 < argc) mask = (uint32_t)std::strtoul(argv[++i], nullptr, 0);
        else {
            std::fprintf(stderr, "unknown argument %s\n", a.c_str());
            return 2;
        }
    }
    if (mode != "composite" && mode != "mip" && mode != "iso" && mode != "minip" && mode != "mean") {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    // --mpr AXIS:POSITION[:NSAMPLES:SPACING:OP]
    vr_mpr_plane plane{};
    if (!mpr.empty()) {
        const std::vector<std::string> f = split_colons(mpr);
        const int axis = f[0] == "sagittal" ? 0 : f[0] == "coronal" ? 1 : f[0] == "axial" ? 2 : -1;
        const int op = f.size() == 5 ? (f[4] == "max" ? VR_MPR_MAX : f[4] == "min" ? VR_MPR_MIN
                                        : f[4] == "mean" ? VR_MPR_MEAN : -1)
                                     : VR_MPR_MAX;
        if (axis < 0 || (f.size() != 2 && f.size() != 5) || op < 0) {
            std::fprintf(stderr, "bad --mpr %s (AXIS:POSITION[:NSAMPLES:SPACING:OP])\n", mpr.c_str());
            return 2;
        }
        const uint32_t ns = f.size() == 5 ? (uint32_t)std::strtoul(f[2].c_str(), nullptr, 10) : 1u;
        const float spacing = f.size() == 5 ? std::strtof(f[3].c_str(), nullptr) : 0.0f;
        if (vr_mpr_axis_plane(axis, std::strtof(f[1].c_str(), nullptr), W, H, ns, spacing, op, &plane) != VR_OK) {
            std::fprintf(stderr, "bad --mpr %s: %s\n", mpr.c_str(), vr_last_error(nullptr));
            return 2;
        }
    }
    // --histogram N[:LO:HI]
    uint32_t hist_bins = 0;
    bool hist_range = false;
    float hist_lo = 0.0f, hist_hi = 0.0f;
    if (!hist.empty()) {
        const std::vector<std::string> f = split_colons(hist);
        double n = 0.0, lo = 0.0, hi = 1.0;
        bool ok = (f.size() == 1 || f.size() == 3) && parse_double(f[0], &n) && n >= 1.0 &&
                  n <= (double)VR_HIST_MAX_BINS && n == std::floor(n);
        if (ok && f.size() == 3) {
            ok = parse_double(f[1], &lo) && parse_double(f[2], &hi);
            hist_lo = (float)lo;
            hist_hi = (float)hi;
            ok = ok && std::isfinite(hist_lo) && std::isfinite(hist_hi) && hist_lo < hist_hi;
            hist_range = true;
        }
        if (!ok) {
            std::fprintf(stderr, "bad --histogram %s (N[:LO:HI], 1 <= N <= %d, finite LO < HI)\n",
                         hist.c_str(), VR_HIST_MAX_BINS);
            return 2;
        }
        hist_bins = (uint32_t)n;
    }
    // --window P_LO:P_HI
    double win_lo = 0.0, win_hi = 1.0;
    if (!window.empty()) {
        const std::vector<std::string> f = split_colons(window);
        if (f.size() != 2 || !parse_double(f[0], &win_lo) || !parse_double(f[1], &win_hi) ||
            !(win_lo >= 0.0 && win_lo < win_hi && win_hi <= 1.0)) {
            std::fprintf(stderr, "bad --window %s (P_LO:P_HI, 0 <= P_LO < P_HI <= 1)\n", window.c_str());
            return 2;
        }
    }
    // --pick X,Y --hit KIND[:THRESHOLD]
    uint32_t pick_x = 0, pick_y = 0;
    int hit_kind = -1;
    float hit_threshold = 0.5f;
    if (!pick.empty() || !hit.empty()) {
        const std::vector<std::string> f = split_colons(hit);
        hit_kind = f[0] == "entry" ? VR_HIT_ENTRY : f[0] == "opacity" ? VR_HIT_OPACITY
                   : f[0] == "max" ? VR_HIT_MAX : f[0] == "min" ? VR_HIT_MIN
                   : f[0] == "iso" ? VR_HIT_ISO : -1;
        double th = 0.5;
        char tail = 0;
        const bool ok = hit_kind >= 0 && f.size() <= 2 && (f.size() == 1 || parse_double(f[1], &th)) &&
                        th > 0.0 && th <= 1.0 &&
                        std::sscanf(pick.c_str(), "%u,%u%c", &pick_x, &pick_y, &tail) == 2;
        if (!ok) {
            std::fprintf(stderr, "bad --pick %s --hit %s (X,Y and entry|opacity|max|min|iso[:THRESHOLD], "
                                 "0 < THRESHOLD <= 1)\n", pick.c_str(), hit.c_str());
            return 2;
        }
        hit_threshold = (float)th;
    }
    // --label LO:HI[:26] [--seed X,Y,Z]
    float label_lo = 0.0f, label_hi = 0.0f;
    uint32_t label_conn = 6, seed_xyz[3] = {0, 0, 0};
    if (!label.empty() || !seed.empty()) {
        const std::vector<std::string> f = split_colons(label);
        double lo = 0.0, hi = 0.0;
        char tail = 0;
        bool ok = (f.size() == 2 || (f.size() == 3 && f[2] == "26")) && parse_double(f[0], &lo) &&
                  parse_double(f[1], &hi) && lo <= hi;
        if (ok && !seed.empty())
            ok = std::sscanf(seed.c_str(), "%u,%u,%u%c", &seed_xyz[0], &seed_xyz[1], &seed_xyz[2], &tail) == 3;
        if (!ok) {
            std::fprintf(stderr, "bad --label %s --seed %s (LO:HI[:26] with LO <= HI, and X,Y,Z)\n", label.c_str(),
                         seed.c_str());
            return 2;
        }
        label_lo = (float)lo;
        label_hi = (float)hi;
        label_conn = f.size() == 3 ? 26u : 6u;
    }
    try {
        Vol::Rendering::Hip::OffscreenPass pass = mask ? Vol::Rendering::Hip::OffscreenPass(
                                                             nullptr, W, H, Vol::Rendering::Hip::DeviceMask{mask})
                                                       : Vol::Rendering::Hip::OffscreenPass(W, H);
        if (src.rfind("synthetic:", 0) == 0) {
            const uint32_t n = (uint32_t)std::atoi(src.c_str() + 10);
            float lo, hi;
            if (vr_generate_volume(pass.handle(), 0, VR_DTYPE_F32, n, n, n, 2024, &lo, &hi) != VR_OK)
                throw std::runtime_error(vr_last_error(pass.handle()));
        } else {
            vr_dataset ds{};
            if (vr_nrrd_load(src.c_str(), &ds) != 0) throw std::runtime_error(vr_host_last_error());
            const int rc = vr_set_volume(pass.handle(), ds.data, ds.dtype, ds.dims[0], ds.dims[1],
                                         ds.dims[2], ds.vmin, ds.vmax);
            vr_dataset_free(&ds);
            if (rc != VR_OK) throw std::runtime_error(vr_last_error(pass.handle()));
        }
        if (hist_bins) {  // the histogram in place of the image
            float mm[2] = {0.0f, 1.0f};
            if (!hist_range) {
                vr_debug_volume_info(pass.handle(), nullptr, mm, nullptr);
                hist_lo = mm[0];
                hist_hi = mm[1];
            }
            vr_hist_info info{};
            const std::vector<uint64_t> bins = pass.histogram(hist_bins, hist_lo, hist_hi, &info);
            FILE *fp = std::fopen(out.c_str(), "wb");
            if (!fp) throw std::runtime_error("cannot write " + out);
            std::fprintf(fp, "{\"nbins\": %u, \"lo\": ", hist_bins);
            print_float(fp, hist_lo);
            std::fprintf(fp, ", \"hi\": ");
            print_float(fp, hist_hi);
            std::fprintf(fp, ", \"bins\": [");
            for (uint32_t b = 0; b < hist_bins; ++b)
                std::fprintf(fp, b ? ", %llu" : "%llu", (unsigned long long)bins[b]);
            std::fprintf(fp, "], \"voxels\": %llu, \"below\": %llu, \"above\": %llu, \"nan\": %llu, \"vmin\": ",
                         (unsigned long long)info.voxels, (unsigned long long)info.below,
                         (unsigned long long)info.above, (unsigned long long)info.nan);
            print_float(fp, info.vmin);
            std::fprintf(fp, ", \"vmax\": ");
            print_float(fp, info.vmax);
            std::fprintf(fp, "}\n");
            std::fclose(fp);
            std::printf("histogram of %llu voxels in %u bins -> %s\n", (unsigned long long)info.voxels,
                        hist_bins, out.c_str());
            return 0;
        }
        if (!mesh.empty()) {  // the isosurface as a PLY in place of the image
            bool closed = true;
            std::string ply = mesh;
            if (ply.size() > 5 && ply.compare(ply.size() - 5, 5, ":open") == 0) {
                closed = false;
                ply.resize(ply.size() - 5);
            }
            const auto m = pass.extract_mesh(iso, closed, true);
            uint32_t dims[3] = {1, 1, 1};
            vr_debug_volume_info(pass.handle(), dims, nullptr, nullptr);
            // texture coordinates -> voxel units: voxel i's centre at i
            const float scale[3] = {(float)dims[0], (float)dims[1], (float)dims[2]}, offset[3] = {-0.5f, -0.5f, -0.5f};
            if (vr_mesh_write_ply(ply.c_str(), m.vertices.data(), m.info.vertices, m.triangles.data(),
                                  m.info.triangles, scale, offset) != 0)
                throw std::runtime_error(std::string("cannot write ") + ply + ": " + vr_host_last_error());
            std::printf("{\"vertices\": %llu, \"triangles\": %llu, \"inside_voxels\": %llu}\n",
                        (unsigned long long)m.info.vertices, (unsigned long long)m.info.triangles,
                        (unsigned long long)m.info.inside_voxels);
            return 0;
        }
        if (!label.empty()) {  // the components of a value window in place of the image
            // one labelling: the seed's record is the one its label names
            const auto l = pass.label_components(label_lo, label_hi, label_conn);
            const vr_label_info &info = l.info;
            vr_label_component c{};
            if (!seed.empty()) {
                uint32_t dims[3] = {0, 0, 0};
                vr_debug_volume_info(pass.handle(), dims, nullptr, nullptr);
                if (seed_xyz[0] >= dims[0] || seed_xyz[1] >= dims[1] || seed_xyz[2] >= dims[2])
                    throw std::runtime_error("seed lies outside the volume");
                const uint32_t lab = l.labels[seed_xyz[0] + (size_t)dims[0] * (seed_xyz[1] + (size_t)dims[1] * seed_xyz[2])];
                size_t a = 0, b = l.components.size();  // sorted by label
                while (a < b) {
                    const size_t m = (a + b) / 2;
                    if (l.components[m].label < lab) a = m + 1; else b = m;
                }
                if (lab && a < l.components.size() && l.components[a].label == lab) c = l.components[a];
            }
            std::printf("{\"voxels\": %llu, \"in_voxels\": %llu, \"components\": %llu, \"largest_voxels\": %llu, "
                        "\"largest_label\": %u",
                        (unsigned long long)info.voxels, (unsigned long long)info.in_voxels,
                        (unsigned long long)info.components, (unsigned long long)info.largest_voxels,
                        info.largest_label);
            if (!seed.empty())
                std::printf(", \"seed\": {\"label\": %u, \"voxels\": %llu, \"bbox_min\": [%u, %u, %u], "
                            "\"bbox_max\": [%u, %u, %u], \"sum\": [%llu, %llu, %llu]}",
                            c.label, (unsigned long long)c.voxels, c.bbox_min[0], c.bbox_min[1], c.bbox_min[2],
                            c.bbox_max[0], c.bbox_max[1], c.bbox_max[2], (unsigned long long)c.sum[0],
                            (unsigned long long)c.sum[1], (unsigned long long)c.sum[2]);
            std::printf("}\n");
            return 0;
        }
        if (!window.empty()) {  // the percentile window of a 4096-bin histogram over the exact range
            float mm[2] = {0.0f, 1.0f};
            vr_debug_volume_info(pass.handle(), nullptr, mm, nullptr);
            vr_hist_info info{};
            if (!(mm[0] < mm[1])) mm[0] = 0.0f, mm[1] = 1.0f;  // any range: this call is for info
            pass.histogram(1, mm[0], mm[1], &info);
            if (!(std::isfinite(info.vmin) && std::isfinite(info.vmax) && info.vmin < info.vmax))
                throw std::runtime_error("--window needs a volume with more than one finite value");
            const std::vector<uint64_t> bins = pass.histogram(VR_HIST_MAX_BINS, info.vmin, info.vmax);
            float w0 = 0.0f, w1 = 1.0f;
            if (vr_hist_window(bins.data(), VR_HIST_MAX_BINS, info.vmin, info.vmax, win_lo, win_hi, &w0,
                               &w1) != VR_OK)
                throw std::runtime_error(vr_last_error(nullptr));
            pass.value_range_changed(w0, w1);
            std::printf("window %.9g .. %.9g\n", (double)w0, (double)w1);
        }
        // transfer function as the UI produces it (main_window.cpp:248-257)
        vr_gradient *g = vr_gradient_create();
        if (tfname == "demo") {  // alpha markers (0,0) (0.14,0) (1,1)
            vr_gradient_set_alpha_marker(g, 0, 0.0f, 0.0f);
            float s[4];
            vr_gradient_sample(g, 0.14f, s);
            int idx = vr_gradient_add_alpha_marker(g, 0.14f, s[3]);
            vr_gradient_set_alpha_marker(g, (size_t)idx, 0.14f, 0.0f);
        }
        std::vector<uint32_t> tf(256);
        vr_gradient_discretize(g, tf.size(), tf.data());
        vr_gradient_destroy(g);
        pass.transfer_function_changed(tf);

        vr_orbit_camera oc;
        vr_cam_init(&oc);
        vr_cam_rotate(&oc, rx, ry);
        oc.radius = radius;
        Vol::Rendering::Hip::Camera cam{};
        vr_cam_view(&oc, cam.view);
        vr_cam_position(&oc, cam.position);
        pass.render_mode_changed(mode == "mip"     ? VR_MODE_MIP
                                 : mode == "iso"   ? VR_MODE_ISO
                                 : mode == "minip" ? VR_MODE_MINIP
                                 : mode == "mean"  ? VR_MODE_MEAN
                                                   : VR_MODE_COMPOSITE);
        pass.isovalue_changed(iso);  // state: read by iso frames only
        pass.params().shading = shading;
        pass.params().exact_gradient = exact_gradient;
        pass.params().skip_empty = skip_empty;
        pass.params().ert_eps = ert;

        if (hit_kind >= 0) {  // the pixel's hit record in place of the image
            const vr_hit h = pass.pick(cam, pick_x, pick_y, hit_kind, hit_threshold);
            std::printf("{\"pos\": [");
            for (int a = 0; a < 3; ++a) {
                if (a) std::printf(", ");
                print_float(stdout, h.pos[a]);
            }
            std::printf("], \"depth\": ");
            print_float(stdout, h.depth);
            std::printf(", \"value\": ");
            print_float(stdout, h.value);
            std::printf(", \"step\": %lld}\n", h.step == 0xFFFFFFFFu ? -1ll : (long long)h.step);
            return 0;
        }

        auto t0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> mpr_img(mpr.empty() ? 0 : (size_t)W * H);
        for (int f = 0; f < frames; ++f) {
            if (mpr.empty())
                pass.render(cam);
            else
                pass.render_mpr(plane, mpr_img.data(), VR_OUT_RGBA8);
        }
        auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count() / frames;
        const std::vector<uint32_t> &img = mpr.empty() ? pass.image() : mpr_img;
        FILE *fp = std::fopen(out.c_str(), "wb");
        if (!fp) throw std::runtime_error("cannot write " + out);
        std::fprintf(fp, "P6\n%u %u\n255\n", W, H);
        for (uint32_t px : img) {
            const unsigned char rgb[3] = {(unsigned char)(px & 0xFF), (unsigned char)((px >> 8) & 0xFF),
                                          (unsigned char)((px >> 16) & 0xFF)};
            std::fwrite(rgb, 1, 3, fp);
        }
        std::fclose(fp);
        std::printf("rendered %ux%u in %.3f ms/frame (incl. device->host copy) -> %s\n", W, H, ms,
                    out.c_str());
    } catch (std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
