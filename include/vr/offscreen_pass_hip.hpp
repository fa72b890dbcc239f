// offscreen_pass_hip.hpp — header-only C++ drop-in for Vol::Rendering::OffscreenPass
// (reference: src/rendering/offscreen_pass.h:27-148) over the C ABI in vr.h.
//
// The public surface is the reference's, with the same call shapes (offscreen_pass.h:40-54):
//
//   OffscreenPass(VulkanContext *context, uint32_t width, uint32_t height);
//   void record(VkCommandBuffer command_buffer, uint32_t frame_index);
//   void framebuffer_size_changed(uint32_t width, uint32_t height);
//   void volume_dataset_changed(Vol::Data::Dataset &dataset);
//   void slicing_changed(const glm::vec3 &min, const glm::vec3 &max);
//   void transfer_function_changed(const std::vector<glm::uint32_t> &data);
//   VkSampler get_sampler() const;   VkImageView get_image_view() const;
//
// so the reference's callers (vulkan_context.cpp:51, main_pass.cpp:91, imgui_context.cpp:67-74
// and :130-135, importer.cpp:43-46, main_window.cpp:233-238 and :250-257) compile unchanged
// against it (tests/shim/reference_call_shapes.cpp holds those lines verbatim).  The header
// carries no Vulkan, glm or SDL dependency: the host's types come in through a Traits class,
//
//   struct Traits {
//     using Context = VulkanContext;            // constructor's first argument
//     using CommandBuffer = VkCommandBuffer;    // record()'s first argument
//     using Sampler = VkSampler;  using ImageView = VkImageView;
//     static Camera camera();                   // pulled once per record(), as
//                                               // update_uniform_buffer pulls
//                                               // Application::main().get_scene().get_camera()
//                                               // (offscreen_pass.cpp:1155)
//     struct Presenter {                        // the host's colour attachment + sampler
//       Presenter(Context *, uint32_t w, uint32_t h);   // create_color_attachment & co.
//       void resize(uint32_t w, uint32_t h);             // framebuffer_size_changed
//       void present(CommandBuffer, uint32_t frame_index, const FrameImage &);
//                                               // staging buffer + copy_buffer_to_image
//                                               // (offscreen_pass.cpp:1379-1406)
//       Sampler get_sampler() const;  ImageView get_image_view() const;
//     };
//     static uint32_t device_mask();            // OPTIONAL: the GPUs every frame is split
//                                               // over (bit d = device d; vr_create_mask);
//                                               // absent or 0: device 0 alone
//   };
//
// and `using OffscreenPass = Vol::Rendering::Hip::BasicOffscreenPass<Traits>;`.  The HIP
// ray-march renders each frame (the reference's cube draw + volume.frag) into R8G8B8A8_UNORM
// pixels, get_image() is the handle to them, and the Presenter puts them where ImGui samples
// them.  Error behaviour as the reference: every failure throws std::runtime_error, zero
// framebuffer sizes are ignored (offscreen_pass.cpp:237-239), and construction installs the
// 1x1x1 {0} volume and the 1-texel 0xFFFFFFFF transfer function (:118-119).
//
// `HeadlessTraits` (no Vulkan: frames stay in host memory, camera from a callback) serves the
// CLI and tests; `OffscreenPass` below is BasicOffscreenPass<HeadlessTraits>.
#pragma once

#include <cstdint>
#include <functional>
#include <type_traits>
#include <stdexcept>
#include <string>
#include <vector>

#include "vr.h"
#include "vr_modes.h"
#include "vr_iso.h"
#include "vr_mpr.h"
#include "vr_hist.h"
#include "vr_hit.h"
#include "vr_mesh.h"
#include "vr_label.h"

namespace Vol::Rendering::Hip {

// Vol::Data::Dataset (src/data/dataset.h:9-13), float voxels as the reference loader produces.
struct Dataset {
    uint32_t dimensions[3];
    float min, max;
    std::vector<float> data;
};

struct Camera {
    float view[16];     // glm::mat4 column-major (Camera::get_view, camera.cpp:42-48)
    float position[3];  // Camera::get_position (camera.cpp:36-40)
};

// The frame record() produced: W*H R8G8B8A8_UNORM pixels (R in the low byte), row 0 at the
// top, in host memory owned by the pass (valid until the next record() or resize).
struct FrameImage {
    const uint32_t *rgba8 = nullptr;
    uint32_t width = 0, height = 0;
    uint32_t frame_index = 0;  // the frame_index record() was called with
    uint64_t frame = 0;        // frames recorded so far
};

// No Vulkan: frames stay in host memory; the camera comes from a settable callback.
struct HeadlessTraits {
    using Context = void;
    using CommandBuffer = void *;
    using Sampler = const FrameImage *;
    using ImageView = const FrameImage *;
    static std::function<Camera()> &camera_source()
    {
        static std::function<Camera()> f;
        return f;
    }
    static Camera camera()
    {
        if (!camera_source()) throw std::runtime_error("HeadlessTraits: no camera source set");
        return camera_source()();
    }
    struct Presenter {
        FrameImage last;
        Presenter(Context *, uint32_t, uint32_t) {}
        void resize(uint32_t, uint32_t) { last = FrameImage{}; }
        void present(CommandBuffer, uint32_t, const FrameImage &img) { last = img; }
        Sampler get_sampler() const { return &last; }
        ImageView get_image_view() const { return &last; }
    };
};

// The GPUs a pass renders on: an explicit DeviceMask argument, else Traits::device_mask() when
// the host's Traits declares it, else device 0.  The reference's construction call
// (vulkan_context.cpp:51, `new OffscreenPass(this, 100, 100)`) thus stays unchanged while a
// Traits with device_mask() = 0xFF renders every frame across a node's 8 GPUs.
struct DeviceMask {
    uint32_t bits;
};

namespace detail {
template <class T, class = void>
struct has_device_mask : std::false_type {};
template <class T>
struct has_device_mask<T, std::void_t<decltype(T::device_mask())>> : std::true_type {};
template <class T>
uint32_t traits_device_mask()
{
    if constexpr (has_device_mask<T>::value)
        return (uint32_t)T::device_mask();
    else
        return 0u;
}
inline vr_ctx *create_ctx(uint32_t mask, int device, uint32_t w, uint32_t h)
{
    return mask ? vr_create_mask(mask, w, h) : vr_create(device, w, h);
}
}  // namespace detail

template <class Traits>
class BasicOffscreenPass {
  public:
    using Context = typename Traits::Context;
    using CommandBuffer = typename Traits::CommandBuffer;
    using Sampler = typename Traits::Sampler;
    using ImageView = typename Traits::ImageView;

    // The host's glm clip form (vr_params.depth_zero_to_one, ABI 8).  glm fixes it when it is
    // first included (setup.hpp: GLM_CONFIG_CLIP_CONTROL from GLM_FORCE_DEPTH_ZERO_TO_ONE), so
    // read glm's own configuration when glm came before this header; without glm the default
    // [-1, 1] form -- the reference's build, whose define at offscreen_pass.cpp:3 comes after
    // glm's first include through offscreen_pass.h:3.
    static constexpr int32_t host_depth_zero_to_one()
    {
#if defined(GLM_CONFIG_CLIP_CONTROL) && defined(GLM_CLIP_CONTROL_ZO_BIT)
        return (GLM_CONFIG_CLIP_CONTROL & GLM_CLIP_CONTROL_ZO_BIT) ? 1 : 0;
#else
        return 0;
#endif
    }

    // offscreen_pass.cpp:112-134 (the GPUs: Traits::device_mask() if declared, else `device`)
    explicit BasicOffscreenPass(Context *context, uint32_t width, uint32_t height, int device = 0)
        : ctx_(detail::create_ctx(detail::traits_device_mask<Traits>(), device, width, height)),
          presenter_(context, width, height), width_(width), height_(height)
    {
        if (!ctx_) throw std::runtime_error(std::string("vr_create: ") + vr_last_error(nullptr));
        vr_params_default(&params_);
        params_.depth_zero_to_one = host_depth_zero_to_one();
    }
    // every frame split over the devices of `mask` (vr_create_mask)
    BasicOffscreenPass(Context *context, uint32_t width, uint32_t height, DeviceMask mask)
        : ctx_(vr_create_mask(mask.bits, width, height)), presenter_(context, width, height),
          width_(width), height_(height)
    {
        if (!ctx_) throw std::runtime_error(std::string("vr_create_mask: ") + vr_last_error(nullptr));
        vr_params_default(&params_);
        params_.depth_zero_to_one = host_depth_zero_to_one();
    }
    uint32_t device_mask() const
    {
        uint32_t m = 0;
        vr_get_device_mask(ctx_, &m);
        return m;
    }
    ~BasicOffscreenPass() { vr_destroy(ctx_); }
    BasicOffscreenPass(const BasicOffscreenPass &) = delete;
    BasicOffscreenPass &operator=(const BasicOffscreenPass &) = delete;

    // offscreen_pass.cpp:163-230 + update_uniform_buffer :1152-1171: pull the camera, render
    // the frame (HIP), hand it to the presenter for this command buffer.
    void record(CommandBuffer command_buffer, uint32_t frame_index)
    {
        const Camera camera = Traits::camera();
        render(camera);
        FrameImage img = get_image();
        img.frame_index = frame_index;
        presenter_.present(command_buffer, frame_index, img);
    }

    void framebuffer_size_changed(uint32_t width, uint32_t height)  // :232-255
    {
        if (width == 0 || height == 0) return;
        check(vr_resize(ctx_, width, height));
        width_ = width;
        height_ = height;
        image_.clear();
        presenter_.resize(width, height);
    }
    // :257-269; DatasetT: Vol::Data::Dataset ({glm::u32vec3 dimensions; float min, max;
    // std::vector<float> data}) or Hip::Dataset
    template <class DatasetT>
    void volume_dataset_changed(DatasetT &dataset)
    {
        check(vr_set_volume(ctx_, dataset.data.data(), VR_DTYPE_F32, dataset.dimensions[0],
                            dataset.dimensions[1], dataset.dimensions[2], dataset.min, dataset.max));
    }
    // :271-277; Vec3: glm::vec3 or anything indexable by [0..2]
    template <class Vec3>
    void slicing_changed(const Vec3 &min, const Vec3 &max)
    {
        const float a[3] = {(float)min[0], (float)min[1], (float)min[2]};
        const float b[3] = {(float)max[0], (float)max[1], (float)max[2]};
        check(vr_set_slicing(ctx_, a, b));
    }
    void transfer_function_changed(const std::vector<uint32_t> &data)  // :279-288
    {
        check(vr_set_transfer_function(ctx_, data.data(), (uint32_t)data.size()));
    }

    // Extension (vr_modes.h): VR_MODE_COMPOSITE, the reference's composite, VR_MODE_MIP,
    // maximum-intensity projection, VR_MODE_ISO, the first-hit isosurface, or VR_MODE_MINIP /
    // VR_MODE_MEAN, the minimum- and mean-intensity projections, for the frames
    // recorded from now on (a UI toggle calls it like slicing_changed)
    void render_mode_changed(int mode) { check(vr_set_render_mode(ctx_, mode)); }
    int render_mode() const
    {
        int m = VR_MODE_COMPOSITE;
        vr_get_render_mode(ctx_, &m);
        return m;
    }

    // Extension (vr_iso.h): the density of the VR_MODE_ISO surface, in the volume's own units,
    // for the frames recorded from now on (a UI slider calls it like slicing_changed)
    void isovalue_changed(float v) { check(vr_set_isovalue(ctx_, v)); }
    float isovalue() const
    {
        float v = 0.0f;
        vr_get_isovalue(ctx_, &v);
        return v;
    }

    // offscreen_pass.h:53-54: the presenter's sampler / view of the frame's image
    Sampler get_sampler() const { return presenter_.get_sampler(); }
    ImageView get_image_view() const { return presenter_.get_image_view(); }
    // the image handle: the last frame's pixels (empty before the first record())
    FrameImage get_image() const
    {
        FrameImage f;
        f.rgba8 = image_.empty() ? nullptr : image_.data();
        f.width = width_;
        f.height = height_;
        f.frame = frames_;
        return f;
    }

    // One frame for an explicit camera into the pass's host image (no presenter).
    const std::vector<uint32_t> &render(const Camera &camera)
    {
        vr_camera cam{};
        for (int i = 0; i < 16; ++i) cam.view[i] = camera.view[i];
        for (int i = 0; i < 3; ++i) cam.position[i] = camera.position[i];
        image_.resize((size_t)width_ * height_);
        check(vr_render(ctx_, &cam, &params_, image_.data(), VR_OUT_RGBA8));
        ++frames_;
        return image_;
    }
    // Same into device memory on a HIP stream (no host round trip), e.g. for Vulkan interop.
    void render_device(const Camera &camera, void *out_dev, void *hip_stream)
    {
        vr_camera cam{};
        for (int i = 0; i < 16; ++i) cam.view[i] = camera.view[i];
        for (int i = 0; i < 3; ++i) cam.position[i] = camera.position[i];
        check(vr_render_device(ctx_, &cam, &params_, out_dev, VR_OUT_RGBA8, 16, 0, 1, hip_stream));
    }

    // Extension (vr_mpr.h): a multi-planar reformat image -- a plane through the volume, thin or
    // a slab -- of the plane's own size (plane.width * plane.height pixels of format `fmt`, a
    // vr_out_format) into host memory; the render mode, the isovalue and the frame image stay as
    // they are.  Only params().clear_color is read.
    void render_mpr(const vr_mpr_plane &plane, void *out, int fmt)
    {
        check(vr_mpr_render(ctx_, &plane, &params_, out, fmt));
    }
    // Same into device memory on a HIP stream (asynchronous).
    void render_mpr_device(const vr_mpr_plane &plane, void *out_dev, int fmt, void *hip_stream)
    {
        check(vr_mpr_render_device(ctx_, &plane, &params_, out_dev, fmt, hip_stream));
    }

    // Extension (vr_hist.h): the value histogram of the resident volume over [lo, hi] in nbins
    // bins -- of the whole volume, or of the half-open voxel box [box_min, box_max) -- computed on
    // the device; the counts are returned, the out-of-range counts and the exact data range go to
    // *info (when not null).  The context's state and every frame stay as they are.
    std::vector<uint64_t> histogram(uint32_t nbins, float lo, float hi, vr_hist_info *info = nullptr,
                                    const uint32_t *box_min = nullptr, const uint32_t *box_max = nullptr)
    {
        vr_hist_request req{};
        req.lo = lo;
        req.hi = hi;
        req.nbins = nbins;
        req.use_box = box_min && box_max ? 1u : 0u;
        for (int a = 0; a < 3 && req.use_box; ++a) {
            req.box_min[a] = box_min[a];
            req.box_max[a] = box_max[a];
        }
        std::vector<uint64_t> bins(nbins && nbins <= VR_HIST_MAX_BINS ? nbins : 1u);
        vr_hist_info local{};
        check(vr_histogram(ctx_, &req, bins.data(), info ? info : &local));
        return bins;
    }
    // Extension (vr_hist.h): a new value window (Dataset.min / max) for the resident voxels,
    // without the re-upload volume_dataset_changed would need.
    void value_range_changed(float vmin, float vmax) { check(vr_set_value_range(ctx_, vmin, vmax)); }

    // Extension (vr_hit.h): where the pixels of this camera's frame come from -- one vr_hit per
    // pixel of the framebuffer, or of the pixel rectangle rect = {x0, y0, w, h} (row-major, top
    // row first): the point `kind` (a vr_hit_kind) finds along the pixel's ray, its distance from
    // the camera, the density there and the step.  Pass the kind that matches the frame shown;
    // threshold is VR_HIT_OPACITY's.  The context's state and every frame stay as they are.
    std::vector<vr_hit> hit_image(const Camera &camera, int kind, float threshold = 0.5f,
                                  const uint32_t *rect = nullptr)
    {
        vr_camera cam{};
        for (int i = 0; i < 16; ++i) cam.view[i] = camera.view[i];
        for (int i = 0; i < 3; ++i) cam.position[i] = camera.position[i];
        vr_hit_request req{};
        req.kind = kind;
        req.threshold = threshold;
        req.use_rect = rect ? 1u : 0u;
        for (int a = 0; a < 4 && rect; ++a) req.rect[a] = rect[a];
        const uint32_t w = rect ? rect[2] : width_, h = rect ? rect[3] : height_;
        // (a rectangle the call refuses may be of any size: the vector is sized by a valid one)
        const bool fits = !rect || ((uint64_t)rect[0] + w <= width_ && (uint64_t)rect[1] + h <= height_);
        std::vector<vr_hit> out(fits && w && h ? (size_t)w * h : 1u);
        check(vr_hit_render(ctx_, &cam, &params_, &req, out.data()));
        return out;
    }
    // Extension (vr_hit.h): the record of one framebuffer pixel, e.g. under a mouse click; a miss
    // has step 0xFFFFFFFF and depth +infinity.
    vr_hit pick(const Camera &camera, uint32_t px, uint32_t py, int kind, float threshold = 0.5f)
    {
        vr_camera cam{};
        for (int i = 0; i < 16; ++i) cam.view[i] = camera.view[i];
        for (int i = 0; i < 3; ++i) cam.position[i] = camera.position[i];
        vr_hit_request req{};
        req.kind = kind;
        req.threshold = threshold;
        vr_hit out{};
        check(vr_pick(ctx_, &cam, &params_, &req, px, py, &out));
        return out;
    }

    // Extension (vr_mesh.h): the isosurface at `iso` (density units) as an indexed triangle mesh,
    // extracted on the device: vertex records (texture coordinates as vr_hit.pos, outward unit
    // normals) and three indices per triangle.  closed: the surface is capped where a face of the
    // cube or of the voxel box [box_min, box_max) cuts it.  The context's state and every frame
    // stay as they are; vr_host.h vr_mesh_write_ply saves the result.
    struct Mesh {
        std::vector<vr_mesh_vertex> vertices;
        std::vector<uint32_t> triangles;  // 3 per triangle
        vr_mesh_info info{};
    };
    Mesh extract_mesh(float iso, bool closed = true, bool normals = true, const uint32_t *box_min = nullptr,
                      const uint32_t *box_max = nullptr)
    {
        vr_mesh_request req{};
        req.iso = iso;
        req.closed = closed ? 1u : 0u;
        req.normals = normals ? 1u : 0u;
        req.use_box = box_min && box_max ? 1u : 0u;
        for (int a = 0; a < 3 && req.use_box; ++a) {
            req.box_min[a] = box_min[a];
            req.box_max[a] = box_max[a];
        }
        Mesh m;
        check(vr_mesh_count(ctx_, &req, &m.info));
        const uint64_t nv = m.info.vertices, nt = m.info.triangles;
        m.vertices.resize(nv ? (size_t)nv : 1u);  // (never a NULL buffer)
        m.triangles.resize(nt ? (size_t)nt * 3 : 3u);
        check(vr_mesh_extract(ctx_, &req, m.vertices.data(), nv, m.triangles.data(), nt, &m.info));
        m.vertices.resize((size_t)nv);
        m.triangles.resize((size_t)nt * 3);
        return m;
    }

    // Extension (vr_label.h): the connected components of the value window [lo, hi] (density
    // units, either bound may be infinite) under 6- or 26-connectivity, labelled on the device:
    // one label per voxel of the volume or of the voxel box [box_min, box_max) in box-linear order
    // (0: not in the window; else 1 + the smallest index of the voxel's component) and one record
    // per component, sorted by label.  The context's state and every frame stay as they are.
    struct Labels {
        std::vector<uint32_t> labels;
        std::vector<vr_label_component> components;
        vr_label_info info{};
    };
    Labels label_components(float lo, float hi, uint32_t connectivity = 6, const uint32_t *box_min = nullptr,
                            const uint32_t *box_max = nullptr)
    {
        const vr_label_request req = label_request(lo, hi, connectivity, box_min, box_max);
        Labels l;
        // One labelling where the table has at most 65536 records: a larger one is sized by the
        // first call's VR_ENOSPC info (complete by then) and labelled once more.  A box the library
        // will refuse counts as no voxels here, and the call says why.
        const uint64_t n = label_voxels(req);
        uint64_t cap = 65536;
        l.labels.resize(n ? (size_t)n : 1u);  // (never a NULL buffer)
        l.components.resize((size_t)cap);
        int rc = vr_label_components(ctx_, &req, l.labels.data(), n, l.components.data(), cap, &l.info);
        if (rc == VR_ENOSPC && l.info.voxels == n && l.info.components > cap) {
            cap = l.info.components;
            l.components.resize((size_t)cap);
            rc = vr_label_components(ctx_, &req, l.labels.data(), n, l.components.data(), cap, &l.info);
        }
        check(rc);
        l.labels.resize((size_t)n);
        l.components.resize((size_t)l.info.components);
        return l;
    }
    // The component of the window that holds volume voxel `seed`: a mask byte per voxel of the
    // volume or the box (1: the seed's component) and the component's record; all zero where the
    // seed is not in the window.
    struct Region {
        std::vector<uint8_t> mask;
        vr_label_component component{};
    };
    Region grow_region(const uint32_t seed[3], float lo, float hi, uint32_t connectivity = 6,
                       const uint32_t *box_min = nullptr, const uint32_t *box_max = nullptr)
    {
        const vr_label_request req = label_request(lo, hi, connectivity, box_min, box_max);
        const uint64_t n = label_voxels(req);
        Region r;
        r.mask.resize(n ? (size_t)n : 1u);  // (never a NULL buffer)
        check(vr_region_grow(ctx_, &req, seed, r.mask.data(), n, &r.component));
        r.mask.resize((size_t)n);
        return r;
    }
    // The voxels of a request's box, or of the volume; 0 for a box the library refuses (empty,
    // inverted, beyond the volume or of more than 2^32 - 1 voxels), so that no buffer is sized by it.
    uint64_t label_voxels(const vr_label_request &req)
    {
        uint32_t dims[3] = {0, 0, 0};
        check(vr_debug_volume_info(ctx_, dims, nullptr, nullptr));
        uint64_t n = 1;
        for (int a = 0; a < 3; ++a) {
            const uint32_t lo = req.use_box ? req.box_min[a] : 0u, hi = req.use_box ? req.box_max[a] : dims[a];
            if (lo >= hi || hi > dims[a] || n > 0xFFFFFFFFull / (hi - lo)) return 0;
            n *= hi - lo;
        }
        return n;
    }
    static vr_label_request label_request(float lo, float hi, uint32_t connectivity, const uint32_t *box_min,
                                          const uint32_t *box_max)
    {
        vr_label_request req{};
        req.lo = lo;
        req.hi = hi;
        req.connectivity = connectivity;
        req.use_box = box_min && box_max ? 1u : 0u;
        for (int a = 0; a < 3 && req.use_box; ++a) {
            req.box_min[a] = box_min[a];
            req.box_max[a] = box_max[a];
        }
        return req;
    }

    const std::vector<uint32_t> &image() const { return image_; }
    vr_params &params() { return params_; }  // step, ERT, shading (reference defaults)
    vr_ctx *handle() { return ctx_; }
    typename Traits::Presenter &presenter() { return presenter_; }

  private:
    void check(int rc)
    {
        if (rc != VR_OK) throw std::runtime_error(vr_last_error(ctx_));
    }
    vr_ctx *ctx_;
    typename Traits::Presenter presenter_;
    uint32_t width_, height_;
    uint64_t frames_ = 0;
    vr_params params_{};
    std::vector<uint32_t> image_;
};

// Headless form: OffscreenPass(nullptr, w, h) or OffscreenPass(w, h).
class OffscreenPass : public BasicOffscreenPass<HeadlessTraits> {
  public:
    using BasicOffscreenPass<HeadlessTraits>::BasicOffscreenPass;
    OffscreenPass(uint32_t width, uint32_t height, int device = 0)
        : BasicOffscreenPass<HeadlessTraits>(nullptr, width, height, device)
    {
    }
};

}  // namespace Vol::Rendering::Hip
