// vr_ctx.h — private to csrc/vr_api*.hip: the context behind the C ABI and the host scaffold every
// device call is built from -- errors (fail, HIP_TRY), the multi-device delegation (on_replica), a
// timed interval (Interval) and a grow-on-demand device block (DevBlock, reserve).  vr_api.hip
// defines what is declared here; an analysis family (vr_api_<family>.hip) adds its request check,
// its argument struct and its list of passes on top.
#pragma once

#include "../../include/vr/vr.h"
#include "../../include/vr/vr_debug.h"
#include "../../include/vr/vr_modes.h"
#include "../../include/vr/vr_iso.h"
#include "../../include/vr/vr_mpr.h"
#include "../../include/vr/vr_hist.h"
#include "../../include/vr/vr_hit.h"
#include "../../include/vr/vr_label.h"
#include "../../include/vr/vr_mesh.h"
#include "vr_internal.h"
#include "vr_group.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

// (every includer is a vr_api*.hip: the rest of each is the vr namespace's, with explicit fmaf only)
using namespace vr;
#pragma clang fp contract(off)

namespace vr {
// A device block of the context, grown on demand by reserve(); p is NULL exactly while bytes is 0.
struct DevBlock {
    void *p = nullptr;
    size_t bytes = 0;
};
}

// vr_render (host output): row bands per frame, each copied to the host while later bands
// render (kHostBandMinRows rows at least, vr_internal.h).  C3 into pageable host memory, ms
// per frame, three rounds (profiles/r03/host_bands/): 4 bands 0.589-0.603 shaded, 0.470-0.488
// unshaded; 8 bands 0.730-0.753 / 0.557-0.560; 16 bands 1.13-1.63 / 0.86-0.90.  A page-locked
// destination changes nothing (4 bands 0.582 against 0.583; 2 bands 0.635-0.655, both
// kinds; profiles/r03/host_pinned/): the bands' own launches, not the copies, set the time.
#ifndef VR_HOST_BANDS
#define VR_HOST_BANDS 4
#endif
constexpr int kRenderBands = VR_HOST_BANDS;

struct vr_ctx {
    int device = 0;
    uint32_t width = 0, height = 0;
    // volume (bricked, native storage type)
    void *bricks = nullptr;
    size_t brick_bytes = 0;
    int storage = ST_F32;
    int layout = ST_F32;  // brick layout code (storage | kQuadFlag for 8-bit yz-quads)
    // the last frame's view (view_dense_rows): image x along the bricks' rows, dense sampling
    bool dense_rows = false;
    double pixel_span = 0.0;  // voxels per pixel step at the volume centre (view_dense_rows)
    double axis_align = 1.0;  // largest |component| of the centre ray's unit direction
    int ray_axis = 2;         // the volume axis of that component (0 x, 1 y, 2 z)
    double row_align = 1.0;   // |x component| of the unit pixel step along the image x axis
    // f32 volumes: further resident copies in the alternative geometries (kAltFlag for
    // oblique views, the plain and stencil copies for sparse ones, the y-major copy for
    // dense-row views along y), each built lazily on the first frame that wants it after a
    // volume change
    struct AltCopy {
        void *bricks = nullptr;  // stream-ordered allocation (hipMallocAsync)
        size_t bytes = 0;
        bool valid = false, failed = false;
        uint64_t used = 0;  // frame_no of the latest frame that read it (eviction order)
    } alt[4];
    uint32_t nx = 1, ny = 1, nz = 1;
    float vmin = 0.0f, vmax = 1.0f;
    // transfer function (decoded, linear float RGBA)
    float4 *tf = nullptr;
    uint32_t tf_n = 0;
    uint32_t *tf_nz = nullptr;  // prefix count of nonzero-alpha texels (tf_n + 1)
    float smin[3] = {0.0f, 0.0f, 0.0f};
    float smax[3] = {1.0f, 1.0f, 1.0f};
    int render_mode = VR_MODE_COMPOSITE;  // vr_modes.h: context state, like the slice box
    float isovalue = 0.0f;                // vr_iso.h: context state, read in VR_MODE_ISO only
    // empty-space classification (skip_empty), built lazily: per-brick value range after a
    // volume change, the brick distance field after a volume or TF change
    float2 *brick_range = nullptr;
    uint8_t *skip_dist = nullptr;  // 2 x nbricks: distance field + pass scratch
    size_t nbricks_alloc = 0;
    bool range_valid = false, dist_valid = false;
    // f32 shading: precomputed central differences (3 x the bricked density), built lazily
    // on the first shaded frame after a volume change; absent when memory is short
    float *grad = nullptr;  // stream-ordered allocation (hipMallocAsync)
    size_t grad_bytes = 0;
    bool grad_valid = false;
    uint64_t grad_used = 0;  // frame_no of the latest frame that read it
    bool grad_half = false;      // the field's precision (vr_params.exact_gradient == 0: binary16)
    // the y-major binary16 field (vr_internal.h F32Y; launch_grad_field ymajor): what a shaded
    // frame on the y-major copy reads in place of `grad`; opportunistic as that copy (ensure_yfield)
    float *ygrad = nullptr;  // stream-ordered allocation (hipMallocAsync)
    size_t ygrad_bytes = 0;
    bool ygrad_valid = false;
    int ygrad_scale_log2 = 0;
    int grad_scale_log2 = 0;     // and its scale (field_scale_log2 of the data's own range)
    // f32 storage: the stored voxels' min and max, zero border included (measured on the bricks
    // at upload): the binary16 field's scale comes from these, never from the caller's
    // vmin/vmax, which may be a display window narrower than the data
    float data_lo = 0.0f, data_hi = 1.0f;
    // adaptive tile order (tile_order 4): per launch geometry, the last launch's per-tile
    // durations and the workgroup -> tile permutation built from them
    // Keyed by the launch stream too: frames in flight on different streams each own their
    // duration/permutation buffers, so one stream's order kernel never rewrites a permutation
    // another stream's march kernel is reading.
    // Keyed by the row shard as well: one stream may render several shares of a frame (the
    // row bands of vr_render), each with its own tile durations.
    struct TileSched {
        uint32_t tiles_x = 0, tiles_y = 0, supers_x = 0, per_xcd = 0;
        uint32_t row_block = 0, rank = 0, nranks = 0, share_w0 = 1, share_w = 1;
        int pair = 0;
        uint32_t kernel = 0;  // variant_tile_key: another kernel's tile durations differ
        void *stream = nullptr;
        uint32_t *cost = nullptr, *perm = nullptr, *lists = nullptr;
        bool have_perm = false;
        uint32_t launches = 0;
    };
    std::vector<TileSched> sched;
    // lazily built derived fields (gradient, skip-empty) are produced on the stream of the
    // frame that first needs them; frames on other streams wait for this event
    hipEvent_t built_ev = nullptr;
    bool built_recorded = false;
    // Frame fences (round 6): for each stream that launched frames of this context, an event
    // recorded after its latest frame.  A derived structure that frames in flight may still read
    // is freed (or rewritten) stream-ordered on the evicting frame's stream after that stream
    // waited on every other stream's fence -- no device synchronisation on the frame path.
    struct Fence {
        hipStream_t stream;
        hipEvent_t ev;
        uint64_t used;
        bool external;        // recorded by the caller (vr_dist slot streams, vr_group.h)
        uint64_t build_seen;  // build_gen this stream last waited for (ensure_derived)
    };
    std::vector<Fence> fences;
    uint64_t build_gen = 0;  // records of built_ev so far
    uint64_t frame_no = 0;  // launches so far (the derived structures' recency)
    FrameVariant last_variant;  // the last frame or count launch (vr_debug_last_kernel_name)
    std::string last_mpr_name;  // not empty: an MPR or histogram launch (vr_mpr.h, vr_hist.h) came after it
    // derived-structure history (vr_memory_report, ABI 9)
    uint64_t n_builds = 0, n_evictions = 0, n_downgrades = 0;
    uint32_t last_downgrade = 0;
    // scratch
    unsigned long long *counters = nullptr;
    DevBlock frame_dev;
    // vr_mpr_render (host output): its image, whose size is the plane's and not the framebuffer's
    DevBlock mpr_dev;
    // vr_histogram (vr_hist.h): HistArgs::out (kHistOutWords 64-bit words), then the edge table
    DevBlock hist_dev;
    // vr_hit_render, vr_pick (vr_hit.h, host output): the records, grown on demand
    DevBlock hit_dev;
    // vr_mesh_* (vr_mesh.h): the passes' scratch (vr_internal.h MeshScratch), and vr_mesh_extract's
    // device copies of the two host buffers; all grown on demand
    DevBlock mesh_dev, mesh_out_dev;
    // vr_label_*, vr_region_grow* (vr_label.h): the context's own labels (4 bytes per voxel of the
    // box), the root table (vr_internal.h LabelScratch), the component records and vr_region_grow's
    // device copy of the host mask; all grown on demand
    DevBlock label_dev, label_aux_dev, label_tab_dev, label_out_dev;
    // vr_edt_squared*, vr_mask_morph* (vr_morph.h; csrc/vr_api_morph.hip in lib/libvr_amd_morph.so):
    // the morphology's distance (4 bytes per voxel of the grid), the intermediate mask of open and
    // close (1 byte per voxel), the counters, and the host forms' device copies of their arrays; all
    // grown on demand.  morph_last_name: the family's last kernel (vr_morph_last_kernel_name)
    DevBlock morph_dist_dev, morph_tmp_dev, morph_cnt_dev, morph_io_dev;
    const char *morph_last_name = "";
    // vr_mask_label*, vr_mask_select* (vr_maskcc.h; csrc/vr_api_maskcc.hip in lib/libvr_amd_maskcc.so):
    // vr_mask_select's labels (4 bytes per voxel of the grid), the root table and the counters, the
    // records with their keep flags, and the host forms' device copies of their arrays; all grown on
    // demand.  maskcc_last_name: the family's last kernel (vr_maskcc_last_kernel_name)
    DevBlock maskcc_lab_dev, maskcc_aux_dev, maskcc_tab_dev, maskcc_io_dev;
    const char *maskcc_last_name = "";
    // kernel ms of the last call's passes (vr_maskcc_kernels.h MccPass), taken while timing is
    // enabled; 0 for a pass that call did not run (vr_debug_maskcc_pass_ms, csrc/vr_api_maskcc.hip)
    float maskcc_pass_ms[9] = {};
    // vr_mask_stats*, vr_label_stats*, vr_mask_window* (vr_mstat.h; csrc/vr_api_mstat.hip in
    // lib/libvr_amd_mstat.so): the counters, the histogram's counts and edges and per record its
    // accumulators, its record and its compacted label (vr_mstat_host.h MstatGeom), and the host
    // forms' device copies of their arrays; both grown on demand.  mstat_last_name: the family's last
    // kernel (vr_mstat_last_kernel_name)
    DevBlock mstat_aux_dev, mstat_io_dev;
    const char *mstat_last_name = "";
    // vr_mask_occupancy_device, vr_mask_hit_render*, vr_mask_pick, vr_mask_slice* (vr_mview.h;
    // csrc/vr_api_mview.hip in lib/libvr_amd_mview.so): the counters of a call, and the host forms'
    // and the pick's device copies of their array and their output; both grown on demand.
    // mview_last_name: the family's last kernel (vr_mview_last_kernel_name)
    DevBlock mview_cnt_dev, mview_io_dev;
    const char *mview_last_name = "";
    // vr_mask_mesh_count*, vr_mask_mesh_extract* (vr_mmesh.h; csrc/vr_api_mmesh.hip in
    // lib/libvr_amd_mmesh.so): the inside bits, the words, prefixes and sums of a call
    // (vr_mmesh_host.h MmeshScratch), the two `local` arrays of the smoothing sweeps, and the host
    // forms' device copies of their array and of their mesh; all grown on demand.
    // mmesh_last_name: the family's last kernel (vr_mmesh_last_kernel_name)
    DevBlock mmesh_aux_dev, mmesh_loc_dev, mmesh_io_dev, mmesh_out_dev;
    const char *mmesh_last_name = "";
    // vr_debug_label_pass_ms: kernel ms of the last label call's passes (vr_internal.h LabelPassSlot),
    // taken while timing is enabled; 0 for a pass that call did not run
    float label_pass_ms[kLabelPassSlots] = {};
    // vr_render (host output): row bands rendered on two streams while finished bands copy
    // to the host on a third, so the PCIe copy hides behind the rest of the frame
    hipStream_t band_stream[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr;
    hipEvent_t band_ev[kRenderBands] = {};
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending;
    double timed_ms = 0.0;
    uint64_t timed_launches = 0;
    // launch-policy overrides for tests and A/B experiments (include/vr/vr_debug.h); the
    // product path never reads the process environment
    struct Knobs {
        int pipeline = -1, pair = -1, pair_lanes = 0, grad_field = -1, u8_layout = -1,
            tile_order = 0, narrow = 1, alt = -1, mip_inflight = 0, field_order = -1, hist_agg = -1,
            hit_inflight = -1;
    } knobs;
    // multi-device context (vr_create_mask): one member context per device of the mask, the
    // volume/TF/slicing replicated on each, frames rendered across them by `group`
    std::vector<vr_ctx *> members;
    vr::Group *group = nullptr;
    uint32_t device_mask = 0;
    hipStream_t group_stream = nullptr;  // vr_render's frame stream (device 0)
    // row blocks over ranks for vr_render_device (nranks > 1), vr_assemble_rows and every frame
    // of a multi-device context (vr_set_row_share; vr_internal.h RowShare)
    RowShare share{1, 1};
    // device bytes the derived structures (difference field, alternative copies, skip-empty
    // classification) may take together (vr_set_memory_budget): VR_MEMORY_BUDGET_DEFAULT
    // (kDerivedBudgetBricks x the bricks), VR_MEMORY_BUDGET_UNLIMITED, or a byte count
    uint64_t budget = VR_MEMORY_BUDGET_DEFAULT;
    std::string err;
};

namespace vr {

// A refused call: the message on the context (the thread, for a NULL context), the code returned;
// hip_fail: the same for a HIP error (VR_ENOMEM or VR_EIO).
int fail(vr_ctx *c, int code, const std::string &msg);
int hip_fail(vr_ctx *c, hipError_t e, const char *what);

#define HIP_TRY(c, expr, what)                        \
    do {                                              \
        hipError_t _e = (expr);                       \
        if (_e != hipSuccess) return hip_fail(c, _e, what); \
    } while (0)

int wait_idle(vr_ctx *c);  // waits for the context's device (resource swaps)
int check_params(vr_ctx *c, const vr_params *p);
// The camera and parameter checks and the ray constants of one rank's share of a frame.
int build_params(vr_ctx *c, const vr_camera *cam, const vr_params *p, void *out, int out_format,
                 uint32_t row_block, uint32_t rank, uint32_t nranks, RowShare share, MarchParams &P);
int read_counters(vr_ctx *c, vr_stats *out);  // a counting launch's five counters (synchronous)

// ordered f32 key (launch_minmax, the histogram's extremes) -> the float
inline float unorder(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// ---- multi-device contexts (vr_create_mask) ----
inline bool is_group(const vr_ctx *c) { return c && c->group; }

// Resource swaps on a multi-device context: every issued frame done on every device first.
inline int group_idle(vr_ctx *c)
{
    std::string m;
    return group_synchronize(c->group, &m) != VR_OK ? fail(c, VR_EIO, m) : VR_OK;
}

// A member's failure reported on the multi-device context.
inline int member_rc(vr_ctx *c, vr_ctx *m, int rc)
{
    if (rc != VR_OK) c->err = m->err;
    return rc;
}

// A call that only reads the scene, on a multi-device context: once the group is idle, on the
// lowest device, which holds a replica.  call(m): the entry point itself on member m.
template <class F>
int on_replica(vr_ctx *c, F call)
{
    if (int rc = group_idle(c)) return rc;
    return member_rc(c, c->members[0], call(c->members[0]));
}

// A setter on a multi-device context: once the group is idle, on every member.
template <class F>
int on_members(vr_ctx *c, F call)
{
    if (int rc = group_idle(c)) return rc;
    for (vr_ctx *m : c->members)
        if (int rc = call(m)) return member_rc(c, m, rc);
    return VR_OK;
}

hipEvent_t pooled_event(vr_ctx *c);  // an event for kernel timing from the context's pool

// One timed interval on a stream: with timing enabled, begin() and end() record a pair of pooled
// events around the launches between them and queue the pair for vr_timing_read (one launch of its
// count); without, both do nothing.  An interval dropped before end() -- an early return on an
// error -- hands its events back to the pool.  Reusable after end().
struct Interval {
    vr_ctx *c = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    Interval() = default;
    Interval(const Interval &) = delete;
    ~Interval()
    {
        for (hipEvent_t e : {e0, e1})
            if (e) c->ev_pool.push_back(e);
    }
    int begin(vr_ctx *ctx, hipStream_t stream)
    {
        c = ctx;
        s = stream;
        if (!c->timing) return VR_OK;  // read once: the pair is recorded and queued together
        e0 = pooled_event(c);
        e1 = pooled_event(c);
        if (!e0 || !e1) return fail(c, VR_EIO, "hipEventCreate failed");
        HIP_TRY(c, hipEventRecord(e0, s), "hipEventRecord");
        return VR_OK;
    }
    int end()
    {
        if (!e0) return VR_OK;
        HIP_TRY(c, hipEventRecord(e1, s), "hipEventRecord");
        c->ev_pending.emplace_back(e0, e1);
        e0 = e1 = nullptr;
        return VR_OK;
    }
};

// Block b of at least `need` bytes: one that is too small is freed and allocated anew, its contents
// lost (`what` names the allocation in an error).
// idle_first: not NULL where the device is drained before the old block is freed (the text names
// that wait in an error): a block that a *_device call's passes read on the caller's stream, which
// an earlier call's may still be doing.  NULL where the call that filled the block also copied it
// out synchronously, so nothing in flight reads it.
int reserve(vr_ctx *c, DevBlock &b, size_t need, const char *what, const char *idle_first);

}  // namespace vr
