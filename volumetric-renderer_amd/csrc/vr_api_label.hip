// vr_api_label.hip — connected components and region growing (include/vr/vr_label.h) on the host
// scaffold of vr_ctx.h.
#include "vr_ctx.h"
#include "vr_label_host.h"

namespace {
// What vr_label.h refuses before it looks at the context: the NULL arguments and the request's own
// fields (csrc/vr_label_host.h); no HIP call.
int check_label_request(vr_ctx *c, const vr_label_request *req, const void *a, const void *b, const void *d)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    if (!req || !a || !b || !d) return fail(c, VR_EINVAL, "NULL argument");
    if (const char *m = label_request_error(req->lo, req->hi, req->connectivity, req->use_box))
        return fail(c, VR_EINVAL, m);
    return VR_OK;
}

// The context's blocks of this family grow behind a wait for the device: an earlier call's passes
// may still read the old block on another stream (reserve's idle_first).
constexpr const char *kLabelIdle = "hipDeviceSynchronize (label scratch)";

// One call's passes on stream s; c is a single-device context.  The timing events bracket the
// labelling passes as one interval, the table passes as another and a region grow's mask pass as a
// third (the copies of the counts to the host and the host's waits lie between them).
struct LabelRun {
    vr_ctx *c;
    hipStream_t s;
    LabelArgs A;
    LabelBox box;
    Interval timed;

    int end()
    {
        const hipEvent_t e0 = timed.e0, e1 = timed.e1;  // (both NULL without timing)
        if (int rc = timed.end()) return rc;
        last0 = e0;
        last1 = e1;
        return VR_OK;
    }
    // Per-pass times for vr_debug_label_pass_ms (timing enabled only): an event after every pass
    // but an interval's last, whose end is the interval's own e1; read by passes_read after the
    // call's wait for the stream.  The interval itself stays one pair in ev_pending.
    hipEvent_t last0 = nullptr, last1 = nullptr;
    std::vector<std::pair<int, hipEvent_t>> marks;  // (the slot that ended, the event after it)
    int mark(int slot)
    {
        if (!timed.e0) return VR_OK;
        hipEvent_t e = pooled_event(c);
        if (!e) return fail(c, VR_EIO, "hipEventCreate failed");
        HIP_TRY(c, hipEventRecord(e, s), "hipEventRecord");
        marks.emplace_back(slot, e);
        return VR_OK;
    }
    // after end() and a wait for s: the slots of `marks`, then last_slot up to the interval's end
    int passes_read(int last_slot)
    {
        if (!last0 || !last1) return VR_OK;
        hipEvent_t from = last0;
        for (auto &m : marks) {
            HIP_TRY(c, hipEventElapsedTime(&c->label_pass_ms[m.first], from, m.second), "hipEventElapsedTime");
            if (from != last0) c->ev_pool.push_back(from);
            from = m.second;
        }
        HIP_TRY(c, hipEventElapsedTime(&c->label_pass_ms[last_slot], from, last1), "hipEventElapsedTime");
        if (from != last0) c->ev_pool.push_back(from);
        marks.clear();
        last0 = last1 = nullptr;
        return VR_OK;
    }

    // The volume and the box: everything the host knows before a kernel.  No HIP call.
    int resolve(const vr_label_request *req)
    {
        if (!c->bricks) return fail(c, VR_EINVAL, "no volume");
        const uint32_t dims[3] = {c->nx, c->ny, c->nz};
        if (const char *m = label_box_resolve(req->use_box, req->box_min, req->box_max, dims, &box))
            return fail(c, VR_EINVAL, m);
        std::memset(&A, 0, sizeof A);
        const uint32_t cells[3] = {(uint32_t)brick_cells(c->layout, 0), (uint32_t)brick_cells(c->layout, 1),
                                   (uint32_t)brick_cells(c->layout, 2)};
        const uint64_t nwork = box_brick_range(box, cells, (uint32_t)kPad, A.b0, A.nb);
        if (nwork >= 1ull << 31) return fail(c, VR_EINVAL, "label box holds too many bricks");
        for (int a = 0; a < 3; ++a) {
            A.blo[a] = box.lo[a];
            A.bhi[a] = box.hi[a];
            A.ext[a] = box.ext[a];
        }
        A.lo = req->lo;
        A.hi = req->hi;
        A.nwork = (uint32_t)nwork;
        A.nvox = (uint32_t)box.voxels;
        A.nwords = (uint32_t)((box.voxels + 63) / 64);
        A.nchunks = (uint32_t)((box.voxels + kLabelChunk - 1) / kLabelChunk);
        A.nbx = bricks_for(c->nx, 0, c->layout);
        A.nby = bricks_for(c->ny, 1, c->layout);
        A.vol = c->bricks;
        return VR_OK;
    }
    // The context's own label array, for the calls that hand no labels out on the device.
    int own_labels()
    {
        HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
        return reserve(c, c->label_dev, (size_t)box.voxels * 4, "hipMalloc(labels)", kLabelIdle);
    }
    // The labelling passes into labels_dev, then the counts to the host (waits for s).  *I is
    // written only on VR_OK: voxels, in_voxels and components.
    int label(const vr_label_request *req, void *labels_dev, vr_label_info *I)
    {
        HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
        const LabelScratch sc = label_scratch(box.voxels);
        if (int rc = reserve(c, c->label_aux_dev, sc.bytes, "hipMalloc(label root table)", kLabelIdle)) return rc;
        char *base = static_cast<char *>(c->label_aux_dev.p);
        A.P = static_cast<uint32_t *>(labels_dev);
        A.mask = reinterpret_cast<unsigned long long *>(base + sc.mask);
        A.wpre = reinterpret_cast<uint32_t *>(base + sc.wpre);
        A.chunk = reinterpret_cast<uint32_t *>(base + sc.chunk);
        A.out = reinterpret_cast<unsigned long long *>(base + sc.out);
        HIP_TRY(c, hipMemsetAsync(A.out, 0, 32, s), "hipMemset(label counts)");
        for (float &v : c->label_pass_ms) v = 0.0f;
        if (int rc = timed.begin(c, s)) return rc;
        std::string name;
        for (int pass = 0; pass < kLabelPasses; ++pass) {  // local, seam, flatten, scan
            HIP_TRY(c, launch_label(c->layout, (int)req->connectivity, pass, A, s, &name), "label launch");
            if (pass + 1 < kLabelPasses)
                if (int rc = mark(kLabelLocal + pass)) return rc;
        }
        c->last_mpr_name = name;
        if (int rc = end()) return rc;
        unsigned long long h[2];
        HIP_TRY(c, hipMemcpyAsync(h, A.out, sizeof h, hipMemcpyDeviceToHost, s), "hipMemcpy(label counts)");
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(label counts)");
        if (int rc = passes_read(kLabelScan)) return rc;
        std::memset(I, 0, sizeof *I);
        I->voxels = box.voxels;
        I->components = h[0];
        I->in_voxels = h[1];
        return VR_OK;
    }
    // The component table of I->components records into the context's block (A.comps), and the
    // largest component into *I (waits for s).
    int table(vr_label_info *I)
    {
        if (!I->components) return VR_OK;
        if (int rc = reserve(c, c->label_tab_dev, (size_t)I->components * kLabelComponentBytes,
                             "hipMalloc(label components)", kLabelIdle))
            return rc;
        A.comps = c->label_tab_dev.p;
        A.ncomps = (uint32_t)I->components;
        if (int rc = timed.begin(c, s)) return rc;
        for (int pass = 0; pass < 3; ++pass) {  // init, accumulate, largest
            HIP_TRY(c, launch_label_table(pass, A, s), "label table launch");
            if (pass < 2)
                if (int rc = mark(kLabelTableInit + pass)) return rc;
        }
        if (int rc = end()) return rc;
        unsigned long long key = 0;
        HIP_TRY(c, hipMemcpyAsync(&key, A.out + 2, sizeof key, hipMemcpyDeviceToHost, s), "hipMemcpy(label largest)");
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(label largest)");
        if (int rc = passes_read(kLabelLargest)) return rc;
        I->largest_voxels = key >> 32;
        I->largest_label = ~(uint32_t)key;
        return VR_OK;
    }
    // The seed's component: the mask into mask_dev and its record into *comp (waits for s).
    int grow(const vr_label_request *req, const uint32_t seed[3], void *mask_dev, vr_label_component *comp)
    {
        if (int rc = own_labels()) return rc;
        vr_label_info I;
        if (int rc = label(req, c->label_dev.p, &I)) return rc;
        uint32_t lab = 0;
        HIP_TRY(c, hipMemcpyAsync(&lab, A.P + (size_t)label_linear(box, seed), sizeof lab, hipMemcpyDeviceToHost, s),
                "hipMemcpy(seed label)");
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(seed label)");
        vr_label_component R;
        std::memset(&R, 0, sizeof R);
        if (!lab) {
            HIP_TRY(c, hipMemsetAsync(mask_dev, 0, (size_t)box.voxels, s), "hipMemset(region mask)");
        } else {
            if (int rc = reserve(c, c->label_tab_dev, kLabelComponentBytes, "hipMalloc(label components)", kLabelIdle))
                return rc;
            A.comps = c->label_tab_dev.p;
            A.ncomps = 1;
            A.grow = static_cast<uint8_t *>(mask_dev);
            A.seed_label = lab;
            if (int rc = timed.begin(c, s)) return rc;
            HIP_TRY(c, launch_label_table(0, A, s), "label table launch");
            if (int rc = mark(kLabelTableInit)) return rc;
            HIP_TRY(c, launch_label_grow(A, s), "region grow launch");
            if (int rc = end()) return rc;
            HIP_TRY(c, hipMemcpyAsync(&R, A.comps, sizeof R, hipMemcpyDeviceToHost, s), "hipMemcpy(region record)");
        }
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(region grow)");
        if (lab)
            if (int rc = passes_read(kLabelGrow)) return rc;
        R.label = lab;
        *comp = R;
        return VR_OK;
    }
};
static_assert(sizeof(vr_label_component) == kLabelComponentBytes && sizeof(vr_label_info) == 40 &&
                  sizeof(vr_label_request) == 40,
              "vr_label.h");
}  // namespace

extern "C" {

int vr_label_count(vr_ctx *c, const vr_label_request *req, vr_label_info *info)
{
    if (int rc = check_label_request(c, req, info, info, info)) return rc;
    if (is_group(c)) return on_replica(c, [&](vr_ctx *m) { return vr_label_count(m, req, info); });
    LabelRun R{c, nullptr};
    if (int rc = R.resolve(req)) return rc;
    if (int rc = R.own_labels()) return rc;
    vr_label_info I;
    if (int rc = R.label(req, c->label_dev.p, &I)) return rc;
    if (int rc = R.table(&I)) return rc;
    *info = I;
    return VR_OK;
}

int vr_label_components_device(vr_ctx *c, const vr_label_request *req, void *labels_dev, uint64_t lcap,
                               void *comps_dev, uint64_t ccap, vr_label_info *info, void *stream)
{
    if (int rc = check_label_request(c, req, labels_dev, comps_dev, info)) return rc;
    if (!label_pointer_ok(labels_dev)) return fail(c, VR_EINVAL, "labels_dev must be 4-byte aligned");
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) {
            return vr_label_components_device(m, req, labels_dev, lcap, comps_dev, ccap, info, stream);
        });
    LabelRun R{c, static_cast<hipStream_t>(stream)};
    if (int rc = R.resolve(req)) return rc;
    if (!label_capacity_ok(lcap, R.box.voxels)) {
        *info = vr_label_info{R.box.voxels};  // known on the host: the voxels alone, every other count 0
        return fail(c, VR_ENOSPC, "label buffer is smaller than the box (see the info's voxels)");
    }
    vr_label_info I;
    if (int rc = R.label(req, labels_dev, &I)) return rc;
    if (int rc = R.table(&I)) return rc;
    if (!label_capacity_ok(ccap, I.components)) {
        *info = I;
        return fail(c, VR_ENOSPC, "component buffer is smaller than the table (see the info's components)");
    }
    if (I.components) {
        HIP_TRY(c, hipMemcpyAsync(comps_dev, R.A.comps, (size_t)I.components * kLabelComponentBytes,
                                  hipMemcpyDeviceToDevice, R.s), "hipMemcpy(label components)");
        HIP_TRY(c, hipStreamSynchronize(R.s), "hipStreamSynchronize(label components)");
    }
    *info = I;
    return VR_OK;
}

int vr_label_components(vr_ctx *c, const vr_label_request *req, uint32_t *labels_host, uint64_t lcap,
                        vr_label_component *comps_host, uint64_t ccap, vr_label_info *info)
{
    if (int rc = check_label_request(c, req, labels_host, comps_host, info)) return rc;
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) {
            return vr_label_components(m, req, labels_host, lcap, comps_host, ccap, info);
        });
    LabelRun R{c, nullptr};
    if (int rc = R.resolve(req)) return rc;
    if (!label_capacity_ok(lcap, R.box.voxels)) {
        *info = vr_label_info{R.box.voxels};  // known on the host: the voxels alone, every other count 0
        return fail(c, VR_ENOSPC, "label buffer is smaller than the box (see the info's voxels)");
    }
    if (int rc = R.own_labels()) return rc;
    vr_label_info I;
    if (int rc = R.label(req, c->label_dev.p, &I)) return rc;
    if (int rc = R.table(&I)) return rc;
    HIP_TRY(c, hipMemcpy(labels_host, c->label_dev.p, (size_t)R.box.voxels * 4, hipMemcpyDeviceToHost),
            "hipMemcpy(labels)");
    if (!label_capacity_ok(ccap, I.components)) {
        *info = I;
        return fail(c, VR_ENOSPC, "component buffer is smaller than the table (see the info's components)");
    }
    if (I.components)
        HIP_TRY(c, hipMemcpy(comps_host, R.A.comps, (size_t)I.components * kLabelComponentBytes,
                             hipMemcpyDeviceToHost), "hipMemcpy(label components)");
    *info = I;
    return VR_OK;
}

int vr_region_grow_device(vr_ctx *c, const vr_label_request *req, const uint32_t seed[3], void *mask_dev,
                          uint64_t mcap, vr_label_component *comp_out, void *stream)
{
    if (int rc = check_label_request(c, req, seed, mask_dev, comp_out)) return rc;
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) {
            return vr_region_grow_device(m, req, seed, mask_dev, mcap, comp_out, stream);
        });
    LabelRun R{c, static_cast<hipStream_t>(stream)};
    if (int rc = R.resolve(req)) return rc;
    if (!label_seed_ok(R.box, seed)) return fail(c, VR_EINVAL, "seed lies outside the box");
    if (!label_capacity_ok(mcap, R.box.voxels))
        return fail(c, VR_ENOSPC, "mask buffer is smaller than the box");
    return R.grow(req, seed, mask_dev, comp_out);
}

int vr_region_grow(vr_ctx *c, const vr_label_request *req, const uint32_t seed[3], uint8_t *mask_host,
                   uint64_t mcap, vr_label_component *comp_out)
{
    if (int rc = check_label_request(c, req, seed, mask_host, comp_out)) return rc;
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) { return vr_region_grow(m, req, seed, mask_host, mcap, comp_out); });
    LabelRun R{c, nullptr};
    if (int rc = R.resolve(req)) return rc;
    if (!label_seed_ok(R.box, seed)) return fail(c, VR_EINVAL, "seed lies outside the box");
    if (!label_capacity_ok(mcap, R.box.voxels))
        return fail(c, VR_ENOSPC, "mask buffer is smaller than the box");
    HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    if (int rc = reserve(c, c->label_out_dev, (size_t)R.box.voxels, "hipMalloc(region mask)", kLabelIdle)) return rc;
    vr_label_component comp;
    if (int rc = R.grow(req, seed, c->label_out_dev.p, &comp)) return rc;
    HIP_TRY(c, hipMemcpy(mask_host, c->label_out_dev.p, (size_t)R.box.voxels, hipMemcpyDeviceToHost),
            "hipMemcpy(region mask)");
    *comp_out = comp;
    return VR_OK;
}

}  // extern "C"
