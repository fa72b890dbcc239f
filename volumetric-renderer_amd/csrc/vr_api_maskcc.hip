// vr_api_maskcc.hip — the components of a mask: labels, records, selection and hole filling
// (include/vr/vr_maskcc.h) on the host scaffold of vr_ctx.h and vr_mask_call.h.  Built into lib/libvr_amd_maskcc.so,
// which takes the scaffold (fail, hip_fail, reserve, pooled_event, the group's wait) from
// libvr_amd.so.
#include "vr_mask_call.h"
#include "../../include/vr/vr_maskcc.h"
#include "vr_maskcc_kernels.h"

namespace {
static_assert(VR_MASKCC_MAX_EXTENT == kMaskMaxExtent && VR_MASK_FILL_HOLES + 1 == kMccRules &&
                  VR_MASK_KEEP_LARGEST == kMccKeepLargest &&
                  VR_MASK_KEEP_MIN_VOXELS == kMccKeepMinVoxels && VR_MASK_KEEP_SEED == kMccKeepSeed &&
                  VR_MASK_FILL_HOLES == kMccFillHoles && sizeof(vr_mask_select_request) == 32 &&
                  sizeof(vr_mask_select_info) == 40 && sizeof(vr_label_component) == kMccRecordBytes &&
                  sizeof(vr_label_info) == 40,
              "vr_maskcc.h");

// The context's blocks of this family grow behind a wait for the device: an earlier call's passes
// may still read the old block on another stream (reserve's idle_first).
constexpr const char *kMccIdle = "hipDeviceSynchronize (maskcc scratch)";

// One call's passes on stream s; c is a single-device context.  The timing events bracket the
// labelling passes as one interval, the record passes as another and the selection as a third (the
// copies of the counts to the host and the host's waits lie between them).
struct MccRun {
    vr_ctx *c;
    hipStream_t s;
    MaskGrid g;
    MccArgs A;
    uint32_t conn = 0;
    Interval timed;

    // Per-pass times for vr_debug_maskcc_pass_ms (timing enabled only): an event after every pass,
    // read by passes_read after the call's wait for the stream.  The interval itself stays one pair
    // in ev_pending, which owns its first event.
    hipEvent_t from = nullptr;
    std::vector<std::pair<int, hipEvent_t>> marks;  // (the pass that ended, the event after it)
    ~MccRun()
    {
        for (auto &m : marks) c->ev_pool.push_back(m.second);
    }
    int start()
    {
        if (int rc = timed.begin(c, s)) return rc;
        from = timed.e0;  // (NULL without timing)
        return VR_OK;
    }
    int pass(MccPass p)
    {
        HIP_TRY(c, launch_mcc(p, A, g, conn, s, &c->maskcc_last_name), "maskcc launch");
        if (!from) return VR_OK;
        hipEvent_t e = pooled_event(c);
        if (!e) return fail(c, VR_EIO, "hipEventCreate failed");
        marks.emplace_back((int)p, e);
        HIP_TRY(c, hipEventRecord(e, s), "hipEventRecord");
        return VR_OK;
    }
    // after timed.end() and a wait for s
    int passes_read()
    {
        hipEvent_t prev = from;
        for (auto &m : marks) {
            if (prev) HIP_TRY(c, hipEventElapsedTime(&c->maskcc_pass_ms[m.first], prev, m.second), "hipEventElapsedTime");
            prev = m.second;
        }
        for (auto &m : marks) c->ev_pool.push_back(m.second);
        marks.clear();
        from = nullptr;
        return VR_OK;
    }
    // The root table and the counters, zeroed; the labels go to labels_dev.
    int begin(const void *mask, uint32_t elem_bytes, uint32_t connectivity, bool invert, void *labels_dev)
    {
        HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
        const MccGeom G = mcc_geometry(g);
        if (int rc = reserve(c, c->maskcc_aux_dev, G.bytes, "hipMalloc(maskcc root table)", kMccIdle)) return rc;
        char *base = static_cast<char *>(c->maskcc_aux_dev.p);
        std::memset(&A, 0, sizeof A);
        A.mask = mask;
        A.P = static_cast<uint32_t *>(labels_dev);
        A.bits = reinterpret_cast<unsigned long long *>(base + G.bits);
        A.wpre = reinterpret_cast<uint32_t *>(base + G.wpre);
        A.chunk = reinterpret_cast<uint32_t *>(base + G.chunk);
        A.cnt = reinterpret_cast<unsigned long long *>(base + G.cnt);
        for (int a = 0; a < 3; ++a) A.ext[a] = g.ext[a];
        A.nvox = (uint32_t)g.voxels;
        A.nwords = G.nwords;
        A.nchunks = G.nchunks;
        A.elem_bytes = elem_bytes;
        A.invert = invert;
        conn = connectivity;
        HIP_TRY(c, hipMemsetAsync(A.cnt, 0, kMccCounters * 8, s), "hipMemset(maskcc counters)");
        for (float &v : c->maskcc_pass_ms) v = 0.0f;
        return VR_OK;
    }
    // The labelling passes, then the counts to the host (waits for s).  *I is written only on
    // VR_OK: voxels, in_voxels and components.
    int label(vr_label_info *I)
    {
        if (int rc = start()) return rc;
        for (MccPass p : {kMccRows, kMccLink, kMccFlatten, kMccScan})
            if (int rc = pass(p)) return rc;
        if (int rc = timed.end()) return rc;
        unsigned long long h[2];
        HIP_TRY(c, hipMemcpyAsync(h, A.cnt, sizeof h, hipMemcpyDeviceToHost, s), "hipMemcpy(maskcc counts)");
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(maskcc counts)");
        if (int rc = passes_read()) return rc;
        std::memset(I, 0, sizeof *I);
        I->voxels = g.voxels;
        I->components = h[kMccCntComps];
        I->in_voxels = h[kMccCntIn];
        return VR_OK;
    }
    // The records of I->components components into the context's block (A.comps, the flags behind
    // them), and the largest component into *I (waits for s).
    int table(vr_label_info *I)
    {
        if (!I->components) return VR_OK;
        const size_t n = (size_t)I->components;
        if (int rc = reserve(c, c->maskcc_tab_dev, n * kMccRecordBytes + n, "hipMalloc(maskcc records)", kMccIdle))
            return rc;
        A.comps = c->maskcc_tab_dev.p;
        A.flags = static_cast<uint8_t *>(c->maskcc_tab_dev.p) + n * kMccRecordBytes;
        A.ncomps = (uint32_t)n;
        if (int rc = start()) return rc;
        for (MccPass p : {kMccTableInit, kMccAccum, kMccLargest})
            if (int rc = pass(p)) return rc;
        if (int rc = timed.end()) return rc;
        unsigned long long key = 0;
        HIP_TRY(c, hipMemcpyAsync(&key, A.cnt + kMccCntLargest, sizeof key, hipMemcpyDeviceToHost, s),
                "hipMemcpy(maskcc largest)");
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(maskcc largest)");
        if (int rc = passes_read()) return rc;
        I->largest_voxels = key >> 32;
        I->largest_label = ~(uint32_t)key;
        return VR_OK;
    }
    // vr_mask_select*: labels in the context's block, records, flags and the sweep into out_dev.
    int select(const vr_mask_select_request *req, const void *mask, uint32_t elem_bytes, void *out_dev,
               vr_mask_select_info *S)
    {
        HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
        if (int rc = reserve(c, c->maskcc_lab_dev, (size_t)g.voxels * 4, "hipMalloc(maskcc labels)", kMccIdle)) return rc;
        const bool fill = req->rule == VR_MASK_FILL_HOLES;
        if (int rc = begin(mask, elem_bytes, req->connectivity, fill, c->maskcc_lab_dev.p)) return rc;
        vr_label_info I;
        if (int rc = label(&I)) return rc;
        if (int rc = table(&I)) return rc;
        A.out = static_cast<uint8_t *>(out_dev);
        A.rule = req->rule;
        A.min_voxels = req->min_voxels;
        A.seed = req->rule == VR_MASK_KEEP_SEED ? mcc_linear(g, req->seed) : 0u;
        if (int rc = start()) return rc;
        if (I.components)
            if (int rc = pass(kMccKeep)) return rc;
        if (int rc = pass(kMccSelect)) return rc;
        if (int rc = timed.end()) return rc;
        unsigned long long h[2];
        HIP_TRY(c, hipMemcpyAsync(h, A.cnt + kMccCntOnes, sizeof h, hipMemcpyDeviceToHost, s), "hipMemcpy(maskcc counts)");
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(maskcc select)");
        if (int rc = passes_read()) return rc;
        static_assert(kMccCntKept == kMccCntOnes + 1, "one copy");
        std::memset(S, 0, sizeof *S);
        S->voxels = g.voxels;
        S->in_set = fill ? g.voxels - I.in_voxels : I.in_voxels;  // (the labelled voxels are the unset ones)
        S->out_set = h[0];
        S->components = I.components;
        S->kept = h[1];
        return VR_OK;
    }
};

constexpr const char *kCcapMsg = "record buffer is smaller than the table (see the info's components)";
}  // namespace

extern "C" {

int vr_mask_label_device(vr_ctx *c, const uint32_t ext[3], const void *mask_dev, uint32_t elem_bytes,
                         uint32_t connectivity, void *labels_dev, uint64_t lcap, void *comps_dev, uint64_t ccap,
                         vr_label_info *info, void *stream)
{
    MccRun R{c, static_cast<hipStream_t>(stream)};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mcc_check_label(ext, mask_dev, elem_bytes, connectivity, labels_dev, lcap, comps_dev, ccap, info,
                                   true, &R.g, msg);
        },
        [&](vr_ctx *m) {
            return vr_mask_label_device(m, ext, mask_dev, elem_bytes, connectivity, labels_dev, lcap, comps_dev, ccap,
                                        info, stream);
        },
        nullptr,
        [&](vr_label_info *I) {
            if (int rc = R.begin(mask_dev, elem_bytes, connectivity, false, labels_dev)) return rc;
            if (int rc = R.label(I)) return rc;
            if (int rc = R.table(I)) return rc;
            if (ccap < I->components) {
                *info = *I;
                return fail(c, VR_ENOSPC, kCcapMsg);
            }
            if (I->components) {
                HIP_TRY(c, hipMemcpyAsync(comps_dev, R.A.comps, (size_t)I->components * kMccRecordBytes,
                                          hipMemcpyDeviceToDevice, R.s), "hipMemcpy(maskcc records)");
                HIP_TRY(c, hipStreamSynchronize(R.s), "hipStreamSynchronize(maskcc records)");
            }
            return VR_OK;
        });
}

int vr_mask_label(vr_ctx *c, const uint32_t ext[3], const void *mask_host, uint32_t elem_bytes, uint32_t connectivity,
                  uint32_t *labels_host, uint64_t lcap, vr_label_component *comps_host, uint64_t ccap,
                  vr_label_info *info)
{
    MccRun R{c, nullptr};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mcc_check_label(ext, mask_host, elem_bytes, connectivity, labels_host, lcap, comps_host, ccap, info,
                                   false, &R.g, msg);
        },
        [&](vr_ctx *m) {
            return vr_mask_label(m, ext, mask_host, elem_bytes, connectivity, labels_host, lcap, comps_host, ccap, info);
        },
        nullptr,
        [&](vr_label_info *I) {
            MaskStage S{c};
            if (int rc = S.begin(c->maskcc_io_dev, "hipMalloc(maskcc staging)", kMccIdle,
                                 {mask_host, (size_t)R.g.voxels * elem_bytes, "hipMemcpy(mask)"}, {},
                                 (size_t)R.g.voxels * 4))
                return rc;
            if (int rc = R.begin(S.in[0], elem_bytes, connectivity, false, S.out)) return rc;
            if (int rc = R.label(I)) return rc;
            if (int rc = R.table(I)) return rc;
            if (int rc = S.finish(labels_host, "hipMemcpy(labels)")) return rc;
            if (ccap < I->components) {
                *info = *I;
                return fail(c, VR_ENOSPC, kCcapMsg);
            }
            if (I->components)
                HIP_TRY(c, hipMemcpy(comps_host, R.A.comps, (size_t)I->components * kMccRecordBytes, hipMemcpyDeviceToHost),
                        "hipMemcpy(maskcc records)");
            return VR_OK;
        });
}

int vr_mask_select_device(vr_ctx *c, const uint32_t ext[3], const vr_mask_select_request *req, const void *mask_dev,
                          uint32_t elem_bytes, void *out_dev, uint64_t mcap, vr_mask_select_info *info, void *stream)
{
    MccRun R{c, static_cast<hipStream_t>(stream)};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mcc_check_select(ext, req != nullptr, req ? req->rule : 0u, req ? req->connectivity : 0u,
                                    req ? req->seed : nullptr, mask_dev, elem_bytes, out_dev, mcap, info, true, &R.g, msg);
        },
        [&](vr_ctx *m) { return vr_mask_select_device(m, ext, req, mask_dev, elem_bytes, out_dev, mcap, info, stream); },
        nullptr, [&](vr_mask_select_info *S) { return R.select(req, mask_dev, elem_bytes, out_dev, S); });
}

int vr_mask_select(vr_ctx *c, const uint32_t ext[3], const vr_mask_select_request *req, const void *mask_host,
                   uint32_t elem_bytes, uint8_t *out_host, uint64_t mcap, vr_mask_select_info *info)
{
    MccRun R{c, nullptr};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mcc_check_select(ext, req != nullptr, req ? req->rule : 0u, req ? req->connectivity : 0u,
                                    req ? req->seed : nullptr, mask_host, elem_bytes, out_host, mcap, info, false, &R.g,
                                    msg);
        },
        [&](vr_ctx *m) { return vr_mask_select(m, ext, req, mask_host, elem_bytes, out_host, mcap, info); }, nullptr,
        [&](vr_mask_select_info *I) {
            MaskStage S{c};
            if (int rc = S.begin(c->maskcc_io_dev, "hipMalloc(maskcc staging)", kMccIdle,
                                 {mask_host, (size_t)R.g.voxels * elem_bytes, "hipMemcpy(mask)"}, {}, (size_t)R.g.voxels))
                return rc;
            if (int rc = R.select(req, S.in[0], elem_bytes, S.out, I)) return rc;
            return S.finish(out_host, "hipMemcpy(selected mask)");
        });
}

// Debug hook beside vr_debug.h's vr_debug_label_pass_ms (declared in no public header; tools/
// maskcc_bench.py takes it by name): kernel ms of each pass of the last call of this family on the
// context, MccPass order, taken while timing was enabled.
int vr_debug_maskcc_pass_ms(const vr_ctx *c, float ms[9])
{
    if (!c || !ms) return VR_EINVAL;
    if (is_group(c)) return vr_debug_maskcc_pass_ms(c->members[0], ms);
    static_assert(kMccPasses == 9, "maskcc_pass_ms");
    for (int i = 0; i < 9; ++i) ms[i] = c->maskcc_pass_ms[i];
    return VR_OK;
}

const char *vr_maskcc_last_kernel_name(const vr_ctx *c) { return mask_last_kernel_name(c, &vr_ctx::maskcc_last_name); }

}  // extern "C"
