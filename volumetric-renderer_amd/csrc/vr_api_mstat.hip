// vr_api_mstat.hip — the statistics of the volume under a mask or a label array and the
// value-window pass (include/vr/vr_mstat.h) on the host scaffold of vr_ctx.h and vr_mask_call.h.  Built into
// lib/libvr_amd_mstat.so, which takes the scaffold (fail, hip_fail, reserve, pooled_event, the
// group's wait) from libvr_amd.so.
#include "vr_mask_call.h"
#include "../../include/vr/vr_mstat.h"
#include "vr_mstat_kernels.h"

namespace {
static_assert(VR_MSTAT_MAX_EXTENT == kMaskMaxExtent && VR_MSTAT_NONE == kMstatNone &&
                  sizeof(vr_mstat_region) == kMstatRecordBytes &&
                  sizeof(vr_label_component) == kMstatRecordBytes && sizeof(vr_mstat_info) == 32 &&
                  sizeof(vr_morph_info) == 24 && VR_HIST_MAX_BINS == kHistMaxBins,
              "vr_mstat.h");

// The context's blocks of this family grow behind a wait for the device (reserve's idle_first).
constexpr const char *kMstatIdle = "hipDeviceSynchronize (mstat scratch)";

// One call's passes on stream s; c is a single-device context.  The timing events bracket them as
// one interval.
struct MstatRun {
    vr_ctx *c;
    hipStream_t s;
    MaskGrid g;
    MstatArgs A;
    MstatGeom G;
    Interval timed;

    // What needs the context: a volume, and the grid inside it.  Before any output or scratch.
    int admit()
    {
        if (!c->bricks) return fail(c, VR_EINVAL, "no volume");
        const uint32_t dims[3] = {c->nx, c->ny, c->nz};
        if (const char *m = mstat_origin_error(g, dims)) return fail(c, VR_EINVAL, m);
        return VR_OK;
    }
    // The scratch of nrec records, the arguments every pass shares, the counters (with nbins bins
    // behind them) and the accumulators zeroed.  The interval begins before the two memsets: they are
    // work the call needs (48 bytes a record).
    int begin(uint64_t nrec, const void *array, uint32_t elem_bytes, uint32_t nbins)
    {
        HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
        G = mstat_geometry(g, nrec);
        if (int rc = reserve(c, c->mstat_aux_dev, G.bytes, "hipMalloc(mstat scratch)", kMstatIdle)) return rc;
        char *base = static_cast<char *>(c->mstat_aux_dev.p);
        std::memset(&A, 0, sizeof A);
        A.vol = c->bricks;
        A.array = array;
        A.cnt = reinterpret_cast<unsigned long long *>(base + G.cnt);
        A.bins = reinterpret_cast<unsigned long long *>(base + G.bins);
        A.edges = reinterpret_cast<const float *>(base + G.edges);
        A.acc = nrec ? reinterpret_cast<MstatAcc *>(base + G.acc) : nullptr;
        A.rec = nrec ? base + G.rec : nullptr;
        for (int a = 0; a < 3; ++a) {
            A.ext[a] = g.ext[a];
            A.origin[a] = g.origin[a];
        }
        A.nbx = bricks_for(c->nx, 0, c->layout);
        A.nby = bricks_for(c->ny, 1, c->layout);
        A.elem_bytes = elem_bytes;
        A.nrec = (uint32_t)nrec;
        A.nbins = nbins;
        static_assert(kMstatCounters * 8 == 64, "the bins follow the counters: one memset");
        if (int rc = timed.begin(c, s)) return rc;
        HIP_TRY(c, hipMemsetAsync(A.cnt, 0, kMstatCounters * 8 + (size_t)nbins * 8, s), "hipMemset(mstat counters)");
        if (nrec) HIP_TRY(c, hipMemsetAsync(A.acc, 0, (size_t)nrec * kMstatAccBytes, s), "hipMemset(mstat accumulators)");
        return VR_OK;
    }
    int pass(MstatPass p)
    {
        HIP_TRY(c, launch_mstat(p, c->layout, A, g, s, &c->mstat_last_name), "mstat launch");
        return VR_OK;
    }
    // n counters from cnt[first] to the host (waits for s)
    int counters(int first, int n, unsigned long long *h)
    {
        HIP_TRY(c, hipMemcpyAsync(h, A.cnt + first, (size_t)n * 8, hipMemcpyDeviceToHost, s), "hipMemcpy(mstat counters)");
        HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(mstat)");
        return VR_OK;
    }

    // vr_mask_stats*: mask in device memory.  The outputs are written on VR_OK only.
    int stats(const void *mask, uint32_t elem_bytes, const vr_hist_request *hist, uint64_t *bins_host,
              vr_hist_info *hinfo, vr_mstat_region *region_out)
    {
        const uint32_t nbins = hist ? hist->nbins : 0u;
        if (int rc = begin(1, mask, elem_bytes, nbins)) return rc;
        if (hist) {
            float edges[kHistMaxBins];
            hist_edges(hist->lo, hist->hi, nbins, edges);
            HIP_TRY(c, hipMemcpyAsync(const_cast<float *>(A.edges), edges, nbins * sizeof(float), hipMemcpyHostToDevice, s),
                    "hipMemcpy(histogram edges)");
            HIP_TRY(c, hipStreamSynchronize(s), "hipStreamSynchronize(histogram edges)");  // (edges leaves scope)
            A.scale = hist_scale(hist->lo, hist->hi, nbins);
            A.lo = hist->lo;
            A.hi = hist->hi;
        }
        for (MstatPass p : {kMstatMask, kMstatFinalize})
            if (int rc = pass(p)) return rc;
        if (int rc = timed.end()) return rc;
        vr_mstat_region R;
        HIP_TRY(c, hipMemcpyAsync(&R, A.rec, sizeof R, hipMemcpyDeviceToHost, s), "hipMemcpy(mstat region)");
        std::vector<unsigned long long> h(nbins);
        if (nbins)
            HIP_TRY(c, hipMemcpyAsync(h.data(), A.bins, (size_t)nbins * 8, hipMemcpyDeviceToHost, s), "hipMemcpy(mstat bins)");
        unsigned long long side[2];
        static_assert(kMstatCntAbove == kMstatCntBelow + 1, "one copy");
        if (int rc = counters(kMstatCntBelow, 2, side)) return rc;
        if (hist) {
            vr_hist_info I;
            std::memset(&I, 0, sizeof I);
            I.voxels = R.voxels;
            I.below = side[0];
            I.above = side[1];
            I.nan = R.nan;
            I.vmin = R.vmin;
            I.vmax = R.vmax;
            for (uint32_t b = 0; b < nbins; ++b) bins_host[b] = h[b];
            *hinfo = I;
        }
        *region_out = R;
        return VR_OK;
    }
    // vr_label_stats*: labels and table in device memory; the records are left in A.rec and, where
    // regions_dev is not NULL, copied to it (device memory, any alignment) inside the interval.
    int labels(const void *labels_dev, const void *table_dev, uint64_t ntable, void *regions_dev, vr_mstat_info *I)
    {
        if (int rc = begin(ntable, labels_dev, 4, 0)) return rc;
        if (ntable) {
            A.table = table_dev;
            A.labels = reinterpret_cast<uint32_t *>(static_cast<char *>(c->mstat_aux_dev.p) + G.lab);
            if (int rc = pass(kMstatGather)) return rc;
        }
        if (int rc = pass(kMstatLabels)) return rc;
        if (ntable)
            if (int rc = pass(kMstatFinalize)) return rc;
        if (ntable && regions_dev)
            HIP_TRY(c, hipMemcpyAsync(regions_dev, A.rec, (size_t)ntable * kMstatRecordBytes, hipMemcpyDeviceToDevice, s),
                    "hipMemcpy(mstat regions)");
        if (int rc = timed.end()) return rc;
        unsigned long long h[2];
        static_assert(kMstatCntSet == 0 && kMstatCntUnlisted == 1, "one copy");
        if (int rc = counters(kMstatCntSet, 2, h)) return rc;
        std::memset(I, 0, sizeof *I);
        I->voxels = g.voxels;
        I->set = h[0];
        I->unlisted = h[1];
        I->regions = ntable;
        return VR_OK;
    }
    // vr_mask_window*: mask (or NULL) and out in device memory.
    int window(const void *mask, uint32_t elem_bytes, float lo, float hi, void *out, vr_morph_info *I)
    {
        if (int rc = begin(0, mask, elem_bytes, 0)) return rc;
        A.lo = lo;
        A.hi = hi;
        A.out = static_cast<uint8_t *>(out);
        if (int rc = pass(kMstatWindow)) return rc;
        if (int rc = timed.end()) return rc;
        unsigned long long h[kMstatCntOut + 1];
        if (int rc = counters(0, kMstatCntOut + 1, h)) return rc;
        std::memset(I, 0, sizeof *I);
        I->voxels = g.voxels;
        I->in_set = h[kMstatCntSet];
        I->out_set = h[kMstatCntOut];
        return VR_OK;
    }
};

}  // namespace

extern "C" {

// vr_mask_stats*: no info struct and no VR_ENOSPC, so written out on the pieces mask_call is made of.
int vr_mask_stats_device(vr_ctx *c, const uint32_t ext[3], const uint32_t origin[3], const void *mask_dev,
                         uint32_t elem_bytes, const vr_hist_request *hist, uint64_t *bins_host, vr_hist_info *hinfo,
                         vr_mstat_region *region_out, void *stream)
{
    if (!c) return null_ctx();
    MstatRun R{c, static_cast<hipStream_t>(stream)};
    const char *msg;
    if (int rc = mstat_check_stats(ext, origin, mask_dev, elem_bytes, hist != nullptr, hist ? hist->use_box : 0u,
                                   hist ? hist->lo : 0.0f, hist ? hist->hi : 0.0f, hist ? hist->nbins : 0u, bins_host,
                                   hinfo, region_out, true, &R.g, &msg))
        return fail(c, rc, msg);
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) {
            return vr_mask_stats_device(m, ext, origin, mask_dev, elem_bytes, hist, bins_host, hinfo, region_out, stream);
        });
    if (int rc = R.admit()) return rc;
    return R.stats(mask_dev, elem_bytes, hist, bins_host, hinfo, region_out);
}

int vr_mask_stats(vr_ctx *c, const uint32_t ext[3], const uint32_t origin[3], const void *mask_host,
                  uint32_t elem_bytes, const vr_hist_request *hist, uint64_t *bins_host, vr_hist_info *hinfo,
                  vr_mstat_region *region_out)
{
    if (!c) return null_ctx();
    MstatRun R{c, nullptr};
    const char *msg;
    if (int rc = mstat_check_stats(ext, origin, mask_host, elem_bytes, hist != nullptr, hist ? hist->use_box : 0u,
                                   hist ? hist->lo : 0.0f, hist ? hist->hi : 0.0f, hist ? hist->nbins : 0u, bins_host,
                                   hinfo, region_out, false, &R.g, &msg))
        return fail(c, rc, msg);
    if (is_group(c))
        return on_replica(c, [&](vr_ctx *m) {
            return vr_mask_stats(m, ext, origin, mask_host, elem_bytes, hist, bins_host, hinfo, region_out);
        });
    if (int rc = R.admit()) return rc;
    MaskStage S{c};
    if (int rc = S.begin(c->mstat_io_dev, "hipMalloc(mstat staging)", kMstatIdle,
                         {mask_host, (size_t)R.g.voxels * elem_bytes, "hipMemcpy(mask)"}, {}, 0))
        return rc;
    return R.stats(S.in[0], elem_bytes, hist, bins_host, hinfo, region_out);
}

int vr_label_stats_device(vr_ctx *c, const uint32_t ext[3], const uint32_t origin[3], const void *labels_dev,
                          const void *table_dev, uint64_t ntable, void *regions_dev, uint64_t rcap,
                          vr_mstat_info *info, void *stream)
{
    MstatRun R{c, static_cast<hipStream_t>(stream)};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mstat_check_labels(ext, origin, labels_dev, table_dev, ntable, regions_dev, rcap, info, true, &R.g, msg);
        },
        [&](vr_ctx *m) {
            return vr_label_stats_device(m, ext, origin, labels_dev, table_dev, ntable, regions_dev, rcap, info, stream);
        },
        [&] { return R.admit(); },
        [&](vr_mstat_info *I) {
            return R.labels(labels_dev, table_dev, ntable, regions_dev, I);
        });  // (waits for the stream)
}

int vr_label_stats(vr_ctx *c, const uint32_t ext[3], const uint32_t origin[3], const uint32_t *labels_host,
                   const vr_label_component *table_host, uint64_t ntable, vr_mstat_region *regions_host,
                   uint64_t rcap, vr_mstat_info *info)
{
    MstatRun R{c, nullptr};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mstat_check_labels(ext, origin, labels_host, table_host, ntable, regions_host, rcap, info, false,
                                      &R.g, msg);
        },
        [&](vr_ctx *m) { return vr_label_stats(m, ext, origin, labels_host, table_host, ntable, regions_host, rcap, info); },
        [&] { return R.admit(); },
        [&](vr_mstat_info *I) {
            const size_t tab_bytes = (size_t)ntable * kMstatRecordBytes;
            MaskStage S{c};
            if (int rc = S.begin(c->mstat_io_dev, "hipMalloc(mstat staging)", kMstatIdle,
                                 {labels_host, (size_t)R.g.voxels * 4, "hipMemcpy(labels)"},
                                 {table_host, tab_bytes, "hipMemcpy(table)"}, 0))
                return rc;
            if (int rc = R.labels(S.in[0], S.in[1], ntable, nullptr, I)) return rc;
            if (ntable)
                HIP_TRY(c, hipMemcpy(regions_host, R.A.rec, tab_bytes, hipMemcpyDeviceToHost), "hipMemcpy(mstat regions)");
            return VR_OK;
        });
}

int vr_mask_window_device(vr_ctx *c, const uint32_t ext[3], const uint32_t origin[3], const void *mask_dev,
                          uint32_t elem_bytes, float lo, float hi, void *out_dev, uint64_t mcap, vr_morph_info *info,
                          void *stream)
{
    MstatRun R{c, static_cast<hipStream_t>(stream)};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mstat_check_window(ext, origin, mask_dev, elem_bytes, lo, hi, out_dev, mcap, info, true, &R.g, msg);
        },
        [&](vr_ctx *m) {
            return vr_mask_window_device(m, ext, origin, mask_dev, elem_bytes, lo, hi, out_dev, mcap, info, stream);
        },
        [&] { return R.admit(); },
        [&](vr_morph_info *I) { return R.window(mask_dev, elem_bytes, lo, hi, out_dev, I); });
}

int vr_mask_window(vr_ctx *c, const uint32_t ext[3], const uint32_t origin[3], const void *mask_host,
                   uint32_t elem_bytes, float lo, float hi, uint8_t *out_host, uint64_t mcap, vr_morph_info *info)
{
    MstatRun R{c, nullptr};
    return mask_call(
        c, R.g, info,
        [&](const char **msg) {
            return mstat_check_window(ext, origin, mask_host, elem_bytes, lo, hi, out_host, mcap, info, false, &R.g, msg);
        },
        [&](vr_ctx *m) { return vr_mask_window(m, ext, origin, mask_host, elem_bytes, lo, hi, out_host, mcap, info); },
        [&] { return R.admit(); },
        [&](vr_morph_info *I) {
            MaskStage S{c};  // (no mask: S.in[0] stays NULL)
            if (int rc = S.begin(c->mstat_io_dev, "hipMalloc(mstat staging)", kMstatIdle,
                                 {mask_host, (size_t)R.g.voxels * elem_bytes, "hipMemcpy(mask)"}, {}, (size_t)R.g.voxels))
                return rc;
            if (int rc = R.window(S.in[0], elem_bytes, lo, hi, S.out, I)) return rc;
            return S.finish(out_host, "hipMemcpy(window mask)");
        });
}

const char *vr_mstat_last_kernel_name(const vr_ctx *c) { return mask_last_kernel_name(c, &vr_ctx::mstat_last_name); }

}  // extern "C"
