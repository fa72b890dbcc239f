// vr_api_hist.hip — the value histogram and the value window (include/vr/vr_hist.h) on the host
// scaffold of vr_ctx.h.
#include "vr_ctx.h"
#include "vr_hist_host.h"

extern "C" {

int vr_hist_edges(float lo, float hi, uint32_t nbins, float *edges_out)
{
    if (!edges_out) return fail(nullptr, VR_EINVAL, "edges is NULL");
    if (!hist_range_ok(lo, hi, nbins))
        return fail(nullptr, VR_EINVAL, "histogram needs finite lo < hi and 1 <= nbins <= 4096");
    hist_edges(lo, hi, nbins, edges_out);
    return VR_OK;
}

int vr_hist_window(const uint64_t *bins, uint32_t nbins, float lo, float hi, double p_lo,
                   double p_hi, float *vmin_out, float *vmax_out)
{
    if (!hist_window(bins, nbins, lo, hi, p_lo, p_hi, vmin_out, vmax_out))
        return fail(nullptr, VR_EINVAL,
                    "histogram window needs bins with a count, finite lo < hi, 1 <= nbins <= 4096 "
                    "and 0 <= p_lo < p_hi <= 1");
    return VR_OK;
}

int vr_histogram(vr_ctx *c, const vr_hist_request *req, uint64_t *bins_host, vr_hist_info *info)
{
    if (!c || !req || !bins_host || !info) return fail(c, VR_EINVAL, "NULL argument");
    if (!hist_range_ok(req->lo, req->hi, req->nbins))
        return fail(c, VR_EINVAL, "histogram needs finite lo < hi and 1 <= nbins <= 4096");
    if (req->use_box > 1) return fail(c, VR_EINVAL, "histogram use_box must be 0 or 1");
    if (is_group(c)) return on_replica(c, [&](vr_ctx *m) { return vr_histogram(m, req, bins_host, info); });
    if (!c->bricks) return fail(c, VR_EINVAL, "no volume");
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    VoxelBox box;
    if (box_resolve(req->use_box, req->box_min, req->box_max, dims, &box))
        return fail(c, VR_EINVAL, "histogram box is empty or beyond the volume");
    HistArgs A;
    std::memset(&A, 0, sizeof A);
    const uint32_t cells[3] = {(uint32_t)brick_cells(c->layout, 0), (uint32_t)brick_cells(c->layout, 1),
                               (uint32_t)brick_cells(c->layout, 2)};
    A.nwork = (uint32_t)box_brick_range(box, cells, (uint32_t)kPad, A.b0, A.nb);
    for (int a = 0; a < 3; ++a) {
        A.box_min[a] = box.lo[a];
        A.box_max[a] = box.hi[a];
    }
    HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
    const size_t out_bytes = kHistOutWords * sizeof(unsigned long long);
    // (a fixed size: reserved once)
    if (int rc = reserve(c, c->hist_dev, out_bytes + kHistMaxBins * sizeof(float), "hipMalloc(histogram)", nullptr))
        return rc;
    float edges[kHistMaxBins];
    hist_edges(req->lo, req->hi, req->nbins, edges);
    A.vol = c->bricks;
    A.out = static_cast<unsigned long long *>(c->hist_dev.p);
    A.edges = reinterpret_cast<const float *>(static_cast<char *>(c->hist_dev.p) + out_bytes);
    A.scale = hist_scale(req->lo, req->hi, req->nbins);
    A.lo = req->lo;
    A.hi = req->hi;
    A.nbins = req->nbins;
    A.nbx = bricks_for(c->nx, 0, c->layout);
    A.nby = bricks_for(c->ny, 1, c->layout);
    HIP_TRY(c, hipMemcpy(const_cast<float *>(A.edges), edges, req->nbins * sizeof(float),
                         hipMemcpyHostToDevice), "hipMemcpy(histogram edges)");
    HIP_TRY(c, hipMemsetAsync(A.out, 0, out_bytes, nullptr), "hipMemset(histogram)");
    Interval timed;
    if (int rc = timed.begin(c, nullptr)) return rc;
    std::string name;
    // The kernel form (knob VR_KNOB_HIST_AGG overrides).  Plain 8-bit bricks count raw codes, and
    // there a constant volume -- every lane on one LDS word -- takes 4.0x the Gaussians' time unless
    // the wave's leading code is added once (C4: 3.53 -> 1.07 ms, the Gaussians 0.87 -> 1.14 ms);
    // the other layouts bin every voxel first, the constant volume costs them 16 % and the
    // aggregation 10 % on the Gaussians (C3: 0.51 / 0.59 ms against 0.56 / 0.55 ms), so they add
    // singly (profiles/r15/hist/).
    const bool agg = c->knobs.hist_agg >= 0 ? c->knobs.hist_agg == 1 : byte_storage(c->layout);
    HIP_TRY(c, launch_hist(c->layout, agg, A, nullptr, &name), "histogram kernel launch");
    c->last_mpr_name = name;
    if (int rc = timed.end()) return rc;
    std::vector<unsigned long long> h((size_t)req->nbins + 4);
    HIP_TRY(c, hipMemcpy(h.data(), A.out, ((size_t)req->nbins + 4) * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost), "hipMemcpy(histogram)");
    vr_hist_info I;
    std::memset(&I, 0, sizeof I);
    I.below = h[req->nbins + 0];
    I.above = h[req->nbins + 1];
    I.nan = h[req->nbins + 2];
    I.voxels = I.below + I.above + I.nan;
    for (uint32_t b = 0; b < req->nbins; ++b) {
        bins_host[b] = h[b];
        I.voxels += h[b];
    }
    uint32_t ext[2];
    std::memcpy(ext, &h[req->nbins + 3], sizeof ext);
    const bool any = I.voxels > I.nan;
    I.vmin = any ? unorder(~ext[0]) : INFINITY;
    I.vmax = any ? unorder(ext[1]) : -INFINITY;
    *info = I;
    return VR_OK;
}

int vr_set_value_range(vr_ctx *c, float vmin, float vmax)
{
    if (!c) return fail(nullptr, VR_EINVAL, "ctx is NULL");
    if (is_group(c)) return on_members(c, [&](vr_ctx *m) { return vr_set_value_range(m, vmin, vmax); });
    // a frame in flight may read the distance field the next skip_empty frame rebuilds
    if (int rc = wait_idle(c)) return rc;
    c->vmin = vmin;
    c->vmax = vmax;
    c->dist_valid = false;  // built from vmin and range; the brick ranges and the fields stay
    return VR_OK;
}

}  // extern "C"
