// vr_mview_host.h — the host side of include/vr/vr_mview.h: what a request is refused for (the grid
// rule is vr_mask_host.h's; the texts, the source's own fields, the rectangle and the plane are
// here), the cell geometry of the occupancy words, which the kernels share, and
// vr_mview_occupancy_words.  Plain C++ without HIP, so a stand-alone program can run it (under a
// sanitizer, tests/test_mview_cpu.py); vr_api_mview.hip includes it for the entry points,
// vr_mview_kernels.hip for the geometry.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "vr_hit_host.h"  // HitRect
#include "vr_mask_host.h"

#if defined(__HIPCC__)
#define VR_MVIEW_HD __host__ __device__
#else
#define VR_MVIEW_HD
#endif

namespace vr {

constexpr uint32_t kMviewCell = 8;            // VR_MVIEW_CELL: an occupancy cell is 8 x 8 x 8 grid voxels
constexpr uint32_t kMviewCellShift = 3;
constexpr uint32_t kMviewAny = 0, kMviewLabel = 1;  // vr_mview_select
constexpr uint32_t kMviewHitBytes = 32;       // sizeof(vr_mask_hit)
constexpr uint32_t kMviewMiss = 0xFFFFFFFFu;  // a miss record's step and index
constexpr uint32_t kMviewMaxSamples = 4096;   // VR_MPR_MAX_SAMPLES

// vr_mview_source, field for field (vr_api_mview.hip asserts the layout).
struct MviewSource {
    uint32_t ext[3], origin[3];
    uint32_t elem_bytes, select, label, reserved;
    const void *array;
    const void *occupancy;
};

// vr_mpr_plane, field for field.
struct MviewPlane {
    float origin[3], du[3], dv[3], dn[3];
    uint32_t width, height, nsamples;
    int32_t op;
};

// ---- the cells ----
// c[a] = ceil(ext[a] / 8) cells from grid voxel (0, 0, 0); cell (ci, cj, ck) has index
// m = ci + c[0] * (cj + c[1] * ck), bit m & 31 of word m >> 5.  At most 2^32 - 1 voxels in cells of
// 8^3, each cut cell holding at least one voxel row: cells and words fit 32 bits with room.
struct MviewCells {
    uint32_t c[3];
    uint64_t cells, words;
};

VR_MVIEW_HD constexpr uint32_t mview_cells_of(uint32_t n) { return (n + kMviewCell - 1) >> kMviewCellShift; }

VR_MVIEW_HD inline MviewCells mview_cells(const uint32_t ext[3])
{
    MviewCells C;
    for (int a = 0; a < 3; ++a) C.c[a] = mview_cells_of(ext[a]);
    C.cells = (uint64_t)C.c[0] * C.c[1] * C.c[2];
    C.words = (C.cells + 31) >> 5;
    return C;
}

// The cell index of grid voxel (gx, gy, gz) in a grid of c0 x c1 x * cells.
VR_MVIEW_HD constexpr uint32_t mview_cell_index(uint32_t gx, uint32_t gy, uint32_t gz, uint32_t c0, uint32_t c1)
{
    return (gx >> kMviewCellShift) + c0 * ((gy >> kMviewCellShift) + c1 * (gz >> kMviewCellShift));
}

// vr_mview_occupancy_words: pure; 0 for a grid the family refuses (and for NULL).
inline uint64_t mview_occupancy_words(const uint32_t *ext)
{
    MaskGrid g;
    if (!ext || mask_grid_resolve(ext, &g) != kMaskFine) return 0;
    return mview_cells(ext).words;
}

// ---- the texts ----
// The family's texts for the shared rule (vr_mask_host.h MaskReason; the outputs' are below).
constexpr const char *kMviewTexts[kMaskAlign + 1] = {
    nullptr, "mask view: grid extent must lie in [1, 32768]", "mask view: grid holds more than 2^32 - 1 voxels",
    "mask view: elem_bytes must be 1 or 4", "mask view: a 4-byte array must be 4-byte aligned"};
constexpr const char *kMviewNull = "mask view: NULL argument";
constexpr const char *kMviewSelect = "mask view: select must be VR_MVIEW_ANY or VR_MVIEW_LABEL";
constexpr const char *kMviewLabelZero = "mask view: VR_MVIEW_LABEL needs a non-zero label";
constexpr const char *kMviewReserved = "mask view: reserved must be 0";
constexpr const char *kMviewHostOcc = "mask view: a host form takes no occupancy";
constexpr const char *kMviewOccAlign = "mask view: the occupancy words must be 4-byte aligned";
constexpr const char *kMviewOutAlign = "mask view: the output must be 4-byte aligned";
constexpr const char *kMviewOverArray = "mask view: the output overlaps the array";
constexpr const char *kMviewOverOcc = "mask view: the output overlaps the occupancy words";
constexpr const char *kMviewOverInfo = "mask view: the output overlaps the info";
constexpr const char *kMviewRect = "mask view: the rectangle is empty or beyond the framebuffer";
constexpr const char *kMviewRectLarge = "mask view: the rectangle is too large";
constexpr const char *kMviewPick = "mask view: the pick pixel is beyond the framebuffer";
constexpr const char *kMviewOrigin = "mask view: origin + ext lies beyond the volume";
constexpr const char *kMviewPlaneFinite = "mask view: the plane's vectors must be finite";
constexpr const char *kMviewPlaneSize = "mask view: the plane's image size must be non-zero";
constexpr const char *kMviewPlaneLarge = "mask view: the plane's image is too large";
constexpr const char *kMviewPlaneSamples = "mask view: the plane's nsamples must be in [1, 4096]";
constexpr const char *kMviewPlaneOp = "mask view: unknown mpr op";
constexpr const char *kMviewShortRecords = "mask view: the record buffer is smaller than the rectangle (see the info's voxels)";
constexpr const char *kMviewShortPixels = "mask view: the pixel buffer is smaller than the plane's image (see the info's voxels)";
constexpr const char *kMviewShortWords = "mask view: the word buffer is smaller than vr_mview_occupancy_words";

// ---- the source ----
// What every call shares.  device: the array lives in device memory (its alignment binds);
// host_form: the call stages host arrays and takes no occupancy.  kMaskOk with *r resolved, or
// kMaskEinval.
inline int mview_check_source(const MviewSource *s, bool device, bool host_form, MaskGrid *r, const char **msg)
{
    if (!s || !s->array) return mask_refuse(msg, kMviewNull, kMaskEinval);
    if (MaskReason why = mask_grid_resolve(s->ext, r)) return mask_refuse(msg, kMviewTexts[why], kMaskEinval);
    for (int a = 0; a < 3; ++a) r->origin[a] = s->origin[a];
    if (MaskReason why = mask_check_array(s->array, s->elem_bytes, device))
        return mask_refuse(msg, kMviewTexts[why], kMaskEinval);
    if (s->select != kMviewAny && s->select != kMviewLabel) return mask_refuse(msg, kMviewSelect, kMaskEinval);
    if (s->select == kMviewLabel && s->label == 0) return mask_refuse(msg, kMviewLabelZero, kMaskEinval);
    if (s->reserved != 0) return mask_refuse(msg, kMviewReserved, kMaskEinval);
    if (host_form && s->occupancy) return mask_refuse(msg, kMviewHostOcc, kMaskEinval);
    if (!host_form && s->occupancy && !mask_aligned4(s->occupancy)) return mask_refuse(msg, kMviewOccAlign, kMaskEinval);
    return kMaskOk;
}

// The grid against the volume (after the context lookup): origin[a] + ext[a] <= dims[a].
inline const char *mview_origin_error(const MaskGrid &g, const uint32_t dims[3])
{
    for (int a = 0; a < 3; ++a)
        if ((uint64_t)g.origin[a] + g.ext[a] > (uint64_t)dims[a]) return kMviewOrigin;
    return nullptr;
}

// An output of `cap` elements of out_elem bytes, where a full call writes `full`, against the
// source's array and (use_occ) its occupancy words and, for a host form, against the info struct
// of info_bytes.  The overlap texts, or kMaskShort / kMaskFine in *o.
inline const char *mview_output_error(const MviewSource *s, const MaskGrid &r, bool use_occ, const void *out,
                                      uint32_t out_elem, uint64_t cap, uint64_t full, const void *info,
                                      uint64_t info_bytes, bool host_form, MaskReason *o)
{
    *o = mask_check_output(s->array, r.voxels * s->elem_bytes, out, out_elem, cap, full);
    if (*o == kMaskOverlap) return kMviewOverArray;
    if (use_occ && s->occupancy &&
        mask_check_output(s->occupancy, mview_cells(r.ext).words * 4, out, out_elem, cap, full) == kMaskOverlap)
        return kMviewOverOcc;
    if (host_form && mask_check_output(info, info_bytes, out, out_elem, cap, full) == kMaskOverlap) return kMviewOverInfo;
    return nullptr;
}

// vr_mask_occupancy_device: kMaskOk, kMaskEinval (*g untouched) or kMaskEnospc for ocap_words below
// the grid's words with *g resolved.  The source's own occupancy field is not read.
inline int mview_check_occupancy(const MviewSource *s, const void *occ, uint64_t ocap_words, const void *info,
                                 MaskGrid *g, const char **msg)
{
    *msg = nullptr;
    if (!s || !occ || !info) return mask_refuse(msg, kMviewNull, kMaskEinval);
    MaskGrid r;
    MviewSource t = *s;
    t.occupancy = nullptr;
    if (int rc = mview_check_source(&t, true, false, &r, msg)) return rc;
    if (!mask_aligned4(occ)) return mask_refuse(msg, kMviewOutAlign, kMaskEinval);
    MaskReason o;
    if (const char *m = mview_output_error(&t, r, false, occ, 4, ocap_words, mview_cells(r.ext).words, info, 0, false, &o))
        return mask_refuse(msg, m, kMaskEinval);
    return mask_resolved(r, o, kMviewShortWords, g, msg);
}

// The rectangle of a request on a W x H framebuffer (rect NULL: all of it) into *q; nullptr or the text.
inline const char *mview_rect_resolve(const uint32_t *rect, uint32_t W, uint32_t H, HitRect *q)
{
    HitRect t;
    if (hit_rect_resolve(rect ? 1u : 0u, rect, W, H, &t)) return kMviewRect;
    if (((t.w + 15ull) / 16) * ((t.h + 15ull) / 16) >= 1ull << 31) return kMviewRectLarge;
    *q = t;
    return nullptr;
}

// vr_mask_hit_render*: the same for rcap records of the rectangle on the W x H framebuffer.
inline int mview_check_hit(const MviewSource *s, const void *cam, const void *params, const uint32_t *rect, uint32_t W,
                           uint32_t H, const void *out, uint64_t rcap, const void *info, uint64_t info_bytes,
                           bool device, MaskGrid *g, HitRect *q, const char **msg)
{
    *msg = nullptr;
    if (!s || !cam || !params || !out || !info) return mask_refuse(msg, kMviewNull, kMaskEinval);
    MaskGrid r;
    if (int rc = mview_check_source(s, device, !device, &r, msg)) return rc;
    HitRect t;
    if (const char *m = mview_rect_resolve(rect, W, H, &t)) return mask_refuse(msg, m, kMaskEinval);
    if (device && !mask_aligned4(out)) return mask_refuse(msg, kMviewOutAlign, kMaskEinval);
    MaskReason o;
    if (const char *m = mview_output_error(s, r, device, out, kMviewHitBytes, rcap, (uint64_t)t.w * t.h, info, info_bytes,
                                           !device, &o))
        return mask_refuse(msg, m, kMaskEinval);
    *q = t;
    return mask_resolved(r, o, kMviewShortRecords, g, msg);
}

// vr_mask_pick: a device array, one host record; the occupancy field is not read.
inline int mview_check_pick(const MviewSource *s, const void *cam, const void *params, uint32_t px, uint32_t py,
                            uint32_t W, uint32_t H, const void *out, MaskGrid *g, HitRect *q, const char **msg)
{
    *msg = nullptr;
    if (!s || !cam || !params || !out) return mask_refuse(msg, kMviewNull, kMaskEinval);
    MaskGrid r;
    MviewSource t = *s;
    t.occupancy = nullptr;
    if (int rc = mview_check_source(&t, true, false, &r, msg)) return rc;
    if (hit_pick_resolve(px, py, W, H, q)) return mask_refuse(msg, kMviewPick, kMaskEinval);
    *g = r;
    return kMaskOk;
}

// What vr_mpr.h refuses of a plane; nullptr or the text.
inline const char *mview_plane_error(const MviewPlane *pl)
{
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(pl->origin[a]) || !std::isfinite(pl->du[a]) || !std::isfinite(pl->dv[a]) ||
            !std::isfinite(pl->dn[a]))
            return kMviewPlaneFinite;
    if (pl->width == 0 || pl->height == 0) return kMviewPlaneSize;
    if (((pl->width + 15ull) / 16) * ((pl->height + 15ull) / 16) >= 1ull << 31) return kMviewPlaneLarge;
    if (pl->nsamples == 0 || pl->nsamples > kMviewMaxSamples) return kMviewPlaneSamples;
    if (pl->op < 0 || pl->op > 2) return kMviewPlaneOp;
    return nullptr;
}

// vr_mask_slice*: the same for pcap pixels of the plane's image.
inline int mview_check_slice(const MviewSource *s, const MviewPlane *pl, const void *out, uint64_t pcap, const void *info,
                             uint64_t info_bytes, bool device, MaskGrid *g, const char **msg)
{
    *msg = nullptr;
    if (!s || !pl || !out || !info) return mask_refuse(msg, kMviewNull, kMaskEinval);
    MaskGrid r;
    if (int rc = mview_check_source(s, device, !device, &r, msg)) return rc;
    if (const char *m = mview_plane_error(pl)) return mask_refuse(msg, m, kMaskEinval);
    if (device && !mask_aligned4(out)) return mask_refuse(msg, kMviewOutAlign, kMaskEinval);
    MaskReason o;
    if (const char *m = mview_output_error(s, r, device, out, 4, pcap, (uint64_t)pl->width * pl->height, info, info_bytes,
                                           !device, &o))
        return mask_refuse(msg, m, kMaskEinval);
    return mask_resolved(r, o, kMviewShortPixels, g, msg);
}

}  // namespace vr
