/*
 * vr_mview.h — show a device mask or label array: per-pixel first-hit records along the ray every
 * frame walks, the array's elements on an MPR plane, a one-pixel pick, and a coarse occupancy
 * bitmap that lets the march pass over empty space (an addition beside vr.h and the other family
 * headers; VR_ABI_VERSION, vr_params and vr_stats are unchanged).  The entry points live in
 * lib/libvr_amd_mview.so, a fifth library beside libvr_amd.so, libvr_amd_morph.so,
 * libvr_amd_maskcc.so and libvr_amd_mstat.so on the same context: link it with libvr_amd.so
 * (INTEGRATION.md).
 *
 * vr_label.h grows a region from a click, vr_morph.h and vr_maskcc.h clean it up, vr_mstat.h
 * measures it; every one of those calls ends in a mask or a label array in device memory.  These
 * calls show that array without a read-back: the surface of a lesion in the 3D view (the host
 * shades it from `normal` and composites it over a frame with `depth`, which is vr_hit.h's), its
 * outline on the MPR image beside it (the label image of the same plane), and the label of the
 * piece under a click.
 *
 * Source.  A vr_mview_source names the array.  ext, origin, elem_bytes and array are vr_mstat.h's
 * grid: ext[3] = (bx, by, bz) voxels, every extent in [1, 32768], at most 2^32 - 1 voxels,
 * box-linear order l = i + bx * (j + by * k); origin[3] is the VOLUME voxel of grid voxel
 * (0, 0, 0), origin[a] + ext[a] <= dims[a]; elem_bytes is 1 or 4, and a 4-byte array in device
 * memory must be 4-byte aligned (a byte mask may have any address).  An element MATCHES iff it is
 * non-zero (select = VR_MVIEW_ANY; label is ignored) or iff it equals `label`
 * (select = VR_MVIEW_LABEL; label non-zero).  reserved is 0.  occupancy is NULL, or the words
 * vr_mask_occupancy_device wrote for this array, grid, select and label (device forms only; the
 * host forms take NULL, vr_mask_pick and vr_mask_occupancy_device do not read the field).
 *
 * Voxel of a position.  For a texture coordinate p[a] (f32, inside [0, 1] by the walk's bounds
 * test) and the volume's dims[a]: t = p[a] * (float)dims[a], one f32 multiply; v[a] = (int)t,
 * truncated; if v[a] > dims[a] - 1 then v[a] = dims[a] - 1.  Voxel i covers [i/n, (i+1)/n), and
 * the sampler's centre (i + 0.5)/n lies in its middle.  element_at(v) is the array's element at
 * grid voxel v - origin, and 0 for a voxel outside the grid; outside the volume counts as outside
 * the grid.
 *
 * The hit walk.  vr_hit.h's walk, verbatim: the composite's pixel ray and entry point for pixel
 * (x0 + i, y0 + j) of the context's W x H framebuffer, nsteps = int(ray_dist / step), the position
 * update pos = pos + dir * step in f32, the bounds break and the strict slab test against the
 * context's slice box.  At each in-slab sample, in step order, e = element_at(voxel_of(pos)); the
 * first sample whose e matches is the hit, and the record holds that sample's pos, depth (vr_hit.h's
 * formula, verbatim), e, the loop index k and the voxel's box-linear grid index.  Nothing is
 * refined.  An uncovered pixel, or a ray with no matching sample, gets the miss record
 * {0,0,0, +INFINITY, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0,0,0, 0}.  The walk SAMPLES: a structure thinner
 * than `step` can be stepped over.  A caller who needs every voxel on the ray visited passes
 * step <= 1 / max(dims).  The output holds w * h records of 32 bytes, row-major, row 0 the top row
 * of the rectangle (rect = {x0, y0, w, h}; NULL: the whole framebuffer).
 *
 * Normal.  normal[a] = - sum of o[a] * match(element_at(v + o)) over the 26 offsets o in
 * {-1,0,1}^3 \ {0} of the hit voxel v: an exact integer in [-9, 9] that points from the set side
 * to the unset side.  The host normalises it to shade; (0,0,0) is possible (a lone voxel).
 *
 * Info of a hit image.  voxels: the grid's voxel count.  pixels: w * h of the rectangle.  covered:
 * the rectangle's covered pixels, those whose ray enters the cube.  hits: the hit records written.
 * steps and samples count up to and including the step and the in-slab sample that ended the walk,
 * as vr_hit_count_work does.  All of them are functions of the request alone; they do not depend on
 * whether an occupancy is given.
 *
 * Slice.  Positions q come from vr_mpr.h's formula, verbatim (double, left to right, rounded
 * once), s = 0 .. nsamples - 1; the bounds test, then the strict slice-box test.  A pixel is the
 * element (a byte widened to uint32_t) of the first matching in-slab sample in s order, and 0 when
 * there is none.  plane->op is validated and ignored.  Info: pixels = width * height; covered =
 * pixels with at least one step; hits = non-zero pixels; steps and samples count up to and
 * including the sample that ended the pixel's loop.
 *
 * Occupancy.  c[a] = ceil(ext[a] / 8) cells, counted from grid voxel (0,0,0) and not from the
 * volume's voxel 0.  Cell (ci, cj, ck) has index m = ci + c[0] * (cj + c[1] * ck); bit m & 31 of
 * word m >> 5 is set iff some voxel of the cell matches.  There are ceil(c[0]*c[1]*c[2] / 32)
 * words (vr_mview_occupancy_words; never more than 2 MiB), and the unused bits of the last word
 * are 0: every bit is fixed by the request.  Info: cells, cells_set (the set bits) and matching
 * (the matching voxels).  With the words a sample whose cell's bit is clear does not read the
 * array; records and pixels are byte-identical with `occupancy` NULL and with the right words.
 * With wrong or stale words the records are unspecified, but every access stays inside the buffers
 * and the call returns.
 *
 * Forms.  The _device forms work on `stream` and return when their outputs are complete.  The host
 * forms take a host array, stage it through the context's scratch and are synchronous.
 * vr_mask_pick takes a device array and writes one host record: the record of (px, py) in the
 * whole-framebuffer image; it launches one tile.
 *
 * Errors.  VR_EINVAL, with every output untouched, for a NULL argument (rect, stream and occupancy
 * may be NULL), an extent outside [1, 32768], more than 2^32 - 1 voxels, an elem_bytes other than
 * 1 or 4, a misaligned 4-byte array in device memory, an origin or grid beyond the volume (or no
 * volume), a select other than 0 or 1, VR_MVIEW_LABEL with label 0, reserved != 0, a non-NULL
 * occupancy in a host form, occupancy words, an out_dev or an occ_dev that is not 4-byte aligned,
 * an output that overlaps the array, the occupancy or (host forms) the info, an empty rectangle or
 * one beyond the framebuffer, px >= W or py >= H, whatever vr_params and the camera every mode
 * refuses, and whatever vr_mpr.h refuses of a plane.  VR_ENOSPC (vr_mesh.h's) before any kernel
 * for rcap, pcap or ocap_words below what a full call writes: info->voxels set and the info's
 * other fields 0, no buffer touched.  VR_ENOMEM when the scratch cannot be allocated.
 *
 * State.  vr_hit.h's: the calls build, evict and downgrade nothing (vr_memory_report is
 * unchanged) and leave every setting alone: a frame rendered before and after them has identical
 * bytes.  Scratch lives in the context and is freed by vr_destroy.  vr_timing_* brackets each
 * call as one interval.  vr_mview_last_kernel_name names the family's last kernel on the context
 * ("" before the first).  A multi-device context (vr_create_mask) computes on its lowest device,
 * where the buffers must live.
 */
#ifndef VR_VR_MVIEW_H
#define VR_VR_MVIEW_H

#include "vr.h"
#include "vr_mesh.h" /* VR_ENOSPC */
#include "vr_mpr.h"  /* vr_mpr_plane */

#ifdef __cplusplus
extern "C" {
#endif

#define VR_MVIEW_MAX_EXTENT 32768u
#define VR_MVIEW_CELL 8u /* an occupancy cell is 8 x 8 x 8 grid voxels */
enum vr_mview_select { VR_MVIEW_ANY = 0, VR_MVIEW_LABEL = 1 };

typedef struct vr_mview_source {
    uint32_t ext[3], origin[3]; /* vr_mstat.h's grid and origin: origin + ext <= dims */
    uint32_t elem_bytes;        /* 1 or 4 */
    uint32_t select;            /* ANY: an element matches iff it is non-zero; LABEL: iff it equals `label` */
    uint32_t label;             /* LABEL: non-zero; ANY: ignored */
    uint32_t reserved;          /* 0 */
    const void *array;          /* box-linear; device memory (device forms, pick), host (host forms) */
    const void *occupancy;      /* device forms: NULL, or the words vr_mask_occupancy_device wrote for
                                   this array, grid, select and label; host forms: NULL */
} vr_mview_source;

typedef struct vr_mask_hit {
    float    pos[3];   /* the march's f32 pos of the sample that hit, bit for bit */
    float    depth;    /* vr_hit.h's depth formula, verbatim */
    uint32_t element;  /* the array's element there (a byte widened) */
    uint32_t step;     /* loop index k of that sample */
    uint32_t index;    /* box-linear grid index of the voxel */
    int8_t   normal[3];
    uint8_t  reserved; /* 0 */
} vr_mask_hit;         /* 32 bytes; a miss is {0,0,0, +INFINITY, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0,0,0, 0} */

typedef struct vr_mview_info {
    uint64_t voxels, pixels, covered, hits, steps, samples;
} vr_mview_info; /* 48 bytes */

typedef struct vr_mview_occ_info {
    uint64_t voxels, cells, cells_set, matching;
} vr_mview_occ_info; /* 32 bytes */

/* The occupancy words of a grid; pure; 0 for a grid the family refuses. */
uint64_t vr_mview_occupancy_words(const uint32_t ext[3]);
/* The words of the source into occ_dev (ocap_words words), on `stream`; returns when complete. */
int vr_mask_occupancy_device(vr_ctx *ctx, const vr_mview_source *src, void *occ_dev, uint64_t ocap_words,
                             vr_mview_occ_info *info, void *stream);
/* w * h records into out_dev (rcap records), on `stream`; returns when they are complete. */
int vr_mask_hit_render_device(vr_ctx *ctx, const vr_camera *cam, const vr_params *params,
                              const vr_mview_source *src, const uint32_t *rect /* NULL or x0,y0,w,h */,
                              void *out_dev, uint64_t rcap, vr_mview_info *info, void *stream);
/* The same from a host array into a host array. */
int vr_mask_hit_render(vr_ctx *ctx, const vr_camera *cam, const vr_params *params, const vr_mview_source *src,
                       const uint32_t *rect, vr_mask_hit *out_host, uint64_t rcap, vr_mview_info *info);
/* One pixel: the record of (px, py) of a device array into *out_host. */
int vr_mask_pick(vr_ctx *ctx, const vr_camera *cam, const vr_params *params, const vr_mview_source *src,
                 uint32_t px, uint32_t py, vr_mask_hit *out_host);
/* width * height elements into out_dev (pcap uint32_t), on `stream`; returns when complete. */
int vr_mask_slice_device(vr_ctx *ctx, const vr_mpr_plane *plane, const vr_mview_source *src,
                         void *out_dev /* uint32 per pixel */, uint64_t pcap, vr_mview_info *info, void *stream);
/* The same from a host array into a host array. */
int vr_mask_slice(vr_ctx *ctx, const vr_mpr_plane *plane, const vr_mview_source *src, uint32_t *out_host,
                  uint64_t pcap, vr_mview_info *info);
/* The last kernel this family launched on the context. */
const char *vr_mview_last_kernel_name(const vr_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif /* VR_VR_MVIEW_H */
