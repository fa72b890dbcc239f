"""GPU: the view of a mask or a label array (include/vr/vr_mview.h, lib/libvr_amd_mview.so) against
tests/mview_ref.py -- hit records, slices, occupancy words and infos byte for byte over every pixel
and word, with `occupancy` NULL and with the built words; against vr_hit_render, vr_hit_count_work
and vr_mpr_count_work where an all-set or all-zero array makes them say the same; the pick; the chain
from a click to the piece under it; the refusals; stale words; and the context's state."""
import ctypes as C

import numpy as np
import pytest

import edge_shapes as E
import hit_scenes
import label_ref
import label_scenes
import maskcc_ref
import mpr_ref
import mview_ref as R
import mview_scenes as S
import pyoracle
import synth
import vr_amd
from gpu_kit import GUARD, c_plane, context_untouched, device_bytes, err, ext_of, guarded, read_guarded, unchanged
from gpu_kit import stream  # noqa: F401
from range_scenes import FULL, INSET, SLICE, volume

pytestmark = pytest.mark.gpu

F = np.float32
DT = vr_amd.MVIEW_HIT_DTYPE


def make_pass(w, h, vol, box=FULL, **kw):
    rp = vr_amd.OffscreenPass(w, h, **kw)
    rp.volume_dataset_changed(synth.dataset(np.asarray(vol, F)))
    rp.transfer_function_changed(synth.tf_color())
    rp.slicing_changed(*box)
    return rp


class Source:
    """An array in device memory and its vr_mview_source, with or without its occupancy words."""

    def __init__(self, rp, stream, array, origin=(0, 0, 0), label=None, odd=None):
        self.array, self.origin, self.label = array, origin, label
        self.odd = array.dtype.itemsize == 1 if odd is None else odd
        self.keep, self.ptr = device_bytes(array, self.odd)
        self.rp, self.st = rp, stream.cuda_stream
        self.occ = None

    def src(self, occ=False, **kw):
        if occ and self.occ is None:
            self.build()
        return vr_amd.mview_source(ext_of(self.array), self.ptr, self.array.dtype.itemsize, self.origin, self.label,
                                   self.occ_ptr if occ else 0, **kw)

    def build(self):
        n = vr_amd.mview_occupancy_words(ext_of(self.array))
        self.occ, self.occ_ptr, off = guarded(4 * n)
        self.occ_info = self.rp.mask_occupancy_device(self.src(), self.occ_ptr, n, stream=self.st)
        self.words = np.frombuffer(read_guarded(self.occ, off, 4 * n), np.uint32)
        return self.words, self.occ_info

    def intact(self):
        return unchanged(self.keep, self.array, self.odd)


def hits_device(rp, stream, cam, p, S_, occ, rect=None):
    w, h = (rect[2], rect[3]) if rect is not None else rp.size
    t, ptr, off = guarded(32 * w * h)
    info = rp.mask_hit_render_device(cam, p, S_.src(occ), ptr, w * h, rect, stream=stream.cuda_stream)
    # (complete on return: no synchronisation of ours before the copy on another stream)
    return read_guarded(t, off, 32 * w * h), info


def slice_device(rp, stream, pl, S_, occ):
    n = int(pl.width) * int(pl.height)
    t, ptr, off = guarded(4 * n)
    info = rp.mask_slice_device(pl, S_.src(occ), ptr, n, stream=stream.cuda_stream)
    return read_guarded(t, off, 4 * n), info


def check_hits(rp, stream, cam, p, array, want, origin=(0, 0, 0), label=None, rect=None, host=True, what=""):
    """Device form without and with the words, and the host form: the reference's bytes and info."""
    wrec, winfo, _ = want
    src = Source(rp, stream, array, origin, label)
    for occ in (False, True):
        got, info = hits_device(rp, stream, cam, p, src, occ, rect)
        bad = np.frombuffer(got, np.uint32).reshape(-1, 8) != np.frombuffer(wrec.tobytes(), np.uint32).reshape(-1, 8)
        assert got == wrec.tobytes(), (what, occ, int(bad.any(1).sum()), "records differ")
        assert info == winfo, (what, occ, info, winfo)
        elem = "u8" if array.dtype.itemsize == 1 else "u32"
        assert rp.mview_last_kernel_name() == "mview_hit_kernel<%s%s>" % (elem, ", occ" if occ else "")
    assert src.intact()
    words, oinfo, _ = R.occupancy(array, label)
    assert src.words.tobytes() == words.tobytes() and src.occ_info == oinfo, what
    if host:
        rec, info = rp.mask_hit_render(cam, p, array, origin, label, rect)
        assert rec.tobytes() == wrec.tobytes() and info == winfo, (what, "host")
    return src


# ---- 1. hit records against the reference ----------------------------------------------------------------
@pytest.mark.parametrize("step", S.STEPS, ids=["step0.005", "step1/n"])
@pytest.mark.parametrize("i", range(len(hit_scenes.PARITY)))
def test_parity_scenes(gpu, stream, i, step):
    volname, camname, box, tfname, w, h = hit_scenes.PARITY[i]
    vol = volume(volname)
    rp = make_pass(w, h, vol, box)
    try:
        cam = synth.camera(camname).to_vr_camera()
        p = S.params(vol.shape, step)
        want = S.parity_reference(i, step)
        print(hit_scenes.PARITY[i], step, want[1])
        check_hits(rp, stream, cam, p, S.blob_mask(volname), want, what=(i, step))
    finally:
        rp.close()


GRID_CASES = [  # camera, box, frame, rectangle
    ("diag", FULL, (45, 35), None), ("fill_oblique", SLICE, (32, 24), None), ("rotA", INSET, (45, 35), (7, 5, 30, 21)),
    ("rotB", S.OPEN, (32, 24), None),
]


def grid_want(camname, box, frame, rect, array, label=None, step=0.005):
    return R.hit_image(S.grid_scene(camname, box, frame[0], frame[1], step), array, S.GRID_ORIGIN, label, rect)


@pytest.mark.parametrize("case", GRID_CASES, ids=lambda c: "%s-%s-%dx%d" % (c[0], c[1][0][0], c[2][0], c[2][1]))
def test_a_grid_inside_the_volume(gpu, stream, case):
    """37 x 19 x 17 voxels at (5, 3, 2) of 43 x 24 x 20: two words, a cell row across the word boundary, a
    cut cell on every axis; byte masks at an odd address, 4-byte arrays with ANY and with each label."""
    camname, box, frame, rect = case
    rp = make_pass(frame[0], frame[1], S.grid_volume(), box)
    try:
        cam = synth.camera(camname).to_vr_camera()
        for step in S.STEPS:
            p = S.params(S.GRID_VOLUME, step)
            for density in S.DENSITIES:
                m = S.byte_mask(S.GRID_EXT, density)
                check_hits(rp, stream, cam, p, m, grid_want(camname, box, frame, rect, m, None, step), S.GRID_ORIGIN,
                           rect=rect, what=(case, step, density))
        p = S.params(S.GRID_VOLUME, 0.005)
        wm = S.word_mask(S.GRID_EXT)
        for label in (None,) + S.WORD_VALUES:
            want = grid_want(camname, box, frame, rect, wm, label)
            assert label is None or 0 < want[1]["hits"]
            check_hits(rp, stream, cam, p, wm, want, S.GRID_ORIGIN, label, rect, host=label in (None, 256),
                       what=(case, label))
        c = S.corner_voxel(S.GRID_EXT)
        src = check_hits(rp, stream, cam, S.params(S.GRID_VOLUME, None), c,
                         grid_want(camname, box, frame, rect, c, None, None), S.GRID_ORIGIN, rect=rect, what="corner")
        assert list(src.words) == [1, 0]
    finally:
        rp.close()


@pytest.mark.parametrize("ext", S.THIN_GRIDS, ids=lambda e: "x".join(map(str, e)))
def test_grids_one_voxel_thick(gpu, stream, ext):
    rp = make_pass(E.W, E.H, S.grid_volume())
    try:
        m = S.byte_mask(ext, 0.5)
        for camname in E.cameras(ext):
            cam = E.camera(camname).to_vr_camera()
            p = S.params(S.GRID_VOLUME, None)
            v = S.grid_volume()
            sc = pyoracle.Scene.from_params(v, 0.0, 1.0, synth.tf_color(), cam, E.W, E.H, p)
            want = R.hit_image(sc, m, S.GRID_ORIGIN)
            assert want[1]["hits"] >= 1
            check_hits(rp, stream, cam, p, m, want, S.GRID_ORIGIN, what=(ext, camname))
    finally:
        rp.close()


def test_full_volume_grids_and_more_than_one_workgroup(gpu, stream):
    """130 x 70 x 33: 24 occupancy words, a workgroup each; the words and a frame over them."""
    nx, ny, nz = S.BIG_DIMS
    vol = np.zeros((nz, ny, nx), F)
    rp = make_pass(45, 35, vol)
    try:
        cam = synth.camera("fill_oblique").to_vr_camera()
        p = S.params(S.BIG_DIMS, 0.005)
        sc = pyoracle.Scene.from_params(vol, 0.0, 1.0, synth.tf_color(), cam, 45, 35, p)
        for a, label in ((S.byte_mask(S.BIG_DIMS, 0.02), None), (S.word_mask(S.BIG_DIMS), 65536)):
            src = check_hits(rp, stream, cam, p, a, R.hit_image(sc, a, label=label), label=label, host=False, what="big")
            assert len(src.words) == 24 and 0 < src.occ_info["cells_set"] <= src.occ_info["cells"] == 17 * 9 * 5
    finally:
        rp.close()


# ---- 2. occupancy ----------------------------------------------------------------------------------------
def test_occupancy_words(gpu, stream):
    rp = make_pass(16, 16, np.zeros(S.BIG_DIMS[::-1], F))
    try:
        cases = [(S.byte_mask(e, d), None) for e in (S.GRID_EXT,) + S.THIN_GRIDS + ((9, 8, 2), (64, 8, 8), (65, 9, 9))
                 for d in S.DENSITIES + (0.0, 1.0)]
        cases += [(S.word_mask(S.GRID_EXT), l) for l in (None,) + S.WORD_VALUES]
        cases += [(S.corner_voxel(S.GRID_EXT), None), (S.byte_mask(S.BIG_DIMS, 0.0005), None)]
        for a, label in cases:
            src = Source(rp, stream, a, (0, 0, 0), label)
            words, info = src.build()
            wwords, winfo, _ = R.occupancy(a, label)
            assert words.tobytes() == wwords.tobytes() and info == winfo, (a.shape, label, info, winfo)
            assert src.intact() and rp.mview_last_kernel_name() == "mview_occupancy_kernel<%s>" % (
                "u8" if a.dtype.itemsize == 1 else "u32")
    finally:
        rp.close()


# ---- 3. against existing device code, with no reference ---------------------------------------------------
def test_all_set_is_vr_hit_entry_and_all_zero_is_its_count(gpu, stream):
    """The restated pixel_ray against the frames': every pixel of 640 x 360, every synth camera."""
    vol = synth.gaussians_numpy((64, 64, 64), seed=7)
    rp = make_pass(640, 360, vol)
    try:
        p = vr_amd.default_params()
        ones = Source(rp, stream, np.ones((64, 64, 64), np.uint8))
        zeros = Source(rp, stream, np.zeros((64, 64, 64), np.uint32))
        for name in synth.CAMERAS:
            cam = synth.camera(name).to_vr_camera()
            e = rp.hit_image(cam, p, vr_amd.HIT_ENTRY)
            for occ in (False, True):
                got, info = hits_device(rp, stream, cam, p, ones, occ)
                rec = np.frombuffer(got, DT).reshape(360, 640)
                for f in ("pos", "depth", "step"):
                    assert np.array_equal(rec[f].view(np.uint32), e[f].view(np.uint32)), (name, f)
                st = rp.hit_count_work(cam, p, vr_amd.HIT_ENTRY)
                assert (info["covered"], info["hits"], info["steps"], info["samples"]) == (
                    st["rays"], st["shaded_samples"], st["steps"], st["samples"]), name
                got, info = hits_device(rp, stream, cam, p, zeros, occ)
                assert got == R.miss_records(640 * 360).tobytes()
                st = rp.hit_count_work(cam, p, vr_amd.HIT_MAX)
                assert (info["covered"], info["hits"], info["steps"], info["samples"]) == (
                    st["rays"], 0, st["steps"], st["samples"]), (name, info, st)
    finally:
        rp.close()


@pytest.mark.parametrize("dims", E.MPR_VOLUMES, ids=lambda d: "x".join(map(str, d)))
def test_slices(gpu, stream, dims):
    """edge_shapes' planes: thin, five-sample slabs, oblique and 1 x 1; the FULL and an inset box; ANY
    and a label; an all-zero array walks what vr_mpr_count_work counts."""
    vol = E.fill(dims, "noise")
    a = S.word_mask(dims)
    zero = np.zeros(dims[::-1], np.uint8)
    for box in (FULL, INSET):
        rp = make_pass(16, 16, vol, box)
        try:
            srcs = {l: Source(rp, stream, a, (0, 0, 0), l) for l in (None, 256)}
            zsrc = Source(rp, stream, zero)
            for name, pl in E.mpr_planes(dims, E.geometry("f32")):
                vp = c_plane(pl)
                for label, src in srcs.items():
                    wimg, winfo = R.slice_image(dims, a, pl, box, label=label)
                    for occ in (False, True):
                        got, info = slice_device(rp, stream, vp, src, occ)
                        assert got == wimg.tobytes() and info == winfo, (dims, name, label, occ, info, winfo)
                    img, info = rp.mask_slice(vp, a, label=label)
                    assert img.tobytes() == wimg.tobytes() and info == winfo, (dims, name, label, "host")
                got, info = slice_device(rp, stream, vp, zsrc, False)
                st = rp.count_work_mpr(vp)
                assert got == bytes(4 * pl["width"] * pl["height"])
                assert (info["covered"], info["hits"], info["steps"], info["samples"]) == (st["rays"], 0, st["steps"], st["samples"])
            assert all(s.intact() for s in srcs.values()) and rp.mview_last_kernel_name() == "mview_slice_kernel<u8>"
        finally:
            rp.close()


def test_a_slice_of_the_grid_inside_the_volume(gpu, stream):
    rp = make_pass(16, 16, S.grid_volume(), SLICE)
    try:
        a = S.word_mask(S.GRID_EXT)
        src = Source(rp, stream, a, S.GRID_ORIGIN, 65536)
        for pl in (mpr_ref.axis_plane(2, 9.5 / 20, 43, 24, 5, 1.0 / 20), mpr_ref.oblique_plane(0.02, 45, 35, 7),
                   mpr_ref.axis_plane(0, 20.5 / 43, 33, 17)):
            wimg, winfo = R.slice_image(S.GRID_VOLUME, a, pl, SLICE, S.GRID_ORIGIN, 65536)
            assert winfo["hits"] >= 10
            for occ in (False, True):
                got, info = slice_device(rp, stream, c_plane(pl), src, occ)
                assert got == wimg.tobytes() and info == winfo
        assert rp.mview_last_kernel_name() == "mview_slice_kernel<u32, occ>"
    finally:
        rp.close()


# ---- 4. the pick and the chain ---------------------------------------------------------------------------
def test_pick_is_the_images_record(gpu, stream):
    rp = make_pass(45, 35, S.grid_volume())
    try:
        cam = synth.camera("diag").to_vr_camera()
        p = S.params(S.GRID_VOLUME, 0.005)
        m = S.byte_mask(S.GRID_EXT, 0.02)
        src = Source(rp, stream, m, S.GRID_ORIGIN)
        got, info = hits_device(rp, stream, cam, p, src, True)
        rec = np.frombuffer(got, DT).reshape(35, 45)
        hit = rec["step"] != R.MISS
        ys, xs = np.nonzero(hit)
        my, mx = np.nonzero(~hit)
        pixels = list(zip(xs[::max(len(xs) // 10, 1)][:10], ys[::max(len(ys) // 10, 1)][:10])) + \
            list(zip(mx[::max(len(mx) // 10, 1)][:10], my[::max(len(my) // 10, 1)][:10]))
        assert len(pixels) == 20
        for x, y in pixels:
            one = rp.mask_pick(cam, p, src.src(), int(x), int(y))
            assert one.tobytes() == rec[y, x].tobytes(), (x, y)
        assert rp.mview_last_kernel_name() == "mview_hit_kernel<u8>"  # (the words are not read)
        assert rp.mask_pick(cam, p, src.src(True), int(xs[0]), int(ys[0])).tobytes() == rec[ys[0], xs[0]].tobytes()
    finally:
        rp.close()


def test_the_chain_from_a_click_to_its_piece(gpu, stream):
    """vr_region_grow_device with a box gives a mask with origin = box_min: its words, its image, a pick
    on a hit pixel, and vr_mask_select_device seeded with the picked voxel."""
    import torch
    full = label_scenes.noise()
    box = label_scenes.BOX
    lo, hi = 0.5, 1.0
    labels, table, linfo = label_ref.label(full, lo, hi, 6, box)
    shape, n = labels.shape, linfo["voxels"]
    big = table[np.argmax(table["voxels"])]
    at = int(big["label"]) - 1
    seed = tuple(c + o for c, o in zip((at % shape[2], (at // shape[2]) % shape[1], at // (shape[2] * shape[1])), box[0]))
    want_mask = (labels == big["label"]).astype(np.uint8)
    rp = make_pass(45, 35, full)
    try:
        st = stream.cuda_stream
        a = torch.full((n + 8,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        comp = rp.region_grow_device(seed, a.data_ptr(), n, lo, hi, 6, box, stream=st)
        assert comp["voxels"] == int(big["voxels"])
        ext = shape[::-1]
        nw = vr_amd.mview_occupancy_words(ext)
        occ, occ_ptr, off = guarded(4 * nw)
        oinfo = rp.mask_occupancy_device(vr_amd.mview_source(ext, a.data_ptr(), 1, box[0]), occ_ptr, nw, stream=st)
        wwords, winfo, _ = R.occupancy(want_mask)
        assert read_guarded(occ, off, 4 * nw) == wwords.tobytes() and oinfo == winfo and oinfo["matching"] == comp["voxels"]
        src = vr_amd.mview_source(ext, a.data_ptr(), 1, box[0], occupancy_ptr=occ_ptr)
        cam = synth.camera("rotA").to_vr_camera()
        p = S.params(full.shape, None)
        t, ptr, off = guarded(32 * 45 * 35)
        info = rp.mask_hit_render_device(cam, p, src, ptr, 45 * 35, stream=st)
        rec = np.frombuffer(read_guarded(t, off, 32 * 45 * 35), DT).reshape(35, 45)
        sc = pyoracle.Scene.from_params(full, 0.0, 1.0, synth.tf_color(), cam, 45, 35, p)
        wrec, winfo, _ = R.hit_image(sc, want_mask, box[0])
        assert rec.tobytes() == wrec.tobytes() and info == winfo and info["hits"] >= 30
        ys, xs = np.nonzero(rec["step"] != R.MISS)
        y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
        one = rp.mask_pick(cam, p, src, x, y)
        assert one.tobytes() == rec[y, x].tobytes()
        l = int(one["index"])
        gv = (l % ext[0], l // ext[0] % ext[1], l // (ext[0] * ext[1]))
        assert want_mask[gv[2], gv[1], gv[0]] == 1 and one["element"] == 1
        b = torch.full((n + 8,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sinfo = rp.mask_select_device(ext, vr_amd.MASK_KEEP_SEED, a.data_ptr(), 1, b.data_ptr(), n, 6, seed=gv, stream=st)
        wout, wsel = maskcc_ref.select(want_mask, vr_amd.MASK_KEEP_SEED, 6, seed=gv)
        hb = b.cpu().numpy()
        assert hb[:n].tobytes() == wout.tobytes() and np.all(hb[n:] == GUARD) and sinfo == wsel and sinfo["kept"] == 1
    finally:
        rp.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------
def test_every_error_leaves_the_outputs_untouched(gpu, stream):
    import torch
    rp = make_pass(32, 24, S.grid_volume())
    empty = vr_amd.OffscreenPass(32, 24)  # no volume
    try:
        L = vr_amd.mview_lib()
        cam = synth.camera("diag").to_vr_camera()
        p = vr_amd.default_params()
        m = S.byte_mask(S.GRID_EXT, 0.5)
        wm = S.word_mask(S.GRID_EXT)
        src8 = Source(rp, stream, m, S.GRID_ORIGIN, odd=False)
        src32 = Source(rp, stream, wm, S.GRID_ORIGIN)
        src8.build()
        out = torch.full((32 * 32 * 24 + 64,), GUARD, dtype=torch.uint8, device="cuda")
        hout = np.full(32 * 32 * 24 + 64, GUARD, np.uint8)
        torch.cuda.synchronize()
        optr = out.data_ptr()
        info, oinfo, hit = vr_amd.vr_mview_info(), vr_amd.vr_mview_occ_info(), vr_amd.vr_mask_hit()
        for s, n in ((info, 48), (oinfo, 32), (hit, 32)):
            C.memset(C.byref(s), GUARD, n)
        pl = vr_amd.axis_plane(vr_amd.AXIS_AXIAL, 0.5, 32, 24)
        ctx = rp._ctx
        nw = 2
        rect = lambda *r: (C.c_uint32 * 4)(*r)
        ext, org = S.GRID_EXT, S.GRID_ORIGIN

        def all_calls(src, code=-22, text=None, calls="ohdps"):
            """The calls named in `calls` (o: occupancy, h: device hit image, d: device slice, p: pick, s: the
            two host forms) refuse `src`."""
            rcs = []
            if "o" in calls:
                rcs.append(L.vr_mask_occupancy_device(ctx, C.byref(src), optr, nw, C.byref(oinfo), None))
            if "h" in calls:
                rcs.append(L.vr_mask_hit_render_device(ctx, C.byref(cam), C.byref(p), C.byref(src), None, optr, 32 * 24,
                                                       C.byref(info), None))
            if "d" in calls:
                rcs.append(L.vr_mask_slice_device(ctx, C.byref(pl), C.byref(src), optr, 32 * 24, C.byref(info), None))
            if "p" in calls:
                rcs.append(L.vr_mask_pick(ctx, C.byref(cam), C.byref(p), C.byref(src), 3, 3, C.byref(hit)))
            if "s" in calls:
                hs = vr_amd.mview_source(ext_of(m), m.ctypes.data, 1, org)
                for f in ("ext", "origin", "elem_bytes", "select", "label", "reserved"):
                    setattr(hs, f, getattr(src, f))
                hs.occupancy = src.occupancy if text and "host form" in text else None
                rcs.append(L.vr_mask_hit_render(ctx, C.byref(cam), C.byref(p), C.byref(hs), None, hout.ctypes.data, 32 * 24,
                                                C.byref(info)))
                rcs.append(L.vr_mask_slice(ctx, C.byref(pl), C.byref(hs), hout.ctypes.data, 32 * 24, C.byref(info)))
            assert rcs and all(rc == code for rc in rcs), (text, rcs)
            if text:
                assert text in err(rp), (text, err(rp))

        mk = lambda **kw: vr_amd.mview_source(kw.pop("ext", ext), kw.pop("ptr", src8.ptr), kw.pop("eb", 1),
                                              kw.pop("origin", org), **kw)
        all_calls(mk(ext=(0, 19, 17)), text="extent")
        all_calls(mk(ext=(37, 32769, 17)), text="extent")
        all_calls(mk(ext=(32768, 32768, 4)), text="2^32 - 1")
        for eb in (0, 2, 8):
            all_calls(mk(eb=eb), text="elem_bytes")
        all_calls(mk(ptr=src32.ptr + 2, eb=4), text="4-byte aligned", calls="ohdp")
        all_calls(mk(origin=(7, 3, 2)), text="beyond the volume")
        all_calls(mk(origin=(5, 3, 0xFFFFFFFF)), text="beyond the volume")
        all_calls(mk(select=2), text="select")
        all_calls(mk(label=0, select=vr_amd.MVIEW_LABEL), text="non-zero label")
        all_calls(mk(reserved=1), text="reserved")
        all_calls(mk(occupancy_ptr=src8.occ_ptr), text="host form", calls="s")
        all_calls(mk(occupancy_ptr=src8.occ_ptr + 2), text="occupancy words must be 4-byte aligned", calls="hd")
        s = mk()
        s.array = None
        all_calls(s, text="NULL", calls="ohdp")
        # no volume
        good = mk()
        assert L.vr_mask_hit_render_device(empty._ctx, C.byref(cam), C.byref(p), C.byref(good), None, optr, 32 * 24,
                                           C.byref(info), None) == -22
        assert "no volume" in err(empty) or "beyond the volume" in err(empty)  # (no bricks, or the 1-voxel default)
        assert L.vr_mask_occupancy_device(empty._ctx, C.byref(good), optr, nw, C.byref(oinfo), None) == -22
        assert L.vr_mask_pick(empty._ctx, C.byref(cam), C.byref(p), C.byref(good), 0, 0, C.byref(hit)) == -22
        assert L.vr_mask_slice_device(empty._ctx, C.byref(pl), C.byref(good), optr, 32 * 24, C.byref(info), None) == -22
        # NULL arguments
        H, D, O, P_ = L.vr_mask_hit_render_device, L.vr_mask_slice_device, L.vr_mask_occupancy_device, L.vr_mask_pick
        g, c_, p_ = C.byref(good), C.byref(cam), C.byref(p)
        assert H(ctx, None, p_, g, None, optr, 768, C.byref(info), None) == -22
        assert H(ctx, c_, None, g, None, optr, 768, C.byref(info), None) == -22
        assert H(ctx, c_, p_, None, None, optr, 768, C.byref(info), None) == -22
        assert H(ctx, c_, p_, g, None, None, 768, C.byref(info), None) == -22
        assert H(ctx, c_, p_, g, None, optr, 768, None, None) == -22
        assert D(ctx, None, g, optr, 768, C.byref(info), None) == -22 and D(ctx, C.byref(pl), g, None, 768, C.byref(info), None) == -22
        assert D(ctx, C.byref(pl), g, optr, 768, None, None) == -22
        assert O(ctx, g, None, nw, C.byref(oinfo), None) == -22 and O(ctx, g, optr, nw, None, None) == -22
        assert P_(ctx, c_, p_, g, 0, 0, None) == -22 and P_(ctx, None, p_, g, 0, 0, C.byref(hit)) == -22
        # alignment and overlap of the outputs
        assert H(ctx, c_, p_, g, None, optr + 2, 768, C.byref(info), None) == -22 and "4-byte aligned" in err(rp)
        assert D(ctx, C.byref(pl), g, optr + 1, 768, C.byref(info), None) == -22
        assert O(ctx, g, optr + 2, nw, C.byref(oinfo), None) == -22
        inside = src8.ptr - src8.ptr % 4  # (shares bytes with the array)
        assert H(ctx, c_, p_, g, None, inside, 768, C.byref(info), None) == -22 and "overlaps the array" in err(rp)
        assert D(ctx, C.byref(pl), g, inside, 768, C.byref(info), None) == -22
        assert O(ctx, g, inside, nw, C.byref(oinfo), None) == -22
        wo = C.byref(src8.src(True))
        assert H(ctx, c_, p_, wo, None, src8.occ_ptr, 768, C.byref(info), None) == -22 and "overlaps the occupancy" in err(rp)
        assert D(ctx, C.byref(pl), wo, src8.occ_ptr + 4, 768, C.byref(info), None) == -22
        hs = vr_amd.mview_source(ext_of(m), m.ctypes.data, 1, org)
        assert L.vr_mask_hit_render(ctx, c_, p_, C.byref(hs), None, m.ctypes.data, 768, C.byref(info)) == -22
        both = np.full(32 * 768 + 48, GUARD, np.uint8)  # the records and the info in one block
        assert L.vr_mask_hit_render(ctx, c_, p_, C.byref(hs), None, both.ctypes.data, 768,
                                    C.cast(both.ctypes.data + 32 * 768 - 8, C.POINTER(vr_amd.vr_mview_info))) == -22
        assert "overlaps the info" in err(rp) and np.all(both == GUARD)
        # rectangles and the pick pixel
        for r in (rect(0, 0, 0, 5), rect(0, 0, 5, 0), rect(28, 0, 5, 5), rect(0, 20, 5, 5), rect(0xFFFFFFFF, 0, 2, 2)):
            assert H(ctx, c_, p_, g, r, optr, 768, C.byref(info), None) == -22 and "rectangle" in err(rp)
        assert P_(ctx, c_, p_, g, 32, 0, C.byref(hit)) == -22 and P_(ctx, c_, p_, g, 0, 24, C.byref(hit)) == -22
        # the params and the camera every mode refuses
        bad = vr_amd.default_params(step=0.0)
        assert H(ctx, c_, C.byref(bad), g, None, optr, 768, C.byref(info), None) == -22 and "step" in err(rp)
        assert P_(ctx, c_, C.byref(bad), g, 0, 0, C.byref(hit)) == -22
        flat = vr_amd.vr_camera()  # a zero view matrix: proj * view is singular
        assert H(ctx, C.byref(flat), p_, g, None, optr, 768, C.byref(info), None) == -22
        # what vr_mpr.h refuses of a plane
        for field, value in (("width", 0), ("nsamples", 0), ("nsamples", 4097), ("op", 3)):
            bp = vr_amd.axis_plane(vr_amd.AXIS_AXIAL, 0.5, 32, 24)
            setattr(bp, field, value)
            assert D(ctx, C.byref(bp), g, optr, 768, C.byref(info), None) == -22, field
        bp = vr_amd.axis_plane(vr_amd.AXIS_AXIAL, 0.5, 32, 24)
        bp.dn[1] = float("inf")
        assert D(ctx, C.byref(bp), g, optr, 768, C.byref(info), None) == -22 and "finite" in err(rp)
        # nothing was written
        torch.cuda.synchronize()
        assert bool((out == GUARD).all()) and np.all(hout == GUARD)
        assert bytes(info) == bytes([GUARD]) * 48 and bytes(oinfo) == bytes([GUARD]) * 32 and bytes(hit) == bytes([GUARD]) * 32
        assert src8.intact() and src32.intact()

        # VR_ENOSPC one element short on each cap: voxels set, the rest 0, no buffer touched
        voxels = m.size
        assert H(ctx, c_, p_, g, None, optr, 767, C.byref(info), None) == -28
        assert [getattr(info, f) for f, _ in info._fields_] == [voxels, 0, 0, 0, 0, 0]
        C.memset(C.byref(info), GUARD, 48)
        assert H(ctx, c_, p_, g, rect(3, 2, 7, 5), optr, 34, C.byref(info), None) == -28 and info.voxels == voxels
        assert H(ctx, c_, p_, g, rect(3, 2, 7, 5), optr, 35, C.byref(info), None) == 0 and info.pixels == 35
        C.memset(C.byref(info), GUARD, 48)
        assert L.vr_mask_hit_render(ctx, c_, p_, C.byref(hs), None, hout.ctypes.data, 767, C.byref(info)) == -28
        assert [getattr(info, f) for f, _ in info._fields_] == [voxels, 0, 0, 0, 0, 0]
        C.memset(C.byref(info), GUARD, 48)
        assert D(ctx, C.byref(pl), g, optr, 767, C.byref(info), None) == -28
        assert [getattr(info, f) for f, _ in info._fields_] == [voxels, 0, 0, 0, 0, 0]
        assert L.vr_mask_slice(ctx, C.byref(pl), C.byref(hs), hout.ctypes.data, 767, C.byref(info)) == -28
        assert O(ctx, g, optr, nw - 1, C.byref(oinfo), None) == -28
        assert [getattr(oinfo, f) for f, _ in oinfo._fields_] == [voxels, 0, 0, 0]
        # -22 outranks -28: a grid beyond the volume with a short buffer
        assert H(ctx, c_, p_, C.byref(mk(origin=(7, 3, 2))), None, optr, 1, C.byref(info), None) == -22
        assert np.all(hout == GUARD)
        # the binding's own refusals
        with pytest.raises(ValueError):
            rp.mask_hit_render(cam, p, np.zeros((2, 2), np.uint8))
        with pytest.raises(ValueError):
            rp.mask_slice(pl, np.zeros((2, 2, 2), np.uint16))
    finally:
        rp.close()
        empty.close()


def test_stale_occupancy_words_stay_inside_the_buffers(gpu, stream):
    """All-zero words and all-ones words over a real mask: VR_OK, the guards intact; all-ones words say
    "read the array" everywhere, which is the call without words."""
    import torch
    rp = make_pass(45, 35, S.grid_volume())
    try:
        cam = synth.camera("diag").to_vr_camera()
        p = S.params(S.GRID_VOLUME, 0.005)
        m = S.byte_mask(S.GRID_EXT, 0.5)
        want = grid_want("diag", FULL, (45, 35), None, m)
        src = Source(rp, stream, m, S.GRID_ORIGIN)
        src.build()
        pl = mpr_ref.axis_plane(2, 9.5 / 20, 43, 24, 5, 1.0 / 20)
        wimg, winfo = R.slice_image(S.GRID_VOLUME, m, pl, FULL, S.GRID_ORIGIN)
        for fill in (0x00, 0xFF):
            occ, ptr, off = guarded(8)
            occ[off:off + 8] = fill
            torch.cuda.synchronize()
            src.occ, src.occ_ptr = occ, ptr
            got, info = hits_device(rp, stream, cam, p, src, True)
            sgot, sinfo = slice_device(rp, stream, c_plane(pl), src, True)
            assert read_guarded(occ, off, 8) == bytes([fill]) * 8 and src.intact()
            if fill:
                assert got == want[0].tobytes() and info == want[1]
                assert sgot == wimg.tobytes() and sinfo == winfo
            else:  # no cell is set: nothing is read, nothing hits, and every ray is walked to its end
                assert got == R.miss_records(45 * 35).tobytes() and info["hits"] == 0 and info["covered"] == want[1]["covered"]
                assert sgot == bytes(4 * 43 * 24)
    finally:
        rp.close()


# ---- 6. state --------------------------------------------------------------------------------------------
def test_the_calls_leave_the_context_as_it_was(gpu, stream):
    vol = label_scenes.noise()
    rp = hit_scenes.hit_pass(32, 24, np.asarray(vol), synth.tf_color(), 0.5)
    try:
        cam = synth.camera("rotA").to_vr_camera()
        p = vr_amd.default_params(shading=1, skip_empty=1)
        with context_untouched(rp, cam, p):
            assert rp.mview_last_kernel_name() == ""  # a fresh context
            m = S.byte_mask(ext_of(vol), 0.02)
            src = Source(rp, stream, m)
            rp.timing_enable(True)
            rp.timing_reset()
            src.build()
            assert rp.timing_read()[1] == 1 and rp.mview_last_kernel_name() == "mview_occupancy_kernel<u8>"
            rp.timing_reset()
            got, info = hits_device(rp, stream, cam, p, src, True)
            assert rp.timing_read()[1] == 1 and rp.mview_last_kernel_name() == "mview_hit_kernel<u8, occ>"
            sc = pyoracle.Scene.from_params(vol, 0.0, 1.0, synth.tf_color(), cam, 32, 24, p)
            want = R.hit_image(sc, m)
            assert got == want[0].tobytes() and info == want[1]
            rp.timing_reset()
            y, x = np.argwhere(want[0]["step"] != R.MISS)[0]
            assert rp.mask_pick(cam, p, src.src(), int(x), int(y)).tobytes() == want[0][y, x].tobytes()
            assert rp.timing_read()[1] == 1
            rp.timing_reset()
            pl = mpr_ref.axis_plane(2, 0.5, 19, 17, 3, 0.02)
            sgot, sinfo = slice_device(rp, stream, c_plane(pl), src, False)
            assert rp.timing_read()[1] == 1 and rp.mview_last_kernel_name() == "mview_slice_kernel<u8>"
            wimg, winfo = R.slice_image(ext_of(vol), m, pl)
            assert sgot == wimg.tobytes() and sinfo == winfo
            rp.timing_enable(False)
            rp.timing_reset()
            rec, hinfo = rp.mask_hit_render(cam, p, m)
            assert rp.timing_read()[1] == 0 and rec.tobytes() == want[0].tobytes()
    finally:
        rp.close()


def test_a_multi_device_context_computes_on_its_lowest_device(gpu, stream):
    grp = make_pass(32, 24, S.grid_volume(), SLICE, exchange=vr_amd.EXCHANGE_COPY, members=[0, 0])
    try:
        cam = synth.camera("diag").to_vr_camera()
        p = S.params(S.GRID_VOLUME, 0.005)
        wm = S.word_mask(S.GRID_EXT)
        want = grid_want("diag", SLICE, (32, 24), None, wm, 256)
        src = check_hits(grp, stream, cam, p, wm, want, S.GRID_ORIGIN, 256, what="group")
        ys, xs = np.nonzero(want[0]["step"] != R.MISS)
        assert grp.mask_pick(cam, p, src.src(), int(xs[0]), int(ys[0])).tobytes() == want[0][ys[0], xs[0]].tobytes()
        pl = mpr_ref.axis_plane(2, 9.5 / 20, 43, 24, 5, 1.0 / 20)
        wimg, winfo = R.slice_image(S.GRID_VOLUME, wm, pl, SLICE, S.GRID_ORIGIN, 256)
        got, info = slice_device(grp, stream, c_plane(pl), src, True)
        assert got == wimg.tobytes() and info == winfo
        img, info = grp.mask_slice(c_plane(pl), wm, S.GRID_ORIGIN, 256)
        assert img.tobytes() == wimg.tobytes() and info == winfo
        assert grp.mview_last_kernel_name() == "mview_slice_kernel<u32>"
    finally:
        grp.close()
