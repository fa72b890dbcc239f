"""GPU: per-pixel hit records and picking (include/vr/vr_hit.h, hit_kernel).

The reference is tests/hit_ref.py (the oracle's own ray, filter and TF around the five walks,
pinned independently by tests/test_hit_cpu.py); records must equal it bit for bit -- the 24-byte
records are compared as uint32 words -- and vr_hit_count_work's counters must be equal too.
Scenes: tests/hit_scenes.py; volumes and constants: tests/range_scenes.py."""
import ctypes as C

import numpy as np
import pytest

import hit_ref
import hit_scenes
import synth
import vr_amd
from hit_scenes import CUT, KEYS, KIND, PARITY, THRESHOLDS, hit_pass, isovalue, key_kind, reference, words
from range_scenes import FULL, H, STORAGE, W, int_volume, volume

pytestmark = pytest.mark.gpu

F = np.float32
NAME = "void vr::(anonymous namespace)::hit_kernel<%s, %d, %s, %d>(vr::MarchParams, vr::HitArgs)"
P = vr_amd.default_params


def okey(t):
    return ("opacity", float(F(t)))


def check_records(got, want, what):
    a, b = words(got), words(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.any(a != b, axis=-1)
    assert not bad.any(), (what, int(bad.sum()), "records differ; first:",
                           got[bad][0], want[bad][0], np.argwhere(bad)[0].tolist())


def check_scene(rp, cam, walk, keys=KEYS, params=None):
    p = params if params is not None else P()
    for key in keys:
        kind, th = key_kind(key)
        check_records(rp.hit_image(cam, p, kind, th), walk.records[key], key)
        got = rp.hit_count_work(cam, p, kind, th)
        print(key, got)
        assert got == walk.stats[key], (key, got, walk.stats[key])


# ---- 1. parity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("volname,camname,box,tfname,w,h", PARITY)
def test_records_equal_the_reference(gpu, volname, camname, box, tfname, w, h):
    walk = reference(volname, camname, box, tfname, w, h)
    cov = int(walk.covered.sum())
    print(volname, camname, tfname, (w, h), "covered", cov, {str(k): int(walk.hits(k).sum()) for k in KEYS})
    # the scene exercises its kinds (the helper's own output)
    if camname == "near":
        assert cov == 0
    elif (w, h) == (1, 1):
        assert cov == 1 and walk.hits("max").all()
    else:
        hit_scenes.assert_exercised(walk, fourth=(volname, camname, tfname) == ("g13", "rotB", "tfc"))
    if box == CUT:
        assert walk.cap.sum() >= 10
    rp = hit_pass(w, h, volume(volname), synth.TFS[tfname](), isovalue(volume(volname)), box)
    try:
        check_scene(rp, synth.camera(camname).to_vr_camera(), walk)
    finally:
        rp.close()


# ---- 2. samples in flight ---------------------------------------------------------------------------
def test_every_inflight_variant_writes_the_same_bytes(gpu):
    volname, camname, box, tfname, w, h = PARITY[4]
    walk = reference(volname, camname, box, tfname, w, h)
    rp = hit_pass(w, h, volume(volname), synth.TFS[tfname](), isovalue(volume(volname)), box)
    try:
        cam = synth.camera(camname).to_vr_camera()
        for key in KEYS:
            kind, th = key_kind(key)
            imgs = {}
            for k in (1, 2):
                rp.set_knob("hit_inflight", k)
                imgs[k] = rp.hit_image(cam, P(), kind, th)
                assert rp.last_kernel_name() == NAME % ("float", kind, "false", k)
                check_records(imgs[k], walk.records[key], (key, k))
            assert np.array_equal(words(imgs[1]), words(imgs[2]))
        rp.set_knob("hit_inflight", -1)
        for bad in (0, 3, 4, -2):
            assert vr_amd.lib().vr_debug_set_knob(rp._ctx, vr_amd.KNOBS["hit_inflight"], bad) == -22
        assert rp.get_knob("hit_inflight") == -1
    finally:
        rp.close()


# ---- 3. storage types and layouts, the value window ------------------------------------------------------
TAG = {(0, 0): "unsigned char", (1, 0): "signed char", (0, 1): "vr::Quad8<unsigned char>",
       (1, 1): "vr::Quad8<signed char>", (2, None): "unsigned short", (3, None): "short", (4, None): "float"}


@pytest.mark.parametrize("dtype,signed,knobs,storage", STORAGE)
def test_storage_types(gpu, dtype, signed, knobs, storage):
    vf = int_volume(signed)
    walk = reference("int_s" if signed else "int_u", "fill_oblique", FULL, "tfc", vol=vf)
    assert walk.hits("iso").sum() >= 30 and walk.hits("max").sum() >= 30
    rp = hit_pass(W, H, vf.astype(dtype), synth.tf_color(), isovalue(vf), **knobs)
    try:
        assert rp.volume_info()[2] == storage
        cam = synth.camera("fill_oblique").to_vr_camera()
        check_scene(rp, cam, walk, ("iso", "max"))
        # a volume this small keeps its 8-bit voxels in yz-quads unless the knob says otherwise
        quad = knobs.get("u8_layout", 1) if storage < 2 else None
        assert rp.last_kernel_name() == NAME % (TAG[(storage, quad)], KIND["max"], "true", 1)
    finally:
        rp.close()


def test_a_narrow_window_moves_opacity_and_leaves_max(gpu):
    vf = int_volume(False)
    vrange = (20.0, 90.0)
    full = reference("int_u", "fill_oblique", FULL, "tfc", vol=vf)
    walk = reference("int_u", "fill_oblique", FULL, "tfc", vol=vf, vrange=vrange)
    for t in THRESHOLDS[:2]:
        assert walk.hits(okey(t)).sum() >= 30
        assert not np.array_equal(words(walk.records[okey(t)]), words(full.records[okey(t)]))
    assert np.array_equal(words(walk.records["max"]), words(full.records["max"]))
    rp = hit_pass(W, H, vf.astype(np.uint16), synth.tf_color(), isovalue(vf), vrange=vrange)
    try:
        check_scene(rp, synth.camera("fill_oblique").to_vr_camera(), walk,
                    [okey(t) for t in THRESHOLDS] + ["max"])
    finally:
        rp.close()


# ---- 4. rectangles and picking -------------------------------------------------------------------------
def uncovered_rect(covered, w=3, h=2):
    H_, W_ = covered.shape
    for y in range(H_ - h + 1):
        for x in range(W_ - w + 1):
            if not covered[y:y + h, x:x + w].any():
                return (x, y, w, h)
    raise AssertionError("the scene covers every 3 x 2 block")


def test_rectangles_are_windows_of_the_frame(gpu):
    volname, camname, box, tfname, w, h = PARITY[4]
    assert (w, h) == (45, 35)
    walk = reference(volname, camname, box, tfname, w, h)
    empty = uncovered_rect(walk.covered)
    rects = [(0, 0, w, h), (13, 7, 20, 18), (44, 34, 1, 1), empty]
    assert walk.covered[7:25, 13:33].sum() >= 100
    rp = hit_pass(w, h, volume(volname), synth.TFS[tfname](), isovalue(volume(volname)), box)
    try:
        cam = synth.camera(camname).to_vr_camera()
        for key in KEYS:
            kind, th = key_kind(key)
            for k in (1, 2):
                rp.set_knob("hit_inflight", k)
                for r in rects:
                    x0, y0, rw, rh = r
                    want = walk.records[key][y0:y0 + rh, x0:x0 + rw]
                    got = rp.hit_image(cam, P(), kind, th, rect=r)
                    assert got.shape == (rh, rw)
                    check_records(got, want, (key, k, r))
            for r in rects:
                x0, y0, rw, rh = r
                st = rp.hit_count_work(cam, P(), kind, th, rect=r)
                win = (slice(y0, y0 + rh), slice(x0, x0 + rw))
                assert st["rays"] == int(walk.covered[win].sum()), (key, r, st)
                assert st["shaded_samples"] == int(walk.hits(key)[win].sum()) and st["skipped_samples"] == 0
            assert rp.hit_count_work(cam, P(), kind, th, rect=rects[0]) == walk.stats[key]
        assert np.array_equal(words(rp.hit_image(cam, P(), KIND["max"], rect=empty)),
                              words(hit_ref.miss_records((empty[3], empty[2]))))
    finally:
        rp.close()


def test_pick_equals_the_record_of_its_pixel(gpu):
    volname, camname, box, tfname, w, h = PARITY[4]
    walk = reference(volname, camname, box, tfname, w, h)
    rp = hit_pass(w, h, volume(volname), synth.TFS[tfname](), isovalue(volume(volname)), box)
    try:
        cam = synth.camera(camname).to_vr_camera()
        for key in KEYS:
            kind, th = key_kind(key)
            hit = walk.hits(key)
            places = {"hit": np.argwhere(hit), "uncovered": np.argwhere(~walk.covered)}
            if key == "iso" or isinstance(key, tuple):
                places["covered miss"] = np.argwhere(walk.covered & ~hit)
            for what, at in places.items():
                assert len(at) >= 3, (key, what)
                for py, px in (at[0], at[len(at) // 2], at[-1]):
                    got = rp.pick(cam, P(), int(px), int(py), kind, th)
                    check_records(np.asarray(got).reshape(1), walk.records[key][py, px].reshape(1),
                                  (key, what, int(px), int(py)))
                    if what != "hit":
                        assert got["step"] == vr_amd.HIT_MISS_STEP and got["depth"] == np.inf
        assert rp.last_kernel_name() == NAME % ("float", vr_amd.HIT_OPACITY, "false", 1) or \
            rp.last_kernel_name() == NAME % ("float", vr_amd.HIT_OPACITY, "false", 2)
    finally:
        rp.close()


# ---- 5. special values -----------------------------------------------------------------------------------
def special_volume():
    v = np.array(volume("g13"), np.float32)  # (21, 7, 13) = (z, y, x)
    v[:, :, :8] = np.nan                      # the low-x part: NaN only
    v[3, 2, 10] = np.inf
    v[14:16, 3:5, 10:12] = -np.inf
    v[9, 3, 9] = np.inf
    return v


NANBOX = ((0.05, 0.1, 0.1), (0.4, 0.9, 0.9))  # inside the NaN part, a voxel and more from its end


@pytest.mark.parametrize("box", [NANBOX, FULL])
def test_nan_and_infinite_voxels(gpu, box):
    v = special_volume()
    vrange = (0.0, float(np.nanmax(volume("g13"))))
    walk = reference("special", "rotA", box, "tf2", vol=v, vrange=vrange, iso=0.3 * vrange[1])
    ent, mx, mn = walk.records["entry"], walk.records["max"], walk.records["min"]
    if box == NANBOX:  # every sample is NaN: ENTRY hits with a NaN value, MAX and MIN miss
        assert walk.hits("entry").sum() >= 30 and np.isnan(ent["value"][walk.hits("entry")]).all()
        assert not walk.hits("max").any() and not walk.hits("min").any() and not walk.hits("iso").any()
    else:  # MAX and MIN pass over the NaN samples and report infinities where a ray meets one
        both = walk.hits("max") & walk.hits("entry")
        assert (np.isnan(ent["value"][both]) & ~np.isnan(mx["value"][both])).sum() >= 30
        assert not np.isnan(mx["value"][walk.hits("max")]).any()
        assert not np.isnan(mn["value"][walk.hits("min")]).any()
        assert (mx["value"] == np.inf).sum() >= 3 and (mn["value"] == -np.inf).sum() >= 1
        assert (walk.hits("entry") & ~walk.hits("max")).sum() >= 3  # rays of NaN samples only
    rp = hit_pass(W, H, v, synth.tf2(), 0.3 * vrange[1], box, vrange=vrange, narrow=0)
    try:
        # OPACITY where no sample is infinite only: the frame kernels' division by the range turns
        # an infinite density into NaN (texel 0) where the helper's IEEE quotient keeps it (the last
        # texel), in the composite frame as here (csrc/vr_kernels.hip div_by_range, mpr_strip)
        check_scene(rp, synth.camera("rotA").to_vr_camera(), walk,
                    KEYS if box == NANBOX else ("entry", "max", "min", "iso"))
    finally:
        rp.close()


def test_flat_range_reads_texel_zero(gpu):
    """vmin == vmax: the division gives NaN or an infinity and the lookup clamps to texel 0 (or
    the last one), as in the composite."""
    vol = np.full((9, 10, 11), 0.5, np.float32)
    tf = np.full(16, 0x00FFFFFF, np.uint32)
    tf[0] = 0x80FFFFFF  # texel 0: alpha 128/255; the others transparent
    walk = reference("const", "rotA", FULL, "texel0", vol=vol, tf=tf, iso=0.5)
    for t in THRESHOLDS[:2]:
        hit = walk.hits(okey(t))
        assert hit.sum() >= 30
        n = {0.25: 1, 0.9: 4}[t]  # 1 - (127/255)^n >= t
        assert np.array_equal(walk.records[okey(t)]["step"][hit],
                              walk.records["entry"]["step"][hit] + np.uint32(n - 1))
    rp = hit_pass(W, H, vol, tf, 0.5)
    try:
        assert rp.volume_info()[1] == (0.5, 0.5)
        check_scene(rp, synth.camera("rotA").to_vr_camera(), walk)
    finally:
        rp.close()


# ---- 6. cross-check with the shipped frame kernels ------------------------------------------------------
def test_hit_masks_equal_the_frames_own(gpu):
    volname, camname, box, tfname, w, h = PARITY[1]
    vol = volume(volname)
    rp = hit_pass(w, h, vol, synth.TFS[tfname](), isovalue(vol), box)
    try:
        cam = synth.camera(camname).to_vr_camera()
        # the composite's alpha over a clear colour of zeros is fl(A * A), A = 1 - T at the end of
        # the ray; A never falls along a ray, so OPACITY hits exactly where A ends at or above the
        # threshold, and squaring keeps the order wherever the squares differ
        p = P(ert_eps=0.0, clear_color=(0.0, 0.0, 0.0, 0.0))
        alpha = rp.render(cam, p, vr_amd.OUT_RGBA32F)[..., 3]
        for t in THRESHOLDS:
            sq = F(t) * F(t)
            mask = rp.hit_image(cam, p, vr_amd.HIT_OPACITY, t)["step"] != vr_amd.HIT_MISS_STEP
            decided = alpha != sq
            assert np.array_equal(mask[decided], (alpha > sq)[decided]), t
            if t == 1.0:  # fl(A * A) == 1 only for A == 1: there the equal squares decide too
                assert np.array_equal(mask, alpha == 1.0)
            assert 30 <= mask.sum() <= mask.size - 30
        # ISO: opaque where the surface is, the clear colour (alpha 0) elsewhere
        rp.render_mode_changed(vr_amd.MODE_ISO)
        p = P(clear_color=(0.5, 0.25, 0.125, 0.0))
        frame = rp.render(cam, p, vr_amd.OUT_RGBA32F)
        mask = rp.hit_image(cam, p, vr_amd.HIT_ISO)["step"] != vr_amd.HIT_MISS_STEP
        assert np.array_equal(mask, frame[..., 3] == 1.0) and 30 <= mask.sum() <= mask.size - 30
        assert np.all(frame[~mask] == np.array([0.5, 0.25, 0.125, 0.0], F))
        # MIP: some sample where the frame is not the clear colour (alpha 0)
        rp.render_mode_changed(vr_amd.MODE_MIP)
        tfo = (synth.TFS[tfname]() & np.uint32(0x00FFFFFF)) | np.uint32(0x80000000)
        rp.transfer_function_changed(tfo)
        frame = rp.render(cam, p, vr_amd.OUT_RGBA32F)
        mask = rp.hit_image(cam, p, vr_amd.HIT_MAX)["step"] != vr_amd.HIT_MISS_STEP
        assert np.array_equal(mask, frame[..., 3] != 0.0)
    finally:
        rp.close()


# ---- 7. state -----------------------------------------------------------------------------------------------
MODES = [vr_amd.MODE_COMPOSITE, vr_amd.MODE_MIP, vr_amd.MODE_MINIP, vr_amd.MODE_MEAN, vr_amd.MODE_ISO]


def test_hit_images_leave_every_frame_and_the_memory_report_alone(gpu):
    volname, camname, box, tfname, w, h = PARITY[1]
    vol = volume(volname)
    walk = reference(volname, camname, box, tfname, w, h)
    rp = hit_pass(w, h, vol, synth.TFS[tfname](), isovalue(vol), box)
    try:
        cam = synth.camera(camname).to_vr_camera()
        p = P(shading=1, skip_empty=1)
        before = {}
        for m in MODES:
            rp.render_mode_changed(m)
            before[m] = rp.render(cam, p, vr_amd.OUT_RGBA32F)
        rp.render_mode_changed(vr_amd.MODE_MEAN)
        state = (rp.render_mode, rp.isovalue, rp.volume_info())
        rep = rp.memory_report()
        rp.timing_enable(True)
        rp.timing_reset()
        n = 0
        for key in KEYS:
            kind, th = key_kind(key)
            check_records(rp.hit_image(cam, p, kind, th), walk.records[key], key)
            assert rp.last_kernel_name() in (NAME % ("float", kind, "false", 1), NAME % ("float", kind, "false", 2))
            rp.pick(cam, p, 5, 5, kind, th)
            n += 2
            ms, launches = rp.timing_read()
            assert launches == n and ms > 0.0
        rp.hit_count_work(cam, p, vr_amd.HIT_ISO)
        assert rp.last_kernel_name() == NAME % ("float", vr_amd.HIT_ISO, "true", 1)
        rp.timing_enable(False)
        assert rp.memory_report() == rep
        assert (rp.render_mode, rp.isovalue, rp.volume_info()) == state
        for m in MODES:
            rp.render_mode_changed(m)
            assert np.array_equal(rp.render(cam, p, vr_amd.OUT_RGBA32F).view(np.uint32),
                                  before[m].view(np.uint32)), m
            assert "hit_kernel" not in rp.last_kernel_name()
    finally:
        rp.close()


def test_device_output_on_another_stream(gpu):
    import torch
    volname, camname, box, tfname, w, h = PARITY[4]
    walk = reference(volname, camname, box, tfname, w, h)
    rp = hit_pass(w, h, volume(volname), synth.TFS[tfname](), isovalue(volume(volname)), box)
    try:
        cam = synth.camera(camname).to_vr_camera()
        stream = torch.cuda.Stream()
        outs = {}
        for key in KEYS:
            kind, th = key_kind(key)
            outs[key] = torch.zeros((h, w, 6), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            rp.hit_image_device(cam, P(), kind, outs[key].data_ptr(), th, stream=stream.cuda_stream)
        r = (13, 7, 20, 18)
        part = torch.zeros((18, 20, 6), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rp.hit_image_device(cam, P(), vr_amd.HIT_ISO, part.data_ptr(), rect=r, stream=stream.cuda_stream)
        stream.synchronize()
        for key in KEYS:
            got = outs[key].cpu().numpy().view(np.uint32)
            assert np.array_equal(got, words(walk.records[key])), key
        assert np.array_equal(part.cpu().numpy().view(np.uint32), words(walk.records["iso"][7:25, 13:33]))
    finally:
        rp.close()


def test_every_error_leaves_the_output_untouched(gpu):
    import torch
    w, h = 45, 35
    vol = volume("g20")
    rp = hit_pass(w, h, vol, synth.tf_color(), isovalue(vol))
    L = vr_amd.lib()
    try:
        cam = synth.camera("fill_oblique").to_vr_camera()
        good_p = P()
        host = np.full((h, w, 6), 0x77777777, np.uint32)
        dev = torch.full((h, w, 6), 0x77777777, dtype=torch.int32, device="cuda")
        one = vr_amd.vr_hit()
        one.step = 0x77
        st = vr_amd.vr_stats()
        st.rays = 0x77

        def calls(cam_, p_, req_, pick_at=(0, 0), skip_pick=False):
            cp = C.byref(cam_) if cam_ is not None else None
            pp = C.byref(p_) if p_ is not None else None
            rq = C.byref(req_) if req_ is not None else None
            rcs = [L.vr_hit_render(rp._ctx, cp, pp, rq, host.ctypes.data),
                   L.vr_hit_render_device(rp._ctx, cp, pp, rq, C.c_void_p(dev.data_ptr()), None),
                   L.vr_hit_count_work(rp._ctx, cp, pp, rq, C.byref(st))]
            if not skip_pick:
                rcs.append(L.vr_pick(rp._ctx, cp, pp, rq, pick_at[0], pick_at[1], C.byref(one)))
            return rcs

        R = vr_amd.hit_request
        bad_requests = [R(5), R(-1), R(1 << 20),
                        R(vr_amd.HIT_OPACITY, float("nan")), R(vr_amd.HIT_OPACITY, 0.0),
                        R(vr_amd.HIT_OPACITY, -0.1), R(vr_amd.HIT_OPACITY, 1.0000001),
                        R(vr_amd.HIT_OPACITY, float("inf"))]
        for req in bad_requests:
            assert calls(cam, good_p, req) == [-22] * 4, (req.kind, req.threshold)
        # the rectangle (vr_pick ignores it, use_rect included)
        bad_rects = [(0, 0, 0, 1), (0, 0, 1, 0), (45, 0, 1, 1), (0, 35, 1, 1), (44, 34, 2, 1), (44, 34, 1, 2),
                     (1, 0, 0xFFFFFFFF, 1), (0, 1, 1, 0xFFFFFFFF), (0, 0, 46, 35)]
        for r in bad_rects:
            assert calls(cam, good_p, R(vr_amd.HIT_MAX, rect=r), skip_pick=True) == [-22] * 3, r
        req = R(vr_amd.HIT_MAX)
        req.use_rect = 2
        assert calls(cam, good_p, req, skip_pick=True) == [-22] * 3
        assert L.vr_pick(rp._ctx, C.byref(cam), C.byref(good_p), C.byref(req), 3, 3, C.byref(one)) == 0
        one.step = 0x77
        # vr_pick's pixel
        for at in ((45, 0), (0, 35), (0xFFFFFFFF, 0xFFFFFFFF)):
            assert L.vr_pick(rp._ctx, C.byref(cam), C.byref(good_p), C.byref(R(vr_amd.HIT_MAX)), at[0], at[1],
                             C.byref(one)) == -22
        # NULL arguments, and what every mode refuses of vr_params and the camera
        good = R(vr_amd.HIT_ISO)
        assert calls(None, good_p, good) == [-22] * 4
        assert calls(cam, None, good) == [-22] * 4
        assert calls(cam, good_p, None) == [-22] * 4
        cp, pp, rq = C.byref(cam), C.byref(good_p), C.byref(good)
        assert L.vr_hit_render(rp._ctx, cp, pp, rq, None) == -22
        assert L.vr_hit_render_device(rp._ctx, cp, pp, rq, None, None) == -22
        assert L.vr_hit_count_work(rp._ctx, cp, pp, rq, None) == -22
        assert L.vr_pick(rp._ctx, cp, pp, rq, 0, 0, None) == -22
        for bad_p in (P(spec_power=-1), P(step=0.0), P(ray_dist=float("nan"))):
            assert calls(cam, bad_p, good) == [-22] * 4
        flat = synth.camera("fill_oblique").to_vr_camera()
        for i in range(16):
            flat.view[i] = 0.0  # proj * view is singular
        assert calls(flat, good_p, good) == [-22] * 4
        torch.cuda.synchronize()
        assert np.all(host == 0x77777777) and bool((dev == 0x77777777).all())
        assert one.step == 0x77 and st.rays == 0x77
        with pytest.raises(RuntimeError, match="threshold"):
            rp.hit_image(cam, good_p, vr_amd.HIT_OPACITY, 0.0)
        # and the context still works
        assert (rp.hit_image(cam, good_p, vr_amd.HIT_MAX)["step"] != vr_amd.HIT_MISS_STEP).sum() >= 30
    finally:
        rp.close()


@pytest.mark.parametrize("group", [dict(device_mask=1), dict(members=(0, 0, 0))])
def test_member_contexts_give_the_same_records(gpu, group):
    volname, camname, box, tfname, w, h = PARITY[4]
    vol = volume(volname)
    walk = reference(volname, camname, box, tfname, w, h)
    grp = vr_amd.OffscreenPass(w, h, exchange=vr_amd.EXCHANGE_COPY, **group)
    try:
        grp.volume_dataset_changed(synth.dataset(np.asarray(vol)))
        grp.transfer_function_changed(synth.TFS[tfname]())
        grp.slicing_changed(*box)
        grp.isovalue_changed(isovalue(vol))
        cam = synth.camera(camname).to_vr_camera()
        comp = grp.render(cam, P())
        check_scene(grp, cam, walk)
        at = np.argwhere(walk.hits("iso"))[0]
        got = grp.pick(cam, P(), int(at[1]), int(at[0]), vr_amd.HIT_ISO)
        check_records(np.asarray(got).reshape(1), walk.records["iso"][at[0], at[1]].reshape(1), "pick")
        assert "hit_kernel<float, 4, false" in grp.last_kernel_name()
        assert np.array_equal(grp.render(cam, P()).view(np.uint32), comp.view(np.uint32))
    finally:
        grp.close()
