"""GPU: multi-planar reformat (include/vr/vr_mpr.h, mpr_kernel).

The reference is tests/mpr_ref.py (the header's loop from the oracle's own filter and TF, pinned
by the closed forms of tests/test_mpr_cpu.py); images must equal it bit for bit in RGBA32F and
byte for byte in RGBA8, with equal rays, steps and samples.  Scenes: tests/mpr_scenes.py.  Images
are at most 48x36 with at most 9 samples, except the 200x150 ones of the size-independence test
(thin) and of the tile-order test (which needs no reference)."""
import ctypes as C

import numpy as np
import pytest

import mpr_ref
import synth
import vr_amd
from gpu_kit import c_plane
from mpr_scenes import (CLEAR, FULL, INSET, OPS, PITCH_IN, PITCH_OVER, SLICE, closed_form_expected,
                        closed_form_stack, closed_form_volume, face_size, make_plane, reference, volume)
from range_scenes import STORAGE, bits, int_volume

pytestmark = pytest.mark.gpu


def mpr_pass(vol, tf, box=FULL, w=32, h=24, vrange=None, **kw):
    knobs = {k: kw.pop(k) for k in list(kw) if k in vr_amd.KNOBS}
    rp = vr_amd.OffscreenPass(w, h, **kw)
    for k, v in knobs.items():
        rp.set_knob(k, v)
    ds = synth.dataset(np.asarray(vol))
    if vrange is not None:
        ds.vmin, ds.vmax = vrange
    rp.volume_dataset_changed(ds)
    rp.transfer_function_changed(tf)
    rp.slicing_changed(*box)
    return rp


def check_against(rp, pl, ref, st):
    cp = c_plane(pl)
    img = rp.render_mpr(cp, None, vr_amd.OUT_RGBA32F)
    assert img.shape == ref.shape
    assert np.array_equal(bits(img), bits(ref)), f"{(bits(img) != bits(ref)).sum()} words differ"
    img8 = rp.render_mpr(cp, None, vr_amd.OUT_RGBA8)
    assert np.array_equal(img8, vr_amd.unorm8(ref)), "RGBA8"
    w = rp.count_work_mpr(cp)
    assert w == dict(rays=st["rays"], steps=st["steps"], samples=st["samples"], shaded_samples=0,
                     skipped_samples=0), (w, st)


# ---- 1. parity ----------------------------------------------------------------------------------
PARITY = [  # volume, TF, plane, w, h, nsamples, op, box, oblique pitch
    ("g20", "tfc", 0, 32, 24, 5, "max", FULL, None),
    ("g20", "tf2", 1, 32, 24, 5, "min", INSET, None),
    ("g20", "tfc", 2, 45, 35, 5, "mean", SLICE, None),
    ("g20", "tfc", 2, 32, 24, 1, "max", FULL, None),
    ("g20", "tfc", "oblique", 32, 24, 5, "mean", FULL, PITCH_OVER),
    ("g20", "tf2", "oblique", 45, 35, 4, "max", SLICE, PITCH_OVER),
    ("g20", "tfc", "oblique", 45, 35, 7, "min", INSET, PITCH_IN),
    ("g20", "tfc", "oblique", 32, 24, 1, "mean", FULL, PITCH_IN),
    ("g13", "tfc", 0, 45, 35, 3, "mean", FULL, None),
    ("g13", "tf2", 1, 32, 24, 9, "max", SLICE, None),
    ("g13", "tfc", 2, 17, 3, 6, "min", INSET, None),
    ("g13", "tfc", 1, 1, 1, 5, "mean", FULL, None),
    ("g13", "tf2", "oblique", 32, 24, 8, "mean", INSET, PITCH_OVER),
    ("g13", "tfc", "oblique", 45, 35, 2, "min", FULL, PITCH_IN),
    ("g13", "tfc", "oblique", 1, 1, 1, "max", FULL, PITCH_OVER),
    ("blob16", "tfc", 0, 32, 24, 9, "min", INSET, None),
    ("blob16", "tf2", 1, 45, 35, 1, "min", FULL, None),
    ("blob16", "tfc", 2, 32, 24, 7, "max", SLICE, None),
    ("blob16", "tfc", 0, 17, 3, 2, "mean", SLICE, None),
    ("blob16", "tf2", "oblique", 32, 24, 9, "max", FULL, PITCH_OVER),
    ("blob16", "tfc", "oblique", 17, 3, 5, "mean", SLICE, PITCH_IN),
    ("blob16", "tfc", "oblique", 45, 35, 3, "mean", INSET, PITCH_OVER),
    # a slab whose centre plane lies outside the cube while some of its samples lie inside
    ("g20", "tfc", "outside", 17, 3, 9, "max", FULL, None),
    ("g13", "tf2", "outside", 32, 24, 9, "mean", FULL, None),
]


@pytest.mark.parametrize("volname,tfname,kind,w,h,ns,opname,box,pitch", PARITY)
def test_mpr_equals_reference(gpu, volname, tfname, kind, w, h, ns, opname, box, pitch):
    pitch = PITCH_OVER if pitch is None else pitch
    ref, st = reference(volname, tfname, kind, w, h, ns, opname, box, pitch)
    rp = mpr_pass(volume(volname), synth.TFS[tfname](), box)
    try:
        check_against(rp, make_plane(kind, w, h, ns, OPS[opname], pitch), ref, st)
    finally:
        rp.close()


@pytest.mark.parametrize("opname", ["mean", "max"])
def test_every_batch_tail(gpu, opname):
    """nsamples 1 through 9 in turn on one small image: every length of the last batch of four."""
    rp = mpr_pass(volume("g20"), synth.tf_color(), INSET)
    try:
        seen = set()
        for ns in range(1, 10):
            ref, st = reference("g20", "tfc", "oblique", 17, 3, ns, opname, INSET, PITCH_IN)
            check_against(rp, make_plane("oblique", 17, 3, ns, OPS[opname], PITCH_IN), ref, st)
            seen.add(ref.tobytes())
        assert len(seen) == 9
    finally:
        rp.close()


# ---- 2. closed forms, independent of the helper ----------------------------------------------------
@pytest.mark.parametrize("axis,k,half", [(2, 13, 0), (1, 5, 0), (0, 6, 0), (2, 13, 2), (1, 4, 1), (0, 8, 3)])
def test_closed_forms(gpu, axis, k, half):
    """test_mpr_cpu.py's closed forms on the GPU: texel-centre planes over the power-of-two volume
    show one voxel per pixel in the stated orientation, and slabs of spacing 1 / n reduce the
    voxel stack (np.fmax / np.fmin / a sequential f32 sum)."""
    vol = closed_form_volume()
    lo, hi = float(vol.min()), float(vol.max())
    tf = synth.tf_color()
    w, h = face_size(vol.shape, axis)
    n = vol.shape[2 - axis]
    stack = closed_form_stack(vol, axis, k, half)
    assert np.array_equal(stack[half], closed_form_expected(vol, axis, k))
    ns = 2 * half + 1
    acc = np.zeros((h, w), np.float32)
    for layer in stack:
        acc = acc + layer
    want = {"max": np.fmax.reduce(stack), "min": np.fmin.reduce(stack), "mean": acc / np.float32(ns)}
    rp = mpr_pass(vol, tf, narrow=0)
    try:
        for opname, op in OPS.items():
            pl = vr_amd.axis_plane(axis, (k + 0.5) / n, w, h, ns, 1.0 / n if half else 0.0, op)
            img = rp.render_mpr(pl)
            exp = np.array([[mpr_ref.pixel_of(want[opname][py, px], lo, hi, tf) for px in range(w)]
                            for py in range(h)])
            assert np.array_equal(bits(img), bits(exp)), opname
            st = rp.count_work_mpr(pl)
            assert (st["rays"], st["steps"], st["samples"]) == (w * h, w * h * ns, w * h * ns)
    finally:
        rp.close()


# ---- 3. storage types --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,signed,knobs,storage", STORAGE)
def test_storage_types(gpu, dtype, signed, knobs, storage):
    vf = int_volume(signed)
    name = "int_s" if signed else "int_u"
    rp = mpr_pass(vf.astype(dtype), synth.tf_color(), INSET, **knobs)
    try:
        assert rp.volume_info()[2] == storage
        for kind, ns, opname in ((1, 1, "max"), ("oblique", 5, "mean"), (0, 5, "min")):
            ref, st = reference(name, "tfc", kind, 32, 24, ns, opname, INSET, vol=vf)
            check_against(rp, make_plane(kind, 32, 24, ns, OPS[opname]), ref, st)
    finally:
        rp.close()


# ---- 4. NaN ---------------------------------------------------------------------------------------------
def test_nan_voxel_on_the_plane(gpu):
    """MAX and MIN ignore a NaN sample, MEAN propagates it -- also on a thin slice, where the
    three operators differ in nothing else."""
    vol = np.array(volume("g20"))
    vol[8, 9, 10] = np.nan  # between the texel layers the axial plane at 0.37 of 22 slices reads
    lo, hi = float(np.nanmin(vol)), float(np.nanmax(vol))
    rp = mpr_pass(vol, synth.tf_color(), vrange=(lo, hi))
    try:
        for ns in (1, 5):
            imgs = {}
            for opname in OPS:
                ref, st = reference("g20_nan", "tfc", 2, 32, 24, ns, opname, vol=vol)
                check_against(rp, make_plane(2, 32, 24, ns, OPS[opname]), ref, st)
                imgs[opname] = ref
            clean = reference("g20", "tfc", 2, 32, 24, ns, "mean")[0]
            assert not np.array_equal(bits(imgs["mean"]), bits(clean))
            # (thin: a NaN mean and the maximum's -inf both read texel 0, the minimum's +inf the last)
            other = "max" if ns > 1 else "min"
            assert not np.array_equal(bits(imgs["mean"]), bits(imgs[other]))
    finally:
        rp.close()


# ---- 5. the image size is the plane's ---------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(45, 35), (200, 150)])
def test_image_size_is_independent_of_the_framebuffer(gpu, w, h):
    import torch
    ref, st = reference("g20", "tfc", "oblique", w, h, 1, "max", FULL, 1.6 / w)
    pl = make_plane("oblique", w, h, 1, OPS["max"], 1.6 / w)
    rp = mpr_pass(volume("g20"), synth.tf_color(), w=32, h=24)
    try:
        assert rp.size == (32, 24)
        check_against(rp, pl, ref, st)
        cp = c_plane(pl)
        side = torch.cuda.Stream()
        for fmt, tdt, shape in ((vr_amd.OUT_RGBA32F, torch.float32, (h, w, 4)),
                                (vr_amd.OUT_RGBA8, torch.uint8, (h, w, 4))):
            host = rp.render_mpr(cp, None, fmt)
            for stream in (0, side.cuda_stream):
                dev = torch.zeros(shape, dtype=tdt, device="cuda")
                torch.cuda.synchronize()
                rp.render_mpr_device(cp, None, dev.data_ptr(), fmt, stream)
                torch.cuda.synchronize()
                assert np.array_equal(bits(dev.cpu().numpy()), bits(host)), (fmt, stream)
        assert rp.size == (32, 24)
    finally:
        rp.close()


@pytest.mark.parametrize("w,h", [(45, 35), (200, 150), (1, 1)])
def test_tile_orders_render_the_same_bytes(gpu, w, h):
    """Raster tiles (thin slices' own order) and the XCD-interleaved super-tiles (slabs' own), each
    forced by the tile-order knob on images that are no whole number of super-tiles: the same
    bytes and counters, every tile rendered exactly once (the image starts as a sentinel)."""
    import torch
    rp = mpr_pass(volume("g20"), synth.tf_color(), INSET)
    try:
        for ns, opname in ((1, "max"), (6, "mean")):
            cp = c_plane(make_plane("oblique", w, h, ns, OPS[opname], 1.6 / w))
            own = rp.render_mpr(cp)
            work = rp.count_work_mpr(cp)
            for order in (1, 3):
                with rp.knobs(tile_order=order):
                    dev = torch.full((h, w, 4), -7.0, dtype=torch.float32, device="cuda")
                    torch.cuda.synchronize()
                    rp.render_mpr_device(cp, None, dev.data_ptr(), vr_amd.OUT_RGBA32F)
                    torch.cuda.synchronize()
                    assert np.array_equal(bits(dev.cpu().numpy()), bits(own)), (ns, order)
                    assert rp.count_work_mpr(cp) == work
    finally:
        rp.close()


# ---- 6. state ----------------------------------------------------------------------------------------------
def test_mpr_leaves_the_context_as_it_was(gpu):
    """composite frame, MPR, composite frame: identical frames; MPR bytes depend on neither the
    render mode nor the isovalue and leave both; no derived structure is built, evicted or
    downgraded; the timing brackets the MPR kernel and the last kernel name is its own."""
    vol, tf = volume("g20"), synth.tf_color()
    cam = synth.camera("fill_oblique").to_vr_camera()
    pl = c_plane(make_plane("oblique", 45, 35, 5, OPS["mean"], PITCH_OVER))
    thin = c_plane(make_plane(1, 17, 3, 1, OPS["min"]))
    ref = reference("g20", "tfc", "oblique", 45, 35, 5, "mean")[0]
    rp = mpr_pass(vol, tf)
    try:
        p = vr_amd.default_params(shading=1)
        before = rp.render(cam, p)
        frame_kernel = rp.last_kernel_name()
        assert "march" in frame_kernel
        rep = rp.memory_report()
        base = rp.render_mpr(pl)
        assert np.array_equal(bits(base), bits(ref))
        assert rp.last_kernel_name() == "void vr::(anonymous namespace)::mpr_kernel<float, 2, false>(vr::MprArgs)"
        rp.render_mpr(thin)
        assert rp.last_kernel_name() == "void vr::(anonymous namespace)::mpr_kernel<float, 3, false>(vr::MprArgs)"
        rp.count_work_mpr(pl)
        assert rp.last_kernel_name() == "void vr::(anonymous namespace)::mpr_kernel<float, 0, true>(vr::MprArgs)"
        assert np.array_equal(bits(rp.render(cam, p)), bits(before))
        assert rp.last_kernel_name() == frame_kernel
        for mode, iso in ((vr_amd.MODE_MIP, 0.0), (vr_amd.MODE_ISO, 0.4), (vr_amd.MODE_MEAN, -1.0)):
            rp.render_mode_changed(mode)
            rp.isovalue_changed(iso)
            assert np.array_equal(bits(rp.render_mpr(pl)), bits(base))
            assert rp.render_mode == mode and rp.isovalue == pytest.approx(iso)
        # every vr_params field but clear_color is ignored (and still validated)
        odd = vr_amd.default_params(step=0.1, ray_dist=0.3, shading=1, ert_eps=0.5, skip_empty=1,
                                    tile_order=2, wave_shape=1, frames_in_flight=3)
        assert np.array_equal(bits(rp.render_mpr(pl, odd)), bits(base))
        red = rp.render_mpr(pl, vr_amd.default_params(clear_color=(0.5, 0.0, 0.25, 0.75)))
        assert not np.array_equal(bits(red), bits(base))
        outside = np.all(base == CLEAR, axis=-1)
        assert outside.any() and np.all(red[outside] == np.float32([0.5, 0.0, 0.25, 0.75]))
        rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
        rp.isovalue_changed(0.0)
        assert np.array_equal(bits(rp.render(cam, p)), bits(before))
        after = rp.memory_report()
        for k in ("builds", "evictions", "downgrades", "derived_bytes", "field_bytes", "skip_bytes"):
            assert after[k] == rep[k], k
        # timing: one launch per image, none for a count
        rp.timing_enable(True)
        rp.timing_reset()
        rp.render_mpr(pl)
        rp.render_mpr(thin, None, vr_amd.OUT_RGBA8)
        ms, n = rp.timing_read()
        assert n == 2 and ms > 0.0
        rp.timing_enable(False)
    finally:
        rp.close()


def test_tf_slicing_and_volume_changes_take_effect(gpu):
    w, h, ns = 32, 24, 5
    pl = make_plane("oblique", w, h, ns, OPS["max"], PITCH_OVER)
    rp = mpr_pass(volume("g20"), synth.tf_color())
    try:
        check_against(rp, pl, *reference("g20", "tfc", "oblique", w, h, ns, "max"))
        rp.transfer_function_changed(synth.tf2())
        check_against(rp, pl, *reference("g20", "tf2", "oblique", w, h, ns, "max"))
        rp.slicing_changed(*SLICE)
        check_against(rp, pl, *reference("g20", "tf2", "oblique", w, h, ns, "max", SLICE))
        rp.volume_dataset_changed(synth.dataset(np.asarray(volume("g13"))))
        check_against(rp, pl, *reference("g13", "tf2", "oblique", w, h, ns, "max", SLICE))
    finally:
        rp.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------
def test_every_einval_leaves_the_output_untouched(gpu):
    import torch
    L = vr_amd.lib()
    w, h = 17, 3
    good = make_plane("oblique", w, h, 5, OPS["mean"], PITCH_IN)
    ref, st = reference("g20", "tfc", "oblique", w, h, 5, "mean", FULL, PITCH_IN)
    rp = mpr_pass(volume("g20"), synth.tf_color())
    try:
        p = vr_amd.default_params()
        nan, inf = float("nan"), float("inf")
        bad_planes = []
        for field in ("origin", "du", "dv", "dn"):
            for a, x in ((0, nan), (1, inf), (2, -inf)):
                pl = c_plane(good)
                getattr(pl, field)[a] = x
                bad_planes.append(pl)
        for field, x in (("width", 0), ("height", 0), ("nsamples", 0),
                         ("nsamples", vr_amd.MPR_MAX_SAMPLES + 1), ("op", 3), ("op", -1)):
            pl = c_plane(good)
            setattr(pl, field, x)
            bad_planes.append(pl)
        host = np.full((h, w, 4), 7.0, np.float32)
        dev = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda")
        stats = vr_amd.vr_stats()
        stats.rays = 99

        def refused(plane, params, fmt=vr_amd.OUT_RGBA32F, out=True):
            pp = C.byref(plane) if plane is not None else None
            qq = C.byref(params) if params is not None else None
            assert L.vr_mpr_render(rp._ctx, pp, qq, host.ctypes.data if out else None, fmt) == -22
            assert L.vr_mpr_render_device(rp._ctx, pp, qq, C.c_void_p(dev.data_ptr()) if out else None,
                                          fmt, None) == -22
            if out and fmt == vr_amd.OUT_RGBA32F:
                assert L.vr_mpr_count_work(rp._ctx, pp, qq, C.byref(stats)) == -22
            assert rp._ctx and L.vr_last_error(rp._ctx)

        for pl in bad_planes:
            refused(pl, p)
        ok = c_plane(good)
        refused(None, p)
        refused(ok, None)
        refused(ok, p, out=False)
        assert L.vr_mpr_count_work(rp._ctx, C.byref(ok), C.byref(p), None) == -22
        for fmt in (2, -1):
            refused(ok, p, fmt)
        for bad in (dict(step=0.0), dict(step=nan), dict(ray_dist=-1.0), dict(spec_power=-1),
                    dict(frames_in_flight=17), dict(exact_gradient=2), dict(depth_zero_to_one=2)):
            refused(ok, vr_amd.default_params(**bad))
        with pytest.raises(RuntimeError, match="nsamples"):
            rp.render_mpr(bad_planes[-3])
        torch.cuda.synchronize()
        assert np.all(host == 7.0) and bool((dev == 7.0).all()) and stats.rays == 99
        # the largest sample count is accepted, and the context still renders
        big = c_plane(good)
        big.nsamples = vr_amd.MPR_MAX_SAMPLES
        big.width = big.height = 1
        assert rp.count_work_mpr(big)["rays"] == 1
        check_against(rp, good, ref, st)
    finally:
        rp.close()


# ---- 8. multi-device contexts ---------------------------------------------------------------------------------
def test_mask_context_equals_the_single_context(gpu):
    import torch
    w, h = 45, 35
    pl = make_plane("oblique", w, h, 5, OPS["mean"], PITCH_OVER)
    ref, st = reference("g20", "tfc", "oblique", w, h, 5, "mean", SLICE)
    one = mpr_pass(volume("g20"), synth.tf_color(), SLICE)
    grp = mpr_pass(volume("g20"), synth.tf_color(), SLICE, device_mask=1)
    try:
        for rp in (one, grp):
            check_against(rp, pl, ref, st)
        dev = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        grp.render_mpr_device(c_plane(pl), None, dev.data_ptr(), vr_amd.OUT_RGBA8)
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy().view(np.uint8).reshape(h, w, 4), vr_amd.unorm8(ref))
        assert "mpr_kernel<float, 2, false>" in grp.last_kernel_name()
        # frames of the group are what they were
        cam = synth.camera("fill_oblique").to_vr_camera()
        a, b = one.render(cam), grp.render(cam)
        assert np.array_equal(bits(a), bits(b))
    finally:
        one.close()
        grp.close()
