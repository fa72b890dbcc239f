"""GPU: the value histogram and the value-window setter (include/vr/vr_hist.h, hist_kernel).

The reference is tests/hist_ref.py (pinned by the closed forms of tests/test_hist_cpu.py): bins
and info must equal it exactly, on the uploaded array or on what read_volume() returns.  The
volumes are small (at most 96x80x72, and 200x160x140 bytes where the workgroups must walk more
than one brick group); every storage type and brick layout, partial bricks, boxes
and both kernel forms (knob hist_agg) are covered.  The window tests compare a context whose window
was set by value_range_changed with one that was uploaded with that window, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import hist_ref
import synth
import vr_amd
from mpr_scenes import OPS, make_plane
from range_scenes import STORAGE, bits, int_volume, volume

pytestmark = pytest.mark.gpu
F = np.float32
HIST_KERNEL = "void vr::(anonymous namespace)::hist_kernel<%s, %s>(vr::HistArgs)"


def hist_pass(vol, vrange=None, w=32, h=24, tf=None, **kw):
    knobs = {k: kw.pop(k) for k in list(kw) if k in vr_amd.KNOBS}
    rp = vr_amd.OffscreenPass(w, h, **kw)
    for k, v in knobs.items():
        rp.set_knob(k, v)
    vol = np.asarray(vol)
    v = vol.astype(np.float32)
    lo, hi = (float(np.nanmin(v)), float(np.nanmax(v))) if vrange is None else vrange
    rp.volume_dataset_changed(vr_amd.Dataset((vol.shape[2], vol.shape[1], vol.shape[0]), lo, hi, vol))
    rp.transfer_function_changed(synth.tf_color() if tf is None else tf)
    return rp


def check(rp, vol, lo, hi, nbins, box=None):
    """Both kernel forms against the reference; returns the bins."""
    ref_bins, ref_info = hist_ref.histogram(vol, lo, hi, nbins, box)
    for agg in (0, 1):
        rp.set_knob("hist_agg", agg)
        bins, info = rp.histogram(nbins, lo, hi, box)
        assert bins.dtype == np.uint64 and bins.shape == (nbins,)
        assert np.array_equal(bins, ref_bins), (agg, np.nonzero(bins != ref_bins)[0][:8])
        assert hist_ref.same_info(info, ref_info), (agg, info, ref_info)
    rp.set_knob("hist_agg", -1)
    return ref_bins


# ---- 1. every storage type and layout -----------------------------------------------------------
@pytest.mark.parametrize("dtype,signed,knobs,storage", STORAGE)
def test_storage_types(gpu, dtype, signed, knobs, storage):
    vf = int_volume(signed)
    assert vf.shape == (22, 18, 20)
    rp = hist_pass(vf.astype(dtype), **knobs)
    try:
        assert rp.volume_info()[2] == storage
        assert np.array_equal(rp.read_volume(), vf)
        for lo, hi, nbins in ((float(vf.min()), float(vf.max()), 256), (-60, 60, 7), (0, 1, 1),
                              (-1000, 1000, 4096)):
            check(rp, vf, lo, hi, nbins)
        # lo / hi default to the context's window
        bins, info = rp.histogram(16)
        ref_bins, ref_info = hist_ref.histogram(vf, vf.min(), vf.max(), 16)
        assert np.array_equal(bins, ref_bins) and hist_ref.same_info(info, ref_info)
    finally:
        rp.close()


# ---- 2. edge values, special values ---------------------------------------------------------------
def test_edge_values(gpu):
    lo, hi, nbins = -1.3, 2.7, 1000
    v = hist_ref.edge_values(lo, hi, nbins)
    assert v.size == 2002 == 13 * 11 * 14
    vol = np.random.default_rng(5).permutation(v).reshape(14, 11, 13)
    rp = hist_pass(vol, narrow=0)
    try:
        assert np.array_equal(bits(rp.read_volume()), bits(vol))
        for agg in (0, 1):
            rp.set_knob("hist_agg", agg)
            bins, info = rp.histogram(nbins, lo, hi)
            assert np.all(bins == 2) and info["below"] == 1 and info["above"] == 1 and info["nan"] == 0
            assert info["voxels"] == 2002
        check(rp, vol, lo, hi, nbins)
        check(rp, vol, 1.0, float(np.nextafter(F(1), F(2))), 4)  # duplicate edges
    finally:
        rp.close()


def test_special_values(gpu):
    den = np.finfo(np.float32).smallest_subnormal
    vol = np.random.default_rng(9).random((7, 8, 9), dtype=np.float32) * F(0.25) + F(0.5)
    vol[0, 0, 0] = np.nan
    vol[6, 7, 8] = np.nan
    vol[3, 4, 5] = np.inf
    vol[1, 7, 0] = -np.inf
    vol[2, 2, 8] = -0.0
    vol[5, 0, 3] = den
    vol[4, 3, 2] = -den
    vol[6, 0, 0] = 1.0
    rp = hist_pass(vol, vrange=(0.0, 1.0), narrow=0)
    try:
        assert np.array_equal(bits(rp.read_volume()), bits(vol))
        for agg in (0, 1):
            rp.set_knob("hist_agg", agg)
            bins, info = rp.histogram(2, 0.0, 1.0)
            n = vol.size
            assert (info["voxels"], info["nan"], info["above"], info["below"]) == (n, 2, 1, 2)
            assert bins[0] == 2 and bins[1] == n - 2 - 1 - 2 - 2  # -0.0 and the denormal; the rest >= 0.5
            assert info["vmin"] == -np.inf and info["vmax"] == np.inf
        check(rp, vol, 0.0, 1.0, 2)
        check(rp, vol, -1.0, 1.0, 4096)
        # a box without the infinities: finite extremes; a box of NaN alone: none
        check(rp, vol, 0.0, 1.0, 8, ((0, 0, 2), (9, 7, 3)))
        bins, info = rp.histogram(8, 0.0, 1.0, ((0, 0, 0), (1, 1, 1)))
        assert not bins.any() and info["nan"] == 1 == info["voxels"]
        assert info["vmin"] == np.inf and info["vmax"] == -np.inf
    finally:
        rp.close()


# ---- 3. shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (8, 8, 8), (9, 8, 7), (65, 3, 5), (7, 8, 8)])  # nx, ny, nz
@pytest.mark.parametrize("kind", ["u8_plain", "u8_quad", "f32"])
def test_shapes(gpu, shape, kind):
    nx, ny, nz = shape
    rng = np.random.default_rng(nx * 100 + ny * 10 + nz)
    if kind == "f32":
        vol = rng.random((nz, ny, nx), dtype=np.float32)
        knobs = dict(narrow=0)
        cases = ((0.0, 1.0, 64), (0.25, 0.75, 5))
    else:
        vol = rng.integers(0, 256, size=(nz, ny, nx), dtype=np.uint8)
        knobs = dict(u8_layout=0 if kind == "u8_plain" else 1)
        cases = ((0, 256, 256), (10, 200, 7))
    rp = hist_pass(vol, vrange=(0.0, 255.0), **knobs)
    try:
        assert rp.volume_info()[2] == (4 if kind == "f32" else 0)
        for lo, hi, nbins in cases:
            bins = check(rp, vol, lo, hi, nbins)
        if kind != "f32":
            assert np.array_equal(check(rp, vol, 0, 256, 256),
                                  np.bincount(vol.ravel(), minlength=256).astype(np.uint64))
        assert bins.sum() <= nx * ny * nz
    finally:
        rp.close()


# ---- 4. the hot bin, many workgroups ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32])
def test_constant_volume(gpu, dtype):
    vol = np.full((40, 40, 40), 37, dtype)
    rp = hist_pass(vol, vrange=(0.0, 100.0), narrow=0)
    try:
        for agg in (0, 1):
            rp.set_knob("hist_agg", agg)
            bins, info = rp.histogram(100, 0.0, 100.0)
            assert bins[37] == 64000 and bins.sum() == 64000 == info["voxels"]
            assert info["vmin"] == 37 == info["vmax"]
    finally:
        rp.close()


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_generated_volume_against_the_readback(gpu, dtype):
    rp = vr_amd.OffscreenPass(32, 24)
    try:
        lo, hi = rp.generate_volume((96, 80, 72), dtype)
        vol = rp.read_volume()
        assert vol.shape == (72, 80, 96)
        bins = check(rp, vol, lo, hi, 256)
        assert bins.sum() == vol.size and np.count_nonzero(bins) > 50
        check(rp, vol, lo, hi, 4096)
        check(rp, vol, 0.25 * hi, 0.5 * hi, 33, ((5, 0, 7), (96, 41, 70)))
        _, info = rp.histogram(8)  # the window generate_volume set is the data's range
        assert (info["vmin"], info["vmax"]) == (F(lo), F(hi)) and info["below"] == 0 == info["above"]
    finally:
        rp.close()


@pytest.mark.parametrize("dtype,dims,knobs", [(np.float32, (130, 104, 97), {}),
                                              (np.uint8, (200, 160, 140), dict(u8_layout=0))])
def test_more_bricks_than_workgroups(gpu, dtype, dims, knobs):
    """130x104x97 f32 voxels are 3094 bricks, beyond the 2048 workgroups of a launch; 200x160x140
    plain 8-bit voxels are 11340 bricks, beyond the 4 x 2048 the code path's waves take at once:
    every workgroup walks more than one brick (group)."""
    rp = vr_amd.OffscreenPass(32, 24)
    try:
        for k, v in knobs.items():
            rp.set_knob(k, v)
        lo, hi = rp.generate_volume(dims, dtype)
        vol = rp.read_volume()
        assert check(rp, vol, lo, hi, 512).sum() == vol.size
        check(rp, vol, lo, hi, 64, ((1, 1, 1), (dims[0] - 1, dims[1] - 1, dims[2] - 1)))
    finally:
        rp.close()


# ---- 5. boxes ---------------------------------------------------------------------------------------
BOXES = [((0, 0, 0), (20, 18, 22)), ((7, 9, 11), (8, 10, 12)), ((3, 8, 0), (17, 9, 22)),
         ((7, 7, 7), (12, 13, 14)),   # inside one 8^3 brick (padded 9 .. 15)
         ((0, 0, 0), (6, 6, 6)),      # ends on a brick face (padded index 8)
         ((6, 6, 6), (14, 14, 14)),   # starts on one, ends on the next
         ((19, 17, 21), (20, 18, 22))]


@pytest.mark.parametrize("dtype,knobs", [(np.float32, dict(narrow=0)), (np.int16, {}),
                                         (np.uint8, dict(u8_layout=0)), (np.uint8, dict(u8_layout=1))])
def test_boxes(gpu, dtype, knobs):
    vf = int_volume(False)
    rp = hist_pass(vf.astype(dtype), **knobs)
    try:
        whole, _ = rp.histogram(121, 0, 121)
        for box in BOXES:
            bins = check(rp, vf, 0, 121, 121, box)
            n = np.prod(np.subtract(box[1], box[0]))
            assert bins.sum() == n
            if box == BOXES[0]:
                assert np.array_equal(bins, whole)
            if n == 1:
                x, y, z = box[0]
                assert bins[int(vf[z, y, x])] == 1
    finally:
        rp.close()


def test_refused_requests_leave_the_outputs_untouched(gpu):
    L = vr_amd.lib()
    vf = int_volume(False)
    rp = hist_pass(vf)
    try:
        bins = np.full(8, 77, np.uint64)
        bp = bins.ctypes.data_as(C.POINTER(C.c_uint64))
        info = vr_amd.vr_hist_info()
        info.voxels = 77

        def request(lo=0.0, hi=1.0, nbins=8, use_box=0, bmin=(0, 0, 0), bmax=(1, 1, 1)):
            r = vr_amd.vr_hist_request()
            r.lo, r.hi, r.nbins, r.use_box = lo, hi, nbins, use_box
            for a in range(3):
                r.box_min[a], r.box_max[a] = bmin[a], bmax[a]
            return r

        nan, inf = float("nan"), float("inf")
        bad = [request(lo=nan), request(hi=inf), request(lo=-inf), request(lo=1.0), request(lo=2.0),
               request(nbins=0), request(nbins=vr_amd.HIST_MAX_BINS + 1), request(use_box=2),
               request(use_box=1, bmin=(3, 3, 3), bmax=(3, 4, 4)),     # empty
               request(use_box=1, bmin=(5, 3, 3), bmax=(4, 4, 4)),     # reversed
               request(use_box=1, bmax=(21, 1, 1)), request(use_box=1, bmax=(1, 19, 1)),
               request(use_box=1, bmax=(1, 1, 23)),                    # beyond the volume
               request(use_box=1, bmin=(0xFFFFFFFF, 0, 0), bmax=(0, 1, 1))]
        for r in bad:
            assert L.vr_histogram(rp._ctx, C.byref(r), bp, C.byref(info)) == -22
            assert L.vr_last_error(rp._ctx)
        ok = request()
        assert L.vr_histogram(rp._ctx, None, bp, C.byref(info)) == -22
        assert L.vr_histogram(rp._ctx, C.byref(ok), None, C.byref(info)) == -22
        assert L.vr_histogram(rp._ctx, C.byref(ok), bp, None) == -22
        assert np.all(bins == 77) and info.voxels == 77
        with pytest.raises(RuntimeError, match="-22"):
            rp.histogram(8, 0, 1, ((0, 0, 0), (21, 1, 1)))
        # a box is ignored unless use_box is set, and the largest bin count is accepted
        assert L.vr_histogram(rp._ctx, C.byref(request(bmax=(99, 99, 99))), bp, C.byref(info)) == 0
        assert info.voxels == vf.size
        check(rp, vf, 0, 121, vr_amd.HIST_MAX_BINS)
    finally:
        rp.close()


# ---- 6. state -----------------------------------------------------------------------------------------
def test_histogram_leaves_the_context_as_it_was(gpu):
    vol = volume("g20")
    cam = synth.camera("fill_oblique").to_vr_camera()
    pl = make_plane("oblique", 45, 35, 5, OPS["mean"])
    cp = vr_amd.mpr_plane(pl["origin"], pl["du"], pl["dv"], pl["dn"], 45, 35, 5, pl["op"])
    rp = hist_pass(vol, tf=synth.tf_band())
    try:
        p = vr_amd.default_params(shading=1, skip_empty=1)
        rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
        rp.isovalue_changed(0.3)
        rp.slicing_changed((0.1, 0.0, 0.05), (0.9, 1.0, 0.95))
        frame = rp.render(cam, p)
        frame_kernel = rp.last_kernel_name()
        image = rp.render_mpr(cp)
        rep = rp.memory_report()
        info0 = rp.volume_info()
        rp.timing_enable(True)
        rp.timing_reset()
        check(rp, vol, float(vol.min()), float(vol.max()), 256)          # two launches
        rp.set_knob("hist_agg", 0)
        rp.histogram(64, box=((1, 2, 3), (9, 9, 9)))                     # a third
        assert rp.last_kernel_name() == HIST_KERNEL % ("float", "false")
        rp.set_knob("hist_agg", 1)
        rp.histogram(64)
        assert rp.last_kernel_name() == HIST_KERNEL % ("float", "true")
        rp.set_knob("hist_agg", -1)
        ms, n = rp.timing_read()
        assert n == 4 and ms > 0.0
        rp.timing_enable(False)
        after = rp.memory_report()
        for k in ("builds", "evictions", "downgrades", "derived_bytes"):
            assert after[k] == rep[k], k
        assert rp.volume_info() == info0 and rp.render_mode == vr_amd.MODE_COMPOSITE
        assert rp.isovalue == pytest.approx(0.3)
        assert np.array_equal(bits(rp.render_mpr(cp)), bits(image))
        assert np.array_equal(bits(rp.render(cam, p)), bits(frame))
        assert rp.last_kernel_name() == frame_kernel
    finally:
        rp.close()


def test_member_context_gives_the_same_counts(gpu):
    vf = int_volume(True)
    grp = hist_pass(vf.astype(np.int16), members=[0, 0])
    try:
        check(grp, vf, -60, 60, 7)
        check(grp, vf, -1000, 1000, 4096, ((3, 8, 0), (17, 9, 22)))
        assert "hist_kernel<short" in grp.last_kernel_name()
    finally:
        grp.close()


# ---- 7. the value window ------------------------------------------------------------------------------------
def _window_frames(rp, cam, cp):
    """The frames the window enters, as bytes: composite with and without skipping, shaded
    composite, MIP, MEAN, ISO and an MPR image."""
    out = {}
    rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
    for skip in (0, 1):
        out["composite", skip] = rp.render(cam, vr_amd.default_params(skip_empty=skip))
    out["shaded"] = rp.render(cam, vr_amd.default_params(shading=1, skip_empty=1))
    for name, mode in (("mip", vr_amd.MODE_MIP), ("mean", vr_amd.MODE_MEAN), ("iso", vr_amd.MODE_ISO)):
        rp.render_mode_changed(mode)
        out[name] = rp.render(cam, vr_amd.default_params(skip_empty=1))
    rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
    out["mpr"] = rp.render_mpr(cp)
    return {k: bits(v).tobytes() for k, v in out.items()}


@pytest.mark.parametrize("members", [None, [0, 0]])
@pytest.mark.parametrize("window", ["narrow", "wide", "point"])
def test_value_range_changed_equals_an_upload_with_that_window(gpu, members, window):
    vol = volume("g20")
    v0, v1 = float(vol.min()), float(vol.max())
    w0, w1 = {"narrow": (v0 + 0.3 * (v1 - v0), v0 + 0.6 * (v1 - v0)),
              "wide": (v0 - 1.0, v1 + 2.0), "point": (0.5 * (v0 + v1),) * 2}[window]
    cam = synth.camera("fill_oblique").to_vr_camera()
    pl = make_plane("oblique", 32, 24, 5, OPS["max"])
    cp = vr_amd.mpr_plane(pl["origin"], pl["du"], pl["dv"], pl["dn"], 32, 24, 5, pl["op"])
    kw = {} if members is None else dict(members=members)
    tf = synth.tf_band()
    a = hist_pass(vol, (v0, v1), tf=tf, **kw)
    b = hist_pass(vol, (w0, w1), tf=tf, **kw)
    try:
        for rp in (a, b):
            rp.isovalue_changed(0.5 * (w0 + w1) if w0 != w1 else v0 + 0.4 * (v1 - v0))
        # A builds its distance field for the old window first: a stale one would show below
        old = a.render(cam, vr_amd.default_params(skip_empty=1))
        builds = a.memory_report()["builds"]
        a.value_range_changed(w0, w1)
        assert a.volume_info()[1] == (float(F(w0)), float(F(w1))) == b.volume_info()[1]
        fa, fb = _window_frames(a, cam, cp), _window_frames(b, cam, cp)
        for k in fb:
            assert fa[k] == fb[k], k
        assert fa["composite", 0] == fa["composite", 1]
        assert a.memory_report()["builds"] > builds  # the distance field was built again
        if window == "narrow":
            assert fa["composite", 1] != bits(old).tobytes()
        # ... and back: the first window's frame again, and the voxels never moved
        a.value_range_changed(v0, v1)
        assert np.array_equal(bits(a.render(cam, vr_amd.default_params(skip_empty=1))), bits(old))
        assert np.array_equal(bits(a.read_volume()), bits(vol))
    finally:
        a.close()
        b.close()


def test_percentile_window_from_the_histogram(gpu):
    """The use the calls are for: histogram over the exact range, a percentile window, applied."""
    vol = volume("g20")
    rp = hist_pass(vol, vrange=(-5.0, 5.0))
    try:
        _, info = rp.histogram(1, -5.0, 5.0)
        lo, hi = info["vmin"], info["vmax"]
        assert (lo, hi) == (vol.min(), vol.max())
        bins, info = rp.histogram(4096, lo, hi)
        assert info["below"] == 0 == info["above"] and bins.sum() == vol.size
        w = vr_amd.hist_window(bins, lo, hi, 0.05, 0.95)
        assert np.array_equal(bits(F(w)), bits(F(hist_ref.window(bins, lo, hi, 0.05, 0.95))))
        assert lo < w[0] < w[1] < hi
        inside = np.count_nonzero((vol >= w[0]) & (vol < w[1]))
        assert 0.88 * vol.size <= inside <= 0.92 * vol.size
        rp.value_range_changed(*w)
        assert rp.volume_info()[1] == (float(w[0]), float(w[1]))
    finally:
        rp.close()
