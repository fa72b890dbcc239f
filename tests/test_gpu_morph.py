"""GPU: the exact distance transform and ball morphology (include/vr/vr_morph.h, lib/
libvr_amd_morph.so) against tests/morph_ref.py -- every array byte for byte, every info field by
field: both targets, all four ops, both element widths, the host and the device forms, a 1-byte
mask at an odd address, guard bytes past every buffer, the refusals, and the calls chained behind
vr_region_grow_device and vr_label_components_device on a context that renders the same frame
before and after."""
import ctypes as C

import numpy as np
import pytest

import hit_scenes
import label_ref
import label_scenes
import morph_ref as R
import morph_scenes as S
import synth
import vr_amd
from gpu_kit import GUARD32, device_bytes, ext_of
from range_scenes import volume

pytestmark = pytest.mark.gpu

INF = float("inf")
AXIS_KERNEL = "morph_edt_axis_kernel<%d, %d>"


@pytest.fixture(scope="module")
def rp(gpu):
    p = vr_amd.OffscreenPass(16, 16)  # the calls read no volume: the placeholder will do
    yield p
    p.close()


def edt_device(rp, m, target, odd=False, cap_extra=3):
    import torch
    keep, ptr = device_bytes(m, odd)
    d = torch.full((m.size + 8,), GUARD32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    info = rp.distance_transform_device(ext_of(m), ptr, m.dtype.itemsize, d.data_ptr(), m.size + cap_extra,
                                        to_set=target == R.TO_SET, stream=stream.cuda_stream)
    # (complete on return: no synchronisation of ours before the copy on another stream)
    h = d.cpu().numpy().view(np.uint32)
    assert np.all(h[m.size:] == GUARD32)
    assert keep.cpu().numpy()[(1 if odd else 0):][:m.nbytes].tobytes() == m.tobytes()  # the mask is only read
    return h[:m.size].reshape(m.shape), info


def morph_device(rp, m, op, r2, odd=False):
    import torch
    keep, ptr = device_bytes(m, odd)
    o = torch.full((m.size + 9,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    info = rp.morph_device(ext_of(m), op, r2, ptr, m.dtype.itemsize, o.data_ptr() + 1, m.size, stream=stream.cuda_stream)
    h = o.cpu().numpy()
    assert h[0] == 0x77 and np.all(h[m.size + 1:] == 0x77)
    return h[1:m.size + 1].reshape(m.shape), info


# ---- 1. the squared distance ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.SHAPES))
@pytest.mark.parametrize("target", [R.TO_SET, R.TO_UNSET])
def test_edt_equals_the_reference(rp, name, target):
    m = S.mask(name)
    want, want_info = S.reference_edt(name, target)
    for mm in (m, S.as_labels(m)):  # both element widths
        got = rp.distance_transform(mm, to_set=target == R.TO_SET)
        print(name, target, mm.dtype, got["info"])
        assert got["info"] == want_info, (name, target, mm.dtype, got["info"], want_info)
        assert got["dist2"].dtype == np.uint32 and got["dist2"].tobytes() == want.tobytes()
    assert rp.morph_last_kernel_name() == AXIS_KERNEL % (1, 16384)  # the pass along z: no scene is that deep
    # the device form: a 1-byte mask at an odd address, then a 4-byte one; two calls, identical bytes
    d1, i1 = edt_device(rp, m, target, odd=True)
    d2, i2 = edt_device(rp, S.as_labels(m), target)
    d3, i3 = edt_device(rp, m, target, cap_extra=0)
    assert i1 == i2 == i3 == want_info
    assert d1.tobytes() == d2.tobytes() == d3.tobytes() == want.tobytes()


def test_the_corner_the_empty_and_the_full_mask(rp):
    got = rp.distance_transform(S.mask("corner"))
    bx, by, bz = S.SHAPES["corner"]
    assert got["info"] == {"voxels": bx * by * bz, "target_voxels": 1, "max_dist2": S.diagonal2("corner"),
                           "max_index": bx * by * bz - 1}  # the squared diagonal, at the far corner
    got = rp.distance_transform(S.mask("empty"))
    assert np.all(got["dist2"] == vr_amd.EDT_NONE)
    assert got["info"] == {"voxels": 129 * 5 * 3, "target_voxels": 0, "max_dist2": vr_amd.EDT_NONE, "max_index": 0}
    got = rp.distance_transform(S.mask("full"))
    assert not got["dist2"].any() and got["info"]["max_dist2"] == 0 and got["info"]["max_index"] == 0
    for op in (vr_amd.MORPH_ERODE, vr_amd.MORPH_CLOSE):  # the grid's border erodes nothing
        for r2 in (1, 100, S.diagonal2("full") + 1):
            out = rp.morph(S.mask("full"), op, r2)
            assert out["mask"].all() and out["info"]["out_set"] == out["info"]["in_set"] == 129 * 5 * 3


# ---- 2. the four ops -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_morph_equals_the_reference(rp, name):
    m = S.mask(name)
    lab = S.as_labels(m)
    for _, op, r2 in [c for c in S.morph_cases() if c[0] == name]:
        want, want_info = S.reference_morph(name, op, r2)
        got = rp.morph(m, op, r2)
        assert got["info"] == want_info, (name, op, r2, got["info"], want_info)
        assert got["mask"].dtype == np.uint8 and got["mask"].tobytes() == want.tobytes(), (name, op, r2)
        if r2 == 0:
            assert got["mask"].tobytes() == m.tobytes()
        if r2 in (3, 9):  # the 4-byte mask, and the device form from an odd address into an odd address
            got4 = rp.morph(lab, op, r2)
            assert got4["info"] == want_info and got4["mask"].tobytes() == want.tobytes(), (name, op, r2)
            dm, di = morph_device(rp, m, op, r2, odd=True)
            dm4, di4 = morph_device(rp, lab, op, r2)
            assert di == di4 == want_info and dm.tobytes() == dm4.tobytes() == want.tobytes(), (name, op, r2)
    assert rp.morph_last_kernel_name() == AXIS_KERNEL % (2, 16384)


def test_the_long_column_runs_the_long_column_kernel(rp):
    """A column of more than 16384 voxels is staged by the 32768-word instantiation."""
    m = S.mask("long_y")
    assert m.shape[1] > 16384
    # the last kernel is the pass along z, whose columns are one voxel long; the pass along y ran the
    # long-column kernel, and the same grid turned so that z is long names it
    t = np.ascontiguousarray(m.transpose(1, 0, 2))  # (bz, by, bx) = (16400, 1, 3)
    want, want_info = R.edt(t, R.TO_SET)
    got = rp.distance_transform(t)
    assert got["info"] == want_info and got["dist2"].tobytes() == want.tobytes()
    assert rp.morph_last_kernel_name() == AXIS_KERNEL % (1, 32768)
    out = rp.morph(t, vr_amd.MORPH_CLOSE, 100)
    wm, wi = R.morph(t, R.CLOSE, 100)
    assert out["info"] == wi and out["mask"].tobytes() == wm.tobytes()
    assert rp.morph_last_kernel_name() == AXIS_KERNEL % (2, 32768)


# ---- 3. errors -------------------------------------------------------------------------------------------
def test_every_error_leaves_the_outputs_untouched(rp):
    import torch
    L = vr_amd.morph_lib()
    m = S.mask("rows129")
    n = m.size
    ext = (C.c_uint32 * 3)(*ext_of(m))
    keep, mp = device_bytes(S.as_labels(m))
    d = torch.full((n + 4,), GUARD32, dtype=torch.int32, device="cuda")
    o = torch.full((n + 4,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ei, mi = vr_amd.vr_edt_info(), vr_amd.vr_morph_info()
    vp = C.c_void_p

    def fresh():
        C.memset(C.byref(ei), 0x77, 24)
        C.memset(C.byref(mi), 0x77, 24)

    def edt(ext=ext, mask=mp, eb=4, target=0, dist=d.data_ptr(), cap=n, info=C.byref(ei)):
        return L.vr_edt_squared_device(rp._ctx, ext, vp(mask), eb, target, vp(dist), cap, info, None)

    def morph(ext=ext, op=2, r2=9, mask=mp, eb=4, out=o.data_ptr(), cap=n, info=C.byref(mi)):
        return L.vr_mask_morph_device(rp._ctx, ext, op, r2, vp(mask), eb, vp(out), cap, info, None)

    fresh()
    # dcap / mcap one short: -28 before any kernel, the voxels set and nothing else
    assert edt(cap=n - 1) == -28 and b"smaller" in vr_amd.lib().vr_last_error(rp._ctx)
    assert (ei.voxels, ei.target_voxels, ei.max_dist2, ei.max_index) == (n, 0, 0, 0)
    assert morph(cap=n - 1) == -28 and (mi.voxels, mi.in_set, mi.out_set) == (n, 0, 0)
    hd = np.zeros(n, np.uint32)
    hd[:] = GUARD32
    ho = np.full(n, 0x77, np.uint8)
    assert L.vr_edt_squared(rp._ctx, ext, m.ctypes.data, 1, 0, hd.ctypes.data, n - 1, C.byref(ei)) == -28
    assert L.vr_mask_morph(rp._ctx, ext, 0, 1, m.ctypes.data, 1, ho.ctypes.data, n - 1, C.byref(mi)) == -28
    fresh()
    bad = [edt(ext=None), edt(mask=None), edt(dist=None), edt(info=None),
           edt(ext=(C.c_uint32 * 3)(129, 0, 3)), edt(ext=(C.c_uint32 * 3)(32769, 1, 1)),
           edt(ext=(C.c_uint32 * 3)(32768, 32768, 4)),
           edt(eb=2), edt(eb=0), edt(target=2), edt(target=2, cap=0),
           edt(mask=mp + 1), edt(mask=mp + 2), edt(dist=d.data_ptr() + 2, cap=n),
           edt(dist=mp, cap=n), edt(dist=mp + 4 * (n - 1), cap=n), edt(mask=d.data_ptr() + 4, dist=d.data_ptr()),
           morph(ext=None), morph(mask=None), morph(out=None), morph(info=None),
           morph(ext=(C.c_uint32 * 3)(0, 5, 3)), morph(eb=3), morph(op=4), morph(op=0xFFFFFFFF),
           morph(r2=0xFFFFFFFF), morph(r2=0xFFFFFFFF, cap=0), morph(mask=mp + 3),
           morph(out=mp + 4 * n - 1), morph(mask=o.data_ptr(), eb=1, out=o.data_ptr() + 3, cap=n)]
    assert bad == [-22] * len(bad), bad
    assert bytes(ei) == b"\x77" * 24 and bytes(mi) == b"\x77" * 24
    torch.cuda.synchronize()
    assert np.all(d.cpu().numpy().view(np.uint32) == GUARD32) and np.all(o.cpu().numpy() == 0x77)
    assert np.all(hd == GUARD32) and np.all(ho == 0x77)
    assert keep.cpu().numpy()[:4 * n].tobytes() == S.as_labels(m).tobytes()
    # r2 just below the sentinel is a radius like any other: everything within reach of a set voxel
    assert morph(op=0, r2=0xFFFFFFFE) == 0 and (mi.voxels, mi.out_set) == (n, n)
    # the binding refuses what is no mask
    with pytest.raises(ValueError):
        rp.distance_transform(np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError):
        rp.morph(np.zeros((2, 2, 2), np.float32), 0, 1)


# ---- 4. chained behind the label calls, on a context that renders ---------------------------------------
def test_region_grow_then_open_and_labels_then_edt(gpu):
    import torch
    name, lo, hi = "bigball", 20.25, INF
    vol = label_scenes.SCENES[name]()
    labels, rec, linfo = label_scenes.reference(name, lo, hi, 6)
    rp = vr_amd.OffscreenPass(16, 16)
    try:
        rp.volume_dataset_changed(synth.dataset(np.asarray(vol)))
        bz, by, bx = labels.shape
        n = labels.size
        l = int(np.flatnonzero(labels.reshape(-1) == linfo["largest_label"])[-1])
        seed = (l % bx, (l // bx) % by, l // (bx * by))
        want_mask, want_comp = label_ref.region_grow(vol, seed, lo, hi, 6, None, labelled=(labels, rec, linfo))
        dm = torch.full((n + 16,), 0x77, dtype=torch.uint8, device="cuda")
        do = torch.full((n + 16,), 0x77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        comp = rp.region_grow_device(seed, dm.data_ptr(), n, lo, hi, 6, None, stream=stream.cuda_stream)
        assert comp == want_comp
        for op, r2 in ((vr_amd.MORPH_OPEN, 9), (vr_amd.MORPH_ERODE, 4), (vr_amd.MORPH_CLOSE, 2)):
            info = rp.morph_device((bx, by, bz), op, r2, dm.data_ptr(), 1, do.data_ptr(), n, stream=stream.cuda_stream)
            want, want_info = R.morph(want_mask, op, r2)
            h = do.cpu().numpy()
            assert info == want_info and h[:n].tobytes() == want.tobytes() and np.all(h[n:] == 0x77), (op, r2)
            assert 0 < info["out_set"]
        assert dm.cpu().numpy()[:n].tobytes() == want_mask.tobytes()
        # the labels of the window as a 4-byte mask
        nc = linfo["components"]
        dl = torch.full((n + 8,), GUARD32, dtype=torch.int32, device="cuda")
        dc = torch.full((nc * 16 + 16,), GUARD32, dtype=torch.int32, device="cuda")
        dd = torch.full((n + 8,), GUARD32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert rp.label_device(dl.data_ptr(), n, dc.data_ptr(), nc, lo, hi, 6, None, stream=stream.cuda_stream) == linfo
        for target in (R.TO_SET, R.TO_UNSET):
            info = rp.distance_transform_device((bx, by, bz), dl.data_ptr(), 4, dd.data_ptr(), n,
                                                to_set=target == R.TO_SET, stream=stream.cuda_stream)
            want, want_info = R.edt(labels, target)
            h = dd.cpu().numpy().view(np.uint32)
            assert info == want_info and h[:n].tobytes() == want.tobytes() and np.all(h[n:] == GUARD32)
        # the thickest point of the ball: the largest distance to the outside
        assert info["max_dist2"] >= 25
        assert dl.cpu().numpy().view(np.uint32)[:n].tobytes() == labels.tobytes()
    finally:
        rp.close()


def test_morph_calls_leave_every_frame_and_the_memory_report_alone(gpu):
    vol = volume("g20")
    iso = hit_scenes.isovalue(vol)
    rp = hit_scenes.hit_pass(32, 24, vol, synth.tf_color(), iso)
    try:
        cam = synth.camera("rotA").to_vr_camera()
        p = vr_amd.default_params(shading=1, skip_empty=1)
        modes = (vr_amd.MODE_COMPOSITE, vr_amd.MODE_MIP, vr_amd.MODE_ISO)
        before = {}
        for md in modes:
            rp.render_mode_changed(md)
            before[md] = rp.render(cam, p, vr_amd.OUT_RGBA32F)
        state = (rp.render_mode, rp.isovalue, rp.volume_info())
        rep = rp.memory_report()
        last = rp.last_kernel_name()
        assert rp.morph_last_kernel_name() == ""
        m = S.mask("sparse70")
        rp.timing_enable(True)
        rp.timing_reset()
        assert rp.distance_transform(m)["info"] == S.reference_edt("sparse70", R.TO_SET)[1]
        ms, launches = rp.timing_read()
        assert launches == 1 and ms > 0.0  # one interval per transform
        assert rp.morph_last_kernel_name() == AXIS_KERNEL % (1, 16384)
        for op, want in ((vr_amd.MORPH_DILATE, 1), (vr_amd.MORPH_ERODE, 1), (vr_amd.MORPH_OPEN, 2),
                         (vr_amd.MORPH_CLOSE, 2)):
            rp.timing_reset()
            out = rp.morph(m, op, 9)
            assert out["mask"].tobytes() == S.reference_morph("sparse70", op, 9)[0].tobytes()
            ms, launches = rp.timing_read()
            assert launches == want and ms > 0.0, (op, launches)
        assert rp.morph_last_kernel_name() == AXIS_KERNEL % (2, 16384)
        rp.timing_enable(False)
        rp.timing_reset()
        rp.morph(m, vr_amd.MORPH_OPEN, 1)
        assert rp.timing_read()[1] == 0
        assert rp.memory_report() == rep and rp.last_kernel_name() == last
        assert (rp.render_mode, rp.isovalue, rp.volume_info()) == state
        for md in modes:
            rp.render_mode_changed(md)
            assert np.array_equal(rp.render(cam, p, vr_amd.OUT_RGBA32F).view(np.uint32),
                                  before[md].view(np.uint32)), md
    finally:
        rp.close()


def test_a_multi_device_context_computes_on_its_lowest_device(gpu):
    grp = vr_amd.OffscreenPass(16, 16, exchange=vr_amd.EXCHANGE_COPY, members=[0, 0])
    try:
        m = S.mask("rows129")
        for target in (R.TO_SET, R.TO_UNSET):
            got = grp.distance_transform(m, to_set=target == R.TO_SET)
            want, want_info = S.reference_edt("rows129", target)
            assert got["info"] == want_info and got["dist2"].tobytes() == want.tobytes()
        d, info = edt_device(grp, m, R.TO_SET, odd=True)
        assert info == S.reference_edt("rows129", R.TO_SET)[1]
        for op in range(4):
            out = grp.morph(m, op, 2)
            want, want_info = S.reference_morph("rows129", op, 2)
            assert out["info"] == want_info and out["mask"].tobytes() == want.tobytes()
        assert grp.morph_last_kernel_name() == AXIS_KERNEL % (2, 16384)
    finally:
        grp.close()
