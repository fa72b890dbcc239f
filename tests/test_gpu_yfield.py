"""GPU: the y-major binary16 difference field (vr.h VR_DERIVED_YMAJOR_FIELD, knob field_order) that
march_y_kernel<vr::F32HY, true> reads beside the y-major copy, and that kernel's fallback to the
shared z-major field.

Two volumes on a 160 x 96 frame: 40 x 24 x 56 (a 6 x 4 x 8 brick grid: a swapped nby / nbz in the
y-major slot order shows) and 9 x 7 x 17 (2 x 2 x 3 bricks, the top y-layers of the volume in the
upper brick's first rows and aprons).  Four cameras (rays along y, z, x and a diagonal), both
output formats: every shaded frame forced onto the copy with the y-major field (knobs
alt_geometry = 5, grad_field = 1, field_order = 1), and with the z-major field (field_order = 0),
equals the 8^3 bricks' frame and the oracle with the binary16 field's rounding, bit for bit.  Then
a non-default slab, 3 row shards, a two-member context, frames in flight while the field is
evicted (by a frame that needs the room, and by a budget change), and the memory rules (built
into spare budget only, evicted first, a downgrade only when forced)."""
import numpy as np
import pytest
import torch

import pyoracle
import synth
import vr_amd

pytestmark = pytest.mark.gpu

W, H = 160, 96
CAMS = {  # tools/view_sweep.py's views
    "fill": dict(radius=1.6, rotate=None),             # ray along y
    "top_z": dict(radius=1.6, rotate=(0.0, 360.0)),    # ray along z
    "side_x": dict(radius=1.6, rotate=(360.0, 0.0)),   # ray along x
    "diag": dict(radius=2.0, rotate=(180.0, 140.0)),
}
Y_NAME = "march_y_kernel<vr::F32HY, true>(vr::MarchParams)"
YFIELD = 7  # vr.h VR_DERIVED_YMAJOR_FIELD
SLAB = ((0.1, 0.2, 0.05), (0.9, 0.7, 0.8))
TF = synth.tf_band(0.15, 0.9)
FORMATS = ((vr_amd.OUT_RGBA32F, torch.float32, 4), (vr_amd.OUT_RGBA8, torch.uint8, 4))


def _volume(dims, seed):
    v = synth.gaussians_numpy(dims, seed=seed).astype(np.float32)
    v.setflags(write=False)
    return v


VOLS = {"40x24x56": _volume((40, 24, 56), 91), "9x7x17": _volume((9, 7, 17), 93)}
BIG = VOLS["40x24x56"]
_oracle = {}


def cam(name):
    return vr_amd.make_camera(**CAMS[name]).to_vr_camera()


def params(**kw):
    # frames in flight: the single-lane throughput kernels (a serial shaded frame this small runs
    # lane groups, which read the 8^3 bricks)
    kw.setdefault("frames_in_flight", 3)
    return vr_amd.default_params(shading=1, ert_eps=1e-5, **kw)


def oracle(vol, camname, slab=None):
    """The shaded frame with the binary16 field's rounding; computed once per view, read-only."""
    key = (id(vol), camname, slab)
    if key not in _oracle:
        args = (vol, float(vol.min()), float(vol.max()), TF, cam(camname), W, H, params())
        if slab:
            args += (list(slab[0]), list(slab[1]))
        ref, _ = pyoracle.Scene.from_params(*args, grad_f16=True).render()
        ref = np.ascontiguousarray(ref, np.float32)
        ref.setflags(write=False)
        _oracle[key] = ref
    return _oracle[key]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


def new_pass(vol, **kw):
    r = vr_amd.OffscreenPass(W, H, **(kw or dict(device=0)))
    r.volume_dataset_changed(synth.dataset(vol))
    r.transfer_function_changed(TF)
    # the z-major field (3x the bricks), the copy (1x) and the y-major field (3x) side by side are
    # beyond the default budget (5x), and the y-major field evicts nothing
    r.set_memory_budget(2 ** 64 - 1)
    return r


@pytest.fixture(scope="module", params=list(VOLS))
def scene(gpu, request):
    vol = VOLS[request.param]
    r = new_pass(vol)
    yield r, vol
    r.close()


def forced(rp, field_order=1):
    return rp.knobs(alt_geometry=5, grad_field=1, field_order=field_order)


def base(rp):
    return rp.knobs(alt_geometry=0, grad_field=1)


def check_view(rp, vol, camname, field_order, slab=None):
    c, p = cam(camname), params()
    with base(rp):
        b32 = rp.render(c, p, vr_amd.OUT_RGBA32F)
        b8 = rp.render(c, p, vr_amd.OUT_RGBA8)
        bname = rp.last_kernel_name()
    with forced(rp, field_order):
        y32 = rp.render(c, p, vr_amd.OUT_RGBA32F)
        y8 = rp.render(c, p, vr_amd.OUT_RGBA8)
        name, last = rp.kernel_name(p), rp.last_kernel_name()
        m = rp.memory_report()
    what = (camname, field_order, slab)
    assert "march_kernel<vr::F32H," in bname, (what, bname)
    assert last == name and name.endswith(Y_NAME), (what, name, last)
    assert (m["ymajor_field_bytes"] > 0) == (field_order == 1), (what, m)
    ref = oracle(vol, camname, slab)
    assert same_bits(y32, b32) and np.array_equal(y8, b8), what
    assert same_bits(y32, ref), what
    assert np.array_equal(y8, vr_amd.unorm8(ref)), what


@pytest.mark.parametrize("camname", list(CAMS))
def test_forced_field_renders_the_bricks_frame_and_the_oracle(scene, camname):
    rp, vol = scene
    check_view(rp, vol, camname, 1)


@pytest.mark.parametrize("volname", list(VOLS))
def test_fallback_to_the_z_major_field(gpu, volname):
    """field_order = 0 on a context that never had the y-major field: the same kernel, the same
    bits, from the copy in its y-major brick order and the z-major field."""
    vol = VOLS[volname]
    r = new_pass(vol)
    try:
        for camname in CAMS:
            check_view(r, vol, camname, 0)
        m = r.memory_report()
        assert m["ymajor_field_bytes"] == 0 and m["field_bytes"] > 0 and m["ymajor_copy_bytes"] > 0
    finally:
        r.close()


def test_non_default_slab(scene):
    rp, vol = scene
    rp.slicing_changed(*SLAB)
    try:
        for camname in CAMS:
            check_view(rp, vol, camname, 1, SLAB)
    finally:
        rp.slicing_changed((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def oracle_in(vol, fmt, camname):
    ref = oracle(vol, camname)
    return ref.view(np.uint32) if fmt == vr_amd.OUT_RGBA32F else vr_amd.unorm8(ref)


def bits(t, fmt):
    a = t.cpu().numpy()
    return a.view(np.uint32) if fmt == vr_amd.OUT_RGBA32F else a


def test_three_row_shards(scene):
    """Every camera, both formats, row blocks of 16 and 8: the three shards assembled equal the
    oracle."""
    rp, vol = scene
    p = params()
    for camname, (fmt, dt, ch), row_block in [(c, f, b) for c in CAMS for f in FORMATS
                                              for b in (16, 8)]:
        c = cam(camname)
        sr = vr_amd.shard_rows(H, row_block, 3)
        g = torch.empty((3, sr, W, ch), dtype=dt, device="cuda")
        out = torch.empty((H, W, ch), dtype=dt, device="cuda")
        with forced(rp):
            for r in range(3):
                rp.render_device(c, p, g[r].data_ptr(), fmt, row_block, r, 3)
                assert rp.last_kernel_name().endswith(Y_NAME)
            rp.assemble_rows(g.data_ptr(), out.data_ptr(), fmt, row_block, 3)
            assert rp.memory_report()["ymajor_field_bytes"] > 0
        torch.cuda.synchronize()
        assert np.array_equal(bits(out, fmt), oracle_in(vol, fmt, camname)), (camname, fmt, row_block)


def test_every_member_of_a_context_reads_its_own_field(gpu):
    grp = new_pass(BIG, members=(0, 0), exchange=vr_amd.EXCHANGE_COPY)
    try:
        frame = torch.empty((H, W), dtype=torch.int32, device="cuda")
        p = params()
        with forced(grp):
            for _ in range(2):  # the second frame: every member's structures are in place
                grp.render_device(cam("fill"), p, frame.data_ptr(), vr_amd.OUT_RGBA8, 8, 0, 1)
            torch.cuda.synchronize()
            assert grp.last_kernel_name().endswith(Y_NAME)
            m = grp.memory_report()
            assert m["ymajor_field_bytes"] > 0 and m["field_bytes"] == 0
        got = frame.cpu().numpy().view(np.uint8).reshape(H, W, 4)
        assert np.array_equal(got, vr_amd.unorm8(oracle(BIG, "fill")))
    finally:
        grp.close()


def free_all(r):
    """Lowering the budget below what is held frees every derived structure."""
    r.set_memory_budget(1)
    m = r.memory_report()
    assert m["derived_bytes"] == 0 and m["ymajor_field_bytes"] == 0


@pytest.mark.parametrize("how", ("room", "budget"))
def test_frames_in_flight_while_the_field_is_evicted(gpu, how):
    """Three streams, no host wait between the frames.  After the fourth frame the y-major field is
    evicted -- "room": by a frame that needs room for another copy (a stream-ordered release
    behind the frames in flight); "budget": by a budget change -- and the frames after it read
    the z-major field.  Every frame is the oracle's, in both formats."""
    r = new_pass(BIG)
    try:
        p = params()
        with forced(r):
            r.render(cam("fill"), p, vr_amd.OUT_RGBA32F)
            m = r.memory_report()
        Y, F = m["ymajor_copy_bytes"], m["ymajor_field_bytes"]
        assert Y > 0 and F > 0 and m["field_bytes"] == 0
        order = list(CAMS) * 3
        streams = [torch.cuda.Stream() for _ in range(3)]
        for fmt, dt, ch in FORMATS:
            outs = [torch.empty((H, W, ch), dtype=dt, device="cuda") for _ in order]
            other = torch.empty((H, W, ch), dtype=dt, device="cuda")
            seen = []
            free_all(r)
            r.set_memory_budget(Y + F + 4096)
            with forced(r):
                for i, name in enumerate(order):
                    if i == 4 and how == "room":  # an unshaded oblique-copy frame
                        e0 = r.memory_report()["evictions"]
                        r.set_knob("alt_geometry", 1)
                        r.render_device(cam("diag"), vr_amd.default_params(frames_in_flight=3),
                                        other.data_ptr(), fmt, 16, 0, 1, streams[0].cuda_stream)
                        r.set_knob("alt_geometry", 5)
                        m = r.memory_report()
                        assert m["ymajor_field_bytes"] == 0 and m["oblique_copy_bytes"] > 4096
                        assert m["evictions"] == e0 + 1 and m["ymajor_copy_bytes"] == Y
                    if i == 4 and how == "budget":  # room for one field, not for both
                        r.set_memory_budget(F + 2048)
                        assert r.memory_report()["ymajor_field_bytes"] == 0
                    r.render_device(cam(name), p, outs[i].data_ptr(), fmt, 16, 0, 1,
                                    streams[i % 3].cuda_stream)
                    seen.append(r.memory_report()["ymajor_field_bytes"] > 0)
                torch.cuda.synchronize()
            assert all(seen[:4]) and not any(seen[4:]), seen
            for i, name in enumerate(order):
                assert np.array_equal(bits(outs[i], fmt), oracle_in(BIG, fmt, name)), (fmt, i, name)
    finally:
        r.close()


def test_default_knobs_keep_todays_names(scene):
    """These volumes are far below the Infinity Cache: the policy leaves them on the 8^3 bricks
    and builds no y-major structure."""
    rp, vol = scene
    p = params()
    m0 = rp.memory_report()
    img = rp.render(cam("fill"), p, vr_amd.OUT_RGBA32F)
    assert "march_kernel<vr::F32H, true, false, false, true, true>" in rp.last_kernel_name()
    assert rp.kernel_name(p) == rp.last_kernel_name()
    assert same_bits(img, oracle(vol, "fill"))
    m1 = rp.memory_report()
    assert m1["ymajor_field_bytes"] == m0["ymajor_field_bytes"]
    assert m1["ymajor_copy_bytes"] == m0["ymajor_copy_bytes"] and m1["downgrades"] == m0["downgrades"]


def test_memory_rules(gpu):
    r = new_pass(BIG)
    try:
        c, p = cam("fill"), params()
        ref = oracle(BIG, "fill")
        r.set_memory_budget(2 ** 64 - 1)

        def render(**knobs):
            with r.knobs(**knobs):
                img = r.render(c, p, vr_amd.OUT_RGBA32F)
                return img, r.last_kernel_name(), r.memory_report()

        FORCE = dict(alt_geometry=5, grad_field=1, field_order=1)
        # the copy first (an unshaded frame), then the field: one build on first use, no z-major
        # field beside it, none after
        with r.knobs(alt_geometry=5):
            r.render(c, vr_amd.default_params(frames_in_flight=3), vr_amd.OUT_RGBA32F)
        m0 = r.memory_report()
        assert m0["ymajor_copy_bytes"] > 0 and m0["ymajor_field_bytes"] == 0
        img, name, m1 = render(**FORCE)
        assert name.endswith(Y_NAME) and same_bits(img, ref)
        Y, F = m1["ymajor_copy_bytes"], m1["ymajor_field_bytes"]
        assert m1["builds"] == m0["builds"] + 1 and F == 3 * m1["volume_bytes"]
        assert m1["field_bytes"] == 0 and m1["derived_bytes"] == Y + F
        img, name, m = render(**FORCE)
        assert m["builds"] == m1["builds"] and same_bits(img, ref)
        # left to the policy (field_order -1) a forced copy keeps the z-major field: no downgrade
        # for the y-major one's absence
        free_all(r)
        r.set_memory_budget(2 ** 64 - 1)
        img, name, m = render(alt_geometry=5, grad_field=1)
        assert name.endswith(Y_NAME) and same_bits(img, ref)
        assert m["ymajor_field_bytes"] == 0 and m["field_bytes"] == F and m["downgrades"] == m1["downgrades"]

        # another volume of the same size: the copy and the field are rebuilt from it
        free_all(r)
        r.set_memory_budget(2 ** 64 - 1)
        render(**FORCE)
        b0 = r.memory_report()["builds"]
        vol2 = _volume(BIG.shape[::-1], 92)
        r.volume_dataset_changed(synth.dataset(vol2))
        img, name, m = render(**FORCE)
        assert name.endswith(Y_NAME) and m["builds"] == b0 + 2 and m["field_bytes"] == 0
        ref2, _ = pyoracle.Scene.from_params(vol2, float(vol2.min()), float(vol2.max()), TF, c, W, H,
                                             p, grad_f16=True).render()
        assert same_bits(img, ref2)
        r.volume_dataset_changed(synth.dataset(BIG))

        # a budget with the z-major field and the copy in it and no room for the y-major field:
        # nothing is evicted for it; forced, that is one downgrade; the frame reads the z-major field
        free_all(r)
        r.set_memory_budget(Y + 2 * F - 1)
        img, name, m2 = render(alt_geometry=5, grad_field=1)
        assert m2["field_bytes"] == F and m2["ymajor_copy_bytes"] == Y
        img, name, m3 = render(**FORCE)
        assert name.endswith(Y_NAME) and same_bits(img, ref)
        assert m3["ymajor_field_bytes"] == 0 and m3["field_bytes"] == F and m3["ymajor_copy_bytes"] == Y
        assert m3["evictions"] == m2["evictions"] and m3["builds"] == m2["builds"]
        assert m3["downgrades"] == m2["downgrades"] + 1 and m3["last_downgrade"] == YFIELD

        # evicted first, before the copy: the oblique copy's room comes from the field alone
        free_all(r)
        r.set_memory_budget(Y + F + 4096)
        img, name, m4 = render(**FORCE)
        assert m4["ymajor_field_bytes"] == F and m4["field_bytes"] == 0
        with r.knobs(alt_geometry=1):
            r.render(cam("diag"), vr_amd.default_params(frames_in_flight=3), vr_amd.OUT_RGBA32F)
            m5 = r.memory_report()
        assert "vr::F32Alt" in r.last_kernel_name()
        assert m5["ymajor_field_bytes"] == 0 and m5["ymajor_copy_bytes"] == Y
        assert m5["oblique_copy_bytes"] > 0 and m5["evictions"] == m4["evictions"] + 1

        # a view that needs the z-major field evicts the y-major one: one eviction, the same frame
        free_all(r)
        r.set_memory_budget(Y + F + 4096)
        img, name, m6 = render(**FORCE)
        assert m6["ymajor_field_bytes"] == F
        img, name, m7 = render(alt_geometry=0, grad_field=1)
        assert "march_kernel<vr::F32H," in name and same_bits(img, ref)
        assert m7["ymajor_field_bytes"] == 0 and m7["field_bytes"] == F
        assert m7["ymajor_copy_bytes"] == Y and m7["evictions"] == m6["evictions"] + 1
        # and it does not come back while the room is taken: no thrashing
        img, name, m8 = render(**FORCE)
        assert name.endswith(Y_NAME) and same_bits(img, ref)
        assert m8["ymajor_field_bytes"] == 0 and m8["evictions"] == m7["evictions"]
        assert m8["builds"] == m7["builds"]
    finally:
        r.close()
