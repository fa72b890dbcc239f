"""GPU: the y-major copy of an f32 volume (csrc/vr_internal.h F32Y, knob alt_geometry = 5) and
its kernels (march_y_kernel<vr::F32Y, false>, march_y_kernel<vr::F32HY, true>).

A 40 x 24 x 56 volume (non-cubic, a multiple of 8 on no axis: a swapped nby / nbz or a wrong top
layer of a brick shows) on a 160 x 96 frame, four cameras (rays along y, z, x and a diagonal),
unshaded and shaded, both output formats: every frame forced onto the copy equals the 8^3
bricks' frame (knob 0) and the oracle bit for bit -- the oracle restating the binary16 field's
rounding where the kernel name contains F32H.  Then a non-default slab, 3 row shards, 3 frames in
flight and a two-member context; the launches knob 5 cannot serve; the names; the memory rules
(one build, a rebuild per volume, nothing evicted for it, evicted first)."""
import numpy as np
import pytest
import torch

import pyoracle
import synth
import vr_amd

pytestmark = pytest.mark.gpu

W, H = 160, 96
DIMS = (40, 24, 56)
CAMS = {  # tools/view_sweep.py's views
    "fill": dict(radius=1.6, rotate=None),             # ray along y
    "top_z": dict(radius=1.6, rotate=(0.0, 360.0)),    # ray along z
    "side_x": dict(radius=1.6, rotate=(360.0, 0.0)),   # ray along x
    "diag": dict(radius=2.0, rotate=(180.0, 140.0)),
}
Y_NAME = {0: "march_y_kernel<vr::F32Y, false>(vr::MarchParams)",
          1: "march_y_kernel<vr::F32HY, true>(vr::MarchParams)"}
YMAJOR = 6  # vr.h VR_DERIVED_YMAJOR_COPY
SLAB = ((0.1, 0.2, 0.05), (0.9, 0.7, 0.8))

VOL = synth.gaussians_numpy(DIMS, seed=91).astype(np.float32)
VOL.setflags(write=False)
VMIN, VMAX = float(VOL.min()), float(VOL.max())
TF = synth.tf_band(0.15, 0.9)
_oracle = {}


def cam(name):
    return vr_amd.make_camera(**CAMS[name]).to_vr_camera()


def params(shading, **kw):
    # frames in flight: the single-lane throughput kernels (a serial shaded frame this small runs
    # lane groups, which read the 8^3 bricks)
    kw.setdefault("frames_in_flight", 3)
    return vr_amd.default_params(shading=shading, ert_eps=1e-5, **kw)


def oracle(camname, shading, half, slab=None, vol=VOL):
    key = (camname, shading, half, slab, id(vol))
    if key not in _oracle:
        p = params(shading)
        args = (vol, float(vol.min()), float(vol.max()), TF, cam(camname), W, H, p)
        if slab:
            args += (list(slab[0]), list(slab[1]))
        ref, _ = pyoracle.Scene.from_params(*args, grad_f16=half).render()
        ref = np.ascontiguousarray(ref, np.float32)
        ref.setflags(write=False)
        _oracle[key] = ref
    return _oracle[key]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def rp(gpu):
    r = vr_amd.OffscreenPass(W, H, device=0)
    r.volume_dataset_changed(synth.dataset(VOL))
    r.transfer_function_changed(TF)
    yield r
    r.close()


def forced(rp, shading):
    """Knobs that put every eligible launch on the copy: shaded frames need the field on every
    view (the policy gives it to dense-row views only)."""
    return rp.knobs(alt_geometry=5, grad_field=1) if shading else rp.knobs(alt_geometry=5)


def base(rp, shading):
    return rp.knobs(alt_geometry=0, grad_field=1) if shading else rp.knobs(alt_geometry=0)


def check_view(rp, camname, shading, slab=None):
    c, p = cam(camname), params(shading)
    with base(rp, shading):
        b32 = rp.render(c, p, vr_amd.OUT_RGBA32F)
        b8 = rp.render(c, p, vr_amd.OUT_RGBA8)
        bname = rp.last_kernel_name()
    with forced(rp, shading):
        y32 = rp.render(c, p, vr_amd.OUT_RGBA32F)
        y8 = rp.render(c, p, vr_amd.OUT_RGBA8)
        name, last = rp.kernel_name(p), rp.last_kernel_name()
    what = (camname, shading, slab)
    assert "march_kernel<" in bname and ("vr::F32H," in bname) == bool(shading), (what, bname)
    assert last == name and name.endswith(Y_NAME[shading]), (what, name, last)
    ref = oracle(camname, shading, "F32H" in name, slab)
    assert same_bits(y32, b32) and np.array_equal(y8, b8), what
    assert same_bits(y32, ref), what
    assert np.array_equal(y8, vr_amd.unorm8(ref)), what


@pytest.mark.parametrize("camname", list(CAMS))
@pytest.mark.parametrize("shading", (0, 1))
def test_forced_copy_renders_the_bricks_frame_and_the_oracle(rp, camname, shading):
    check_view(rp, camname, shading)


@pytest.mark.parametrize("shading", (0, 1))
def test_non_default_slab(rp, shading):
    rp.slicing_changed(*SLAB)
    try:
        for camname in CAMS:
            check_view(rp, camname, shading, SLAB)
    finally:
        rp.slicing_changed((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


FORMATS = ((vr_amd.OUT_RGBA32F, torch.float32, 4), (vr_amd.OUT_RGBA8, torch.uint8, 4))


def oracle_in(fmt, camname, shading):
    ref = oracle(camname, shading, bool(shading))
    return ref.view(np.uint32) if fmt == vr_amd.OUT_RGBA32F else vr_amd.unorm8(ref)


def bits(t, fmt):
    a = t.cpu().numpy()
    return a.view(np.uint32) if fmt == vr_amd.OUT_RGBA32F else a


@pytest.mark.parametrize("shading", (0, 1))
def test_three_row_shards(rp, shading):
    """Every camera, both formats, row blocks of 16 and 8: the three shards assembled equal the
    knob-0 shards assembled and the oracle."""
    p = params(shading)
    for camname, (fmt, dt, ch), row_block in [(c, f, b) for c in CAMS for f in FORMATS
                                              for b in (16, 8)]:
        c = cam(camname)
        sr = vr_amd.shard_rows(H, row_block, 3)
        frames = {}
        for which, knobs in (("bricks", base), ("copy", forced)):
            g = torch.empty((3, sr, W, ch), dtype=dt, device="cuda")
            out = torch.empty((H, W, ch), dtype=dt, device="cuda")
            with knobs(rp, shading):
                for r in range(3):
                    rp.render_device(c, p, g[r].data_ptr(), fmt, row_block, r, 3)
                    assert ("march_y_kernel" in rp.last_kernel_name()) == (which == "copy")
                rp.assemble_rows(g.data_ptr(), out.data_ptr(), fmt, row_block, 3)
            torch.cuda.synchronize()
            frames[which] = bits(out, fmt)
        what = (camname, shading, fmt, row_block)
        assert rp.last_kernel_name().endswith(Y_NAME[shading]), what
        assert np.array_equal(frames["copy"], frames["bricks"]), what
        assert np.array_equal(frames["copy"], oracle_in(fmt, camname, shading)), what


@pytest.mark.parametrize("shading", (0, 1))
def test_three_frames_in_flight(rp, shading):
    """Both formats, every camera three times over three streams with no host wait between the
    frames: each equals the knob-0 frame enqueued the same way and the oracle."""
    p = params(shading)
    order = list(CAMS) * 3
    streams = [torch.cuda.Stream() for _ in range(3)]
    for fmt, dt, ch in FORMATS:
        frames = {}
        for which, knobs in (("bricks", base), ("copy", forced)):
            outs = [torch.empty((H, W, ch), dtype=dt, device="cuda") for _ in order]
            with knobs(rp, shading):
                for i, name in enumerate(order):
                    rp.render_device(cam(name), p, outs[i].data_ptr(), fmt, 16, 0, 1,
                                     streams[i % 3].cuda_stream)
                    if which == "copy":
                        assert rp.last_kernel_name().endswith(Y_NAME[shading]), (i, name)
                torch.cuda.synchronize()
            frames[which] = [bits(o, fmt) for o in outs]
        for i, name in enumerate(order):
            assert np.array_equal(frames["copy"][i], frames["bricks"][i]), (fmt, i, name)
            assert np.array_equal(frames["copy"][i], oracle_in(fmt, name, shading)), (fmt, i, name)


def test_every_member_of_a_context_reads_its_own_copy(gpu):
    grp = vr_amd.OffscreenPass(W, H, members=(0, 0), exchange=vr_amd.EXCHANGE_COPY)
    try:
        grp.volume_dataset_changed(synth.dataset(VOL))
        grp.transfer_function_changed(TF)
        frame = torch.empty((H, W), dtype=torch.int32, device="cuda")
        for shading in (0, 1):
            p = params(shading)
            with forced(grp, shading):
                for _ in range(2):  # the second frame: every member's copy is in place
                    grp.render_device(cam("fill"), p, frame.data_ptr(), vr_amd.OUT_RGBA8, 8, 0, 1)
                torch.cuda.synchronize()
                assert grp.last_kernel_name().endswith(Y_NAME[shading])
                assert grp.memory_report()["ymajor_copy_bytes"] > 0
            got = frame.cpu().numpy().view(np.uint8).reshape(H, W, 4)
            assert np.array_equal(got, vr_amd.unorm8(oracle("fill", shading, bool(shading))))
    finally:
        grp.close()


def test_fallbacks_under_the_knob(rp):
    """What the copy's kernels do not serve stays on the 8^3 bricks: the same bits, an 8^3 name."""
    c = cam("fill")
    tf257 = synth.tf_band(0.15, 0.9, 257)
    cases = [("tf257", dict(), dict(shading=1), tf257),
             ("skip_empty", dict(), dict(shading=1, skip_empty=1), None),
             ("exact_gradient", dict(), dict(shading=1, exact_gradient=1), None),
             ("stencil_gradient", dict(grad_field=0), dict(shading=1), None),
             ("lane_groups", dict(pair=1), dict(shading=1, frames_in_flight=1), None),
             ("not_pipelined", dict(pipeline=0), dict(shading=0), None)]
    try:
        for what, knobs, pk, tf in cases:
            p = vr_amd.default_params(ert_eps=1e-5, **dict(dict(frames_in_flight=3), **pk))
            if tf is not None:
                rp.transfer_function_changed(tf)
            with rp.knobs(alt_geometry=0, **knobs):
                want = rp.render(c, p, vr_amd.OUT_RGBA32F)
                wname = rp.last_kernel_name()
            with rp.knobs(alt_geometry=5, **knobs):
                got = rp.render(c, p, vr_amd.OUT_RGBA32F)
                name = rp.last_kernel_name()
                if what != "lane_groups":  # (vr_kernel_name names the single-lane variant)
                    assert rp.kernel_name(p) == name, what
            assert name == wname and "march_y_kernel" not in name, (what, name, wname)
            assert same_bits(got, want), what
            if tf is not None:
                rp.transfer_function_changed(TF)
    finally:
        rp.transfer_function_changed(TF)
    # the counting pass of a frame that reads the copy walks the 8^3 bricks
    p = params(1)
    with base(rp, 1):
        want = rp.count_work(c, p)
    with forced(rp, 1):
        rp.render(c, p, vr_amd.OUT_RGBA32F)
        assert rp.last_kernel_name().endswith(Y_NAME[1])
        assert rp.count_work(c, p) == want
        assert "march_kernel<vr::F32H, true, true," in rp.last_kernel_name()


def test_default_knobs_keep_todays_names(rp):
    """This volume is far below the Infinity Cache: the policy leaves it on the 8^3 bricks."""
    for shading, tag in ((0, "march_kernel<float, false, false, false, false, true>"),
                         (1, "march_kernel<vr::F32H, true, false, false, true, true>")):
        p = params(shading)
        img = rp.render(cam("fill"), p, vr_amd.OUT_RGBA32F)
        assert tag in rp.last_kernel_name() and rp.kernel_name(p) == rp.last_kernel_name()
        assert same_bits(img, oracle("fill", shading, bool(shading)))


def test_memory_rules(gpu):
    r = vr_amd.OffscreenPass(W, H, device=0)
    try:
        r.volume_dataset_changed(synth.dataset(VOL))
        r.transfer_function_changed(TF)
        c, p = cam("fill"), params(0)
        ref = oracle("fill", 0, False)
        r.set_memory_budget(2 ** 64 - 1)
        m0 = r.memory_report()
        assert m0["ymajor_copy_bytes"] == 0
        def render_with(alt):
            r.set_knob("alt_geometry", alt)
            return r.render(c, p, vr_amd.OUT_RGBA32F)

        # first use: one build; later frames none
        assert same_bits(render_with(5), ref)
        m1 = r.memory_report()
        assert m1["builds"] == m0["builds"] + 1 and m1["ymajor_copy_bytes"] > m1["volume_bytes"]
        assert m1["derived_bytes"] == m1["ymajor_copy_bytes"]
        r.render(c, p, vr_amd.OUT_RGBA32F)
        assert r.memory_report()["builds"] == m1["builds"]
        # another volume of the same size: the copy is rebuilt from it
        vol2 = synth.gaussians_numpy(DIMS, seed=92).astype(np.float32)
        r.volume_dataset_changed(synth.dataset(vol2))
        img = r.render(c, p, vr_amd.OUT_RGBA32F)
        assert r.last_kernel_name().endswith(Y_NAME[0])
        assert r.memory_report()["builds"] == m1["builds"] + 1
        assert same_bits(img, oracle("fill", 0, False, None, vol2))
        r.volume_dataset_changed(synth.dataset(VOL))
        # sizes of the plain and oblique copies of this volume
        render_with(3)
        render_with(1)
        m = r.memory_report()
        P, O, Y = m["plain_copy_bytes"], m["oblique_copy_bytes"], m1["ymajor_copy_bytes"]
        assert P > 0 and O > 0

        # a budget too small for the copy: the 8^3 bricks, the same frame, nothing evicted
        r.set_memory_budget(P + Y - 1)  # (lowering it frees everything)
        render_with(3)
        e0 = r.memory_report()
        assert e0["plain_copy_bytes"] == P
        img = render_with(5)
        m2 = r.memory_report()
        assert "march_kernel<float," in r.last_kernel_name() and same_bits(img, ref)
        assert m2["ymajor_copy_bytes"] == 0 and m2["plain_copy_bytes"] == P
        assert m2["evictions"] == e0["evictions"] and m2["builds"] == e0["builds"]
        assert m2["downgrades"] == e0["downgrades"] + 1 and m2["last_downgrade"] == YMAJOR

        # evicted first: the plain copy is older, yet the oblique copy's room comes from
        # the y-major one
        budget = P + max(Y, O) + 4096
        assert P + Y + O > budget
        r.set_memory_budget(2 ** 64 - 1)
        r.set_memory_budget(budget)
        render_with(3)
        img = render_with(5)
        m3 = r.memory_report()
        assert r.last_kernel_name().endswith(Y_NAME[0]) and same_bits(img, ref)
        assert m3["plain_copy_bytes"] == P and m3["ymajor_copy_bytes"] == Y
        img = render_with(1)
        m4 = r.memory_report()
        assert "vr::F32Alt" in r.last_kernel_name() and same_bits(img, ref)
        assert m4["ymajor_copy_bytes"] == 0 and m4["plain_copy_bytes"] == P
        assert m4["oblique_copy_bytes"] == O and m4["evictions"] == m3["evictions"] + 1
    finally:
        r.close()
