"""GPU: minimum- and mean-intensity projection (include/vr/vr_modes.h, proj_kernel).

The reference is tests/proj_ref.py (the oracle's own ray, filter, TF and blend around np.fmin
or an f32 running sum in step order, pinned against the C oracle by tests/test_proj_cpu.py);
frames must equal it bit for bit in RGBA32F and byte for byte in RGBA8, with equal rays, steps
and in-slab samples (fetched + skipped), for skip_empty 0 and 1.  Scenes, passes and checks:
tests/range_scenes.py."""
import os
import subprocess

import numpy as np
import pytest

import synth
import vr_amd
from range_scenes import (CLEAR, FULL, H, INSET, SLICE, STORAGE, W, bits, check_against, int_volume,
                          mode_pass, reference, skip_pair, volume)

pytestmark = pytest.mark.gpu

MODES = {"minip": vr_amd.MODE_MINIP, "mean": vr_amd.MODE_MEAN}
OP = {"minip": 0, "mean": 1}  # proj_kernel's second template argument


# ---- 1. parity --------------------------------------------------------------------------------
PARITY = [  # MinIP mostly with an inset box: what the mode is for
    ("minip", "g20", "rotA", "tfc", INSET, W, H),
    ("minip", "g20", "fill_oblique", "tf2", SLICE, W, H),
    ("minip", "g20", "near", "tfc", INSET, W, H),
    ("minip", "g20", "default", "tfc", INSET, 45, 35),
    ("minip", "g13", "rotA", "tfc", INSET, W, H),
    ("minip", "g13", "default", "tf2", SLICE, W, H),
    ("minip", "g13", "fill_oblique", "tfc", FULL, 1, 1),
    ("minip", "blob16", "fill_oblique", "tfc", INSET, W, H),
    ("minip", "blob16", "near", "tf2", SLICE, W, H),
    ("minip", "blob16", "default", "tfc", FULL, W, H),
    ("mean", "blob16", "default", "tfc", FULL, W, H),
    ("mean", "blob16", "fill_oblique", "tf2", FULL, W, H),
    ("mean", "g20", "rotA", "tf2", SLICE, W, H),
    ("mean", "g20", "fill_oblique", "tf2", SLICE, W, H),
    ("mean", "g20", "near", "tfc", FULL, W, H),
    ("mean", "g20", "rotA", "tf2", FULL, 45, 35),
    ("mean", "g13", "rotA", "tfc", INSET, W, H),
    ("mean", "g13", "default", "tf2", SLICE, W, H),
    ("mean", "g13", "fill_oblique", "tfc", FULL, 1, 1),
    ("mean", "blob16", "near", "tf2", INSET, W, H),
]


@pytest.mark.parametrize("mode,volname,camname,tfname,box,w,h", PARITY)
def test_projection_equals_reference(gpu, mode, volname, camname, tfname, box, w, h):
    ref, st = reference(mode, volname, camname, tfname, box, w, h)
    rp = mode_pass(mode, w, h, volume(volname), synth.TFS[tfname](), box)
    try:
        check_against(rp, synth.camera(camname).to_vr_camera(), ref, st)
    finally:
        rp.close()


# ---- 2. closed forms, independent of the helper --------------------------------------------------
def test_constant_volume_closed_form(gpu):
    """A constant 0.5 volume, box inset beyond half a voxel, so every sample is exactly 0.5: the
    mean is exactly 0.5 (every partial sum k / 2 and the quotient are exact), and MinIP, MIP and
    the mean give the same pixel.  Under the one-texel TF (c, a) it is c a a + 0.11 (1 - a),
    alpha a a + 1 - a; under a ramp all three still agree bit for bit.  Which pixels have a
    sample: the composite frame of the same scene."""
    vol = np.full((20, 18, 22), 0.5, np.float32)
    box = ((0.1, 0.1, 0.1), (0.9, 0.9, 0.9))
    cam = synth.camera("fill_oblique").to_vr_camera()
    a = np.float32(128.0) / np.float32(255.0)
    for tf in (np.array([0x80FFFFFF], np.uint32), synth.tf2()):
        rp = mode_pass("mean", 45, 35, vol, tf, box, vrange=(0.0, 1.0))
        try:
            frames = {}
            for mode in (vr_amd.MODE_MEAN, vr_amd.MODE_MINIP, vr_amd.MODE_MIP):
                rp.render_mode_changed(mode)
                for skip in (0, 1):
                    frames[mode, skip] = rp.render(cam, vr_amd.default_params(skip_empty=skip))
            base = frames[vr_amd.MODE_MIP, 0]
            assert all(np.array_equal(bits(f), bits(base)) for f in frames.values())
            rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
            hit = np.any(rp.render(cam, vr_amd.default_params()) != CLEAR, axis=-1)
            assert 0 < hit.sum() < hit.size
            assert np.all(base[~hit] == CLEAR)
            assert len(np.unique(bits(base[hit]), axis=0)) == 1  # one value, whatever the ray's length
            if tf.size == 1:
                T = np.float32(1) - a
                A = np.float32(1) - T
                omA = np.float32(1) - A
                rgb = (np.float32(1.0) * a) * A + np.float32(0.11) * omA
                alpha = A * A + np.float32(1.0) * omA
                assert np.all(base[hit][:, :3] == rgb) and np.all(base[hit][:, 3] == alpha)
        finally:
            rp.close()


@pytest.mark.parametrize("mode", MODES)
def test_transparent_tf_and_flat_range(gpu, mode):
    rp = mode_pass(mode, W, H, volume("g20"), np.zeros(16, np.uint32))
    try:
        cam = synth.camera("rotA").to_vr_camera()
        for skip in (0, 1):
            img = rp.render(cam, vr_amd.default_params(skip_empty=skip))
            assert np.all(img == CLEAR)
    finally:
        rp.close()
    # vmin == vmax: the division gives NaN or an infinity, as in the reference helper
    vol = np.full((9, 10, 11), 0.5, np.float32)
    ref, st = reference(mode, "const", "rotA", "tfc", vol=vol)
    rp = mode_pass(mode, W, H, vol, synth.tf_color())
    try:
        check_against(rp, synth.camera("rotA").to_vr_camera(), ref, st)
    finally:
        rp.close()


# ---- 3. storage types ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,signed,knobs,storage", STORAGE)
def test_storage_types(gpu, mode, dtype, signed, knobs, storage):
    vf = int_volume(signed)
    ref, st = reference(mode, "int_s" if signed else "int_u", "fill_oblique", "tfc", INSET, vol=vf)
    rp = mode_pass(mode, W, H, vf.astype(dtype), synth.tf_color(), INSET, **knobs)
    try:
        assert rp.volume_info()[2] == storage
        check_against(rp, synth.camera("fill_oblique").to_vr_camera(), ref, st)
    finally:
        rp.close()


# ---- 4. samples in flight ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,knobs", [(np.float32, {}), (np.uint8, dict(u8_layout=0)),
                                         (np.uint8, dict(u8_layout=1)), (np.int16, {})])
def test_every_inflight_variant_renders_the_same_bytes(gpu, mode, dtype, knobs):
    signed = dtype == np.int16
    vf = int_volume(signed)
    ref, st = reference(mode, "int_s" if signed else "int_u", "fill_oblique", "tfc", INSET, vol=vf)
    rp = mode_pass(mode, 45, 35, vf.astype(dtype), synth.tf_color(), INSET, **knobs)
    try:
        cam = synth.camera("fill_oblique").to_vr_camera()
        frames = {}
        for k in (1, 2, 4):
            rp.set_knob("mip_inflight", k)
            for skip in (0, 1):
                p = vr_amd.default_params(skip_empty=skip)
                frames[k, skip] = rp.render(cam, p)
                name = rp.kernel_name(p)
                assert "proj_kernel<" in name and f", {OP[mode]}, false, " in name, name
                assert name.endswith(("true" if skip else "false") + f", {k}>(vr::MarchParams, vr::ProjArgs)"), name
                assert rp.last_kernel_name() == name
        base = bits(frames[1, 0])
        assert all(np.array_equal(bits(f), base) for f in frames.values())
        # and the smaller frame of the reference, K = 4
        rp.framebuffer_size_changed(W, H)
        check_against(rp, cam, ref, st)
    finally:
        rp.close()


# ---- 5. range skipping -------------------------------------------------------------------------------
def model_skips(volname, vol, camname, box, vrange=None):
    """In-slab samples in constant bricks, from the helper's model of the stored f32 ranges."""
    return reference("mean", volname, camname, "tf2", box, vol=vol, vrange=vrange)[1]["const_samples"]


@pytest.mark.parametrize("camname", ["rotA", "fill_oblique"])
@pytest.mark.parametrize("mode,dtype", [("mean", np.float32), ("mean", np.uint8), ("minip", np.float32),
                                        ("minip", np.uint8)])
def test_skipping_is_exact(gpu, mode, dtype, camname):
    """skip_empty 0 against 1 on the plateau volume (50 of its 180 bricks store one value): the
    same bits and the same in-slab samples; for the f32 mean the skipped samples are exactly the
    helper's model (10,808 of 59,013 and 18,015 of 93,276 on the full box), for MinIP some are
    skipped -- and still so after a TF change (no rebuild), a volume change (one rebuild), with
    one NaN voxel, with an infinite constant region (fetched) and with a region of mixed zeros;
    with a memory budget of 0 nothing is skipped and the frame reports one downgrade."""
    v = volume("plateau")
    exact = mode == "mean" and dtype == np.float32
    if dtype == np.uint8:
        v = np.rint(v / v.max() * 255.0).astype(np.uint8)
    cam = synth.camera(camname).to_vr_camera()
    rp = mode_pass(mode, W, H, v, synth.tf2())
    try:
        first, w = skip_pair(rp, cam)
        print(mode, camname, np.dtype(dtype).name, w)
        assert w["skipped_samples"] > 0
        if exact:
            ref, st = reference(mode, "plateau", camname, "tf2")
            assert np.array_equal(bits(first), bits(ref))
            assert w["skipped_samples"] == st["const_samples"] and w["samples"] == st["samples"] - st["const_samples"]
            rp.slicing_changed(*SLICE)
            _, ws = skip_pair(rp, cam)
            assert ws["skipped_samples"] == model_skips("plateau", None, camname, SLICE) > 0
            rp.slicing_changed(*FULL)
        builds = rp.memory_report()["builds"]
        rp.transfer_function_changed(synth.tf_color())  # invalidates nothing these modes read
        other, w2 = skip_pair(rp, cam)
        assert w2 == w and rp.memory_report()["builds"] == builds
        assert not np.array_equal(bits(other), bits(first))
        v2 = np.ascontiguousarray(v[::-1])  # a volume change rebuilds the ranges
        rp.volume_dataset_changed(synth.dataset(v2))
        _, w3 = skip_pair(rp, cam)
        assert w3["skipped_samples"] > 0 and rp.memory_report()["builds"] == builds + 1
        if exact:
            assert w3["skipped_samples"] == model_skips("plateau_rev", v2, camname, FULL)
        if dtype == np.float32:
            ds = synth.dataset(v)
            cz, cy, cx = (n // 2 for n in v.shape)
            specials = {"nan": v.copy(), "inf": v.copy(), "zeros": v.copy()}
            specials["nan"][cz, cy, cx] = np.nan
            specials["inf"][2:20, 2:20, 2:20] = np.inf  # holds whole bricks: all-inf ranges
            specials["zeros"][:12:2, :, :] = -0.0  # the low corner's zeros, every other slice negative
            specials["zeros"][:12][v[:12] != 0] = v[:12][v[:12] != 0]
            for name, sv in specials.items():
                rp.volume_dataset_changed(vr_amd.Dataset(ds.dims, ds.vmin, ds.vmax, sv))
                img, wsp = skip_pair(rp, cam)
                if exact:
                    sref, sst = reference(mode, "plateau_" + name, camname, "tfc", vol=sv,
                                          vrange=(ds.vmin, ds.vmax))  # (the TF is tf_color by now)
                    assert wsp["skipped_samples"] == sst["const_samples"] > 0, name
                    assert np.array_equal(bits(img), bits(sref)), name
        down = rp.memory_report()["downgrades"]
        rp.set_memory_budget(0)
        a, w4 = skip_pair(rp, cam, vr_amd.OUT_RGBA8)
        assert w4["skipped_samples"] == 0
        m = rp.memory_report()
        assert m["downgrades"] == down + 1 and vr_amd.DERIVED[m["last_downgrade"]] == "skip"
    finally:
        rp.close()


# ---- 6. plumbing ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_row_shards_assemble_to_the_full_frame(gpu, mode):
    import torch
    w, h = 75, 53
    rp = mode_pass(mode, w, h, volume("g20"), synth.tf_color(), INSET)
    try:
        cam = synth.camera("rotA").to_vr_camera()
        for skip in (0, 1):
            p = vr_amd.default_params(skip_empty=skip)
            full = torch.empty((h, w), dtype=torch.int32, device="cuda")
            rp.render_device(cam, p, full.data_ptr(), vr_amd.OUT_RGBA8, 16, 0, 1)
            whole = rp.count_work(cam, p)
            for share, nranks, rb in (((1, 1), 2, 16), ((1, 1), 3, 8), ((1, 1), 5, 1), ((7, 8), 3, 8)):
                rp.set_row_share(*share)
                sr = rp.shard_rows(h, rb, nranks)
                gathered = torch.zeros((nranks, sr, w), dtype=torch.int32, device="cuda")
                for r in range(nranks):
                    rp.render_device(cam, p, gathered[r].data_ptr(), vr_amd.OUT_RGBA8, rb, r, nranks)
                out = torch.empty((h, w), dtype=torch.int32, device="cuda")
                rp.assemble_rows(gathered.data_ptr(), out.data_ptr(), vr_amd.OUT_RGBA8, rb, nranks)
                torch.cuda.synchronize()
                assert torch.equal(out, full), (skip, share, nranks, rb)
                parts = [rp.count_work(cam, p, rb, r, nranks) for r in range(nranks)]
                tot = {k: sum(x[k] for x in parts) for k in whole}
                if not skip or mode == "mean":  # (the mean's skips do not depend on the ray's past)
                    assert tot == whole
                assert tot["rays"] == whole["rays"] and tot["steps"] == whole["steps"]
                assert tot["samples"] + tot["skipped_samples"] == whole["samples"] + whole["skipped_samples"]
            rp.set_row_share(1, 1)
    finally:
        rp.close()


@pytest.mark.parametrize("members", [(0, 0), (0, 0, 0)])
def test_member_contexts_equal_the_single_context(gpu, members):
    w, h = 75, 61
    vol, tf = volume("g20"), synth.tf_color()
    grp = vr_amd.OffscreenPass(w, h, members=members, exchange=vr_amd.EXCHANGE_COPY)
    one = vr_amd.OffscreenPass(w, h)
    try:
        for rp in (grp, one):
            rp.volume_dataset_changed(synth.dataset(np.asarray(vol)))
            rp.transfer_function_changed(tf)
            rp.slicing_changed(*INSET)
        cam = synth.camera("fill_oblique").to_vr_camera()
        p = vr_amd.default_params(skip_empty=1)
        comp = grp.render(cam, p)
        for mode in MODES.values():
            grp.render_mode_changed(mode)  # forwarded to every member
            one.render_mode_changed(mode)
            assert grp.render_mode == mode and "proj_kernel" in grp.kernel_name(p)
            for fmt in (vr_amd.OUT_RGBA8, vr_amd.OUT_RGBA32F):
                a, b = one.render(cam, p, fmt), grp.render(cam, p, fmt)
                assert np.array_equal(bits(a), bits(b))
            assert grp.count_work(cam, p) == one.count_work(cam, p)
        grp.render_mode_changed(vr_amd.MODE_COMPOSITE)
        assert np.array_equal(bits(grp.render(cam, p)), bits(comp))
    finally:
        grp.close()
        one.close()


@pytest.mark.parametrize("mode", MODES)
def test_frames_in_flight_on_three_streams(gpu, mode):
    import torch
    w, h = 75, 53
    rp = mode_pass(mode, w, h, volume("g20"), synth.tf_color(), INSET)
    try:
        cam = synth.camera("fill_oblique").to_vr_camera()
        for skip in (0, 1):
            p = vr_amd.default_params(skip_empty=skip, frames_in_flight=3)
            ref = torch.empty((h, w), dtype=torch.int32, device="cuda")
            rp.render_device(cam, vr_amd.default_params(skip_empty=skip), ref.data_ptr(), vr_amd.OUT_RGBA8)
            torch.cuda.synchronize()
            streams = [torch.cuda.Stream() for _ in range(3)]
            outs = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(6)]
            for i, o in enumerate(outs):
                rp.render_device(cam, p, o.data_ptr(), vr_amd.OUT_RGBA8, 16, 0, 1, streams[i % 3].cuda_stream)
            torch.cuda.synchronize()
            for i, o in enumerate(outs):
                assert torch.equal(o, ref), (skip, i)
    finally:
        rp.close()


def test_mode_round_trips_leave_the_other_modes_untouched(gpu):
    """Composite, MIP and ISO frames before and after MinIP and mean frames are the same bits;
    the two modes build the ranges and nothing else, evict nothing, ignore shading and ert_eps
    and still validate every vr_params field; 2, 5 and -1 stay refused."""
    vol, tf = volume("g20"), synth.tf_color()
    cam = synth.camera("fill_oblique").to_vr_camera()
    rp = vr_amd.OffscreenPass(45, 35)
    try:
        rp.volume_dataset_changed(synth.dataset(np.asarray(vol)))
        rp.transfer_function_changed(tf)
        rp.isovalue_changed(0.3 * float(vol.max()))
        p = vr_amd.default_params(shading=1, exact_gradient=1)
        with rp.knobs(grad_field=1):  # the difference field is built
            before = {}
            for mode in (vr_amd.MODE_COMPOSITE, vr_amd.MODE_MIP, vr_amd.MODE_ISO):
                rp.render_mode_changed(mode)
                before[mode] = rp.render(cam, p)
            assert rp.memory_report()["field_bytes"] > 0
            rep = rp.memory_report()
            shown = {}
            for mode in MODES.values():
                rp.render_mode_changed(mode)
                frames = [rp.render(cam, vr_amd.default_params(shading=s, ert_eps=e, skip_empty=k))
                          for s in (0, 1) for e in (0.0, 1e-3) for k in (0, 1)]
                assert all(np.array_equal(bits(f), bits(frames[0])) for f in frames)
                assert all(not np.array_equal(bits(frames[0]), bits(b)) for b in before.values())
                shown[mode] = frames[0]
                for bad in (2, 5, -1):
                    assert vr_amd.lib().vr_set_render_mode(rp._ctx, bad) == -22
                    assert rp.render_mode == mode
                with pytest.raises(RuntimeError, match="unknown render mode"):
                    rp.render_mode_changed(5)
                with pytest.raises(RuntimeError, match="spec_power"):
                    rp.render(cam, vr_amd.default_params(spec_power=-1))
            assert not np.array_equal(bits(shown[vr_amd.MODE_MINIP]), bits(shown[vr_amd.MODE_MEAN]))
            after = rp.memory_report()  # the ranges and nothing else; nothing evicted
            assert after["field_bytes"] == rep["field_bytes"] and after["evictions"] == rep["evictions"]
            assert after["builds"] == rep["builds"] + 1
            for mode in (vr_amd.MODE_ISO, vr_amd.MODE_MIP, vr_amd.MODE_MEAN, vr_amd.MODE_COMPOSITE,
                         vr_amd.MODE_MINIP, vr_amd.MODE_ISO, vr_amd.MODE_COMPOSITE, vr_amd.MODE_MIP):
                rp.render_mode_changed(mode)
                want = before[mode] if mode in before else shown[mode]
                assert np.array_equal(bits(rp.render(cam, p)), bits(want)), mode
            rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
            assert "march_kernel" in rp.kernel_name(p)
    finally:
        rp.close()


def test_host_row_bands_prepare_and_timing(gpu):
    import torch
    w, h = 40, 256  # vr_render splits a frame this tall into row bands
    rp = mode_pass("mean", w, h, volume("g20"), synth.tf_color())
    try:
        cam = synth.camera("fill").to_vr_camera()
        for mode in MODES:
            rp.render_mode_changed(MODES[mode])
            for skip in (0, 1):
                p = vr_amd.default_params(skip_empty=skip)
                dev = torch.empty((h, w), dtype=torch.int32, device="cuda")
                rp.render_device(cam, p, dev.data_ptr(), vr_amd.OUT_RGBA8)
                torch.cuda.synchronize()
                host = rp.render(cam, p, vr_amd.OUT_RGBA8)
                assert np.array_equal(host.view(np.int32)[..., 0], dev.cpu().numpy())
                name = rp.kernel_name(p)
                assert f"proj_kernel<float, {OP[mode]}, false, " + ("true" if skip else "false") in name, name
        rp.prepare(cam, vr_amd.default_params(skip_empty=1))
        rp.timing_enable(True)
        rp.timing_reset()
        rp.render(cam, vr_amd.default_params(), vr_amd.OUT_RGBA8)
        ms, n = rp.timing_read()
        assert n == 4 and ms > 0.0
    finally:
        rp.close()


# ---- 7. CLI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_cli_mode(gpu, tmp_path, mode):
    cli = os.path.join(os.path.dirname(vr_amd.LIB_PATH), "vr_cli")
    w, h = 96, 64
    out = str(tmp_path / "f.ppm")
    rp = vr_amd.OffscreenPass(w, h)
    try:
        rp.generate_volume((40, 40, 40), np.float32, seed=2024)
        rp.transfer_function_changed(synth.tf2())
        cam = vr_amd.make_camera(radius=2.0, rotate=(100.0, 60.0)).to_vr_camera()
        comp = rp.render(cam, vr_amd.default_params(), vr_amd.OUT_RGBA8)
        rp.render_mode_changed(MODES[mode])
        ref = rp.render(cam, vr_amd.default_params(), vr_amd.OUT_RGBA8)
    finally:
        rp.close()
    for extra in ([], ["--skip-empty"]):
        r = subprocess.run([cli, "synthetic:40", out, "--size", f"{w}x{h}", "--radius", "2", "--rotate",
                            "100,60", "--tf", "demo", "--mode", mode, *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        data = open(out, "rb").read().split(b"\n", 3)
        img = np.frombuffer(data[3], np.uint8).reshape(h, w, 3)
        assert np.array_equal(img, ref[..., :3]) and not np.array_equal(img, comp[..., :3])
