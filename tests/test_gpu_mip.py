"""GPU: maximum-intensity projection (include/vr/vr_modes.h, mip_kernel).

The reference is tests/proj_ref.py, mode "mip" (the oracle's own ray, filter, TF and blend around
np.fmax, pinned against the C oracle by tests/test_mip_cpu.py); frames must equal it bit for bit
in RGBA32F and byte for byte in RGBA8, with equal rays, steps and in-slab samples (fetched +
skipped).  Scenes, passes and checks: tests/range_scenes.py."""
import os
import subprocess

import numpy as np
import pytest

import pyoracle
import synth
import vr_amd
from range_scenes import (CLEAR, FULL, H, SLICE, STORAGE, W, bits, check_against, int_volume, mode_pass,
                          reference, skip_pair, volume)

pytestmark = pytest.mark.gpu


# ---- 1. parity --------------------------------------------------------------------------------
PARITY = [
    ("blob16", "default", "tfc", FULL, W, H),
    ("blob16", "fill_oblique", "tf2", FULL, W, H),
    ("g20", "rotA", "tfc", FULL, W, H),
    ("g20", "fill_oblique", "tf2", SLICE, W, H),
    ("g20", "near", "tfc", FULL, W, H),
    ("g20", "rotA", "tf2", FULL, 45, 35),
    ("g13", "rotA", "tfc", FULL, W, H),
    ("g13", "default", "tf2", SLICE, W, H),
    ("g13", "fill_oblique", "tfc", FULL, 1, 1),
    ("blob16", "near", "tf2", SLICE, W, H),
]


@pytest.mark.parametrize("volname,camname,tfname,box,w,h", PARITY)
def test_mip_equals_reference(gpu, volname, camname, tfname, box, w, h):
    ref, st = reference("mip", volname, camname, tfname, box, w, h)
    rp = mode_pass("mip", w, h, volume(volname), synth.TFS[tfname](), box)
    try:
        check_against(rp, synth.camera(camname).to_vr_camera(), ref, st)
    finally:
        rp.close()


# ---- 2. closed form, independent of the helper ----------------------------------------------------
def test_constant_tf_closed_form(gpu):
    """One-texel TF (c, a): a pixel with a sample is c a a + 0.11 (1 - a), alpha a a + 1 - a;
    every other pixel is the clear colour.  Which pixels have a sample: the composite frame of
    the same scene (its colour differs from the clear colour's exactly there)."""
    tf = np.array([0x80FFFFFF], np.uint32)  # linear white, alpha 128 / 255
    a = np.float32(128.0) / np.float32(255.0)
    rp = mode_pass("mip", 45, 35, volume("g20"), tf, SLICE)
    try:
        cam = synth.camera("fill_oblique").to_vr_camera()
        p = vr_amd.default_params()
        img = rp.render(cam, p)
        rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
        hit = rp.render(cam, p)[..., 0] != CLEAR[0]  # composite: at least 0.5 of white
        assert 0 < hit.sum() < hit.size
        T = np.float32(1) - a
        A = np.float32(1) - T
        omA = np.float32(1) - A
        rgb = (np.float32(1.0) * a) * A + np.float32(0.11) * omA
        alpha = A * A + np.float32(1.0) * omA
        assert np.all(img[hit][:, :3] == rgb) and np.all(img[hit][:, 3] == alpha)
        assert abs(float(rgb) - (a * a + 0.11 * (1 - a))) < 1e-6 and abs(float(alpha) - (a * a + 1 - a)) < 1e-6
        assert np.all(img[~hit] == CLEAR)
    finally:
        rp.close()


def test_transparent_tf_and_constant_volume(gpu):
    rp = mode_pass("mip", W, H, volume("g20"), np.zeros(16, np.uint32))
    try:
        cam = synth.camera("rotA").to_vr_camera()
        for skip in (0, 1):
            img = rp.render(cam, vr_amd.default_params(skip_empty=skip))
            assert np.all(img == CLEAR)
    finally:
        rp.close()
    # vmin == vmax: the division gives NaN or an infinity, as in the reference helper
    vol = np.full((9, 10, 11), 0.5, np.float32)
    ref, st = reference("mip", "const", "rotA", "tfc", vol=vol)
    rp = mode_pass("mip", W, H, vol, synth.tf_color())
    try:
        check_against(rp, synth.camera("rotA").to_vr_camera(), ref, st)
    finally:
        rp.close()


# ---- 3. storage types ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,signed,knobs,storage", STORAGE)
def test_storage_types(gpu, dtype, signed, knobs, storage):
    vf = int_volume(signed)
    ref, st = reference("mip", "int_s" if signed else "int_u", "fill_oblique", "tfc", vol=vf)
    rp = mode_pass("mip", W, H, vf.astype(dtype), synth.tf_color(), **knobs)
    try:
        assert rp.volume_info()[2] == storage
        check_against(rp, synth.camera("fill_oblique").to_vr_camera(), ref, st)
    finally:
        rp.close()


# ---- 4. range skipping -------------------------------------------------------------------------------
@pytest.mark.parametrize("volname,camname", [("blob32", "rotA"), ("g40", "fill")])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_skipping_is_exact(gpu, volname, camname, dtype):
    """skip_empty 0 against 1: the same bits, the same in-slab samples, some of them skipped
    (a CPU model of 8^3 bricks finds 7,129 of 59,013 and 14,781 of 92,892 skippable on the f32
    scenes) -- and still so after a TF change, a volume change and with one NaN voxel; with a
    memory budget of 0 nothing is skipped and the frame reports one downgrade."""
    v = synth.gaussian_blob(32) if volname == "blob32" else synth.gaussians_numpy((40, 36, 44), seed=5)
    if dtype == np.uint8:
        v = np.rint(v / v.max() * 255.0).astype(np.uint8)
    cam = synth.camera(camname).to_vr_camera()
    rp = mode_pass("mip", W, H, v, synth.tf2())
    try:
        first, w = skip_pair(rp, cam)
        print(volname, np.dtype(dtype).name, w)
        assert w["skipped_samples"] > 0
        builds = rp.memory_report()["builds"]
        rp.transfer_function_changed(synth.tf_color())  # invalidates nothing MIP reads
        other, w2 = skip_pair(rp, cam)
        assert w2 == w and rp.memory_report()["builds"] == builds
        assert not np.array_equal(bits(other), bits(first))
        v2 = np.ascontiguousarray(v[::-1])  # a volume change rebuilds the ranges
        rp.volume_dataset_changed(synth.dataset(v2))
        _, w3 = skip_pair(rp, cam)
        assert w3["skipped_samples"] > 0 and rp.memory_report()["builds"] == builds + 1
        if dtype == np.float32:
            v3 = v.copy()
            v3[v.shape[0] // 2, v.shape[1] // 2, v.shape[2] // 2] = np.nan
            ds = synth.dataset(v)
            rp.volume_dataset_changed(vr_amd.Dataset(ds.dims, ds.vmin, ds.vmax, v3))
            skip_pair(rp, cam)
        down = rp.memory_report()["downgrades"]
        rp.set_memory_budget(0)
        a, w4 = skip_pair(rp, cam, vr_amd.OUT_RGBA8)
        assert w4["skipped_samples"] == 0
        m = rp.memory_report()
        assert m["downgrades"] == down + 1 and vr_amd.DERIVED[m["last_downgrade"]] == "skip"
    finally:
        rp.close()


# ---- 5. samples in flight ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,knobs", [(np.float32, {}), (np.uint8, dict(u8_layout=0)),
                                         (np.uint8, dict(u8_layout=1)), (np.int16, {})])
def test_every_inflight_variant_renders_the_same_bytes(gpu, dtype, knobs):
    signed = dtype == np.int16
    vf = int_volume(signed)
    ref, st = reference("mip", "int_s" if signed else "int_u", "fill_oblique", "tfc", vol=vf)
    rp = mode_pass("mip", 45, 35, vf.astype(dtype), synth.tf_color(), **knobs)
    try:
        cam = synth.camera("fill_oblique").to_vr_camera()
        frames = {}
        for k in (1, 2, 4):
            rp.set_knob("mip_inflight", k)
            for skip in (0, 1):
                p = vr_amd.default_params(skip_empty=skip)
                frames[k, skip] = rp.render(cam, p)
                assert f", {k}>" in rp.kernel_name(p)
        base = bits(frames[1, 0])
        assert all(np.array_equal(bits(f), base) for f in frames.values())
        # and the smaller frame of the reference, K = 4
        rp.framebuffer_size_changed(W, H)
        check_against(rp, cam, ref, st)
    finally:
        rp.close()


# ---- 6. plumbing ---------------------------------------------------------------------------------------
def test_row_shards_assemble_to_the_full_frame(gpu):
    import torch
    w, h = 75, 53
    rp = mode_pass("mip", w, h, volume("g20"), synth.tf_color())
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
                if not skip:  # (which samples a skipping ray leaves out is the same per ray)
                    assert tot == whole
                assert tot["rays"] == whole["rays"] and tot["steps"] == whole["steps"]
            rp.set_row_share(1, 1)
    finally:
        rp.close()


@pytest.mark.parametrize("members", [(0, 0), (0, 0, 0)])
def test_member_contexts_equal_the_single_context(gpu, members):
    w, h = 75, 61
    vol, tf = volume("g20"), synth.tf_color()
    one = mode_pass("mip", w, h, vol, tf)
    grp = vr_amd.OffscreenPass(w, h, members=members, exchange=vr_amd.EXCHANGE_COPY)
    try:
        grp.volume_dataset_changed(synth.dataset(np.asarray(vol)))
        grp.transfer_function_changed(tf)
        cam = synth.camera("fill_oblique").to_vr_camera()
        p = vr_amd.default_params(skip_empty=1)
        comp = grp.render(cam, p)
        grp.render_mode_changed(vr_amd.MODE_MIP)  # forwarded to every member
        assert grp.render_mode == vr_amd.MODE_MIP and "mip_kernel" in grp.kernel_name(p)
        for fmt in (vr_amd.OUT_RGBA8, vr_amd.OUT_RGBA32F):
            a, b = one.render(cam, p, fmt), grp.render(cam, p, fmt)
            assert np.array_equal(bits(a), bits(b))
        assert grp.count_work(cam, p) == one.count_work(cam, p)
        grp.render_mode_changed(vr_amd.MODE_COMPOSITE)
        assert np.array_equal(bits(grp.render(cam, p)), bits(comp))
    finally:
        grp.close()
        one.close()


def test_frames_in_flight_on_three_streams(gpu):
    import torch
    w, h = 75, 53
    rp = mode_pass("mip", w, h, volume("g20"), synth.tf2())
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


def test_host_row_bands_and_kernel_name(gpu):
    import torch
    w, h = 40, 256  # vr_render splits a frame this tall into row bands
    rp = mode_pass("mip", w, h, volume("g20"), synth.tf_color())
    try:
        cam = synth.camera("fill").to_vr_camera()
        for skip in (0, 1):
            p = vr_amd.default_params(skip_empty=skip)
            dev = torch.empty((h, w), dtype=torch.int32, device="cuda")
            rp.render_device(cam, p, dev.data_ptr(), vr_amd.OUT_RGBA8)
            torch.cuda.synchronize()
            host = rp.render(cam, p, vr_amd.OUT_RGBA8)
            assert np.array_equal(host.view(np.int32)[..., 0], dev.cpu().numpy())
            name = rp.kernel_name(p)
            assert "mip_kernel<float, false, " + ("true" if skip else "false") in name, name
        rp.prepare(cam, vr_amd.default_params(skip_empty=1))
        rp.timing_enable(True)
        rp.timing_reset()
        rp.render(cam, vr_amd.default_params(), vr_amd.OUT_RGBA8)
        ms, n = rp.timing_read()
        assert n == 4 and ms > 0.0
    finally:
        rp.close()


# ---- 7. mode switching ---------------------------------------------------------------------------------
def test_mode_switching_leaves_the_composite_untouched(gpu):
    vol, tf = volume("g20"), synth.tf_color()
    cam = synth.camera("fill_oblique").to_vr_camera()
    rp = vr_amd.OffscreenPass(45, 35)
    try:
        rp.volume_dataset_changed(synth.dataset(np.asarray(vol)))
        rp.transfer_function_changed(tf)
        assert rp.render_mode == vr_amd.MODE_COMPOSITE
        p = vr_amd.default_params(shading=1, exact_gradient=1)
        with rp.knobs(grad_field=1):  # the difference field is built
            before = rp.render(cam, p)
            assert rp.memory_report()["field_bytes"] > 0
            ds = synth.dataset(np.asarray(vol))
            ref, _ = pyoracle.Scene.from_params(vol, ds.vmin, ds.vmax, tf, cam, 45, 35, p).render()
            assert np.array_equal(bits(before), bits(ref))
            rp.render_mode_changed(vr_amd.MODE_MIP)
            rep = rp.memory_report()
            frames = [rp.render(cam, vr_amd.default_params(shading=s, ert_eps=e, skip_empty=k))
                      for s in (0, 1) for e in (0.0, 1e-3) for k in (0, 1)]
            assert all(np.array_equal(bits(f), bits(frames[0])) for f in frames)
            assert not np.array_equal(bits(frames[0]), bits(before))
            after = rp.memory_report()  # MIP built the ranges and nothing else, evicted nothing
            assert after["field_bytes"] == rep["field_bytes"] and after["evictions"] == rep["evictions"]
            assert after["builds"] == rep["builds"] + 1
            # an unknown mode: VR_EINVAL, the mode stays
            for bad in (2, -1):
                assert vr_amd.lib().vr_set_render_mode(rp._ctx, bad) == -22
                assert rp.render_mode == vr_amd.MODE_MIP
            with pytest.raises(RuntimeError, match="unknown render mode"):
                rp.render_mode_changed(5)
            rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
            assert "march_kernel" in rp.kernel_name(p)
            assert np.array_equal(bits(rp.render(cam, p)), bits(before))
            # check_params still validates every field in MIP mode
            rp.render_mode_changed(vr_amd.MODE_MIP)
            with pytest.raises(RuntimeError, match="spec_power"):
                rp.render(cam, vr_amd.default_params(spec_power=-1))
    finally:
        rp.close()


# ---- 8. CLI ---------------------------------------------------------------------------------------------
def test_cli_mode_mip(gpu, tmp_path):
    cli = os.path.join(os.path.dirname(vr_amd.LIB_PATH), "vr_cli")
    w, h = 96, 64
    out = str(tmp_path / "f.ppm")
    for extra in ([], ["--skip-empty"]):
        r = subprocess.run([cli, "synthetic:40", out, "--size", f"{w}x{h}", "--radius", "2", "--rotate",
                            "100,60", "--tf", "demo", "--mode", "mip", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        data = open(out, "rb").read().split(b"\n", 3)
        img = np.frombuffer(data[3], np.uint8).reshape(h, w, 3)
        rp = vr_amd.OffscreenPass(w, h)
        try:
            rp.generate_volume((40, 40, 40), np.float32, seed=2024)
            rp.transfer_function_changed(synth.tf2())
            cam = vr_amd.make_camera(radius=2.0, rotate=(100.0, 60.0)).to_vr_camera()
            comp = rp.render(cam, vr_amd.default_params(), vr_amd.OUT_RGBA8)
            rp.render_mode_changed(vr_amd.MODE_MIP)
            ref = rp.render(cam, vr_amd.default_params(), vr_amd.OUT_RGBA8)
        finally:
            rp.close()
        assert np.array_equal(img, ref[..., :3]) and not np.array_equal(img, comp[..., :3])
    r = subprocess.run([cli, "synthetic:8", out, "--mode", "average"], capture_output=True, text=True)
    assert r.returncode == 2
