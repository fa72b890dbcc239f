"""GPU: first-hit isosurface rendering (include/vr/vr_iso.h, iso_kernel).

The reference is tests/iso_ref.py (the oracle's own ray, filter and TF around the first-hit
search, with the gradient and the Phong model restated from oracle/oracle.c and pinned against
the C oracle by tests/test_iso_cpu.py); frames must equal it bit for bit in RGBA32F and byte for
byte in RGBA8, with equal rays, steps, search samples (fetched + skipped) and shaded rays.
Scene constants and volumes: tests/range_scenes.py."""
import os
import subprocess

import numpy as np
import pytest

import iso_ref
import pyoracle
import synth
import vr_amd
from range_scenes import CLEAR, FULL, H, SLICE, W, bits, int_volume, volume

pytestmark = pytest.mark.gpu

CUT = ((0.45, 0.0, 0.0), (1.0, 1.0, 0.55))
def isovalue(v, f):
    lo, hi = float(np.min(v)), float(np.max(v))
    return np.float32(lo + f * (hi - lo))


def iso_pass(w, h, vol, tf, iso, box=FULL, vrange=None, **knobs):
    rp = vr_amd.OffscreenPass(w, h)
    for k, v in knobs.items():
        rp.set_knob(k, v)
    ds = synth.dataset(np.asarray(vol))
    if vrange is not None:
        ds.vmin, ds.vmax = vrange
    rp.volume_dataset_changed(ds)
    rp.transfer_function_changed(tf)
    rp.slicing_changed(*box)
    rp.render_mode_changed(vr_amd.MODE_ISO)
    rp.isovalue_changed(iso)
    assert rp.render_mode == vr_amd.MODE_ISO and np.float32(rp.isovalue) == np.float32(iso)
    return rp


def reference(volname, camname, iso, box=FULL, w=W, h=H, shading=1, vol=None, vrange=None, **params):
    """(frame, stats, hit step, cap) of iso_ref for a named scene, computed once per session."""
    def make():
        v = np.asarray(volume(volname) if vol is None else vol, dtype=np.float32)
        lo, hi = (float(v.min()), float(v.max())) if vrange is None else vrange
        return pyoracle.Scene.from_params(v, lo, hi, synth.tf_color(), synth.camera(camname).to_vr_camera(),
                                          w, h, vr_amd.default_params(shading=shading, **params),
                                          smin=box[0], smax=box[1])
    key = (volname, camname, box, w, h, shading, vrange, tuple(sorted(params.items())))
    return iso_ref.cached(key, make, iso)


def check_against(rp, cam, ref, st, shading=1, skips=(0, 1), **params):
    for skip in skips:
        p = vr_amd.default_params(skip_empty=skip, shading=shading, **params)
        img = rp.render(cam, p, vr_amd.OUT_RGBA32F)
        assert np.array_equal(bits(img), bits(ref)), f"skip {skip}: {(bits(img) != bits(ref)).sum()} words differ"
        img8 = rp.render(cam, p, vr_amd.OUT_RGBA8)
        assert np.array_equal(img8, vr_amd.unorm8(ref)), f"skip {skip} (RGBA8)"
        w = rp.count_work(cam, p)
        print(skip, w, st)
        assert (w["rays"], w["steps"]) == (st["rays"], st["steps"]), (skip, w, st)
        assert w["samples"] + w["skipped_samples"] == st["samples"], (skip, w, st)
        assert w["shaded_samples"] == st["shaded_samples"], (skip, w, st)
        if not skip:
            assert w["skipped_samples"] == 0


# ---- 1. parity --------------------------------------------------------------------------------
PARITY = [  # volume, camera, box, W, H, f, shading
    ("g20", "rotA", FULL, W, H, 0.2, 1),
    ("g20", "fill_oblique", SLICE, W, H, 0.2, 1),
    ("g20", "fill_oblique", CUT, 45, 35, 0.15, 1),
    ("g20", "rotB", FULL, W, H, 0.3, 1),
    ("g13", "rotA", FULL, W, H, 0.2, 1),
    ("g13", "default", SLICE, W, H, 0.15, 1),
    ("g13", "diag", CUT, W, H, 0.2, 1),
    ("blob16", "rotA", CUT, W, H, 0.3, 0),
    ("blob16", "fill_oblique", CUT, W, H, 0.3, 1),
    ("g13", "fill_oblique", FULL, 1, 1, 0.1, 1),
    ("g20", "near", FULL, W, H, 0.6, 1),
]


@pytest.mark.parametrize("volname,camname,box,w,h,f,shading", PARITY)
def test_iso_equals_reference(gpu, volname, camname, box, w, h, f, shading):
    iso = isovalue(volume(volname), f)
    ref, st, hit_step, cap = reference(volname, camname, iso, box, w, h, shading)
    hits = int((hit_step >= 0).sum())
    print(volname, camname, st, "hits", hits, "caps", int(cap.sum()),
          "hit step mod 4", np.bincount(hit_step[hit_step >= 0] % 4, minlength=4).tolist())
    # the scene exercises what it is here for (the helper's own output)
    if camname == "near":
        assert st["rays"] == 0 and np.all(ref == CLEAR)
    elif (w, h) != (1, 1):
        assert hits >= 30
        assert st["shaded_samples"] == (hits if shading else 0)
    else:
        assert hits == 1
    if box == CUT:
        assert cap.sum() >= 10
    if box == FULL and volname in ("g20", "g13") and (w, h) == (W, H) and camname != "near":
        assert np.all(np.bincount(hit_step[hit_step >= 0] % 4, minlength=4) > 0)
    rp = iso_pass(w, h, volume(volname), synth.tf_color(), iso, box)
    try:
        check_against(rp, synth.camera(camname).to_vr_camera(), ref, st, shading)
    finally:
        rp.close()


# ---- 2. storage types and layouts ----------------------------------------------------------------
STORAGE = [  # upload dtype, signed values, knobs, expected storage type, vrange
    (np.uint8, False, dict(u8_layout=0), 0, None), (np.uint8, False, dict(u8_layout=1), 0, None),
    (np.int8, True, dict(u8_layout=0), 1, None), (np.int8, True, dict(u8_layout=1), 1, None),
    (np.uint16, False, {}, 2, None), (np.int16, True, {}, 3, None),
    (np.float32, True, dict(narrow=0), 4, None),
    (np.uint16, False, {}, 2, (20.0, 90.0)),  # the colour window is narrower than the data
]


@pytest.mark.parametrize("dtype,signed,knobs,storage,vrange", STORAGE)
def test_storage_types(gpu, dtype, signed, knobs, storage, vrange):
    vf = int_volume(signed)
    iso = isovalue(vf, 0.3)
    ref, st, hit_step, _ = reference("int_s" if signed else "int_u", "fill_oblique", iso, vol=vf,
                                     vrange=vrange)
    assert (hit_step >= 0).sum() >= 30
    if vrange is not None:  # the surface does not move, its colour does
        full, _, hs_full, _ = reference("int_u", "fill_oblique", iso, vol=vf)
        assert np.array_equal(hs_full, hit_step) and not np.array_equal(bits(full), bits(ref))
    rp = iso_pass(W, H, vf.astype(dtype), synth.tf_color(), iso, vrange=vrange, **knobs)
    try:
        assert rp.volume_info()[2] == storage
        check_against(rp, synth.camera("fill_oblique").to_vr_camera(), ref, st)
    finally:
        rp.close()


# ---- 3. samples in flight ---------------------------------------------------------------------------
@pytest.mark.parametrize("scene", [PARITY[0], PARITY[2]])
def test_every_inflight_variant_renders_the_same_bytes(gpu, scene):
    volname, camname, box, w, h, f, shading = scene
    iso = isovalue(volume(volname), f)
    ref, st, _, _ = reference(volname, camname, iso, box, w, h, shading)
    rp = iso_pass(w, h, volume(volname), synth.tf_color(), iso, box)
    try:
        cam = synth.camera(camname).to_vr_camera()
        for k in (1, 2, 4):
            rp.set_knob("mip_inflight", k)
            for skip in (0, 1):
                p = vr_amd.default_params(skip_empty=skip, shading=shading)
                img = rp.render(cam, p)
                assert np.array_equal(bits(img), bits(ref)), (k, skip)
                name = rp.last_kernel_name()
                assert "iso_kernel<float, false, " + ("true" if skip else "false") + f", {k}>" in name, name
                assert rp.kernel_name(p) == name
    finally:
        rp.close()


# ---- 4. closed forms, independent of the helper ------------------------------------------------------
def test_isovalue_above_the_maximum_is_the_clear_colour(gpu):
    v = np.rint(volume("g20") / volume("g20").max() * 200.0).astype(np.uint8)
    rp = iso_pass(W, H, v, synth.tf_color(), 201.0)
    try:
        cam = synth.camera("fill_oblique").to_vr_camera()
        for skip in (0, 1):
            p = vr_amd.default_params(skip_empty=skip, shading=1)
            assert np.all(rp.render(cam, p) == CLEAR)
            w = rp.count_work(cam, p)
            assert w["rays"] > 0 and w["shaded_samples"] == 0
            if skip:
                assert w["samples"] == 0 and w["skipped_samples"] > 0
            else:
                assert w["samples"] > 0
    finally:
        rp.close()


def test_isovalue_below_everything_shows_every_sampled_ray(gpu):
    """iso = -1 on a non-negative volume: every ray with an in-slab sample hits at it (a cap),
    unshaded: the TF colour at t = (iso - vmin) / range, alpha 1.  Which rays have a sample:
    the MIP frame of the same scene (alpha 128/255 everywhere: it differs from the clear
    colour's alpha exactly there)."""
    tf = (synth.tf_color() & np.uint32(0x00FFFFFF)) | np.uint32(0x80000000)
    vol = volume("g20")
    assert vol.min() >= 0.0
    rp = iso_pass(45, 35, vol, tf, -1.0, SLICE)
    try:
        cam = synth.camera("fill_oblique").to_vr_camera()
        p = vr_amd.default_params(shading=0)
        img = rp.render(cam, p)
        rp.render_mode_changed(vr_amd.MODE_MIP)
        mip = rp.render(cam, p)
        sampled = np.any(mip != CLEAR, axis=-1)
        assert 0 < sampled.sum() < sampled.size
        assert np.array_equal(np.any(img != CLEAR, axis=-1), sampled)
        ds = synth.dataset(np.asarray(vol))
        t = (np.float32(-1.0) - np.float32(ds.vmin)) / (np.float32(ds.vmax) - np.float32(ds.vmin))
        c = pyoracle.tf_sample(tf, t)
        want = np.array([c[0], c[1], c[2], 1.0], np.float32)
        assert np.all(img[sampled] == want)
    finally:
        rp.close()


def test_half_space_is_lit_by_the_ray_direction(gpu):
    """v = 1 for x >= n/2, else 0, isovalue 0.5, ambient 0, diffuse 1, specular 0: the surface is
    the plane x = 0.5 with the gradient along x, so away from the volume's faces a hit pixel is
    c |dir_x| (the sign-free headlight, the axis order)."""
    n = 16
    vol = np.zeros((n, n, n), np.float32)
    vol[:, :, n // 2:] = 1.0
    w, h = 45, 35
    cam = synth.camera("diag").to_vr_camera()
    p = vr_amd.default_params(shading=1, ambient=0.0, diffuse=1.0, specular=0.0)
    sc = pyoracle.Scene.from_params(vol, 0.0, 1.0, synth.tf_color(), cam, w, h, p)
    c = pyoracle.tf_sample(synth.tf_color(), np.float32(0.5))
    rp = iso_pass(w, h, vol, synth.tf_color(), 0.5)
    try:
        img = rp.render(cam, p)
    finally:
        rp.close()
    checked = 0
    for py in range(h):
        for px in range(w):
            ok, tex, _frag, d = sc.pixel_ray(px, py)
            # rays that enter the empty half and cross the plane x = 0.5 well inside the cube
            if not ok or abs(d[0]) < 0.1 or (0.5 - tex[0]) / d[0] <= 0.1 or not tex[0] < 0.4:
                continue
            t = (0.5 - tex[0]) / d[0]
            y, z = tex[1] + t * d[1], tex[2] + t * d[2]
            if not (0.2 < y < 0.8 and 0.2 < z < 0.8):
                continue
            want = np.array([c[0], c[1], c[2]], np.float64) * abs(float(d[0]))
            assert np.all(np.abs(img[py, px, :3] - want) <= 1e-5), (px, py, img[py, px], want)
            assert img[py, px, 3] == 1.0
            checked += 1
    assert checked >= 30


# ---- 5. state -----------------------------------------------------------------------------------------
def test_isovalue_state(gpu):
    vol, tf = volume("g20"), synth.tf_color()
    rp = vr_amd.OffscreenPass(W, H)
    try:
        assert rp.isovalue == 0.0
        rp.volume_dataset_changed(synth.dataset(np.asarray(vol)))
        rp.transfer_function_changed(tf)
        rp.isovalue_changed(0.25)
        rp.volume_dataset_changed(synth.dataset(np.asarray(volume("g13"))))
        rp.transfer_function_changed(synth.tf2())
        for mode in (vr_amd.MODE_ISO, vr_amd.MODE_MIP, vr_amd.MODE_COMPOSITE, vr_amd.MODE_ISO):
            rp.render_mode_changed(mode)
            assert rp.isovalue == 0.25
        L = vr_amd.lib()
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert L.vr_set_isovalue(rp._ctx, bad) == -22
            assert rp.isovalue == 0.25
        with pytest.raises(RuntimeError, match="not finite"):
            rp.isovalue_changed(float("nan"))
        for bad in (2, -1):  # 2 stays unassigned
            assert L.vr_set_render_mode(rp._ctx, bad) == -22
            assert rp.render_mode == vr_amd.MODE_ISO
        with pytest.raises(RuntimeError, match="spec_power"):
            rp.render(synth.camera("rotA").to_vr_camera(), vr_amd.default_params(spec_power=-1))
    finally:
        rp.close()


# ---- 6. nothing else moves ----------------------------------------------------------------------------
def test_iso_frames_leave_the_composite_and_mip_untouched(gpu):
    vol, tf = volume("g20"), synth.tf_color()
    cam = synth.camera("fill_oblique").to_vr_camera()
    iso = isovalue(vol, 0.2)
    ref, st, _, _ = reference("g20", "fill_oblique", iso, FULL, 45, 35)
    rp = vr_amd.OffscreenPass(45, 35)
    try:
        rp.volume_dataset_changed(synth.dataset(np.asarray(vol)))
        rp.transfer_function_changed(tf)
        rp.isovalue_changed(iso)
        p = vr_amd.default_params(shading=1, exact_gradient=1)
        with rp.knobs(grad_field=1):  # the difference field is built
            before = rp.render(cam, p)
            assert rp.memory_report()["field_bytes"] > 0
            rp.render_mode_changed(vr_amd.MODE_MIP)
            mip_before = rp.render(cam, vr_amd.default_params())
            rp.render_mode_changed(vr_amd.MODE_ISO)
            rep = rp.memory_report()
            frames = [rp.render(cam, vr_amd.default_params(shading=1, ert_eps=e, exact_gradient=x, skip_empty=k))
                      for e in (0.0, 1e-3) for x in (0, 1) for k in (0, 1)]
            assert all(np.array_equal(bits(f), bits(ref)) for f in frames)
            assert "iso_kernel" in rp.kernel_name(p) and "iso_kernel" in rp.last_kernel_name()
            after = rp.memory_report()  # ISO built the ranges and nothing else, evicted nothing
            assert after["field_bytes"] == rep["field_bytes"] and after["evictions"] == rep["evictions"]
            assert after["builds"] == rep["builds"] + 1
            rp.render_mode_changed(vr_amd.MODE_MIP)
            assert np.array_equal(bits(rp.render(cam, vr_amd.default_params())), bits(mip_before))
            rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
            assert "march_kernel" in rp.kernel_name(p)
            assert np.array_equal(bits(rp.render(cam, p)), bits(before))
    finally:
        rp.close()


def test_budget_zero_renders_the_same_bytes_with_one_downgrade(gpu):
    vol = volume("g20")
    iso = isovalue(vol, 0.2)
    ref, st, _, _ = reference("g20", "fill_oblique", iso, FULL, 45, 35)
    rp = iso_pass(45, 35, vol, synth.tf_color(), iso)
    try:
        cam = synth.camera("fill_oblique").to_vr_camera()
        rp.set_memory_budget(0)
        down = rp.memory_report()["downgrades"]
        p = vr_amd.default_params(skip_empty=1, shading=1)
        assert np.array_equal(bits(rp.render(cam, p)), bits(ref))
        m = rp.memory_report()
        assert m["downgrades"] == down + 1 and vr_amd.DERIVED[m["last_downgrade"]] == "skip"
        assert "iso_kernel<float, false, false" in rp.last_kernel_name()
        w = rp.count_work(cam, p)
        assert w["skipped_samples"] == 0 and w["samples"] == st["samples"]
    finally:
        rp.close()


def test_prepare_builds_the_ranges(gpu):
    vol = volume("g20")
    rp = iso_pass(W, H, vol, synth.tf_color(), isovalue(vol, 0.2))
    try:
        cam = synth.camera("rotA").to_vr_camera()
        p = vr_amd.default_params(skip_empty=1, shading=1)
        builds = rp.memory_report()["builds"]
        assert "iso_kernel<float, false, false" in rp.kernel_name(p)
        rp.prepare(cam, p)
        assert rp.memory_report()["builds"] == builds + 1
        assert "iso_kernel<float, false, true" in rp.kernel_name(p)
        rp.isovalue_changed(isovalue(vol, 0.4))  # invalidates nothing
        rp.transfer_function_changed(synth.tf2())
        rp.render(cam, p)
        assert rp.memory_report()["builds"] == builds + 1
        rp.timing_enable(True)
        rp.timing_reset()
        rp.render(cam, p, vr_amd.OUT_RGBA8)
        ms, n = rp.timing_read()
        assert n == 1 and ms > 0.0
    finally:
        rp.close()


# ---- 7. shards, members, streams ---------------------------------------------------------------------
def test_row_shards_assemble_to_the_full_frame(gpu):
    import torch
    w, h = 45, 35
    vol = volume("g20")
    rp = iso_pass(w, h, vol, synth.tf_color(), isovalue(vol, 0.2))
    try:
        cam = synth.camera("fill_oblique").to_vr_camera()
        for skip in (0, 1):
            p = vr_amd.default_params(skip_empty=skip, shading=1)
            full = torch.empty((h, w), dtype=torch.int32, device="cuda")
            rp.render_device(cam, p, full.data_ptr(), vr_amd.OUT_RGBA8, 16, 0, 1)
            whole = rp.count_work(cam, p)
            nranks, rb = 3, 8
            sr = rp.shard_rows(h, rb, nranks)
            gathered = torch.zeros((nranks, sr, w), dtype=torch.int32, device="cuda")
            for r in range(nranks):
                rp.render_device(cam, p, gathered[r].data_ptr(), vr_amd.OUT_RGBA8, rb, r, nranks)
            out = torch.empty((h, w), dtype=torch.int32, device="cuda")
            rp.assemble_rows(gathered.data_ptr(), out.data_ptr(), vr_amd.OUT_RGBA8, rb, nranks)
            torch.cuda.synchronize()
            assert torch.equal(out, full), skip
            assert np.array_equal(full.cpu().numpy().view(np.uint8).reshape(h, w, 4),
                                  rp.render(cam, p, vr_amd.OUT_RGBA8))
            parts = [rp.count_work(cam, p, rb, r, nranks) for r in range(nranks)]
            assert {k: sum(x[k] for x in parts) for k in whole} == whole
    finally:
        rp.close()


@pytest.mark.parametrize("group", [dict(device_mask=1), dict(members=(0, 0, 0))])
def test_member_contexts_equal_the_single_context(gpu, group):
    w, h = 45, 35
    vol, tf = volume("g20"), synth.tf_color()
    iso = isovalue(vol, 0.2)
    one = iso_pass(w, h, vol, tf, iso)
    grp = vr_amd.OffscreenPass(w, h, exchange=vr_amd.EXCHANGE_COPY, **group)
    try:
        grp.volume_dataset_changed(synth.dataset(np.asarray(vol)))
        grp.transfer_function_changed(tf)
        cam = synth.camera("fill_oblique").to_vr_camera()
        p = vr_amd.default_params(skip_empty=1, shading=1)
        comp = grp.render(cam, p)
        grp.render_mode_changed(vr_amd.MODE_ISO)  # both forwarded to every member
        grp.isovalue_changed(iso)
        assert grp.render_mode == vr_amd.MODE_ISO and np.float32(grp.isovalue) == iso
        assert "iso_kernel" in grp.kernel_name(p)
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
    w, h = 45, 35
    vol = volume("g20")
    rp = iso_pass(w, h, vol, synth.tf_color(), isovalue(vol, 0.2))
    try:
        cam = synth.camera("fill_oblique").to_vr_camera()
        for skip in (0, 1):
            p = vr_amd.default_params(skip_empty=skip, shading=1, frames_in_flight=3)
            ref = torch.empty((h, w), dtype=torch.int32, device="cuda")
            rp.render_device(cam, vr_amd.default_params(skip_empty=skip, shading=1), ref.data_ptr(),
                             vr_amd.OUT_RGBA8)
            torch.cuda.synchronize()
            streams = [torch.cuda.Stream() for _ in range(3)]
            outs = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(3)]
            for i, o in enumerate(outs):
                rp.render_device(cam, p, o.data_ptr(), vr_amd.OUT_RGBA8, 16, 0, 1, streams[i].cuda_stream)
            torch.cuda.synchronize()
            for i, o in enumerate(outs):
                assert torch.equal(o, ref), (skip, i)
    finally:
        rp.close()


# ---- 8. CLI ---------------------------------------------------------------------------------------------
def test_cli_mode_iso(gpu, tmp_path):
    cli = os.path.join(os.path.dirname(vr_amd.LIB_PATH), "vr_cli")
    w, h = 96, 64
    out = str(tmp_path / "f.ppm")
    rp = vr_amd.OffscreenPass(w, h)
    try:
        lo, hi = rp.generate_volume((40, 40, 40), np.float32, seed=2024)[:2]
        iso = float(np.float32(lo + 0.3 * (hi - lo)))
        rp.transfer_function_changed(synth.tf2())
        cam = vr_amd.make_camera(radius=2.0, rotate=(100.0, 60.0)).to_vr_camera()
        comp = rp.render(cam, vr_amd.default_params(), vr_amd.OUT_RGBA8)
        rp.render_mode_changed(vr_amd.MODE_ISO)
        rp.isovalue_changed(iso)
        ref = rp.render(cam, vr_amd.default_params(shading=1), vr_amd.OUT_RGBA8)
    finally:
        rp.close()
    assert np.any(ref[..., :3] != vr_amd.unorm8(CLEAR)[:3])
    for extra in ([], ["--skip-empty"]):
        r = subprocess.run([cli, "synthetic:40", out, "--size", f"{w}x{h}", "--radius", "2", "--rotate",
                            "100,60", "--tf", "demo", "--shading", "--mode", "iso", "--iso", repr(iso), *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        data = open(out, "rb").read().split(b"\n", 3)
        img = np.frombuffer(data[3], np.uint8).reshape(h, w, 3)
        assert np.array_equal(img, ref[..., :3]) and not np.array_equal(img, comp[..., :3])
    # --iso without --mode iso sets the state and renders the composite
    r = subprocess.run([cli, "synthetic:40", out, "--size", f"{w}x{h}", "--radius", "2", "--rotate", "100,60",
                        "--tf", "demo", "--iso", repr(iso)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = np.frombuffer(open(out, "rb").read().split(b"\n", 3)[3], np.uint8).reshape(h, w, 3)
    assert np.array_equal(img, comp[..., :3])
    r = subprocess.run([cli, "synthetic:8", out, "--mode", "average"], capture_output=True, text=True)
    assert r.returncode == 2
