"""GPU: the kernel a launch runs is the kernel the host names (csrc/vr_variant.h).

Every variant family is forced through the vr_debug.h knobs on small scenes that still cross
every edge: a 20 x 18 x 22 volume (more than one brick per axis, a multiple of none), a 50 x 35
frame (partial tiles in x and y, also of the 16 x 8 and 16 x 4 lane-group tiles), a 256-texel TF
and a 257-texel one (past the LDS copy).  After each frame vr_debug_last_kernel_name must be
what vr_kernel_name predicts -- the march_pair_kernel of the same type, shade and field flags
where lane groups ran, the counting variant after vr_count_work -- and the frame must equal
the oracle bit for bit.  One oracle frame per (volume, TF, shading, gradient precision, mode),
shared by every knob setting."""
import itertools
import re

import numpy as np
import pytest

import proj_ref
import pyoracle
import synth
import vr_amd

pytestmark = pytest.mark.gpu

W, H = 50, 35
DIMS = (20, 18, 22)
CAM = "fill_oblique"  # fills the frame: the partial tiles hold rays
MIP_CAM = "default"   # the Python MIP reference is slow: fewer rays


def _volume(kind):
    base = synth.gaussians_numpy(DIMS, seed=11)
    if kind == "f32":
        v = base.astype(np.float32)
    elif kind == "u16":
        v = np.rint(base / base.max() * 40000).astype(np.uint16)
    else:  # u8_plain, u8_quad: the same voxels in the two 8-bit layouts
        v = np.rint(base / base.max() * 255).astype(np.uint8)
    v.setflags(write=False)
    return v


VOLUMES = {k: _volume(k) for k in ("f32", "u8", "u16")}
STORAGES = {"f32": ("f32", -1), "u8_plain": ("u8", 0), "u8_quad": ("u8", 1), "u16": ("u16", -1)}
TYPE_TAG = {"f32": "float", "u8_plain": "unsigned char", "u8_quad": "vr::Quad8<unsigned char>",
            "u16": "unsigned short"}
TFS = {n: synth.tf_band(0.2, 0.95, n) for n in (256, 257)}
_oracle = {}


def oracle(vol, tf_n, shading, f16):
    key = (vol, tf_n, shading, f16)
    if key not in _oracle:
        v = VOLUMES[vol].astype(np.float32)
        p = vr_amd.default_params(shading=shading)
        ref, _ = pyoracle.Scene.from_params(v, float(v.min()), float(v.max()), TFS[tf_n],
                                            synth.camera(CAM).to_vr_camera(), W, H, p,
                                            grad_f16=f16).render()
        ref.setflags(write=False)
        _oracle[key] = ref
    return _oracle[key]


def mip_oracle(vol):
    def make():
        v = VOLUMES[vol].astype(np.float32)
        return pyoracle.Scene.from_params(v, float(v.min()), float(v.max()), TFS[256],
                                          synth.camera(MIP_CAM).to_vr_camera(), W, H,
                                          vr_amd.default_params())
    return proj_ref.cached(("variant", vol, MIP_CAM, W, H), make, "mip")[0]


def same_bits(img, ref):
    return np.array_equal(np.ascontiguousarray(img, np.float32).view(np.uint32),
                          np.ascontiguousarray(ref, np.float32).view(np.uint32))


MARCH = re.compile(r"^(.*::)march_kernel<(.+), (true|false), (true|false), (true|false), "
                   r"(true|false), (true|false)>\(vr::MarchParams\)$")
MIP = re.compile(r"^(.*::)mip_kernel<(.+), (true|false), (true|false), (\d)>(\(.*\))$")


def pair_name(name, lanes):
    ns, vt, shade, _count, _skip, gf, _pipe = MARCH.match(name).groups()
    return f"{ns}march_pair_kernel<{vt}, {shade}, {gf}, {lanes}>(vr::MarchParams)"


def count_name(name):
    m = MARCH.match(name)
    if m:
        ns, vt, shade, _count, skip, gf, _pipe = m.groups()
        return f"{ns}march_kernel<{vt}, {shade}, true, {skip}, {gf}, false>(vr::MarchParams)"
    ns, vt, _count, skip, _k, args = MIP.match(name).groups()
    return f"{ns}mip_kernel<{vt}, true, {skip}, 1>{args}"


@pytest.fixture(scope="module")
def rp(gpu):
    r = vr_amd.OffscreenPass(W, H, device=0)
    assert r.last_kernel_name() == ""
    yield r
    r.close()


def upload(rp, storage):
    vol, u8_layout = STORAGES[storage]
    with rp.knobs(u8_layout=u8_layout):
        rp.volume_dataset_changed(synth.dataset(VOLUMES[vol]))
    return vol


def composite_cases(storage):
    """(knobs, params, lanes that run or 0, name fragment expected or None)"""
    f32 = storage == "f32"
    fields = (0, 1) if f32 else (0,)
    exacts = (0, 1) if f32 else (1,)
    for pipe, gf, shading, exact, skip in itertools.product((0, 1), fields, (0, 1), exacts, (0, 1)):
        yield (dict(pipeline=pipe, grad_field=gf, alt_geometry=0, pair=0),
               dict(shading=shading, exact_gradient=exact, skip_empty=skip), 0, None)
    for lanes, gf, shading, exact in itertools.product((2, 4), fields, (0, 1), exacts):
        yield (dict(pipeline=0, grad_field=gf, alt_geometry=0, pair=1, pair_lanes=lanes),
               dict(shading=shading, exact_gradient=exact, skip_empty=0), lanes, None)
    if f32:
        for alt, pipe, shading in itertools.product((1, 3, 4), (0, 1), (0, 1)):
            yield (dict(pipeline=pipe, grad_field=0, alt_geometry=alt, pair=0),
                   dict(shading=shading, skip_empty=0), 0, {1: "F32Alt", 3: "F32P", 4: "F32S"}[alt])


@pytest.mark.parametrize("storage", list(STORAGES))
def test_composite_launch_runs_the_named_kernel(rp, storage):
    vol = upload(rp, storage)
    cam = synth.camera(CAM).to_vr_camera()
    seen = set()
    for tf_n in (256, 257):
        rp.transfer_function_changed(TFS[tf_n])
        for knobs, params, lanes, fragment in composite_cases(storage):
            what = (storage, tf_n, knobs, params)
            p = vr_amd.default_params(**params)
            if tf_n > 256:
                lanes = 0  # lane groups stage the TF in LDS: such frames run single-lane
            # the binary16 field: shaded f32 frames told to read the field, exact_gradient 0
            half = bool(storage == "f32" and params["shading"] and knobs["grad_field"] == 1 and
                        params.get("exact_gradient") == 0)
            with rp.knobs(**knobs):
                img = rp.render(cam, p, vr_amd.OUT_RGBA32F)
                name, last = rp.kernel_name(p), rp.last_kernel_name()
                assert last == (pair_name(name, lanes) if lanes else name), what
                tag = "vr::F32H" if half else ("vr::" + fragment if fragment else TYPE_TAG[storage])
                assert MARCH.match(name).group(2) == tag, what
                if fragment is None and not lanes:
                    rp.count_work(cam, p)
                    assert rp.last_kernel_name() == count_name(name), what
            ref = oracle(vol, tf_n, params["shading"], half)
            assert same_bits(img, ref), what
            seen.add(last)
            if tf_n > 256:  # past the LDS copy: no pipelined kernel either
                assert MARCH.match(last).group(7) == "false", what
    # the families this storage type has, each reached
    assert any("march_pair_kernel" in n and ", 4>" in n for n in seen)
    assert any("march_pair_kernel" in n and ", 2>" in n for n in seen)
    assert any(MARCH.match(n) and MARCH.match(n).group(7) == "true" for n in seen)
    assert any(MARCH.match(n) and MARCH.match(n).group(5) == "true" for n in seen)
    if storage == "f32":
        for tag in ("vr::F32H", "vr::F32Alt", "vr::F32P", "vr::F32S"):
            assert any(f"<{tag}," in n for n in seen), tag
        assert any(MARCH.match(n) and MARCH.match(n).groups()[1:] ==
                   ("float", "true", "false", "false", "true", "true") for n in seen)


@pytest.mark.parametrize("storage", list(STORAGES))
def test_mip_launch_runs_the_named_kernel(rp, storage):
    vol = upload(rp, storage)
    rp.transfer_function_changed(TFS[256])
    cam = synth.camera(MIP_CAM).to_vr_camera()
    ref = mip_oracle(vol)
    rp.render_mode_changed(vr_amd.MODE_MIP)
    try:
        for k, skip in itertools.product((1, 2, 4), (0, 1)):
            p = vr_amd.default_params(skip_empty=skip)
            with rp.knobs(mip_inflight=k):
                img = rp.render(cam, p, vr_amd.OUT_RGBA32F)
                name = rp.kernel_name(p)
                assert rp.last_kernel_name() == name, (storage, k, skip)
                assert MIP.match(name).groups()[1:5] == (
                    TYPE_TAG[storage], "false", "true" if skip else "false", str(k)), name
                rp.count_work(cam, p)
                assert rp.last_kernel_name() == count_name(name), (storage, k, skip)
            assert same_bits(img, ref), (storage, k, skip)
    finally:
        rp.render_mode_changed(vr_amd.MODE_COMPOSITE)
