"""GPU: what the analysis calls (vr_hist.h, vr_label.h, vr_mesh.h) refuse, pinned by return code and
by the exact vr_last_error text.  One context, one generated 12 x 10 x 9 f32 volume, a few seconds.
Every case is refused on the host before any launch, or is a VR_ENOSPC after a normal count.

The texts are read from tests/golden/refusal_messages.json, which `python tests/test_gpu_refusals.py`
records (VR_AMD_LIB chooses the library: the file was recorded with the build of the commit before
the calls moved out of vr_api.hip, not with the code under test).

"No volume" cannot be reached through the ABI: a context always holds a volume, a fresh one the
one-voxel placeholder it is created with (vr_label.h says so).  The `fresh_*` cases therefore ask a
fresh context for the box of the volume that is uploaded only afterwards, once per family."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import vr_amd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusal_messages.json")
DIMS = (12, 10, 9)
VOXELS = DIMS[0] * DIMS[1] * DIMS[2]
WHOLE = ((0, 0, 0), DIMS)
EMPTY = ((3, 3, 3), (3, 4, 4))
BEYOND = ((0, 0, 0), (13, 10, 9))
EINVAL, ENOSPC = -22, -28
INF = float("inf")


def _hist_request(box=None, use_box=None, nbins=16, lo=0.0, hi=1.0):
    req = vr_amd.vr_hist_request()
    req.lo, req.hi, req.nbins = lo, hi, nbins
    if box is not None:
        req.use_box = 1
        for a in range(3):
            req.box_min[a], req.box_max[a] = box[0][a], box[1][a]
    if use_box is not None:
        req.use_box = use_box
    return req


def _with_use_box(req, use_box):
    req.use_box = use_box
    return req


def drive():
    """Every refusal once: {case: (rc, vr_last_error text, facts the case checks beside them)}."""
    L = vr_amd.lib()
    rp = vr_amd.OffscreenPass(64, 48, device=0)
    ctx = rp._ctx
    out = {}

    def note(name, rc, **facts):
        out[name] = (int(rc), L.vr_last_error(ctx).decode(), facts)

    bins = np.full(16, 77, np.uint64)
    labels = np.full(VOXELS, 0x77777777, np.uint32)
    comps = np.zeros(4, vr_amd.LABEL_COMPONENT_DTYPE)
    comps.view(np.uint8)[:] = 0x77
    mask = np.full(VOXELS, 0x77, np.uint8)
    verts = np.zeros(1 << 14, vr_amd.MESH_VERTEX_DTYPE)
    tris = np.zeros((1 << 15, 3), np.uint32)
    seed_in = (C.c_uint32 * 3)(3, 3, 3)

    def hist(name, req):
        info = vr_amd.vr_hist_info()
        C.memset(C.byref(info), 0x77, C.sizeof(info))
        rc = L.vr_histogram(ctx, C.byref(req), bins.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info))
        note(name, rc, untouched=bytes(info) == b"\x77" * C.sizeof(info) and bool(np.all(bins == 77)))

    def label_count(name, req):
        info = vr_amd.vr_label_info()
        C.memset(C.byref(info), 0x77, C.sizeof(info))
        rc = L.vr_label_count(ctx, C.byref(req), C.byref(info))
        note(name, rc, untouched=bytes(info) == b"\x77" * C.sizeof(info))

    def mesh_count(name, req):
        info = vr_amd.vr_mesh_info()
        C.memset(C.byref(info), 0x77, C.sizeof(info))
        rc = L.vr_mesh_count(ctx, C.byref(req), C.byref(info))
        note(name, rc, untouched=bytes(info) == b"\x77" * C.sizeof(info))

    def grow(name, req, seed, mcap):
        comp = vr_amd.vr_label_component()
        C.memset(C.byref(comp), 0x77, C.sizeof(comp))
        rc = L.vr_region_grow(ctx, C.byref(req), seed, mask.ctypes.data, mcap, C.byref(comp))
        note(name, rc, untouched=bytes(comp) == b"\x77" * C.sizeof(comp) and bool(np.all(mask == 0x77)))

    # a fresh context holds the one-voxel placeholder: the box of the volume to come lies beyond it
    hist("fresh_hist", _hist_request(WHOLE))
    label_count("fresh_label", vr_amd.label_request(-INF, INF, 6, WHOLE))
    mesh_count("fresh_mesh", vr_amd.mesh_request(0.5, box=WHOLE))

    lo, hi = rp.generate_volume(DIMS, np.float32, seed=7)
    assert lo < hi
    iso = 0.5 * (lo + hi)

    # the request box: empty, beyond the volume, use_box = 2
    for tag, box in (("empty", EMPTY), ("beyond", BEYOND)):
        hist(f"hist_box_{tag}", _hist_request(box))
        label_count(f"label_box_{tag}", vr_amd.label_request(-INF, INF, 6, box))
        mesh_count(f"mesh_box_{tag}", vr_amd.mesh_request(iso, box=box))
    hist("hist_use_box_2", _hist_request(use_box=2))
    label_count("label_use_box_2", _with_use_box(vr_amd.label_request(-INF, INF, 6), 2))
    mesh_count("mesh_use_box_2", _with_use_box(vr_amd.mesh_request(iso), 2))
    # the request's own fields, one per family
    hist("hist_nbins_0", _hist_request(nbins=0))
    label_count("label_connectivity_5", vr_amd.label_request(-INF, INF, 5))
    mesh_count("mesh_iso_nan", vr_amd.mesh_request(float("nan")))

    # a seed outside the box; a misaligned device label buffer (refused before it is looked at)
    inner = vr_amd.label_request(-INF, INF, 6, ((2, 2, 2), (6, 6, 6)))
    grow("seed_outside", inner, (C.c_uint32 * 3)(1, 3, 3), VOXELS)
    info = vr_amd.vr_label_info()
    rc = L.vr_label_components_device(ctx, C.byref(inner), C.c_void_p(0x1002), 64, C.c_void_p(0x1000), 4,
                                      C.byref(info), None)
    note("labels_dev_misaligned", rc)

    # capacities one too small.  The window takes every voxel: one component of VOXELS voxels.
    every = vr_amd.label_request(-INF, INF, 6)
    want = rp.label_count(-INF, INF, 6)
    assert want["voxels"] == VOXELS and want["components"] == 1
    info = vr_amd.vr_label_info()
    C.memset(C.byref(info), 0x77, C.sizeof(info))
    rc = L.vr_label_components(ctx, C.byref(every), labels.ctypes.data, VOXELS - 1, comps.ctypes.data, 4,
                               C.byref(info))
    note("lcap", rc, info=rp._label_info(info), buffers_untouched=bool(np.all(labels == 0x77777777)),
         want={"voxels": VOXELS, "in_voxels": 0, "components": 0, "largest_voxels": 0, "largest_label": 0})
    rc = L.vr_label_components(ctx, C.byref(every), labels.ctypes.data, VOXELS, comps.ctypes.data, 0,
                               C.byref(info))
    note("ccap", rc, info=rp._label_info(info), want=want,
         buffers_untouched=bool(np.all(comps.view(np.uint8) == 0x77)), labels_complete=bool(np.all(labels == 1)))
    grow("mcap", every, seed_in, VOXELS - 1)
    mwant = rp.mesh_count(iso)
    assert mwant["vertices"] > 0 and mwant["triangles"] > 0
    minfo = vr_amd.vr_mesh_info()
    mreq = vr_amd.mesh_request(iso)
    rc = L.vr_mesh_extract(ctx, C.byref(mreq), verts.ctypes.data, mwant["vertices"] - 1, tris.ctypes.data,
                           mwant["triangles"], C.byref(minfo))
    note("vcap", rc, info=rp._mesh_info(minfo), want=mwant,
         buffers_untouched=not verts.view(np.uint8).any() and not tris.any())
    rp.close()
    return out


@pytest.fixture(scope="module")
def refusals(gpu):
    return drive()


def _golden():
    return json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}  # (none yet while it is recorded)


@pytest.mark.gpu
def test_every_recorded_refusal_is_driven(refusals):
    assert set(refusals) == set(_golden()) and len(refusals) >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_golden()))
def test_refusal_code_and_text(refusals, case):
    rc, text, facts = refusals[case]
    g = _golden()[case]
    assert (rc, text) == (g["rc"], g["error"])
    assert rc == (ENOSPC if case in ("lcap", "ccap", "mcap", "vcap") else EINVAL)
    if "untouched" in facts:
        assert facts["untouched"]
    if "want" in facts:  # the info's counts, filled as vr_label.h and vr_mesh.h say
        assert facts["info"] == facts["want"] and facts["buffers_untouched"]
        assert facts.get("labels_complete", True)


if __name__ == "__main__":
    recorded = {k: {"rc": rc, "error": text} for k, (rc, text, _) in sorted(drive().items())}
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=1)
        f.write("\n")
    print(f"recorded {GOLDEN} with {vr_amd.LIB_PATH}")
