"""GPU: every analysis call and render mode on thin volumes and on boxes at brick seams
(tests/edge_shapes.py says which and why; tests/test_edge_shapes_cpu.py shows on the references
alone that the scenes reach what they are here for).

Volumes of 1 to 15 voxels per axis -- every extent at which the brick count changes or the last
voxel meets a seam, on every axis -- as f32, uint16, 8-bit quads and plain 8-bit bricks; boxes of
19 x 17 x 21 one voxel thick, of one voxel, and with their faces on the seams.  Every output is
compared bit for bit with the Python reference of its call (label_ref, mesh_ref, hist_ref's window
through the three-way tie, pyoracle, proj_ref, iso_ref, hit_ref, mpr_ref), through the comparisons
of the per-feature tests; the device forms write into tensors sized by the reference's counts and
filled with a guard word."""
import numpy as np
import pytest

import edge_shapes as E
import hit_scenes
import label_ref
import label_scenes
import mesh_scenes
import mpr_ref
import proj_ref
import pyoracle
import range_scenes
import synth
import vr_amd
from gpu_kit import GUARD32
from gpu_kit import stream  # noqa: F401
from test_gpu_hit import check_records
from test_gpu_iso import check_against as check_iso
from test_gpu_label import NAME as LABEL_NAME
from test_gpu_label import check_labels, label_pass
from test_gpu_mesh import NAME as MESH_NAME
from test_gpu_mesh import check_mesh
from test_gpu_mpr import check_against as check_mpr
from test_gpu_mpr import mpr_pass

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")
SLACK = 64
P = vr_amd.default_params


def dims_id(d):
    return "x".join(str(v) for v in d) if isinstance(d[0], int) else "%s-%s" % (dims_id(d[0]), dims_id(d[1]))


def dev_guarded(nwords):
    import torch
    return torch.full((int(nwords) + SLACK,), GUARD32, dtype=torch.int32, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint32)


def label_into_guarded(rp, ref, lo, hi, conn, box, stream, what):
    """vr_label_components_device into tensors of exactly the reference's counts: more would be
    VR_ENOSPC, and nothing may be written past them.  Returns the label and record words."""
    import torch
    labels, rec, want = ref
    n, nc = want["voxels"], want["components"]
    dl, dc = dev_guarded(n), dev_guarded(nc * 16)
    torch.cuda.synchronize()
    info = rp.label_device(dl.data_ptr(), n, dc.data_ptr(), nc, lo, hi, conn, box, stream=stream.cuda_stream)
    hl, hc = host(dl), host(dc)
    assert info == want, (what, info, want)
    assert hl[:n].tobytes() == labels.tobytes() and hc[:nc * 16].tobytes() == rec.tobytes(), what
    assert np.all(hl[n:] == GUARD32) and np.all(hc[nc * 16:] == GUARD32), (what, "written past the counts")
    return hl[:n], hc[:nc * 16]


def grow_into_guarded(rp, seed, want_mask, want_comp, lo, hi, conn, box, stream, what):
    import torch
    n = want_mask.size
    dm = torch.full((n + SLACK,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    comp = rp.region_grow_device(seed, dm.data_ptr(), n, lo, hi, conn, box, stream=stream.cuda_stream)
    hm = dm.cpu().numpy()
    assert comp == want_comp, (what, comp, want_comp)
    assert hm[:n].tobytes() == want_mask.tobytes(), what
    assert np.all(hm[n:] == 0x77), (what, "written past the mask")


def check_grow(rp, vol, seed, ref, lo, hi, conn, box, stream, what, inside=None):
    want_mask, want_comp = label_ref.region_grow(vol, seed, lo, hi, conn, box, labelled=ref)
    mask, comp = rp.region_grow(seed, lo, hi, conn, box)
    assert mask.dtype == np.uint8 and mask.shape == want_mask.shape
    assert mask.tobytes() == want_mask.tobytes(), (what, seed)
    assert comp == want_comp, (what, seed, comp, want_comp)
    assert int(mask.sum()) == comp["voxels"]
    if inside is not None:
        assert (comp["voxels"] > 0) == inside, (what, seed, comp)
    grow_into_guarded(rp, seed, want_mask, want_comp, lo, hi, conn, box, stream, (what, seed))


def mesh_into_guarded(rp, ref, iso, closed, normals, box, stream, what, canonical=True):
    """vr_mesh_extract_device into tensors of exactly the reference's counts.  Returns the vertex
    and triangle words (canonical = False: the caller compares them with the host form's bytes)."""
    import torch
    nv, nt = ref.info["vertices"], ref.info["triangles"]
    dv, dt = dev_guarded(nv * 6), dev_guarded(nt * 3)
    torch.cuda.synchronize()
    info = rp.mesh_device(dv.data_ptr(), nv, dt.data_ptr(), nt, iso, closed, normals, box, stream=stream.cuda_stream)
    hv, ht = host(dv), host(dt)
    assert info == ref.info, (what, info, ref.info)
    verts = hv[:nv * 6].view(vr_amd.MESH_VERTEX_DTYPE)
    tris = ht[:nt * 3].reshape(-1, 3)
    assert nt == 0 or int(tris.max()) < nv, what
    if canonical:
        mesh_scenes.assert_same_mesh((verts, tris), (ref.verts, ref.tris), what)
    assert np.all(hv[nv * 6:] == GUARD32) and np.all(ht[nt * 3:] == GUARD32), (what, "written past the counts")
    return hv[:nv * 6], ht[:nt * 3]


# ---- 1. the analysis calls on every volume, fill and layout ---------------------------------------------
# One context per test.  The calls of one (volume, fill, layout) are four tests, so that none
# takes longer than the per-context tests of the features themselves (most of a test's time is its
# reference's).
def analysis_labels(rp, stream, dims, name, layout, vol, tag):
    """Labelling: two windows, 6 and 26, the host form, the count, the device form."""
    for lo, hi, conn in E.label_cases(dims, name):
        what = (dims, name, layout, lo, hi, conn)
        ref = E.label_reference(dims, name, lo, hi, conn)
        assert label_scenes.pinned(ref[2]) == E.LABEL_PINS[(dims, name, lo, hi, conn)]
        check_labels(rp, ref, lo, hi, conn, None, what)
        assert rp.last_kernel_name() == LABEL_NAME % (tag, conn)
        label_into_guarded(rp, ref, lo, hi, conn, None, stream, what)


def analysis_grow(rp, stream, dims, name, layout, vol, tag):
    """Region growing: voxel 0, the last voxel, a voxel on every seam, a voxel that is not in."""
    outside_seen = False
    for lo, hi in E.WINDOWS[name]:
        for conn in (6, 26):
            ref = E.label_reference(dims, name, lo, hi, conn)
            seeds, outside = E.grow_seeds(dims, ref[0], E.geometry(layout))
            for seed in seeds:
                check_grow(rp, vol, seed, ref, lo, hi, conn, None, stream, (dims, name, layout, lo, hi, conn))
            assert rp.last_kernel_name() == LABEL_NAME % (tag, conn)
            if outside is not None:
                outside_seen = True
                check_grow(rp, vol, outside, ref, lo, hi, conn, None, stream, (dims, name, layout, "outside"),
                           inside=False)
    assert outside_seen


def analysis_mesh(iso):
    def run(rp, stream, dims, name, layout, vol, tag):
        """The mesh at one isovalue: closed and open, with and without normals; the three-way tie."""
        for closed in (True, False):
            for normals in (True, False):
                what = (dims, name, layout, iso, closed, normals)
                ref = E.mesh_reference(dims, name, iso, closed, normals)
                pin = E.MESH_PINS[(dims, name, iso, closed)]
                assert (ref.info["vertices"], ref.info["triangles"], ref.info["inside_voxels"]) == pin
                verts, _ = check_mesh(rp, ref, iso, closed, normals, None, what)
                assert rp.last_kernel_name() == MESH_NAME % tag
                if not normals:
                    assert not verts["normal"].view(np.uint32).any()
                mesh_into_guarded(rp, ref, iso, closed, normals, None, stream, what)
        # the mesh's inside voxels, the window [iso, inf]'s in-voxels, the histogram's count of [iso, max]
        inside = E.MESH_PINS[(dims, name, iso, True)][2]
        assert rp.mesh_count(iso, False, False)["inside_voxels"] == inside == int((vol >= F(iso)).sum())
        assert rp.label_count(iso, INF, 6)["in_voxels"] == inside
        top = float(np.nextafter(F(max(float(vol.max()), iso)), F(INF)))
        bins, _ = rp.histogram(1, iso, top)
        assert int(bins[0]) == inside, (dims, name, layout, iso, int(bins[0]), inside)
    return run


ANALYSIS = {"label": analysis_labels, "grow": analysis_grow,
            "mesh%g" % E.ISOS[0]: analysis_mesh(E.ISOS[0]), "mesh%g" % E.ISOS[1]: analysis_mesh(E.ISOS[1])}


@pytest.mark.parametrize("call", list(ANALYSIS))
@pytest.mark.parametrize("layout", list(E.LAYOUTS))
@pytest.mark.parametrize("name", E.FILLS)
@pytest.mark.parametrize("dims", E.VOLUMES, ids=dims_id)
def test_analysis_calls(gpu, stream, dims, name, layout, call):
    dtype, knobs, storage, tag = E.LAYOUTS[layout]
    vol = E.fill(dims, name)
    rp = label_pass(vol.astype(dtype), **knobs)
    try:
        info = rp.volume_info()
        assert tuple(info[0]) == dims and info[2] == storage
        ANALYSIS[call](rp, stream, dims, name, layout, vol, tag)
    finally:
        rp.close()


# ---- 2. boxes of 19 x 17 x 21 at the seams ------------------------------------------------------------------
_box_pass = {}


@pytest.fixture(scope="module")
def box_pass(gpu):
    """One context per layout for the whole module (the volumes are never modified)."""
    def get(layout):
        if layout not in _box_pass:
            dtype, knobs, storage, _ = E.LAYOUTS[layout]
            rp = label_pass(E.box_volume(layout).astype(dtype), **knobs)
            assert rp.volume_info()[2] == storage
            _box_pass[layout] = rp
        return _box_pass[layout]
    yield get
    for rp in _box_pass.values():
        rp.close()
    _box_pass.clear()


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("layout", E.BOX_LAYOUTS)
@pytest.mark.parametrize("box", E.BOXES, ids=dims_id)
def test_labels_of_boxes_at_the_seams(gpu, stream, box_pass, box, layout, conn):
    rp = box_pass(layout)
    tag = E.LAYOUTS[layout][3]
    s = E.box_scale(layout)
    lo, hi = E.BOX_WINDOW[0] * s, E.BOX_WINDOW[1] * s
    what = (layout, box, conn)
    ref = E.box_label_reference(layout, box, conn)
    assert label_scenes.pinned(ref[2]) == E.BOX_LABEL_PINS[(layout, box, conn)]
    assert (ref[2]["in_voxels"] == 0) == (box in E.EMPTY_BOXES[layout])
    labels, rec, _ = check_labels(rp, ref, lo, hi, conn, box, what)
    assert rp.last_kernel_name() == LABEL_NAME % (tag, conn)
    # the device form on a second stream writes the same bytes
    dl, dc = label_into_guarded(rp, ref, lo, hi, conn, box, stream, what)
    assert dl.tobytes() == labels.tobytes() and dc.tobytes() == rec.tobytes()
    check_grow(rp, E.box_volume(layout), E.box_seed(box, ref[0]), ref, lo, hi, conn, box, stream, what,
               inside=ref[2]["in_voxels"] > 0)
    if box == E.WHOLE:  # the whole volume as a box: the call without a box, byte for byte
        l0, r0, i0 = rp.label(lo, hi, conn, None)
        assert i0 == ref[2] and l0.tobytes() == labels.tobytes() and r0.tobytes() == rec.tobytes()


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("layout", E.BOX_LAYOUTS)
@pytest.mark.parametrize("box", E.BOXES, ids=dims_id)
def test_meshes_of_boxes_at_the_seams(gpu, stream, box_pass, box, layout, closed):
    rp = box_pass(layout)
    tag = E.LAYOUTS[layout][3]
    iso = E.BOX_ISO * E.box_scale(layout)
    normals = E.box_normals(box)
    what = (layout, box, closed)
    ref = E.box_mesh_reference(layout, box, closed, normals)
    assert (ref.info["vertices"], ref.info["triangles"], ref.info["inside_voxels"]) == \
        E.BOX_MESH_PINS[(layout, box, closed)]
    verts, tris = check_mesh(rp, ref, iso, closed, normals, box, what)
    assert rp.last_kernel_name() == MESH_NAME % tag
    # the device form on a second stream writes the same bytes
    dv, dt = mesh_into_guarded(rp, ref, iso, closed, normals, box, stream, what, canonical=False)
    assert dv.tobytes() == verts.tobytes() and dt.tobytes() == tris.tobytes()
    if box == E.WHOLE:
        v0, t0, i0 = rp.mesh(iso, closed, normals, None)
        assert i0 == ref.info and v0.tobytes() == verts.tobytes() and t0.tobytes() == tris.tobytes()


# ---- 3. frames and hit records on a grid one brick thin -------------------------------------------------------
_ray_pass = {}


@pytest.fixture(scope="module")
def ray_pass(gpu):
    """One context per volume and layout, shared by the tests of that volume (the eight used last
    stay open); a test sets the slicing box and the mode it needs."""
    def get(dims, layout):
        if (dims, layout) not in _ray_pass:
            while len(_ray_pass) >= 8:
                _ray_pass.pop(next(iter(_ray_pass))).close()
            dtype, knobs, storage, _ = E.LAYOUTS[layout]
            vol = E.fill(dims, "noise")
            rp = hit_scenes.hit_pass(E.W, E.H, vol.astype(dtype), synth.tf_color(), E.isovalue(vol), **knobs)
            assert tuple(rp.volume_info()[0]) == dims and rp.volume_info()[2] == storage
            _ray_pass[(dims, layout)] = rp
        _ray_pass[(dims, layout)] = _ray_pass.pop((dims, layout))  # most recently used last
        return _ray_pass[(dims, layout)]
    yield get
    for rp in _ray_pass.values():
        rp.close()
    _ray_pass.clear()


def ray_setup(ray_pass, dims, camname, boxname, layout, mode):
    rp = ray_pass(dims, layout)
    box = E.ray_box(dims, boxname, layout)
    rp.slicing_changed(*box)
    rp.render_mode_changed(mode)
    return rp, box, E.camera(camname).to_vr_camera()


RAY = pytest.mark.parametrize("dims,camname,boxname", E.ray_scenes(),
                              ids=["%s-%s-%s" % (dims_id(d), c, b) for d, c, b in E.ray_scenes()])
RAY_LAYOUT = pytest.mark.parametrize("layout", E.RAY_LAYOUTS)


@RAY_LAYOUT
@RAY
def test_composite_frames(gpu, ray_pass, dims, camname, boxname, layout):
    rp, box, cam = ray_setup(ray_pass, dims, camname, boxname, layout, vr_amd.MODE_COMPOSITE)
    vol = E.fill(dims, "noise")
    for shading, exact in ((0, 0), (1, 0), (1, 1)):
        for skip in (0, 1):
            p = P(shading=shading, exact_gradient=exact, skip_empty=skip)
            img = rp.render(cam, p, vr_amd.OUT_RGBA32F)
            half = "F32H" in rp.kernel_name(p)  # the oracle restates the binary16 field where it is read
            sc = pyoracle.Scene.from_params(vol, float(vol.min()), float(vol.max()), synth.tf_color(), cam, E.W, E.H,
                                            p, box[0], box[1], grad_f16=half)
            ref, st = sc.render()
            ref = ref.astype(F)
            assert np.array_equal(range_scenes.bits(img), range_scenes.bits(ref)), \
                (shading, exact, skip, int((range_scenes.bits(img) != range_scenes.bits(ref)).sum()), "words differ")
            cw = rp.count_work(cam, p)
            assert (cw["rays"], cw["steps"], cw["shaded_samples"]) == (st["rays"], st["steps"], st["shaded_samples"]), \
                (shading, exact, skip, cw, st)
            assert cw["samples"] + cw["skipped_samples"] == st["samples"], (shading, exact, skip, cw, st)
            if not skip:
                assert cw["skipped_samples"] == 0


@pytest.mark.parametrize("mode", list(range_scenes.RENDER_MODES))
@RAY_LAYOUT
@RAY
def test_projection_frames(gpu, ray_pass, dims, camname, boxname, layout, mode):
    rp, box, cam = ray_setup(ray_pass, dims, camname, boxname, layout, range_scenes.RENDER_MODES[mode])
    ref, st = proj_ref.cached(("edge", dims, camname, box), lambda: E.make_scene(dims, camname, box), mode)
    range_scenes.check_against(rp, cam, ref, st)


@RAY_LAYOUT
@RAY
def test_iso_frames(gpu, ray_pass, dims, camname, boxname, layout):
    rp, box, cam = ray_setup(ray_pass, dims, camname, boxname, layout, vr_amd.MODE_ISO)
    for shading in (0, 1):
        ref, st, hit_step, _ = E.iso_reference(dims, camname, box, shading)
        assert st["rays"] >= 30 and int((hit_step >= 0).sum()) >= 20
        check_iso(rp, cam, ref, st, shading)


BAND = 4  # image rows per test: the reference's walk of a whole frame takes 0.4 s


@pytest.mark.parametrize("row0", range(0, E.H, BAND))
@RAY_LAYOUT
@RAY
def test_hit_records(gpu, ray_pass, dims, camname, boxname, layout, row0):
    """Every kind and threshold over one band of rows (vr_hit_request's rectangle); the bands
    cover the frame."""
    rp, box, cam = ray_setup(ray_pass, dims, camname, boxname, layout, vr_amd.MODE_COMPOSITE)
    rect = (0, row0, E.W, BAND)
    walk = E.hit_reference(dims, camname, box, hit_scenes.THRESHOLDS, rect)
    for key in hit_scenes.KEYS:
        kind, th = hit_scenes.key_kind(key)
        want = walk.records[key][row0:row0 + BAND]
        check_records(rp.hit_image(cam, P(), kind, th, rect=rect), want, (key, rect))
        got = rp.hit_count_work(cam, P(), kind, th, rect=rect)
        assert got == walk.stats[key], (key, rect, got, walk.stats[key])
        # one pick per kind and threshold: its pixel's record
        at = np.argwhere(walk.hits(key))
        py, px = at[len(at) // 2] if len(at) else (row0, E.W // 2)
        got = rp.pick(cam, P(), int(px), int(py), kind, th)
        check_records(np.asarray(got).reshape(1), walk.records[key][py, px].reshape(1), (key, int(px), int(py)))


# ---- 4. MPR through the first, seam and last voxel layers ----------------------------------------------------------
@pytest.mark.parametrize("group", ["axis0", "axis1", "axis2", "other"])
@pytest.mark.parametrize("layout", E.RAY_LAYOUTS)
@pytest.mark.parametrize("dims", E.MPR_VOLUMES, ids=dims_id)
def test_mpr_planes(gpu, dims, layout, group):
    dtype, knobs, storage, _ = E.LAYOUTS[layout]
    vol = E.fill(dims, "noise")
    rp = mpr_pass(vol.astype(dtype), synth.tf_color(), E.FULL, w=E.W, h=E.H, **knobs)
    try:
        assert rp.volume_info()[2] == storage
        planes = [(n, pl) for n, pl in E.mpr_planes(dims, E.geometry(layout)) if (n.startswith(group) if group != "other" else not n.startswith("axis"))]
        assert planes
        for name, pl in planes:
            ref, st = mpr_ref.cached(("edge", dims, name),
                                     lambda: mpr_ref.render(vol, float(vol.min()), float(vol.max()), synth.tf_color(), pl,
                                                            E.FULL, mpr_ref.CLEAR))
            print(name, st)
            check_mpr(rp, pl, ref, st)
    finally:
        rp.close()
