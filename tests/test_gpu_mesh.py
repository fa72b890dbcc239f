"""GPU: the isosurface as an indexed triangle mesh (include/vr/vr_mesh.h; mesh_classify_kernel,
the two scans, mesh_vertex_kernel, mesh_quad_kernel).

The reference is tests/mesh_ref.py (the header's method in numpy f32, pinned independently by
tests/test_mesh_cpu.py).  Every comparison is bit for bit in mesh_scenes' canonical form -- the
order of vertices and triangles is unspecified -- and the three counts must be equal.
Scenes: tests/mesh_scenes.py."""
import ctypes as C

import numpy as np
import pytest

import hit_scenes
import mesh_ref
import mesh_scenes as S
import synth
import vr_amd
from range_scenes import STORAGE, int_volume, volume

pytestmark = pytest.mark.gpu

F = np.float32
NAME = "void vr::(anonymous namespace)::mesh_classify_kernel<%s>(vr::MeshArgs)"
TAG = {(0, 0): "unsigned char", (1, 0): "signed char", (0, 1): "vr::Quad8<unsigned char>",
       (1, 1): "vr::Quad8<signed char>", (2, None): "unsigned short", (3, None): "short", (4, None): "float"}


def mesh_pass(vol, w=16, h=16, vrange=None, **knobs):
    rp = vr_amd.OffscreenPass(w, h)
    for k, v in knobs.items():
        rp.set_knob(k, v)
    ds = synth.dataset(np.asarray(vol))
    if vrange is not None:
        ds.vmin, ds.vmax = vrange
    rp.volume_dataset_changed(ds)
    return rp


def check_mesh(rp, ref, iso, closed=True, normals=True, box=None, what=""):
    verts, tris, info = rp.mesh(iso, closed, normals, box)
    print(what, info)
    assert info == ref.info, (what, info, ref.info)
    assert rp.mesh_count(iso, closed, normals, box) == info
    assert verts.dtype == vr_amd.MESH_VERTEX_DTYPE and tris.dtype == np.uint32
    if len(tris):
        assert int(tris.max()) < len(verts)
    S.assert_same_mesh((verts, tris), (ref.verts, ref.tris), what)
    return verts, tris


# ---- 1, 2, 3. parity: brick crossings, caps and rims, an interior box, noise -------------------------
@pytest.mark.parametrize("name,closed,box", list(S.CASES))
@pytest.mark.parametrize("normals", [True, False])
def test_mesh_equals_the_reference(gpu, name, closed, box, normals):
    ref = S.reference(name, closed, normals, box)
    assert (ref.info["vertices"], ref.info["triangles"], ref.info["inside_voxels"]) == S.CASES[(name, closed, box)]
    make, iso = S.SCENES[name]
    rp = mesh_pass(make())
    try:
        verts, _ = check_mesh(rp, ref, iso, closed, normals, box, (name, closed, box, normals))
        if not normals:
            assert not verts["normal"].view(np.uint32).any()  # +0.0f, bit for bit
        assert rp.last_kernel_name() == NAME % "float"
    finally:
        rp.close()


# ---- 4. every storage type and layout ----------------------------------------------------------------
@pytest.mark.parametrize("dtype,signed,knobs,storage", STORAGE)
def test_storage_types(gpu, dtype, signed, knobs, storage):
    vf = int_volume(signed)
    iso = hit_scenes.isovalue(vf)
    key = "int_s" if signed else "int_u"
    rp = mesh_pass(vf.astype(dtype), **knobs)
    try:
        assert rp.volume_info()[2] == storage
        nz, ny, nx = vf.shape
        box = ((1, 2, 3), (nx - 2, ny - 1, nz - 3))
        for closed, b in ((True, None), (False, None), (True, box)):
            ref = mesh_ref.cached(key, lambda: vf, iso, closed, True, b)
            assert ref.info["triangles"] >= 100
            check_mesh(rp, ref, iso, closed, True, b, (key, closed, b))
        quad = knobs.get("u8_layout", 1) if storage < 2 else None
        assert rp.last_kernel_name() == NAME % TAG[(storage, quad)]
    finally:
        rp.close()


# ---- 5. NaN and infinite voxels ----------------------------------------------------------------------
@pytest.mark.parametrize("closed", [True, False])
def test_nan_and_infinite_voxels(gpu, closed):
    """Positions bit for bit; normals only where the reference's is finite (the sign and payload
    of a NaN differ between the host's and the device's arithmetic)."""
    vol = S.specials()
    ref = mesh_ref.cached("specials", S.specials, 0.25, closed, True, None)
    small = S.reference("ball", closed, True, None)
    assert ref.info["vertices"] > small.info["vertices"]  # the special voxels add surface
    finite = np.isfinite(ref.verts["normal"]).all(axis=1)
    assert 3 <= (~finite).sum() and finite.sum() >= 500
    rp = mesh_pass(vol, vrange=(0.0, 6.0))
    try:
        verts, tris, info = rp.mesh(0.25, closed, True)
        assert info == ref.info
        bare = lambda v: np.ascontiguousarray(v["pos"]).view(np.uint32)
        # positions, through the canonical form with the normals blanked
        gv, wv = verts.copy(), ref.verts.copy()
        gv["normal"] = 0
        wv["normal"] = 0
        S.assert_same_mesh((gv, tris), (wv, ref.tris), "positions")
        # a vertex is named by its position here: the reference's positions are distinct
        want = {bare(ref.verts)[i].tobytes(): ref.verts["normal"][i] for i in range(len(ref.verts))}
        assert len(want) == len(ref.verts)
        checked = 0
        for i in range(len(verts)):
            n = want[bare(verts)[i].tobytes()]
            if np.isfinite(n).all():
                assert np.array_equal(n.view(np.uint32), verts["normal"][i].view(np.uint32)), (i, n, verts["normal"][i])
                checked += 1
        assert checked == int(finite.sum())
    finally:
        rp.close()


# ---- 6. more bricks than workgroups, and than one workgroup of the scan covers -----------------------
def test_scan_across_workgroups(gpu):
    vol = S.long_thin()
    ref = mesh_ref.cached("long_thin", lambda: vol.astype(F), 128.0, True, False, None)
    assert ref.info["vertices"] >= 50000
    rp = mesh_pass(vol, u8_layout=0)
    try:
        assert rp.volume_info()[2] == 0
        check_mesh(rp, ref, 128.0, True, False, None, "long_thin")
        assert rp.last_kernel_name() == NAME % "unsigned char"
        # 4 x 4 x 376 bricks of 7 x 8 x 8 cells: past the 2048 workgroups and the 1024-brick chunks
        box = ((2, 3, 100), (22, 20, 2900))
        ref = mesh_ref.cached("long_thin", lambda: vol.astype(F), 128.0, False, False, box)
        check_mesh(rp, ref, 128.0, False, False, box, "long_thin box")
    finally:
        rp.close()


# ---- 7. empty meshes -----------------------------------------------------------------------------------
def test_empty_meshes(gpu):
    vol = S.noise()
    rp = mesh_pass(vol)
    try:
        n = vol.size
        verts, tris, info = rp.mesh(2.0, True, True)  # above the maximum
        assert (len(verts), len(tris)) == (0, 0) and info == dict(vertices=0, triangles=0, inside_voxels=0)
        for iso in (float(vol.min()), -1.0):  # at and below the minimum, open: every node inside
            verts, tris, info = rp.mesh(iso, False, True)
            assert (len(verts), len(tris)) == (0, 0) and info == dict(vertices=0, triangles=0, inside_voxels=n)
        # closed, the ring (+0.0f) is outside at a positive isovalue: the whole box as a surface
        info = rp.mesh_count(float(vol.min()), True, False)
        ref = mesh_ref.extract(vol, float(vol.min()), True, False)
        assert info == ref.info and info["vertices"] > 0 and info["inside_voxels"] == n
        # one node per axis somewhere, open: no cell at all, the voxels still count
        info = rp.mesh_count(0.5, False, True, box=((3, 4, 5), (4, 9, 10)))
        assert info == mesh_ref.extract(vol, 0.5, False, False, ((3, 4, 5), (4, 9, 10))).info
        assert info["vertices"] == 0 and info["inside_voxels"] > 0
    finally:
        rp.close()


# ---- behaviour -------------------------------------------------------------------------------------------
def test_two_extracts_write_identical_bytes_and_the_device_form_equals_the_host_form(gpu):
    import torch
    make, iso = S.SCENES["noise"]
    rp = mesh_pass(make())
    try:
        v1, t1, i1 = rp.mesh(iso)
        v2, t2, i2 = rp.mesh(iso)
        assert i1 == i2 and v1.tobytes() == v2.tobytes() and t1.tobytes() == t2.tobytes()
        nv, nt = i1["vertices"], i1["triangles"]
        stream = torch.cuda.Stream()
        # guard words after the counts' worth of records stay as they were
        dv = torch.full((nv * 6 + 8,), 0x77777777, dtype=torch.int32, device="cuda")
        dt = torch.full((nt * 3 + 8,), 0x77777777, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        info = rp.mesh_device(dv.data_ptr(), nv + 1, dt.data_ptr(), nt + 2, iso, stream=stream.cuda_stream)
        # (complete on return: no synchronisation of ours before the copy on another stream)
        hv, ht = dv.cpu().numpy().view(np.uint32), dt.cpu().numpy().view(np.uint32)
        assert info == i1
        assert hv[:nv * 6].tobytes() == v1.tobytes() and ht[:nt * 3].tobytes() == t1.tobytes()
        assert np.all(hv[nv * 6:] == 0x77777777) and np.all(ht[nt * 3:] == 0x77777777)
    finally:
        rp.close()


def test_short_capacities_and_every_error_leave_the_outputs_untouched(gpu):
    import torch
    make, iso = S.SCENES["ball"]
    rp = mesh_pass(make())
    L = vr_amd.lib()
    try:
        want = rp.mesh_count(iso)
        nv, nt = want["vertices"], want["triangles"]
        hv = np.full(nv * 6, 0x77777777, np.uint32)
        ht = np.full(nt * 3, 0x77777777, np.uint32)
        dv = torch.full((nv * 6,), 0x77777777, dtype=torch.int32, device="cuda")
        dt = torch.full((nt * 3,), 0x77777777, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        info = vr_amd.vr_mesh_info()

        def calls(req, vcap=nv, tcap=nt, inf=info, bufs=True):
            rq = C.byref(req) if req is not None else None
            ip = C.byref(inf) if inf is not None else None
            return [L.vr_mesh_extract(rp._ctx, rq, hv.ctypes.data if bufs else None, vcap,
                                      ht.ctypes.data if bufs else None, tcap, ip),
                    L.vr_mesh_extract_device(rp._ctx, rq, C.c_void_p(dv.data_ptr()) if bufs else None, vcap,
                                             C.c_void_p(dt.data_ptr()) if bufs else None, tcap, ip, None)]

        R = vr_amd.mesh_request
        # each capacity one short: VR_ENOSPC and the needed counts
        for vcap, tcap in ((nv - 1, nt), (nv, nt - 1), (0, 0)):
            for k in range(2):
                info.vertices = info.triangles = info.inside_voxels = 0
                assert calls(R(iso), vcap, tcap)[k] == vr_amd.ENOSPC == -28
                assert (info.vertices, info.triangles, info.inside_voxels) == (nv, nt, want["inside_voxels"])
        assert b"smaller" in L.vr_last_error(rp._ctx)
        # VR_EINVAL: the request's fields, the box, NULL arguments
        info.vertices = info.triangles = info.inside_voxels = info.reserved = 0x77
        bad = [R(float("nan")), R(float("inf")), R(-float("inf"))]
        for field in ("closed", "normals", "use_box"):
            for v in (2, 0xFFFFFFFF):
                r = R(iso)
                setattr(r, field, v)
                bad.append(r)
        nx, ny, nz = S.DIMS
        for box in (((0, 0, 0), (0, 1, 1)), ((3, 3, 3), (3, 4, 4)), ((5, 0, 0), (4, 1, 1)),
                    ((0, 0, 0), (nx + 1, ny, nz)), ((0, 0, 0), (nx, ny + 1, nz)), ((0, 0, 0), (nx, ny, nz + 1)),
                    ((0, 0, 0xFFFFFFFF), (1, 1, 1)), ((0, 0, 0), (1, 0xFFFFFFFF, 1))):
            bad.append(R(iso, box=box))
        for r in bad:
            assert calls(r) == [-22, -22], (r.iso, r.closed, r.normals, r.use_box, list(r.box_min), list(r.box_max))
            assert L.vr_mesh_count(rp._ctx, C.byref(r), C.byref(info)) == -22
        assert calls(None) == [-22, -22] and calls(R(iso), inf=None) == [-22, -22]
        assert calls(R(iso), bufs=False) == [-22, -22]
        assert L.vr_mesh_count(rp._ctx, None, C.byref(info)) == -22
        assert L.vr_mesh_count(rp._ctx, C.byref(R(iso)), None) == -22
        assert (info.vertices, info.triangles, info.inside_voxels, info.reserved) == (0x77,) * 4
        torch.cuda.synchronize()
        assert np.all(hv == 0x77777777) and np.all(ht == 0x77777777)
        assert bool((dv == 0x77777777).all()) and bool((dt == 0x77777777).all())
        with pytest.raises(RuntimeError, match="finite"):
            rp.mesh(float("nan"))
        # and the context still works
        assert calls(R(iso)) == [0, 0] and info.reserved == 0
        assert hv.tobytes() == dv.cpu().numpy().tobytes() and ht.tobytes() == dt.cpu().numpy().tobytes()
    finally:
        rp.close()


MODES = [vr_amd.MODE_COMPOSITE, vr_amd.MODE_MIP, vr_amd.MODE_MINIP, vr_amd.MODE_MEAN, vr_amd.MODE_ISO]


def test_mesh_calls_leave_every_frame_and_the_memory_report_alone(gpu):
    vol = volume("g20")
    iso = hit_scenes.isovalue(vol)
    rp = hit_scenes.hit_pass(32, 24, vol, synth.tf_color(), iso)
    try:
        cam = synth.camera("rotA").to_vr_camera()
        p = vr_amd.default_params(shading=1, skip_empty=1)
        before = {}
        for m in MODES:
            rp.render_mode_changed(m)
            before[m] = rp.render(cam, p, vr_amd.OUT_RGBA32F)
        rp.render_mode_changed(vr_amd.MODE_MEAN)
        state = (rp.render_mode, rp.isovalue, rp.volume_info())
        rep = rp.memory_report()
        rp.timing_enable(True)
        rp.timing_reset()
        verts, tris, info = rp.mesh()  # the context's isovalue
        ref = mesh_ref.cached("g20", lambda: vol, iso, True, True, None)
        assert info == ref.info and info["triangles"] >= 100
        S.assert_same_mesh((verts, tris), (ref.verts, ref.tris), "g20")
        assert rp.last_kernel_name() == NAME % "float"
        ms, launches = rp.timing_read()
        # mesh() counts, then extracts: classify + scans twice, the emit passes once
        assert launches == 3 and ms > 0.0
        rp.timing_enable(False)
        assert rp.memory_report() == rep
        assert (rp.render_mode, rp.isovalue, rp.volume_info()) == state
        for m in MODES:
            rp.render_mode_changed(m)
            assert np.array_equal(rp.render(cam, p, vr_amd.OUT_RGBA32F).view(np.uint32),
                                  before[m].view(np.uint32)), m
            assert "mesh_" not in rp.last_kernel_name()
    finally:
        rp.close()


@pytest.mark.parametrize("group", [dict(device_mask=1), dict(members=(0, 0, 0))])
def test_member_contexts_give_the_same_mesh(gpu, group):
    make, iso = S.SCENES["bigball"]
    ref = S.reference("bigball", True, True, S.BOX)
    grp = vr_amd.OffscreenPass(16, 16, exchange=vr_amd.EXCHANGE_COPY, **group)
    try:
        grp.volume_dataset_changed(synth.dataset(make()))
        grp.transfer_function_changed(synth.tf_color())
        check_mesh(grp, ref, iso, True, True, S.BOX, "members")
        assert grp.last_kernel_name() == NAME % "float"
    finally:
        grp.close()


# ---- the tie to the renderer ------------------------------------------------------------------------------
def test_refined_iso_hits_lie_within_a_cell_diagonal_of_the_mesh(gpu):
    """A refined VR_HIT_ISO point lies within one step (below a voxel here) of a sign change of
    the trilinear field along its ray; a cell the level set crosses is active and holds a vertex:
    hit.pos is within one cell diagonal, in lattice units, of some vertex of the closed mesh."""
    volname, camname, box, tfname, w, h = hit_scenes.PARITY[0]
    vol = volume(volname)
    iso = hit_scenes.isovalue(vol)
    nz, ny, nx = vol.shape
    p = vr_amd.default_params()
    assert p.step * max(nx, ny, nz) < 1.0
    rp = hit_scenes.hit_pass(w, h, vol, synth.TFS[tfname](), iso, box)
    try:
        cam = synth.camera(camname).to_vr_camera()
        rec = rp.hit_image(cam, p, vr_amd.HIT_ISO)
        ent = rp.hit_image(cam, p, vr_amd.HIT_ENTRY)
        hit = rec["step"] != vr_amd.HIT_MISS_STEP
        fine = hit & (rec["step"] != ent["step"])  # a cap is the ray's first in-slab sample
        assert fine.sum() >= 100
        verts, tris, info = rp.mesh(iso, True, False)
        dims = np.asarray((nx, ny, nz), np.float64)
        hp = rec["pos"][fine].astype(np.float64) * dims
        vp = verts["pos"].astype(np.float64) * dims
        d = np.sqrt(((hp[:, None, :] - vp[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
        print("refined hits", int(fine.sum()), "largest distance to a vertex", float(d.max()))
        assert d.max() <= np.sqrt(3.0)
    finally:
        rp.close()


# ---- vr_cli --mesh ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("suffix,closed", [("", True), (":open", False)])
def test_cli_writes_the_mesh_and_prints_its_counts(gpu, tmp_path, suffix, closed):
    import json
    import os
    import subprocess
    n = 20
    rp = vr_amd.OffscreenPass(16, 16)
    try:
        lo, hi = rp.generate_volume((n, n, n), np.float32, seed=2024)
        iso = float(F(lo + 0.3 * (hi - lo)))
        verts, tris, info = rp.mesh(iso, closed, True)
    finally:
        rp.close()
    assert info["triangles"] >= 100
    ply, ppm = tmp_path / "out.ply", tmp_path / "never.ppm"
    cli = os.path.join(os.path.dirname(vr_amd.LIB_PATH), "vr_cli")
    r = subprocess.run([cli, f"synthetic:{n}", str(ppm), "--iso", repr(iso), "--mesh", str(ply) + suffix],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert not ppm.exists()
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == info
    b = ply.read_bytes()
    end = b.index(b"end_header\n") + 11
    assert f"element vertex {info['vertices']}\n".encode() in b[:end]
    assert len(b) == end + 24 * info["vertices"] + 13 * info["triangles"]
    got = np.frombuffer(b, "<f4", info["vertices"] * 6, end).reshape(-1, 6)
    want = verts["pos"] * F(n) + F(-0.5)  # voxel units
    assert np.array_equal(got[:, :3].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, 3:].view(np.uint32), verts["normal"].view(np.uint32))
