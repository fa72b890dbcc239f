"""GPU: connected components of a value window and seeded region growing (include/vr/vr_label.h;
label_local_kernel, label_seam_kernel, label_flatten_kernel, the scan and the table kernels,
label_grow_kernel).

The reference is tests/label_ref.py (hooking and pointer jumping in numpy, pinned against a
breadth-first search and scipy by tests/test_label_cpu.py).  Labels are canonical -- 1 + the
smallest box-linear index of the component -- and the records sorted by label, so every array is
compared byte for byte.  Scenes: tests/label_scenes.py."""
import ctypes as C

import numpy as np
import pytest

import hit_scenes
import label_ref
import label_scenes as S
import synth
import vr_amd
from gpu_kit import GUARD32
from range_scenes import STORAGE, volume

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")
NAME = "void vr::(anonymous namespace)::label_local_kernel<%s, %d>(vr::LabelArgs)"
TAG = {(0, 0): "unsigned char", (1, 0): "signed char", (0, 1): "vr::Quad8<unsigned char>",
       (1, 1): "vr::Quad8<signed char>", (2, None): "unsigned short", (3, None): "short", (4, None): "float"}


def label_pass(vol, w=16, h=16, vrange=None, **knobs):
    rp = vr_amd.OffscreenPass(w, h)
    for k, v in knobs.items():
        rp.set_knob(k, v)
    ds = synth.dataset(np.asarray(vol))
    if vrange is not None:
        ds.vmin, ds.vmax = vrange
    rp.volume_dataset_changed(ds)
    return rp


def check_labels(rp, ref, lo, hi, conn, box, what=""):
    want_labels, want_rec, want_info = ref
    labels, rec, info = rp.label(lo, hi, conn, box)
    print(what, info)
    assert info == want_info, (what, info, want_info)
    assert rp.label_count(lo, hi, conn, box) == info, what
    assert labels.dtype == np.uint32 and labels.shape == want_labels.shape
    assert rec.dtype == vr_amd.LABEL_COMPONENT_DTYPE == label_ref.COMPONENT_DTYPE
    assert labels.tobytes() == want_labels.tobytes(), (what, int((labels != want_labels).sum()), "labels differ")
    assert rec.tobytes() == want_rec.tobytes(), (what, "records differ")
    return labels, rec, info


_scene_pass = {}


@pytest.fixture(scope="module")
def scene_pass():
    """One context per scene for the whole module (the volumes are never modified)."""
    def get(name, **kw):
        if name not in _scene_pass:
            # (narrow = 0: the 0 / 1 scenes stay f32 as well)
            _scene_pass[name] = label_pass(S.SCENES[name](), narrow=0, **kw)
        return _scene_pass[name]
    yield get
    for rp in _scene_pass.values():
        rp.close()
    _scene_pass.clear()


# ---- 1. parity: every scene x connectivity x (whole volume, box) ------------------------------------
@pytest.mark.parametrize("name,lo,hi,conn,box", list(S.CASES))
def test_labels_equal_the_reference(gpu, scene_pass, name, lo, hi, conn, box):
    ref = S.reference(name, lo, hi, conn, box)
    assert S.pinned(ref[2]) == S.CASES[(name, lo, hi, conn, box)]
    rp = scene_pass(name, vrange=(0.0, 6.0)) if name == "specials" else scene_pass(name)
    labels, rec, info = check_labels(rp, ref, lo, hi, conn, box, (name, lo, hi, conn, box))
    assert rp.last_kernel_name() == NAME % ("float", conn)
    # ---- 10. the records' voxels sum to in_voxels; the largest is one of them
    assert int(rec["voxels"].sum()) == info["in_voxels"] <= info["voxels"] == labels.size
    assert info["largest_voxels"] <= info["in_voxels"]
    if info["components"]:
        assert info["largest_voxels"] == int(rec["voxels"].max())


# ---- 2. every storage type and layout ----------------------------------------------------------------
@pytest.mark.parametrize("dtype,signed,knobs,storage", STORAGE)
def test_storage_types(gpu, dtype, signed, knobs, storage):
    vf = S.SCENES["integers"]()  # 0 .. 100: every storage type holds it
    if signed:
        vf = vf - F(50.0)
    key = "integers_s" if signed else "integers_u"
    lo, hi = (10.0, 30.0) if signed else (60.0, 80.0)  # a shell around the ball's core
    rp = label_pass(vf.astype(dtype), **knobs)
    try:
        assert rp.volume_info()[2] == storage
        quad = knobs.get("u8_layout", 1) if storage < 2 else None
        for conn, box in ((6, None), (26, None), (26, S.BOX), (6, S.BOX)):
            ref = label_ref.cached(key, lambda: vf, lo, hi, conn, box)
            assert ref[2]["in_voxels"] >= 100
            check_labels(rp, ref, lo, hi, conn, box, (key, conn, box))
            assert rp.last_kernel_name() == NAME % (TAG[(storage, quad)], conn)
        # the core inside the shell, through an infinite bound
        ref = label_ref.cached(key, lambda: vf, hi + 1.0, INF, 6, None)
        check_labels(rp, ref, hi + 1.0, INF, 6, None, (key, "core"))
    finally:
        rp.close()


# ---- 3. more bricks than workgroups, more chunks than one round of the table's scan -----------------
@pytest.mark.parametrize("name", ["long_thin", "long_checker"])
def test_grids_and_scans_across_workgroups(gpu, name):
    rp = label_pass(S.SCENES[name](), u8_layout=0)
    try:
        assert rp.volume_info()[2] == 0
        for (n, lo, hi, conn, box), pin in S.LONG_CASES.items():
            if n != name:
                continue
            ref = S.reference(n, lo, hi, conn, box)
            assert S.pinned(ref[2]) == pin
            check_labels(rp, ref, lo, hi, conn, box, (n, lo, hi, conn, box))
            assert rp.last_kernel_name() == NAME % ("unsigned char", conn)
    finally:
        rp.close()


# ---- 4. empty and full ---------------------------------------------------------------------------------
def test_empty_and_full_windows(gpu, scene_pass):
    vol = S.SCENES["noise"]()
    rp = scene_pass("noise")
    n = vol.size
    for conn in (6, 26):
        labels, rec, info = rp.label(2.0, 3.0, conn)  # above the maximum
        assert not labels.any() and len(rec) == 0
        assert info == dict(voxels=n, in_voxels=0, components=0, largest_voxels=0, largest_label=0)
        labels, rec, info = rp.label(-INF, INF, conn)  # around everything
        assert np.all(labels == 1) and len(rec) == 1
        assert info == dict(voxels=n, in_voxels=n, components=1, largest_voxels=n, largest_label=1)
        nz, ny, nx = vol.shape
        assert rec[0]["bbox_min"].tolist() == [0, 0, 0] and rec[0]["bbox_max"].tolist() == [nx, ny, nz]
        assert rec[0]["sum"].tolist() == [n * (nx - 1) // 2, n * (ny - 1) // 2, n * (nz - 1) // 2]
    # a box of one voxel, in and not in
    x, y, z = 4, 5, 6
    one = ((x, y, z), (x + 1, y + 1, z + 1))
    v = float(vol[z, y, x])
    labels, rec, info = rp.label(v, v, 6, one)
    assert labels.tolist() == [[[1]]] and info["components"] == 1 and rec[0]["sum"].tolist() == [x, y, z]
    labels, rec, info = rp.label(v + 0.5, 9.0, 26, one)
    assert labels.tolist() == [[[0]]] and info["components"] == 0


def test_a_fresh_context_labels_its_placeholder_volume(gpu):
    """There is no "no volume" state: a context is created with one voxel of value 0."""
    rp = vr_amd.OffscreenPass(16, 16)
    try:
        assert rp.volume_info()[0] == (1, 1, 1)
        labels, rec, info = rp.label(0.0, 0.0)
        assert labels.tolist() == [[[1]]] and len(rec) == 1
        assert info == dict(voxels=1, in_voxels=1, components=1, largest_voxels=1, largest_label=1)
        mask, comp = rp.region_grow((0, 0, 0), 0.5, 1.0, 26)
        assert mask.tolist() == [[[0]]] and comp["voxels"] == 0
    finally:
        rp.close()


def test_more_records_than_the_bindings_first_buffer(gpu):
    """OffscreenPass.label labels once into a 65536-record buffer and again only when the table is
    larger: the long checkerboard's 864000 records come from that second call."""
    ref = S.reference("long_checker", 1.0, 1.0, 6, None)
    assert ref[2]["components"] > 65536
    # (covered byte for byte by test_grids_and_scans_across_workgroups; here: the sizes)
    rp = label_pass(S.SCENES["long_checker"](), u8_layout=0)
    try:
        labels, rec, info = rp.label(1.0, 1.0, 6)
        assert len(rec) == info["components"] == 864000 and rec.tobytes() == ref[1].tobytes()
    finally:
        rp.close()


# ---- 5. region growing ------------------------------------------------------------------------------------
def test_region_grow_equals_the_reference(gpu, scene_pass):
    import torch
    vol = S.SCENES["noise"]()
    rp = scene_pass("noise")
    lo, hi = 0.7, 1.0
    for conn, box in ((6, None), (26, None), (6, S.BOX), (26, S.BOX)):
        ref = S.reference("noise", lo, hi, conn, box)
        labels, rec, _ = ref
        origin = (0, 0, 0) if box is None else box[0]
        # the largest component, one of a single voxel, and the last record's
        picks = [int(np.argmax(rec["voxels"])), int(np.argmin(rec["voxels"])), len(rec) - 1]
        assert len(set(picks)) == 3
        seeds = []
        for i in picks:
            l = int(np.flatnonzero(labels.reshape(-1) == rec["label"][i])[-1])  # its LAST voxel, not its root
            bz, by, bx = labels.shape
            seeds.append((l % bx + origin[0], (l // bx) % by + origin[1], l // (bx * by) + origin[2]))
        out = np.argwhere(labels == 0)[7]
        seeds.append((int(out[2]) + origin[0], int(out[1]) + origin[1], int(out[0]) + origin[2]))
        for k, seed in enumerate(seeds):
            want_mask, want_comp = label_ref.region_grow(vol, seed, lo, hi, conn, box, labelled=ref)
            mask, comp = rp.region_grow(seed, lo, hi, conn, box)
            assert mask.dtype == np.uint8 and mask.tobytes() == want_mask.tobytes(), (conn, box, seed)
            assert comp == want_comp, (conn, box, seed, comp, want_comp)
            assert (comp["voxels"] == 0) == (k == 3) and int(mask.sum()) == comp["voxels"]
            # the device form, with guard bytes past the mask
            dm = torch.full((mask.size + 16,), 0x77, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            stream = torch.cuda.Stream()
            dcomp = rp.region_grow_device(seed, dm.data_ptr(), mask.size, lo, hi, conn, box, stream=stream.cuda_stream)
            hm = dm.cpu().numpy()
            assert dcomp == want_comp and hm[:mask.size].tobytes() == want_mask.tobytes()
            assert np.all(hm[mask.size:] == 0x77)
    assert rp.last_kernel_name() == NAME % ("float", 26)


# ---- 6. two calls, the device form, guard words -------------------------------------------------------------
def test_two_calls_write_identical_bytes_and_the_device_form_equals_the_host_form(gpu, scene_pass):
    import torch
    rp = scene_pass("noise")
    for conn, box, lo, hi in ((6, None, 0.3, 0.6), (26, S.BOX) + S.NOISE26):  # 447 and 42 components
        l1, r1, i1 = rp.label(lo, hi, conn, box)
        l2, r2, i2 = rp.label(lo, hi, conn, box)
        assert i1 == i2 and l1.tobytes() == l2.tobytes() and r1.tobytes() == r2.tobytes()
        n, nc = i1["voxels"], i1["components"]
        assert nc >= 40
        stream = torch.cuda.Stream()
        dl = torch.full((n + 8,), GUARD32, dtype=torch.int32, device="cuda")
        dc = torch.full((nc * 16 + 16,), GUARD32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        info = rp.label_device(dl.data_ptr(), n + 3, dc.data_ptr(), nc + 1, lo, hi, conn, box,
                               stream=stream.cuda_stream)
        # (complete on return: no synchronisation of ours before the copy on another stream)
        hl, hc = dl.cpu().numpy().view(np.uint32), dc.cpu().numpy().view(np.uint32)
        assert info == i1
        assert hl[:n].tobytes() == l1.tobytes() and hc[:nc * 16].tobytes() == r1.tobytes()
        assert np.all(hl[n:] == GUARD32) and np.all(hc[nc * 16:] == GUARD32)


# ---- 7. errors ------------------------------------------------------------------------------------------------
def test_every_error_leaves_the_outputs_untouched(gpu, scene_pass):
    import torch
    rp = scene_pass("noise")
    L = vr_amd.lib()
    lo, hi = 0.7, 1.0
    want_labels, want_rec, want = S.reference("noise", lo, hi, 6, None)
    n, nc = want["voxels"], want["components"]
    hl = np.full(n, GUARD32, np.uint32)
    hc = np.full(nc * 16, GUARD32, np.uint32)
    hm = np.full(n, 0x77, np.uint8)
    dl = torch.full((n,), GUARD32, dtype=torch.int32, device="cuda")
    dc = torch.full((nc * 16,), GUARD32, dtype=torch.int32, device="cuda")
    dm = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    info = vr_amd.vr_label_info()
    comp = vr_amd.vr_label_component()
    seed_in = (C.c_uint32 * 3)(1, 1, 1)

    def untouched():
        torch.cuda.synchronize()
        return (np.all(hl == GUARD32) and np.all(hc == GUARD32) and np.all(hm == 0x77) and bool((dl == GUARD32).all())
                and bool((dc == GUARD32).all()) and bool((dm == 0x77).all()))

    def label_calls(req, lcap=n, ccap=nc, inf=info, bufs=True):
        rq = C.byref(req) if req is not None else None
        ip = C.byref(inf) if inf is not None else None
        p = (lambda a: a) if bufs else (lambda a: None)
        return [L.vr_label_components(rp._ctx, rq, p(hl.ctypes.data), lcap, p(hc.ctypes.data), ccap, ip),
                L.vr_label_components_device(rp._ctx, rq, p(C.c_void_p(dl.data_ptr())), lcap,
                                             p(C.c_void_p(dc.data_ptr())), ccap, ip, None)]

    def grow_calls(req, bufs=True, seed=seed_in, mcap=n, cmp=comp):
        rq = C.byref(req) if req is not None else None
        cp = C.byref(cmp) if cmp is not None else None
        p = (lambda a: a) if bufs else (lambda a: None)
        return [L.vr_region_grow(rp._ctx, rq, seed, p(hm.ctypes.data), mcap, cp),
                L.vr_region_grow_device(rp._ctx, rq, seed, p(C.c_void_p(dm.data_ptr())), mcap, cp, None)]

    def calls(req, lcap=n, ccap=nc, inf=info, bufs=True, mcap=n, cmp=comp):
        return label_calls(req, lcap, ccap, inf, bufs) + grow_calls(req, bufs, seed_in, mcap, cmp)

    R = vr_amd.label_request

    def mark():
        C.memset(C.byref(info), 0x77, C.sizeof(info))
        C.memset(C.byref(comp), 0x77, C.sizeof(comp))

    def marked(i=True, c=True):
        return ((not i or bytes(info) == b"\x77" * 40) and (not c or bytes(comp) == b"\x77" * 64))

    # VR_EINVAL: the request's fields, the box, the seed, NULL arguments
    mark()
    bad = [R(float("nan"), 1.0), R(0.0, float("nan")), R(0.8, 0.7), R(INF, -INF)]
    for conn in (0, 4, 8, 18, 27, 0xFFFFFFFF):
        bad.append(R(lo, hi, conn))
    for v in (2, 0xFFFFFFFF):
        r = R(lo, hi)
        r.use_box = v
        bad.append(r)
    nx, ny, nz = 19, 17, 21
    for box in (((0, 0, 0), (0, 1, 1)), ((3, 3, 3), (3, 4, 4)), ((5, 0, 0), (4, 1, 1)),
                ((0, 0, 0), (nx + 1, ny, nz)), ((0, 0, 0), (nx, ny + 1, nz)), ((0, 0, 0), (nx, ny, nz + 1)),
                ((0, 0, 0xFFFFFFFF), (1, 1, 1)), ((0, 0, 0), (1, 0xFFFFFFFF, 1))):
        bad.append(R(lo, hi, box=box))
    for r in bad:
        assert calls(r) == [-22] * 4, (r.lo, r.hi, r.connectivity, r.use_box, list(r.box_min), list(r.box_max))
        assert L.vr_label_count(rp._ctx, C.byref(r), C.byref(info)) == -22
    assert calls(None) == [-22] * 4 and calls(R(lo, hi), inf=None, cmp=None) == [-22] * 4
    assert calls(R(lo, hi), bufs=False) == [-22] * 4 and grow_calls(R(lo, hi), seed=None) == [-22] * 2
    assert L.vr_label_count(rp._ctx, None, C.byref(info)) == -22
    assert L.vr_label_count(rp._ctx, C.byref(R(lo, hi)), None) == -22
    for seed in ((nx, 0, 0), (0, ny, 0), (0, 0, nz), (0xFFFFFFFF, 0, 0)):
        assert grow_calls(R(lo, hi), seed=(C.c_uint32 * 3)(*seed)) == [-22] * 2
    for seed in ((2, 5, 7), (15, 5, 7), (5, 1, 7), (5, 13, 7), (5, 5, 4), (5, 5, 18)):  # just outside the box
        assert grow_calls(R(lo, hi, box=S.BOX), seed=(C.c_uint32 * 3)(*seed)) == [-22] * 2
    assert b"seed" in L.vr_last_error(rp._ctx)
    # a label buffer that is not 4-byte aligned (the records and the mask need no alignment)
    for off in (1, 2, 3):
        assert L.vr_label_components_device(rp._ctx, C.byref(R(lo, hi)), C.c_void_p(dl.data_ptr() + off), n - 1,
                                            C.c_void_p(dc.data_ptr()), nc, C.byref(info), None) == -22
    assert b"aligned" in L.vr_last_error(rp._ctx)
    assert marked() and untouched()
    # what the binding sizes its buffers by is validated by the library, not before it
    for box in (((5, 0, 0), (4, 1, 1)), ((0, 0, 0), (0, 1, 1)), ((0, 0, 0), (nx + 1, ny, nz))):
        with pytest.raises(RuntimeError, match="box"):
            rp.label(lo, hi, 6, box)
        with pytest.raises(RuntimeError, match="box"):
            rp.region_grow((0, 0, 0), lo, hi, 6, box)
    with pytest.raises(RuntimeError, match="lo <= hi"):
        rp.label(0.8, 0.7)
    # VR_ENOSPC, known on the host: lcap / mcap below the voxels of N; nothing touched but info.voxels
    for lcap in (n - 1, 0):
        for k in range(2):
            mark()
            assert label_calls(R(lo, hi), lcap=lcap)[k] == vr_amd.ENOSPC == -28
            assert (info.voxels, info.in_voxels, info.components, info.largest_voxels, info.largest_label,
                    info.reserved) == (n, 0, 0, 0, 0, 0) and marked(i=False)
        mark()
        assert grow_calls(R(lo, hi), mcap=lcap) == [-28, -28] and marked()
    assert b"smaller" in L.vr_last_error(rp._ctx)
    assert untouched()
    # VR_ENOSPC, ccap below the components: the info complete, the labels complete, no record written
    for ccap in (nc - 1, 0):
        mark()
        got = calls(R(lo, hi), ccap=ccap)
        assert got[:2] == [-28, -28]
        assert vr_amd.OffscreenPass._label_info(info) == want and info.reserved == 0
        torch.cuda.synchronize()
        assert hl.tobytes() == want_labels.tobytes() == dl.cpu().numpy().tobytes()
        assert np.all(hc == GUARD32) and bool((dc == GUARD32).all())
        hl[:] = GUARD32
        dl.fill_(GUARD32)
        hm[:] = 0x77
        dm.fill_(0x77)
    # and the context still works
    assert calls(R(lo, hi)) == [0, 0, 0, 0] and info.reserved == 0
    assert hl.tobytes() == want_labels.tobytes() == dl.cpu().numpy().tobytes()
    assert hc.tobytes() == want_rec.tobytes() == dc.cpu().numpy().tobytes()
    assert hm.tobytes() == dm.cpu().numpy().tobytes()


# ---- 8. state ---------------------------------------------------------------------------------------------------
MODES = [vr_amd.MODE_COMPOSITE, vr_amd.MODE_MIP, vr_amd.MODE_MINIP, vr_amd.MODE_MEAN, vr_amd.MODE_ISO]


def test_label_calls_leave_every_frame_and_the_memory_report_alone(gpu):
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
        ref = label_ref.cached("g20", lambda: vol, iso, INF, 26, None)
        info = rp.label_count(iso, INF, 26)
        assert info == ref[2] and info["components"] >= 1
        assert rp.last_kernel_name() == NAME % ("float", 26)
        ms, launches = rp.timing_read()
        assert launches == 2 and ms > 0.0  # the labelling passes, the table passes
        # the same two intervals pass by pass (vr_debug_label_pass_ms): every pass of the count ran,
        # the mask pass did not, and the parts lie inside the whole
        per = rp.label_pass_ms()
        assert list(per) == list(vr_amd.OffscreenPass.LABEL_PASSES) and per["grow"] == 0.0
        assert all(per[k] > 0.0 for k in per if k != "grow"), per
        assert sum(per.values()) <= ms * 1.001 + 1e-3, (per, ms)
        # ---- 10. the ties to the mesh and the histogram
        assert info["in_voxels"] == rp.mesh_count(iso)["inside_voxels"]
        rp.timing_reset()
        seed = np.unravel_index(int(np.argmax(vol)), vol.shape)[::-1]
        mask, comp = rp.region_grow(seed, iso, INF, 26)
        assert comp["voxels"] == int(mask.sum()) >= 1
        ms, launches = rp.timing_read()
        assert launches == 2 and ms > 0.0  # the labelling passes, the mask pass
        per = rp.label_pass_ms()
        assert per["accumulate"] == per["largest"] == 0.0 and sum(per.values()) <= ms * 1.001 + 1e-3, (per, ms)
        assert all(per[k] > 0.0 for k in ("local", "seam", "flatten", "scan", "table_init", "grow")), per
        rp.timing_enable(False)
        rp.label_count(iso, INF, 6)
        assert not any(rp.label_pass_ms().values())  # timing off: no events, all 0
        assert rp.memory_report() == rep
        assert (rp.render_mode, rp.isovalue, rp.volume_info()) == state
        for m in MODES:
            rp.render_mode_changed(m)
            assert np.array_equal(rp.render(cam, p, vr_amd.OUT_RGBA32F).view(np.uint32),
                                  before[m].view(np.uint32)), m
            assert "label_" not in rp.last_kernel_name()
    finally:
        rp.close()


# ---- 9. member contexts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [dict(device_mask=1), dict(members=(0, 0, 0))])
def test_member_contexts_give_the_same_bytes(gpu, group):
    name, lo, hi, conn, box = "noise", 0.9, 1.0, 26, S.BOX
    ref = S.reference(name, lo, hi, conn, box)
    grp = vr_amd.OffscreenPass(16, 16, exchange=vr_amd.EXCHANGE_COPY, **group)
    try:
        grp.volume_dataset_changed(synth.dataset(S.SCENES[name]()))
        grp.transfer_function_changed(synth.tf_color())
        labels, rec, info = check_labels(grp, ref, lo, hi, conn, box, "members")
        assert grp.last_kernel_name() == NAME % ("float", 26)
        seed = (7, 8, 9)
        want = label_ref.region_grow(None, seed, lo, hi, conn, box, labelled=ref)
        mask, comp = grp.region_grow(seed, lo, hi, conn, box)
        assert mask.tobytes() == want[0].tobytes() and comp == want[1]
    finally:
        grp.close()


# ---- 10. ties -----------------------------------------------------------------------------------------------------
def test_ties_to_the_mesh_and_the_histogram(gpu, scene_pass):
    for name, iso in (("ball", 0.25), ("bigball", 20.25), ("noise", 0.5)):
        rp = scene_pass(name)
        vol = S.SCENES[name]()
        for box in (None, S.BOX):
            info = rp.label_count(iso, INF, 6, box)
            assert info["in_voxels"] == rp.mesh_count(iso, True, False, box)["inside_voxels"]
            # the histogram's count of the same window: one bin from iso to above the maximum
            top = float(np.nextafter(F(vol.max()), F(INF)))
            bins, hinfo = rp.histogram(1, iso, top, box=box)
            assert info["in_voxels"] == int(bins[0])
            labels, rec, info2 = rp.label(iso, INF, 6, box)
            assert int(rec["voxels"].sum()) == info["in_voxels"] and info2 == info
            assert info["largest_voxels"] <= info["in_voxels"]
            if name == "ball":
                assert info["largest_voxels"] == info["in_voxels"] and info["components"] == 1


# ---- 11. vr_cli --label -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn,seeded", [(6, False), (26, True), (6, True)])
def test_cli_prints_what_the_binding_returns(gpu, tmp_path, conn, seeded):
    import json
    import os
    import subprocess
    n = 20
    rp = vr_amd.OffscreenPass(16, 16)
    try:
        vlo, vhi = rp.generate_volume((n, n, n), np.float32, seed=2024)
        lo, hi = float(F(vlo + 0.3 * (vhi - vlo))), float(F(vhi))
        info = rp.label_count(lo, hi, conn)
        vol = rp.read_volume()
        seed = tuple(int(v) for v in np.unravel_index(int(np.argmax(vol)), vol.shape)[::-1])
        _, comp = rp.region_grow(seed, lo, hi, conn)
    finally:
        rp.close()
    assert info["components"] >= 1 and comp["voxels"] >= 1
    ppm = tmp_path / "never.ppm"
    cli = os.path.join(os.path.dirname(vr_amd.LIB_PATH), "vr_cli")
    arg = f"{lo!r}:{hi!r}" + (":26" if conn == 26 else "")
    cmd = [cli, f"synthetic:{n}", str(ppm), "--label", arg]
    if seeded:
        cmd += ["--seed", "%d,%d,%d" % seed]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert not ppm.exists()
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    got = json.loads(lines[0])
    want = dict(info)
    if seeded:
        want["seed"] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in comp.items()}
    assert got == want
