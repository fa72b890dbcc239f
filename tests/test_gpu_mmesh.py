"""GPU: the surface of a mask or of one label as a mesh (include/vr/vr_mmesh.h,
lib/libvr_amd_mmesh.so) against tests/mmesh_ref.py -- vertices, triangles and info byte for byte in
the header's order, closed and open, with and without normals and smoothing, from byte and 4-byte
arrays; the count forms, the host forms, a short capacity, the refusals, the chain from a click to
a mesh on one context, and the context's state."""
import ctypes as C
import os

import numpy as np
import pytest

import label_ref
import maskcc_ref
import mesh_scenes
import mmesh_ref as R
import mmesh_scenes as S
import morph_ref
import synth
import vr_amd
from gpu_kit import GUARD, context_untouched, device_bytes, err, first_difference, guarded, read_guarded, unchanged
from gpu_kit import stream  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
VB, TB = 24, 12  # bytes of a vertex record and of a triangle


def ramp(dims):
    """A volume of the given (nx, ny, nz): a mask mesh reads its dims alone."""
    nx, ny, nz = dims
    return (np.arange(nx * ny * nz, dtype=np.int64) % 251).astype(F).reshape(nz, ny, nx) / F(250.0)


def make_pass(vol, **kw):
    rp = vr_amd.OffscreenPass(32, 24, **kw)
    rp.volume_dataset_changed(synth.dataset(np.asarray(vol, F)))
    rp.transfer_function_changed(synth.tf_color())
    return rp


@pytest.fixture(scope="module")
def passes(gpu):
    """One context per volume size for the whole module: the calls wear it, as a session does."""
    made = {}

    def get(dims):
        if dims not in made:
            made[dims] = make_pass(ramp(dims))
        return made[dims]

    yield get
    for rp in made.values():
        rp.close()


class Source:
    """A scene's array in device memory (a byte mask at an odd address) and its requests."""

    def __init__(self, rp, stream, name):
        self.array, self.dims, self.origin, self.label = S.scene(name)
        self.odd = self.array.dtype.itemsize == 1
        self.keep, self.ptr = device_bytes(self.array, self.odd)
        self.rp, self.st = rp, stream.cuda_stream

    def request(self, closed=True, normals=True, smooth_iters=0, relax=0.5, **kw):
        return vr_amd.mmesh_request(S.ext_of(self.array), self.ptr, self.array.dtype.itemsize, self.origin, self.label,
                                    closed, normals, smooth_iters, relax, **kw)

    def extract(self, want_info, **kw):
        """The device form into guarded buffers of exactly the mesh's size: (verts, tris, info)."""
        nv, nt = want_info["vertices"], want_info["triangles"]
        vt, vptr, voff = guarded(VB * nv)
        tt, tptr, toff = guarded(TB * nt)
        info = self.rp.mask_mesh_extract_device(self.request(**kw), vptr, nv, tptr, nt, stream=self.st)
        # (complete on return: no synchronisation of ours before the copies)
        return read_guarded(vt, voff, VB * nv), read_guarded(tt, toff, TB * nt), info

    def intact(self):
        return unchanged(self.keep, self.array, self.odd)


def check(src, what, **kw):
    want = S.reference(what, **kw)
    gv, gt, info = src.extract(want.info, **kw)
    assert info == want.info, (what, kw, info, want.info)
    assert gt == want.tris.tobytes(), (what, kw, "triangles", first_difference(gt, want.tris.tobytes(), TB))
    assert gv == want.verts.tobytes(), (what, kw, "vertices", first_difference(gv, want.verts.tobytes(), VB))
    return want, gv, gt


REQUESTS = [dict(normals=True, smooth_iters=0), dict(normals=False, smooth_iters=0),
            dict(normals=False, smooth_iters=1, relax=0.5), dict(normals=True, smooth_iters=5, relax=0.5),
            dict(normals=True, smooth_iters=1, relax=1.0), dict(normals=False, smooth_iters=5, relax=1.0)]
PARITY = ["ball", "noise", "inner", "labels", "labels_any", "labels_high", "thin"] + ["row%d" % b for b in S.ROW_EXTS]


# ---- 1. byte for byte ------------------------------------------------------------------------------------
@pytest.mark.parametrize("closed", [True, False], ids=["closed", "open"])
@pytest.mark.parametrize("name", PARITY)
def test_parity(gpu, stream, passes, name, closed):
    rp = passes(S.scene(name)[1])
    src = Source(rp, stream, name)
    for kw in REQUESTS:
        want, gv, gt = check(src, name, closed=closed, **kw)
        assert want.info["vertices"] > 0 and want.info["triangles"] > 0
        assert rp.mmesh_last_kernel_name() == "mmesh_triangle_kernel"
    # the count forms say what the extraction said; a second extraction writes the same bytes
    assert rp.mask_mesh_count_device(src.request(closed), stream=src.st) == want.info
    assert rp.mmesh_last_kernel_name() == "mmesh_scan_kernel"
    assert rp.mask_mesh_count(src.array, src.origin, src.label, closed) == want.info
    gv2, gt2, _ = src.extract(want.info, closed=closed, **REQUESTS[-1])
    assert gv2 == gv and gt2 == gt
    # the host form is the device form
    kw = REQUESTS[3]
    want = S.reference(name, closed=closed, **kw)
    v, t, info = rp.mask_mesh_extract(src.array, src.origin, src.label, closed, kw["normals"], kw["smooth_iters"], kw["relax"])
    assert info == want.info and v.tobytes() == want.verts.tobytes() and t.tobytes() == want.tris.tobytes()
    assert src.intact()


@pytest.mark.parametrize("name", ["slab_x", "slab_y", "slab_z", "zeros", "ones"])
def test_thin_and_uniform_grids(gpu, stream, passes, name):
    """One voxel thick: the open form has no cell and the closed form is two cells thick.  All zero:
    nothing.  All set: the closed form is the box's cap, the open form nothing."""
    rp = passes(S.scene(name)[1])
    src = Source(rp, stream, name)
    for closed in (True, False):
        for kw in (REQUESTS[0], REQUESTS[3]):
            want, gv, gt = check(src, name, closed=closed, **kw)
            empty = not closed or name == "zeros"
            assert (want.info["vertices"] == 0) == empty and (want.info["triangles"] == 0) == empty
        assert rp.mask_mesh_count_device(src.request(closed), stream=src.st) == want.info
        v, t, info = rp.mask_mesh_extract(src.array, src.origin, src.label, closed)
        assert info == want.info and len(v) == info["vertices"] and len(t) == info["triangles"]
    assert want.info["matching"] == int((src.array != 0).sum())
    if name == "ones":
        e = S.ext_of(src.array)
        cap = S.reference(name, closed=True).info
        # the box's cap: a vertex per surface cell of the (e + 1)^3 cells, a quad per surface edge
        assert cap["vertices"] == np.prod([x + 1 for x in e]) - np.prod([x - 1 for x in e])
        assert cap["triangles"] == 4 * (e[0] * e[1] + e[1] * e[2] + e[2] * e[0])
    assert src.intact()


# ---- 2. a short capacity ---------------------------------------------------------------------------------
def test_a_short_capacity_reports_the_needed_sizes(gpu, stream, passes):
    L = vr_amd.mmesh_lib()
    rp = passes(S.scene("ball")[1])
    src = Source(rp, stream, "ball")
    want = S.reference("ball").info
    nv, nt = want["vertices"], want["triangles"]
    vt, vptr, voff = guarded(VB * nv)
    tt, tptr, toff = guarded(TB * nt)
    req = src.request(smooth_iters=2)
    for vcap, tcap in ((nv - 1, nt), (nv, nt - 1), (0, 0), (nv - 1, 2 ** 40)):
        info = vr_amd.vr_mmesh_info()
        C.memset(C.byref(info), GUARD, 32)
        rc = L.vr_mask_mesh_extract_device(rp._ctx, C.byref(req), vptr, vcap, tptr, tcap, C.byref(info), src.st)
        assert rc == vr_amd.ENOSPC and "smaller than the mesh" in err(rp), (vcap, tcap, rc, err(rp))
        assert rp._mmesh_info(info) == want
        assert read_guarded(vt, voff, VB * nv) == bytes([GUARD]) * (VB * nv)
        assert read_guarded(tt, toff, TB * nt) == bytes([GUARD]) * (TB * nt)
    # the host form
    hv, ht = np.full(VB * nv, GUARD, np.uint8), np.full(TB * nt, GUARD, np.uint8)
    hreq = vr_amd.mmesh_request(S.ext_of(src.array), src.array.ctypes.data, 1)
    info = vr_amd.vr_mmesh_info()
    rc = L.vr_mask_mesh_extract(rp._ctx, C.byref(hreq), hv.ctypes.data, nv, ht.ctypes.data, nt - 1, C.byref(info))
    assert rc == vr_amd.ENOSPC and rp._mmesh_info(info) == want and np.all(hv == GUARD) and np.all(ht == GUARD)
    # the sizes it reported are enough
    assert rp.mask_mesh_extract_device(req, vptr, nv, tptr, nt, stream=src.st) == want
    assert src.intact()


# ---- 3. refusals -----------------------------------------------------------------------------------------
def test_every_error_leaves_the_outputs_untouched(gpu, stream, passes):
    import torch
    L = vr_amd.mmesh_lib()
    rp = passes(mesh_scenes.DIMS)
    empty = vr_amd.OffscreenPass(32, 24)  # no volume
    try:
        src = Source(rp, stream, "inner")
        lab = Source(rp, stream, "labels")
        want = S.reference("inner").info
        nv, nt = want["vertices"], want["triangles"]
        vt, vptr, voff = guarded(VB * nv)
        tt, tptr, toff = guarded(TB * nt)
        info = vr_amd.vr_mmesh_info()
        C.memset(C.byref(info), GUARD, 32)
        e, o = S.ext_of(src.array), src.origin
        both = torch.full((VB * nv + TB * nt + 64,), GUARD, dtype=torch.uint8, device="cuda")
        bp = both.data_ptr()

        def refused(text, req, verts=vptr, vcap=nv, tris=tptr, tcap=nt, ctx=None, count=True, inf=info):
            ctx = rp if ctx is None else ctx
            q = C.byref(req) if req is not None else None
            i = C.byref(inf) if inf is not None else None
            rcs = [L.vr_mask_mesh_extract_device(ctx._ctx, q, verts, vcap, tris, tcap, i, src.st)]
            msgs = [err(ctx)]
            if count:
                rcs.append(L.vr_mask_mesh_count_device(ctx._ctx, q, i, src.st))
                msgs.append(err(ctx))
            assert rcs == [-22] * len(rcs) and all(m.startswith("mask mesh:") and text in m for m in msgs), (text, rcs, msgs)
            assert bytes(info) == bytes([GUARD]) * 32
            assert read_guarded(vt, voff, VB * nv) == bytes([GUARD]) * (VB * nv)
            assert read_guarded(tt, toff, TB * nt) == bytes([GUARD]) * (TB * nt)

        R_ = src.request
        refused("NULL", None)
        refused("NULL", R_(), inf=None)
        refused("NULL", R_(), verts=None, count=False)
        refused("NULL", R_(), tris=None, count=False)
        q = R_()
        q.array = None
        refused("NULL", q)
        for bad in ((0, e[1], e[2]), (32769, 1, 1)):
            q = R_()
            q.ext[:] = bad
            refused("extent", q)
        q = R_()
        q.ext[:] = (32768, 32768, 4)
        refused("2^32 - 1 voxels", q)
        refused("elem_bytes", vr_amd.mmesh_request(e, src.ptr, 2, o))
        refused("4-byte aligned", vr_amd.mmesh_request(S.ext_of(lab.array), lab.ptr + 2, 4))
        refused("select", R_(select=2))
        refused("non-zero label", vr_amd.mmesh_request(S.ext_of(lab.array), lab.ptr, 4, select=vr_amd.MVIEW_LABEL))
        refused("closed", R_(closed=2))
        refused("normals", R_(normals=2))
        refused("smooth_iters", R_(smooth_iters=vr_amd.MMESH_MAX_ITERS + 1))
        for bad in (float("nan"), float("inf"), -0.25, 1.5):
            refused("relax", R_(relax=bad))
        refused("reserved", R_(reserved=1))
        refused("an output must be 4-byte aligned", R_(), verts=vptr + 2, count=False)
        refused("an output must be 4-byte aligned", R_(), tris=tptr + 1, count=False)
        refused("overlaps the array", R_(), verts=(src.ptr + 3) & ~3, count=False)
        refused("overlaps the array", R_(), tris=(src.ptr + src.array.nbytes - 1) & ~3, count=False)
        refused("outputs overlap", R_(), verts=bp, tris=bp + VB * nv - 4, count=False)
        refused("beyond the volume", vr_amd.mmesh_request(e, src.ptr, 1, (o[0] + 6, o[1], o[2])))
        refused("beyond the volume", vr_amd.mmesh_request(e, src.ptr, 1, (0xFFFFFFFF, 0, 0)))
        refused("volume", R_(), ctx=empty)  # "no volume" (no bricks) or "beyond the volume" (the 1-voxel default)
        # the host forms: the same rules, and an output over the info
        hv, ht = np.full(VB * nv + 32, GUARD, np.uint8), np.full(TB * nt, GUARD, np.uint8)
        hq = vr_amd.mmesh_request(e, src.array.ctypes.data, 1, o)
        over = C.cast(hv.ctypes.data + 8, C.POINTER(vr_amd.vr_mmesh_info))
        assert L.vr_mask_mesh_extract(rp._ctx, C.byref(hq), hv.ctypes.data, nv, ht.ctypes.data, nt, over) == -22
        assert "overlaps the info" in err(rp)
        hq.relax = 2.0
        assert L.vr_mask_mesh_extract(rp._ctx, C.byref(hq), hv.ctypes.data, nv, ht.ctypes.data, nt, C.byref(info)) == -22
        assert L.vr_mask_mesh_count(rp._ctx, C.byref(hq), C.byref(info)) == -22 and "relax" in err(rp)
        assert np.all(hv == GUARD) and np.all(ht == GUARD) and bytes(info) == bytes([GUARD]) * 32
        assert np.all(both.cpu().numpy() == GUARD)
        # and the context still works
        check(src, "inner", closed=True)
        assert src.intact() and lab.intact()
    finally:
        empty.close()


# ---- 4. the chain ----------------------------------------------------------------------------------------
def test_the_chain_from_a_click_to_a_mesh(gpu, stream, tmp_path):
    """vr_region_grow_device, vr_mask_morph_device (open), vr_mask_select_device (KEEP_SEED) and
    vr_mask_mesh_extract_device on one context, the mask never read back; the references chained on
    the CPU; vr_mesh_write_ply takes the result."""
    import torch
    dims, box = mesh_scenes.DIMS, mesh_scenes.BOX
    vol = np.clip(mesh_scenes.small_ball() / F(12.0) + F(0.5), 0.0, 1.0).astype(F)
    bump = np.random.default_rng(3).random(vol.shape) < 0.04  # specks the open removes
    vol = np.where(bump, F(1.0), vol).astype(F)
    lo, hi, seed = 0.52, 1.0, (8, 8, 10)
    m0, comp0 = label_ref.region_grow(vol, seed, lo, hi, 6, box)
    m1, _ = morph_ref.morph(m0, vr_amd.MORPH_OPEN, 2)
    gseed = tuple(s - b for s, b in zip(seed, box[0]))
    m2, sel = maskcc_ref.select(m1, vr_amd.MASK_KEEP_SEED, 6, seed=gseed)
    assert 0 < int(m2.sum()) < int(m0.sum()) and m2[gseed[2], gseed[1], gseed[0]] == 1
    kw = dict(closed=True, normals=True, smooth_iters=3, relax=0.5)
    want = R.extract(m2, dims, box[0], **kw)
    ext = S.ext_of(m0)
    n = m0.size
    rp = make_pass(vol)
    try:
        st = stream.cuda_stream
        a, b, c = (torch.full((n + 8,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        comp = rp.region_grow_device(seed, a.data_ptr(), n, lo, hi, 6, box, stream=st)
        assert comp["voxels"] == comp0["voxels"]
        rp.morph_device(ext, vr_amd.MORPH_OPEN, 2, a.data_ptr(), 1, b.data_ptr(), n, stream=st)
        sinfo = rp.mask_select_device(ext, vr_amd.MASK_KEEP_SEED, b.data_ptr(), 1, c.data_ptr(), n, 6, seed=gseed, stream=st)
        assert sinfo == sel
        req = vr_amd.mmesh_request(ext, c.data_ptr(), 1, box[0], None, **kw)
        cnt = rp.mask_mesh_count_device(req, stream=st)
        assert cnt == want.info and cnt["matching"] == int(m2.sum())
        nv, nt = cnt["vertices"], cnt["triangles"]
        vt, vptr, voff = guarded(VB * nv)
        tt, tptr, toff = guarded(TB * nt)
        assert rp.mask_mesh_extract_device(req, vptr, nv, tptr, nt, stream=st) == want.info
        gv, gt = read_guarded(vt, voff, VB * nv), read_guarded(tt, toff, TB * nt)
        assert gv == want.verts.tobytes() and gt == want.tris.tobytes()
        assert c.cpu().numpy()[:n].tobytes() == m2.tobytes()  # (read back only now, to check the chain itself)
        verts = np.frombuffer(gv, vr_amd.MESH_VERTEX_DTYPE)
        tris = np.frombuffer(gt, np.uint32).reshape(-1, 3)
        path = str(tmp_path / "piece.ply")
        vr_amd.write_ply(path, verts, tris)
        head = open(path, "rb").read(400)
        assert head.startswith(b"ply") and b"element vertex %d" % nv in head and b"element face %d" % nt in head
        assert os.path.getsize(path) > VB * nv
    finally:
        rp.close()


# ---- 5. state --------------------------------------------------------------------------------------------
def test_the_calls_leave_the_context_as_it_was(gpu, stream):
    a, dims, origin, label = S.scene("ball")
    rp = make_pass(mesh_scenes.small_ball())
    try:
        with context_untouched(rp):
            assert rp.mmesh_last_kernel_name() == ""  # a fresh context
            src = Source(rp, stream, "ball")
            rp.timing_enable(True)
            rp.timing_reset()
            assert rp.mask_mesh_count_device(src.request(), stream=src.st) == S.reference("ball").info
            assert rp.timing_read()[1] == 1 and rp.mmesh_last_kernel_name() == "mmesh_scan_kernel"
            rp.timing_reset()
            check(src, "ball", closed=True, normals=True, smooth_iters=5, relax=0.5)
            assert rp.timing_read()[1] == 1 and rp.mmesh_last_kernel_name() == "mmesh_triangle_kernel"
            rp.timing_reset()
            info = vr_amd.vr_mmesh_info()
            req = src.request()
            vt, vptr, voff = guarded(VB)
            tt, tptr, toff = guarded(TB)
            assert vr_amd.mmesh_lib().vr_mask_mesh_extract_device(rp._ctx, C.byref(req), vptr, 1, tptr, 1, C.byref(info),
                                                                  src.st) == -28
            assert rp.timing_read()[1] == 1  # the count pass ran, and its interval is whole
            rp.timing_enable(False)
            rp.timing_reset()
            v, t, hinfo = rp.mask_mesh_extract(a, origin, label, True, True, 5, 0.5)
            want = S.reference("ball", closed=True, normals=True, smooth_iters=5, relax=0.5)
            assert rp.timing_read()[1] == 0 and v.tobytes() == want.verts.tobytes() and t.tobytes() == want.tris.tobytes()
        assert src.intact()
    finally:
        rp.close()


def test_a_multi_device_context_computes_on_its_lowest_device(gpu, stream):
    grp = make_pass(ramp(mesh_scenes.DIMS), exchange=vr_amd.EXCHANGE_COPY, members=[0, 0])
    try:
        for name in ("inner", "ball"):
            src = Source(grp, stream, name)
            kw = dict(closed=True, normals=True, smooth_iters=5, relax=0.5)
            want, gv, gt = check(src, name, **kw)
            assert grp.mask_mesh_count_device(src.request(), stream=src.st) == want.info
            v, t, info = grp.mask_mesh_extract(src.array, src.origin, src.label, True, True, 5, 0.5)
            assert v.tobytes() == gv and t.tobytes() == gt and info == want.info
        assert grp.mmesh_last_kernel_name() == "mmesh_triangle_kernel"
    finally:
        grp.close()
