"""CPU: the mask mesh's reference, scenes, binding and host checks (include/vr/vr_mmesh.h).

tests/mmesh_ref.py is pinned by something independent of it: unsmoothed and without normals it is
tests/mesh_ref.py's mesh of the 0/1 indicator at iso 0.5, and under smoothing a closed mesh stays
closed and positively oriented.  The scenes are checked to reach what they are for, from the
family's constants in csrc/vr_mmesh_host.h.  The binding is checked against the header and the
libraries; the host checks run stand-alone under AddressSanitizer and UBSan.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mesh_ref
import mesh_scenes
import mmesh_ref as R
import mmesh_scenes as S
import vr_amd
from harness import run_sanitized

ROOT = S.ROOT
F = np.float32
K = S.K


def indicator(name):
    """The scene's 0/1 indicator embedded in a zero array of the volume's size, and its box."""
    a, dims, origin, label = S.scene(name)
    e = S.ext_of(a)
    ind = np.zeros((dims[2], dims[1], dims[0]), F)
    ind[origin[2]:origin[2] + e[2], origin[1]:origin[1] + e[1], origin[0]:origin[0] + e[0]] = R.match(a, label)
    return ind, (origin, tuple(origin[i] + e[i] for i in range(3)))


# ---- the reference is pinned by mesh_ref ---------------------------------------------------------------
@pytest.mark.parametrize("closed", [True, False], ids=["closed", "open"])
@pytest.mark.parametrize("name", ["ball", "noise", "inner", "labels", "row64", "slab_x", "ones", "zeros"])
def test_unsmoothed_is_the_isosurface_of_the_indicator(name, closed):
    got = S.reference(name, closed=closed, normals=False)
    ind, box = indicator(name)
    want = mesh_ref.extract(ind, 0.5, closed, normals=False, box=box)
    mesh_scenes.assert_same_mesh((got.verts, got.tris), (want.verts, want.tris), name)
    assert got.info["vertices"] == want.info["vertices"] and got.info["triangles"] == want.info["triangles"]
    assert got.info["matching"] == want.info["inside_voxels"] and got.info["voxels"] == S.scene(name)[0].size
    if len(got.local):
        assert got.local.min() >= F(1.0) / F(6.0) and got.local.max() <= F(5.0) / F(6.0)
    assert not got.verts["normal"].any()


def test_the_ball_is_mesh_scenes_pinned_case():
    i = S.reference("ball").info
    assert (i["vertices"], i["triangles"], i["matching"]) == mesh_scenes.CASES[("ball", True, None)] == (622, 1240, 792)


def test_the_order_is_the_headers():
    """Vertices in cell-linear order, triangles by owner cell then axis: read off the positions."""
    m = S.reference("noise", closed=True, normals=False)
    dims = np.asarray(m.dims, np.float64)
    cell = np.floor(m.verts["pos"].astype(np.float64) * dims - 0.5).astype(np.int64)  # local in (0, 1)
    nc = [d + 1 for d in m.dims]
    lin = (cell[:, 0] + 1) + nc[0] * ((cell[:, 1] + 1) + nc[1] * (cell[:, 2] + 1))
    assert np.all(np.diff(lin) > 0)
    owner = lin[m.tris].max(axis=1)  # C2 = P is the last of the four cells in cell-linear order
    assert np.all(np.diff(owner) >= 0)
    assert np.array_equal(m.tris[0::2, 0], m.tris[1::2, 0])  # two triangles of a quad share C0


# ---- properties ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ball", "noise", "inner", "labels", "thin"])
def test_closed_meshes_stay_closed_and_oriented_under_smoothing(name):
    base = S.reference(name, closed=True, normals=False)
    for iters, relax in ((0, 0.5), (1, 0.5), (5, 0.5), (5, 1.0)):
        m = S.reference(name, closed=True, normals=False, smooth_iters=iters, relax=relax)
        assert m.tris.tobytes() == base.tris.tobytes()  # connectivity never changes
        assert mesh_ref.edge_report(m.tris)[0]
        assert mesh_ref.signed_volume(m.verts, m.tris, m.dims) > 0
        assert len(m.local) and m.local.min() >= 0 and m.local.max() <= 1
        if iters:
            assert m.verts.tobytes() != base.verts.tobytes()
    still = S.reference(name, closed=True, normals=False, smooth_iters=5, relax=0.0)
    assert still.verts.tobytes() == base.verts.tobytes() and still.tris.tobytes() == base.tris.tobytes()


def test_smoothing_clamps_some_vertex_to_its_cell():
    m = S.reference("ball", closed=True, normals=False, smooth_iters=5, relax=0.5)
    assert m.clamped[:2] == [0, 0] and m.clamped[2] > 0  # first at the third sweep
    assert ((m.local == 0) | (m.local == 1)).any()
    assert sum(S.reference("thin", closed=True, smooth_iters=5, relax=1.0).clamped) > 0


def test_normals_are_unit_or_zero():
    seen_zero = False
    for name in ("ball", "noise", "labels"):
        m = S.reference(name, closed=True, normals=True)
        n = m.verts["normal"].astype(np.float64)
        length = np.sqrt((n * n).sum(axis=1))
        zero = length == 0
        assert np.all(np.abs(length[~zero] - 1.0) < 1e-6) and not np.signbit(m.verts["normal"][zero]).any()
        seen_zero |= bool(zero.any())
        # smoothing and normals do not touch each other
        s = S.reference(name, closed=True, normals=True, smooth_iters=5, relax=0.5)
        assert s.verts["normal"].tobytes() == m.verts["normal"].tobytes()
        assert S.reference(name, closed=True, normals=False).verts["pos"].tobytes() == m.verts["pos"].tobytes()
    assert seen_zero  # the noise mask holds cells whose corners balance
    # the ball's normals point outward: away from its centre
    m = S.reference("ball", closed=True, normals=True)
    out = m.verts["pos"] * np.asarray(m.dims, F) - np.asarray(mesh_scenes.CENTRE, F) - F(0.5)
    assert ((out * m.verts["normal"]).sum(axis=1) > 0).all()


# ---- the scenes reach what they are for ------------------------------------------------------------------
def test_the_scenes_reach_what_they_are_for():
    word = K["kMmeshWord"]
    for closed in (True, False):
        rows = {S.geometry(S.ext_of(S.scene("row%d" % b)[0]), closed)["nc"][0] for b in S.ROW_EXTS}
        assert {word - 1, word, word + 1} <= rows, (closed, rows)  # a cell row ends before, at and after the boundary
        for b in S.ROW_EXTS:  # and the last cells of those rows hold vertices
            m = S.reference("row%d" % b, closed=closed, normals=False)
            g = S.geometry((b, 5, 4), closed)
            x = np.floor(m.verts["pos"][:, 0].astype(np.float64) * b - 0.5).astype(np.int64) + (1 if closed else 0)
            assert x.max() == g["nc"][0] - 1 and (x == word - 1).any() == (g["nc"][0] >= word)
    a, dims, origin, label = S.scene("thin")
    g = S.geometry(S.ext_of(a), True)
    assert g["groups"] > 1 and g["span"] > K["kMmeshScanTile"]  # several scan workgroups, each with a carry
    assert g["cell_words"] > g["span"] and g["groups"] * g["span"] >= g["cell_words"] > (g["groups"] - 1) * g["span"]
    waves = K["kMmeshMaxGroups"] * K["kMmeshWaves"]
    assert g["node_rows"] > K["kMmeshMaxGroups"] and g["node_words"] > waves  # the bits pass strides
    assert S.reference("thin").info["vertices"] > word * K["kMmeshScanTile"]
    a, dims, origin, label = S.scene("inner")
    assert all(o > 0 for o in origin) and all(o + e < d for o, e, d in zip(origin, S.ext_of(a), dims))
    assert a.dtype == np.uint8  # the GPU test places byte arrays at an odd address
    a, dims, origin, label = S.scene("labels")
    assert a.dtype == np.uint32 and label == 2 and len(np.unique(a)) >= 6 and (a == 0).any()
    z, y, x = np.nonzero(a == label)
    touching = {int(v) for v in a[z, y, np.minimum(x + 1, a.shape[2] - 1)]} | {int(v) for v in a[z, np.minimum(y + 1, a.shape[1] - 1), x]}
    assert len(touching - {0, label}) >= 2  # LABEL selects one of several touching labels
    assert S.reference("labels").info["matching"] == int((a == 2).sum()) < S.reference("labels_any").info["matching"]
    assert S.reference("labels_high").info["matching"] == int((a == 0x80000005).sum()) > 0
    for ax, name in enumerate(("slab_x", "slab_y", "slab_z")):
        a = S.scene(name)[0]
        assert S.ext_of(a)[ax] == 1 and S.geometry(S.ext_of(a), False)["cells"] == 0
        assert S.geometry(S.ext_of(a), True)["nc"][ax] == 2 and S.reference(name, closed=False).info["vertices"] == 0
    assert S.reference("ones", closed=True).info["vertices"] > 0 == S.reference("ones", closed=False).info["vertices"]
    assert S.reference("zeros", closed=True).info["vertices"] == 0


# ---- the binding -----------------------------------------------------------------------------------------
def test_every_declared_name_is_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "vr", "vr_mmesh.h")).read()
    for h in ("vr_mesh.h", "vr_mview.h"):
        assert f'#include "{h}"' in src
    assert "#define VR_ENOSPC" not in src and "typedef struct vr_mesh_vertex" not in src  # reused, not redefined
    assert "enum vr_mview_select" not in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))
    assert names == set(vr_amd.MMESH_SYMBOLS) and len(names) == 5
    assert os.path.dirname(vr_amd.MMESH_LIB_PATH) == os.path.dirname(vr_amd.LIB_PATH)
    assert vr_amd.FAMILY_LIBS["mmesh"] == ("VR_AMD_MMESH_LIB", "libvr_amd_mmesh.so")
    nm = lambda path: {l.split()[-1] for l in subprocess.run(
        ["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()
        if " T " in l}
    assert not names - nm(vr_amd.MMESH_LIB_PATH)
    for other in (vr_amd.LIB_PATH, vr_amd.MORPH_LIB_PATH, vr_amd.MASKCC_LIB_PATH, vr_amd.MSTAT_LIB_PATH,
                  vr_amd.MVIEW_LIB_PATH):
        assert not names & nm(other)
    L = vr_amd.mmesh_lib()
    assert all(getattr(L, n).argtypes is not None for n in names)
    assert vr_amd.ABI_VERSION == 9 and vr_amd.lib().vr_abi_version() == 9  # an addition: the ABI stays
    for m in ("mask_mesh_count", "mask_mesh_count_device", "mask_mesh_extract", "mask_mesh_extract_device",
              "mmesh_last_kernel_name"):
        assert callable(getattr(vr_amd.OffscreenPass, m))
    # the sixth library takes the scaffold from the first, found beside it, and nothing from its siblings
    dyn = subprocess.run(["readelf", "-d", vr_amd.MMESH_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libvr_amd.so" in dyn and "$ORIGIN" in dyn
    assert not any(f"libvr_amd_{f}" in dyn for f in ("morph", "maskcc", "mstat", "mview"))
    # the existing families keep their names
    assert list(vr_amd.FAMILY_LIBS) == ["morph", "maskcc", "mstat", "mview", "mmesh"]


def test_struct_layouts_match_header(tmp_path):
    fields = {"vr_mmesh_request": ["ext", "origin", "elem_bytes", "select", "label", "closed", "normals", "smooth_iters",
                                   "relax", "reserved", "array"],
              "vr_mmesh_info": ["voxels", "vertices", "triangles", "matching"]}
    body = "".join(f'  printf("%zu ", sizeof({s}));\n' +
                   "".join(f'  printf("%zu ", offsetof({s}, {f}));\n' for f in fs) for s, fs in fields.items())
    test = '#include "vr/vr_mmesh.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n' + body + \
           '  printf("%d %u %u %d %d %zu\\n", VR_ENOSPC, VR_MMESH_MAX_EXTENT, VR_MMESH_MAX_ITERS, VR_MVIEW_ANY, ' \
           'VR_MVIEW_LABEL, sizeof(vr_mesh_vertex)); return 0; }\n'
    tmp = str(tmp_path / "vr_mmesh_layout")
    with open(tmp + ".c", "w") as f:
        f.write(test)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), tmp + ".c", "-o", tmp], check=True)
    out = [int(x) for x in subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for s, fs in fields.items():
        T = getattr(vr_amd, s)
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fs]
    assert out == want + [-28, vr_amd.MMESH_MAX_EXTENT, vr_amd.MMESH_MAX_ITERS, vr_amd.MVIEW_ANY, vr_amd.MVIEW_LABEL, 24]
    assert C.sizeof(vr_amd.vr_mmesh_request) == 56 + C.sizeof(C.c_void_p) and C.sizeof(vr_amd.vr_mmesh_info) == 32
    assert vr_amd.MESH_VERTEX_DTYPE == R.VERTEX_DTYPE and R.VERTEX_DTYPE.itemsize == K["kMmeshVertexBytes"] == 24
    assert vr_amd.MMESH_MAX_ITERS == K["kMmeshMaxIters"] == 64 and K["kMmeshTriBytes"] == 12
    q = vr_amd.mmesh_request((3, 4, 5), 0x1000, 4, (1, 2, 3), label=7, closed=False, normals=False, smooth_iters=9, relax=0.25)
    assert (list(q.ext), list(q.origin), q.elem_bytes, q.select, q.label, q.closed, q.normals, q.smooth_iters, q.relax,
            q.reserved, q.array) == ([3, 4, 5], [1, 2, 3], 4, vr_amd.MVIEW_LABEL, 7, 0, 0, 9, 0.25, 0, 0x1000)
    assert vr_amd.mmesh_request((1, 1, 1), 8, 1).select == vr_amd.MVIEW_ANY


def test_a_null_context_is_refused_with_the_outputs_untouched():
    L = vr_amd.mmesh_lib()
    info = vr_amd.vr_mmesh_info()
    C.memset(C.byref(info), 0x77, 32)
    mask = np.full(4, 1, np.uint8)
    verts, tris = np.full(24 * 8, 0x77, np.uint8), np.full(12 * 8, 0x77, np.uint8)
    req = vr_amd.mmesh_request((2, 2, 1), mask.ctypes.data, 1)
    assert L.vr_mask_mesh_count_device(None, C.byref(req), C.byref(info), None) == -22
    assert b"NULL" in vr_amd.lib().vr_last_error(None)  # the message is the first library's, as every family's
    assert L.vr_mask_mesh_count(None, C.byref(req), C.byref(info)) == -22
    assert L.vr_mask_mesh_extract_device(None, C.byref(req), verts.ctypes.data, 8, tris.ctypes.data, 8, C.byref(info), None) == -22
    assert L.vr_mask_mesh_extract(None, C.byref(req), verts.ctypes.data, 8, tris.ctypes.data, 8, C.byref(info)) == -22
    assert L.vr_mask_mesh_extract(None, C.byref(req), verts.ctypes.data, 0, tris.ctypes.data, 0, C.byref(info)) == -22  # (not -28)
    assert L.vr_mask_mesh_count_device(None, None, None, None) == -22
    assert L.vr_mask_mesh_count(None, None, None) == -22
    assert L.vr_mask_mesh_extract_device(None, None, None, 0, None, 0, None, None) == -22
    assert L.vr_mask_mesh_extract(None, None, None, 0, None, 0, None) == -22
    assert L.vr_mmesh_last_kernel_name(None) == b""
    assert bytes(info) == b"\x77" * 32 and np.all(verts == 0x77) and np.all(tris == 0x77) and np.all(mask == 1)


# ---- the host helper header, stand-alone, under AddressSanitizer + UBSan ---------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_host_helpers_under_sanitizers(tmp_path):
    """Every refusal that needs no device at its boundary, with its text, and the geometry and scratch
    sizes up to the largest grids, on csrc/vr_mmesh_host.h itself (the library's entry points refuse a
    NULL context before they reach it)."""
    stdout = run_sanitized(tmp_path, "mmesh")
    assert "request rules checked" in stdout and "output rules checked" in stdout
    # the geometry of every printed grid, restated here (tests/mmesh_scenes.py geometry)
    seen, largest = 0, 0
    for line in stdout.splitlines():
        w = line.replace(":", " ").split()
        if w[0] != "geom":
            continue
        ext, closed = [int(x) for x in w[1:4]], int(w[4])
        got = {w[i]: int(w[i + 1]) for i in range(5, len(w), 2)}
        g = S.geometry(ext, closed)
        assert all(got[k] == g[k] for k in ("nw", "cw", "node_words", "cells", "cell_words", "groups", "span")), (line, g)
        words = g["node_words"] * 8 + g["cell_words"] * 16 + (g["cell_words"] * 4 + 7) // 8 * 8
        assert got["scratch"] == words + K["kMmeshMaxGroups"] * 16 + 8
        assert g["node_words"] < 2 ** 32 and g["cell_words"] < 2 ** 32
        largest = max(largest, got["scratch"])
        seen += 1
    assert seen == 30 and largest == 30067146816  # 3 x 32768 x 32768: every row pads to a word
    n = range(1, 13)
    tot = [0, 0, 0]
    for a in n:
        for b in n:
            for c in n:
                for closed in (0, 1):
                    g = S.geometry((a * 11, b, c), closed)
                    tot = [tot[0] + g["node_words"], tot[1] + g["cell_words"], tot[2] + g["cells"]]
    assert "totals %d node words %d cell words %d cells" % tuple(tot) in stdout
