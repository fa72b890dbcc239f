"""CPU: the isosurface mesh (include/vr/vr_mesh.h) -- the reference helper tests/mesh_ref.py pinned
by properties that no implementation detail enters (closedness, orientation, the derived bound
between the mesh's volume and inside_voxels, the tie to the ISO hit records), the binding's symbols
and structs, the refusals that need no device, the C++ shim, the host helper header and the PLY
writer under AddressSanitizer + UBSan in a stand-alone program, the PLY writer of the library
through a reader of the test's own, and the frame kernels' machine code (the mesh_* kernels:
tests/test_kernel_inventory_cpu.py).  No GPU: nothing here creates a context."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hit_scenes
import mesh_ref
import mesh_scenes as S
import vr_amd
from harness import run_sanitized
from range_scenes import volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.dirname(vr_amd.LIB_PATH)
F = np.float32
CLOSED = [k for k in S.CASES if k[1]]


# ---- the reference, pinned before anything is compared with it ----------------------------------------
@pytest.mark.parametrize("name,closed,box", list(S.CASES))
def test_reference_counts_are_the_pinned_ones(name, closed, box):
    m = S.reference(name, closed, False, box)
    assert (m.info["vertices"], m.info["triangles"], m.info["inside_voxels"]) == S.CASES[(name, closed, box)]
    assert m.active_cells == m.info["vertices"]
    if len(m.tris):
        assert int(m.tris.max()) < len(m.verts)
        p = m.verts["pos"]
        lim = 0.5 / np.asarray(m.dims, np.float64)  # the ring cells reach half a voxel out
        assert np.all(p >= -lim - 1e-6) and np.all(p <= 1.0 + lim + 1e-6)


@pytest.mark.parametrize("name,box", [("ball", None), ("bigball", None), ("bigball", S.BOX)])
def test_closed_balls_are_oriented_two_manifolds(name, box):
    m = S.reference(name, True, False, box)
    balanced, counts = mesh_ref.edge_report(m.tris)
    assert balanced and counts == {2}  # every edge twice, once in each direction
    assert mesh_ref.euler(np.unique(m.tris).size, m.tris) == 2
    assert np.unique(m.tris).size == len(m.verts)  # no vertex is left over
    assert mesh_ref.signed_volume(m.verts, m.tris, m.dims) > 0.0  # outward


def test_the_open_ball_away_from_the_faces_is_the_closed_one():
    a, b = S.reference("ball", True, False, None), S.reference("ball", False, False, None)
    S.assert_same_mesh((a.verts, a.tris), (b.verts, b.tris))


def test_an_open_mesh_cut_by_the_faces_has_a_rim():
    m = S.reference("bigball", False, False, None)
    balanced, counts = mesh_ref.edge_report(m.tris)
    assert not balanced and counts == {1, 2}


def test_closed_noise_balances_with_even_counts_and_is_not_manifold():
    m = S.reference("noise", True, False, None)
    balanced, counts = mesh_ref.edge_report(m.tris)
    assert balanced and all(c % 2 == 0 for c in counts) and counts == {2, 4}


@pytest.mark.parametrize("name,closed,box", CLOSED)
def test_volume_is_within_the_active_cells_of_the_inside_voxels(name, closed, box):
    """Derived, not measured: the mesh and the boundary of the union of the inside voxels' unit
    cubes both lie inside the union of the active cells, so the two enclosed volumes differ by at
    most the active cells' volume -- one lattice unit each."""
    m = S.reference(name, closed, False, box)
    v = mesh_ref.signed_volume(m.verts, m.tris, m.dims)
    print(name, box, "volume", v, "inside", m.info["inside_voxels"], "active", m.active_cells)
    assert abs(v - m.info["inside_voxels"]) <= m.active_cells


def test_normals_are_unit_outward_or_zero():
    m = S.reference("ball", True, True, None)
    n = m.verts["normal"].astype(np.float64)
    ln = np.sqrt((n * n).sum(axis=1))
    assert np.all(np.abs(ln - 1.0) < 1e-6)
    # outward from the ball's centre
    c = (np.asarray(S.CENTRE) + 0.5) / np.asarray(S.DIMS)
    out = (m.verts["pos"].astype(np.float64) - c) * np.asarray(S.DIMS)
    assert np.all((out * n).sum(axis=1) > 0.0)
    assert not S.reference("ball", True, False, None).verts["normal"].view(np.uint32).any()


def test_refined_iso_hits_of_the_reference_lie_within_a_cell_diagonal_of_the_mesh():
    """tests/hit_ref.py against tests/mesh_ref.py, before the device is asked the same
    (test_gpu_mesh.py): a refined VR_HIT_ISO point lies within one step -- 0.11 voxels here -- of
    a sign change of the trilinear field, and the cell the level set crosses there is active."""
    volname, camname, box, tfname, w, h = hit_scenes.PARITY[0]
    vol = volume(volname)
    iso = hit_scenes.isovalue(vol)
    walk = hit_scenes.reference(volname, camname, box, tfname, w, h)
    fine = walk.hits("iso") & ~walk.cap
    assert fine.sum() >= 100
    m = mesh_ref.cached(volname, lambda: vol, iso, True, False, None)
    nz, ny, nx = vol.shape
    dims = np.asarray((nx, ny, nz), np.float64)
    hp = walk.records["iso"]["pos"][fine].astype(np.float64) * dims
    vp = m.verts["pos"].astype(np.float64) * dims
    d = np.sqrt(((hp[:, None, :] - vp[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
    print("largest distance to a vertex", d.max())
    assert d.max() <= np.sqrt(3.0)


# ---- the binding ---------------------------------------------------------------------------------------
def test_every_declared_name_is_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "vr", "vr_mesh.h")).read()
    assert "#define VR_ENOSPC (-28)" in src and vr_amd.ENOSPC == -28
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", src))
    assert names == set(vr_amd.MESH_SYMBOLS) and len(names) == 3
    out = subprocess.run(["nm", "-D", "--defined-only", vr_amd.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not (names | {"vr_mesh_write_ply"}) - exported
    L = vr_amd.lib()
    assert all(getattr(L, n).argtypes is not None for n in names)
    assert vr_amd.ABI_VERSION == 9 and L.vr_abi_version() == 9  # an addition: the ABI stays
    assert vr_amd.MESH_VERTEX_DTYPE == mesh_ref.VERTEX_DTYPE and vr_amd.MESH_VERTEX_DTYPE.itemsize == 24


def test_struct_layouts_match_header(tmp_path):
    test = r"""
#include "vr/vr_mesh.h"
#include <stdio.h>
#include <stddef.h>
int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu  %zu %zu %zu  %zu %zu %zu %zu %zu\n",
  sizeof(vr_mesh_request), offsetof(vr_mesh_request, iso), offsetof(vr_mesh_request, closed),
  offsetof(vr_mesh_request, normals), offsetof(vr_mesh_request, use_box),
  offsetof(vr_mesh_request, box_min), offsetof(vr_mesh_request, box_max),
  sizeof(vr_mesh_vertex), offsetof(vr_mesh_vertex, pos), offsetof(vr_mesh_vertex, normal),
  sizeof(vr_mesh_info), offsetof(vr_mesh_info, vertices), offsetof(vr_mesh_info, triangles),
  offsetof(vr_mesh_info, inside_voxels), offsetof(vr_mesh_info, reserved)); return 0; }
"""
    tmp = str(tmp_path / "vr_mesh_layout")
    with open(tmp + ".c", "w") as f:
        f.write(test)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), tmp + ".c", "-o", tmp], check=True)
    out = subprocess.run([tmp], capture_output=True, text=True, check=True).stdout.split()
    R, V, I = vr_amd.vr_mesh_request, vr_amd.vr_mesh_vertex, vr_amd.vr_mesh_info
    assert [int(x) for x in out] == [
        C.sizeof(R), R.iso.offset, R.closed.offset, R.normals.offset, R.use_box.offset, R.box_min.offset,
        R.box_max.offset, C.sizeof(V), V.pos.offset, V.normal.offset,
        C.sizeof(I), I.vertices.offset, I.triangles.offset, I.inside_voxels.offset, I.reserved.offset]
    assert (C.sizeof(R), C.sizeof(V), C.sizeof(I)) == (40, 24, 32)
    D = vr_amd.MESH_VERTEX_DTYPE
    assert [D.fields[n][1] for n in ("pos", "normal")] == [0, 12]


def test_argument_errors_without_a_device():
    """Everything a NULL context refuses: -22, the outputs untouched."""
    L = vr_amd.lib()
    req = vr_amd.mesh_request(0.5)
    info = vr_amd.vr_mesh_info()
    info.vertices = info.triangles = info.inside_voxels = info.reserved = 77
    v = np.full(6, 0x77777777, np.uint32)
    t = np.full(3, 0x77777777, np.uint32)
    assert L.vr_mesh_count(None, C.byref(req), C.byref(info)) == -22
    assert b"NULL" in L.vr_last_error(None)
    assert L.vr_mesh_extract(None, C.byref(req), v.ctypes.data, 1, t.ctypes.data, 1, C.byref(info)) == -22
    assert L.vr_mesh_extract_device(None, C.byref(req), v.ctypes.data, 1, t.ctypes.data, 1, C.byref(info), None) == -22
    assert L.vr_mesh_count(None, None, None) == -22
    assert L.vr_mesh_extract(None, None, None, 0, None, 0, None) == -22
    assert (info.vertices, info.triangles, info.inside_voxels, info.reserved) == (77,) * 4
    assert np.all(v == 0x77777777) and np.all(t == 0x77777777)


# ---- the shim ----------------------------------------------------------------------------------------
def test_shim_compiles_with_extract_mesh(tmp_path):
    src = str(tmp_path / "vr_shim_mesh.cpp")
    exe = str(tmp_path / "vr_shim_mesh")
    with open(src, "w") as f:
        f.write(r"""
#include <vr/offscreen_pass_hip.hpp>
#include <vr/vr_host.h>
#include <cstdio>
int main(int argc, char **)
{
    static_assert(sizeof(vr_mesh_request) == 40 && sizeof(vr_mesh_vertex) == 24 && sizeof(vr_mesh_info) == 32 &&
                      VR_ENOSPC == -28, "vr_mesh.h");
    if (argc > 1) {  // never taken in the CPU test: needs a device
        Vol::Rendering::Hip::OffscreenPass pass(8, 8);
        const uint32_t lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
        const auto m = pass.extract_mesh(0.5f, true, false, lo, hi);
        return m.triangles.size() == 3 * m.info.triangles && m.vertices.size() == m.info.vertices ? 0 : 1;
    }
    vr_mesh_request req{};
    vr_mesh_info info{};
    vr_mesh_vertex v{};
    uint32_t t[3] = {0, 0, 0};
    std::printf("%d %d %d %d\n", vr_mesh_count(nullptr, &req, &info),
                vr_mesh_extract(nullptr, &req, &v, 1, t, 1, &info),
                vr_mesh_extract_device(nullptr, &req, &v, 1, t, 1, &info, nullptr),
                vr_mesh_write_ply(nullptr, &v, 1, t, 1, nullptr, nullptr));
    return 0;
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                        "-o", exe, "-L", LIBDIR, "-lvr_amd", "-Wl,-rpath," + LIBDIR],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "-22 -22 -22 -22"


# ---- the host helper header and the PLY writer, stand-alone, under AddressSanitizer + UBSan --------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_host_helpers_under_sanitizers(tmp_path):
    stdout = run_sanitized(tmp_path, "mesh", args=[str(tmp_path)])
    # the request-check table: the box rule and the cell range, restated here
    seen = 0
    for line in stdout.splitlines():
        w = line.replace(":", " ").split()
        if w[0] != "box":
            continue
        use, closed = int(w[1]), int(w[2])
        lo, hi, dims = ([int(x) for x in w[a:a + 3]] for a in (3, 6, 10))
        ok, clo, chi, nwork = int(w[13]), [int(x) for x in w[14:17]], [int(x) for x in w[17:20]], int(w[20])
        if not use:
            lo, hi = [0, 0, 0], dims
        want_ok = use <= 1 and closed <= 1 and all(lo[a] < hi[a] <= dims[a] for a in range(3))
        assert ok == int(want_ok), line
        if ok:
            assert clo == [lo[a] - closed for a in range(3)], line
            assert chi == [hi[a] - 1 - (1 - closed) for a in range(3)], line
            cells = (7, 8, 8)
            nb = [(hi[a] + 1) // cells[a] - (clo[a] + 2) // cells[a] + 1 for a in range(3)]
            assert nwork == min(nb[0] * nb[1] * nb[2], 2 ** 64 - 1), line
        seen += 1
    assert seen == 20
    assert os.path.exists(tmp_path / "mesh_harness.ply") and not os.path.exists(tmp_path / "mesh_harness_none.ply")


# ---- the library's PLY writer, through a reader of the test's own -----------------------------------------
def read_ply(path):
    b = open(path, "rb").read()
    end = b.index(b"end_header\n") + len(b"end_header\n")
    head = b[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = next(int(l.split()[2]) for l in head if l.startswith("element vertex "))
    nt = next(int(l.split()[2]) for l in head if l.startswith("element face "))
    props = [l.split()[1:] for l in head if l.startswith("property ")]
    assert props == [["float", n] for n in ("x", "y", "z", "nx", "ny", "nz")] + [["list", "uchar", "uint", "vertex_indices"]]
    verts = np.frombuffer(b, "<f4", nv * 6, end).reshape(nv, 6)
    off = end + nv * 24
    assert len(b) == off + nt * 13
    tris = np.empty((nt, 3), np.uint32)
    for i in range(nt):
        n, a, bb, c = struct.unpack_from("<BIII", b, off + 13 * i)
        assert n == 3
        tris[i] = (a, bb, c)
    return verts, tris


def test_ply_round_trip(tmp_path):
    m = S.reference("ball", True, True, None)
    path = str(tmp_path / "ball.ply")
    scale, offset = (19.0, 17.0, 21.0), (-0.5, 0.25, 3.0)
    vr_amd.write_ply(path, m.verts, m.tris, scale, offset)
    verts, tris = read_ply(path)
    assert np.array_equal(tris, m.tris)
    want = m.verts["pos"] * np.asarray(scale, F) + np.asarray(offset, F)
    assert want.dtype == F and np.array_equal(verts[:, :3].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(verts[:, 3:].view(np.uint32), m.verts["normal"].view(np.uint32))
    # no scale and offset: the records as they are; an empty mesh: a header alone
    vr_amd.write_ply(path, m.verts, m.tris)
    verts, tris = read_ply(path)
    assert np.array_equal(verts.view(np.uint32), S.records(m.verts)) and np.array_equal(tris, m.tris)
    vr_amd.write_ply(path, m.verts[:0], m.tris[:0])
    verts, tris = read_ply(path)
    assert verts.shape == (0, 6) and tris.shape == (0, 3)
    # refusals: an index beyond the vertices, an unwritable path
    none = str(tmp_path / "none.ply")
    with pytest.raises(RuntimeError, match="index"):
        vr_amd.write_ply(none, m.verts[:10], m.tris)
    assert not os.path.exists(none)
    with pytest.raises(RuntimeError, match="cannot write"):
        vr_amd.write_ply(str(tmp_path / "no" / "such" / "dir.ply"), m.verts, m.tris)


def test_frame_kernels_keep_the_parents_machine_code():
    """vr_amd.kernel_code_hash (code bytes and descriptors of the frame kernels) is the one the
    committed traffic record was measured on: the parent commit's (831a97d2592b2346 when the mesh
    kernels were added)."""
    want = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))["c3"]["code_hash"]
    assert vr_amd.kernel_code_hash() == want
